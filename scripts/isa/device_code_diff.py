#!/usr/bin/env python3
r"""Is the library's device code the same in two source trees?  The acceptance test of a refactor that must not move an instruction.

Each tree's single-unit device assembly (every kernel implicit in one unit: 254 kernels, ~475 000 lines, about a minute of hipcc) is

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I sparrowrecsys_amd/csrc -DSPRK_SINGLE_TU --cuda-device-only -S \
          sparrowrecsys_amd/csrc/sparrow_hip.hip -o <tree>.s

and the two files are compared line by line after
  * the `__hip_cuid_<hash>` symbol is blanked (it hashes the source TEXT, so any edit moves it), and
  * each --rename OLD=NEW (regular expression, applied to the FIRST file's text) is carried out: a kernel whose template parameter list
    changed has a new mangled name and nothing else new.
An empty diff means the same kernels with the same instructions, register counts, LDS sizes and kernel descriptors.  Exit status 1 otherwise.

    python scripts/isa/device_code_diff.py <old tree or old.s> <new tree or new.s> [--rename OLD=NEW ...] [--keep DIR]

Dropping a trailing `int XP = 0` from k_din_fused<KC, MB, TAIL, ATT, XP> (Itanium mangling: the literal `Li0E` in front of the list's `E`):
    --rename '(11k_din_fusedILi\dELb[01]ELb[01]ELb[01]E)Li0E=\1'"""
import argparse, os, re, subprocess, sys, tempfile


def assembly(src, keep):
    if os.path.isfile(src):
        return open(src).read()
    out = os.path.join(keep, os.path.basename(os.path.abspath(src)) + ".s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", "include", "-I", "sparrowrecsys_amd/csrc", "-DSPRK_SINGLE_TU",
                        "--cuda-device-only", "-S", "sparrowrecsys_amd/csrc/sparrow_hip.hip", "-o", os.path.abspath(out)], cwd=src,
                       capture_output=True, text=True)
    if r.returncode:
        sys.exit("hipcc failed in %s:\n%s" % (src, r.stderr[-4000:]))
    return open(out).read()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--keep", help="directory for the .s files of trees compiled here (default: a temporary one)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        keep = a.keep or tmp
        os.makedirs(keep, exist_ok=True)
        old, new = assembly(a.old, keep), assembly(a.new, keep)
        for r in a.rename:
            pat, _, to = r.partition("=")
            old, n = re.subn(pat, to, old)
            print("rename %s: %d occurrences" % (pat, n))
        paths = []
        for tag, t in (("old", old), ("new", new)):
            t = re.sub(r"__hip_cuid_\w+", "__hip_cuid_", t)
            print("%s: %d kernels, %d lines" % (tag, len(re.findall(r"^\s*\.amdhsa_kernel ", t, re.M)), t.count("\n")))
            paths.append(os.path.join(tmp, tag + ".normalised.s"))
            open(paths[-1], "w").write(t)
        delta = subprocess.run(["diff"] + paths, capture_output=True, text=True).stdout.splitlines()
    for l in delta[:200]:
        print(l)
    print("device code: %s" % ("DIFFERENT (%d diff lines)" % len(delta) if delta else "identical"))
    return 1 if delta else 0


if __name__ == "__main__":
    sys.exit(main())
