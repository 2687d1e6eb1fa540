"""The held-out split on the device (featureeng.split_device: sprk_split_plan + two sprk_take_rows), measured and written to
docs/split_results.md.

Samples shaped like MovieLens-20M's -- the 26 columns of featureeng.build at hist_len 5, the genre, history and numeric columns as
strided views of [n, 8], [n, 5] and [n, 7] matrices, source_row a permutation -- at 1 M and about 19.7 M rows, device resident, in both
modes at sample 0.1 and 1.0 (train 0.8):

  plan / take train / take test   each between two events on the stream, the calls made as split_device makes them: the genre,
                                  history and numeric columns as three row-wide columns (32, 20 and 28 bytes a row)
  takes, every column singly      the two takes with each of the 26 columns taken by its stride (group_matrices=False)
  split_device                    the whole call, its one synchronisation and its allocations included (host clock)
  torch                           the plain-torch route on the device, fed the SAME sampled flags and random sides: torch.kthvalue over
                                  the sampled timestamps for the quantile, then a boolean mask per column (host clock, synchronised)
  split_host                      the definition in numpy over the host copy of the columns (one run)

Warmed, --repeats runs, the median.  The device result is compared with split_host byte for byte.  The figures are recorded, not
judged.  Needs a HIP device.

    python scripts/split_rate.py [--repeats 7] [--sizes 1000000,19700000] [--out docs/split_results.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="1000000,19700000")
    ap.add_argument("--out", default=os.path.join(ROOT, "docs", "split_results.md"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("split_rate.py needs a HIP device")
    from sparrowrecsys_amd import _lib as L
    from sparrowrecsys_amd import featureeng as FE
    lib = L.load_library()
    dev = torch.device("cuda", 0)

    def columns(n):
        g = torch.Generator(device=dev)
        g.manual_seed(n)
        ri = lambda hi, shape, dt=torch.int32: torch.randint(0, hi, shape, generator=g, device=dev, dtype=dt)
        genres, hist = ri(19, (n, 8)), ri(27000, (n, 5))
        dense = torch.rand((n, 7), generator=g, device=dev, dtype=torch.float32)
        return FE._columns_dict(5, ri(138000, (n,)), ri(27000, (n,)), ri(11, (n,)).to(torch.float32) * 0.5, ri(600_000_000, (n,), torch.int64) + 800_000_000, ri(2, (n,)),
                                torch.randperm(n, generator=g, device=dev).to(torch.int32), genres, hist, dense)

    def host_timed(fn):
        ts = []
        for _ in range(a.repeats + 1):                      # the first run warms
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[1:]) * 1e3, out

    p = lambda x: C.c_void_p(None if x is None else x.data_ptr())

    def parts_timed(cols, mode, sample, grouped=True):
        """plan, take train, take test as split_device calls them (grouped: the columns of one matrix as one row-wide column; else every
        column singly), each between events; -> three medians in ms, (n_train, n_test)"""
        n = len(cols["userId"])
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        index = torch.empty((2, n), dtype=torch.int32, device=dev)
        ws = torch.empty(lib.sprk_split_plan_workspace_bytes(n) // 8 + 2, dtype=torch.int64, device=dev)
        key, ts = cols["source_row"].contiguous(), cols["timestamp"].contiguous()
        runs = []
        for _ in range(a.repeats + 1):
            ev = [None] + [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            words = torch.tensor([-1, 0, 0, 0, 0], dtype=torch.int64, device=dev)
            L.check(lib.sprk_split_plan(p(key), 1, p(ts) if mode == "time" else None, n, 0, FE.split_threshold(sample), FE.split_threshold(0.8), 0.8, FE.SPLIT_MODES[mode],
                                        p(index[0]), p(index[1]), p(words), p(ws), ws.numel() * 8, stream))
            counts = [int(v) for v in words.cpu().numpy()[2:4]]
            outs = []
            groups = FE._matrix_groups(cols) if grouped else [[k] for k in cols]
            for which, count in enumerate(counts):
                out = [torch.empty((count, len(g)), dtype=cols[g[0]].dtype, device=dev) for g in groups]
                desc = (L.SplitCol * len(groups))(*(L.SplitCol(cols[g[0]].data_ptr(), cols[g[0]].stride(0) * cols[g[0]].element_size(), len(g) * cols[g[0]].element_size(), 0,
                                                               o.data_ptr()) for g, o in zip(groups, out)))
                outs.append((out, desc))
            ev[1].record()                                  # (the allocations above are no part of the takes)
            for which, count in enumerate(counts):
                L.check(lib.sprk_take_rows(outs[which][1], len(groups), p(index[which]), count, n, stream))
                ev[2 + which].record()
            # the plan's own time: recorded apart, with no host work between its events
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            words.copy_(torch.tensor([-1, 0, 0, 0, 0], dtype=torch.int64))
            e0.record()
            L.check(lib.sprk_split_plan(p(key), 1, p(ts) if mode == "time" else None, n, 0, FE.split_threshold(sample), FE.split_threshold(0.8), 0.8, FE.SPLIT_MODES[mode],
                                        p(index[0]), p(index[1]), p(words), p(ws), ws.numel() * 8, stream))
            e1.record()
            torch.cuda.synchronize()
            runs.append((e0.elapsed_time(e1), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])))
            del outs
        med = [statistics.median(r[i] for r in runs[1:]) for i in range(3)]
        return med, counts

    def torch_route(cols, mode, sampled, random_train):
        if mode == "time":
            ts = cols["timestamp"]
            picked = ts[sampled]
            m = picked.numel()
            r = max(int(np.ceil(np.float64(0.8) * np.float64(m))), 1)
            stamp = torch.kthvalue(picked, r).values
            train = sampled & (ts <= stamp)
        else:
            train = sampled & random_train
        test = sampled & ~train
        return {k: v[train] for k, v in cols.items()}, {k: v[test] for k, v in cols.items()}

    lines = ["# The held-out split on the device: measurements", "",
             "Written by `scripts/split_rate.py` on %s (HIP %s): %d runs after a warm-up, the median.  `plan`, `take train` and `take test` lie between events on the"
             " stream; `split_device`, the torch route and `split_host` are under a host clock that ends in a synchronise." % (torch.cuda.get_device_name(0), torch.version.hip, a.repeats),
             "Samples shaped like MovieLens-20M's: 26 columns, the genre, history and numeric columns as strided views of their matrices; `train` 0.8, seed 0, key `source_row`."
             "  Nothing here is a bar; the figures are recorded.", "",
             "| rows | mode | sample | n_train | n_test | plan ms | take train ms | take test ms | sum ms | takes, every column singly ms | `split_device` ms | torch route ms | `split_host` ms | device = host |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    versus = []                                             # (split_device ms, torch route ms) per row of the table
    for n in [int(s) for s in a.sizes.split(",")]:
        cols = columns(n)
        host = {k: v.cpu().numpy() for k, v in cols.items()}
        for mode in ("random", "time"):
            for sample in (0.1, 1.0):
                (plan_ms, train_ms, test_ms), counts = parts_timed(cols, mode, sample)
                (_, single_train_ms, single_test_ms), _ = parts_timed(cols, mode, sample, grouped=False)
                whole_ms, got = host_timed(lambda: FE.split_device(cols, mode=mode, sample=sample))
                t0 = time.perf_counter()
                want = FE.split_host(host, mode=mode, sample=sample)
                host_ms = (time.perf_counter() - t0) * 1e3
                same = got.n_sampled == want.n_sampled and got.split_timestamp == want.split_timestamp and all(
                    part_g[k].cpu().numpy().tobytes() == np.ascontiguousarray(part_w[k]).tobytes() for part_g, part_w in ((got.train, want.train), (got.test, want.test)) for k in part_w)
                assert same, "the device result differs from the host definition"
                sampled = torch.from_numpy(FE.split_draws(0, host["source_row"], 0) < np.uint64(FE.split_threshold(sample))).to(dev)
                random_train = torch.from_numpy(FE.split_draws(0, host["source_row"], 1) < np.uint64(FE.split_threshold(0.8))).to(dev)
                torch_ms, other = host_timed(lambda: torch_route(cols, mode, sampled, random_train))
                assert all(other[0][k].cpu().numpy().tobytes() == np.ascontiguousarray(want.train[k]).tobytes() for k in want.train), "the torch route differs from the definition"
                del got, other
                versus.append((whole_ms, torch_ms))
                lines.append("| %d | %s | %.1f | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.0f | yes |"
                             % (n, mode, sample, counts[0], counts[1], plan_ms, train_ms, test_ms, plan_ms + train_ms + test_ms, single_train_ms + single_test_ms, whole_ms, torch_ms, host_ms))
                print(lines[-1], flush=True)
        del cols, host
        torch.cuda.empty_cache()
    slower = "slower in every row" if all(r[0] < r[1] for r in versus) else "NOT slower in %d of %d rows" % (sum(r[0] >= r[1] for r in versus), len(versus))
    lines += ["", "For scale: `featureeng.build` produces the 19.7 M samples in 24.7 ms (docs/feature_eng_results.md).", "",
              "Reading the table.  `sum` is what the stream spends; `split_device` adds the call's one synchronisation (the five words), the allocation of the exact"
              " outputs and the ctypes calls.  In time mode the plan's extra cost is the radix select: eight histogram passes over the flags and the sampled"
              " timestamps, each followed by a one-workgroup pick.  `takes, every column singly` is the same two takes with the genre, history and numeric columns"
              " taken one by one through their strides instead of as three row-wide columns: `split_device` groups them (`group_matrices=True`) because of this column.",
              "The torch route is fed the same sampled flags and random sides, so it pays for neither draw; what it pays for is a masked select per column and, in"
              " time mode, `torch.kthvalue` over the sampled timestamps.  It is %s; the C ABI is also what a caller without Python gets." % slower, ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
