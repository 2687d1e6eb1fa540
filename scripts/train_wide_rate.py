"""Rates of trainer_wide.fit on the device (trainer_wide.train_device / sprk_train_wide_fit), for docs/train_wide_results.md.  Needs a HIP device.

Shapes (--shapes): `ref` = WideNDeep.py's (its bucket counts, emb_dim 10, deep 128-128, 10 000 indicator buckets in head/kernel); `c5` =
BASELINE config 5's cross, a 10 M x 32 emb/cross table, on the same deep stack (config 5's emb_dim 32 gives the first Dense kernel 327
input rows, more than the trainers' 256); `c5small` = `c5` with 10 000 cross rows: what `c5`'s step costs without Adam over the 3.8 GB
of cross parameters and moments.  Samples are generated on the device as scripts/train_rate.py generates them (its make_data and
timed_fit are used as they are).  batch_size 4096, packed device-resident arrays, weights resident on the device.  Per tile:

* a host clock around synchronised fits of 1 and of 3 epochs (warmed up, repeated): time per step = the difference over the extra
  steps, set-up (the buckets and the schedule: count, scan, scatter, sort; the copy of the weights) = the one-epoch fit less its steps;
* the same steps under torch on the host's CPU (torch.optim.Adam, dense gradients as Keras has them, 16 threads) on --torch-rows rows;
* train_host on the first --host-rows rows, one epoch, and whether the device gives its bytes there.

    python scripts/train_wide_rate.py --shapes ref --samples 1000000 --tiles 4,8,16,32 --out train_wide_rate_ref.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SHAPES = {"ref": dict(cross_buckets=10000, cross_dim=0), "c5": dict(cross_buckets=10_000_000, cross_dim=32), "c5small": dict(cross_buckets=10000, cross_dim=32)}


def device_weights(torch, fam, seed):
    """Trained-like weights made where they are used (the 10 M x 32 table is 1.28 GB): Glorot-sized kernels, small biases, unit-scale rows."""
    from sparrowrecsys_amd import trainer_wide as TW
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    w = {}
    for k, shape in TW.param_shapes(fam).items():
        if k.startswith("emb/"):
            w[k] = torch.randn(shape, generator=g, device="cuda") / shape[1] ** 0.5
        elif k.endswith("/kernel"):
            lim = (6.0 / ((fam.widths[-1] if k == "head/kernel" else shape[0]) + shape[1])) ** 0.5
            w[k] = (torch.rand(shape, generator=g, device="cuda") * 2 - 1) * lim
        else:
            w[k] = (torch.rand(shape, generator=g, device="cuda") * 2 - 1) * 0.1
    scale = torch.tensor([2000.0, 10000.0, 1.5, 5.0, 200.0, 5.0, 1.5], device="cuda")          # (the numerics are raw: rows scaled to their magnitudes)
    for k, (c, s) in enumerate(zip(fam.xcol, fam.xsub)):
        if c < 0:
            w["dense0/kernel"][k] /= scale[s]
    return w


def torch_steps(fam, w, ids, dense, labels, batch):
    import torch
    import torch.nn.functional as Fn

    from tests import train_wide_cases as TWC
    torch.set_num_threads(16)
    p = {k: v.cpu().clone().requires_grad_(True) for k, v in w.items()}
    opt = torch.optim.Adam(list(p.values()), lr=0.001, eps=1e-7)
    ids, dense, labels = ids.cpu().numpy(), dense.cpu(), labels.cpu()
    t0 = time.perf_counter()
    for b0 in range(0, len(labels), batch):
        opt.zero_grad()
        Fn.binary_cross_entropy_with_logits(TWC.torch_logit(fam, p, ids[b0:b0 + batch], dense[b0:b0 + batch], torch.float32), labels[b0:b0 + batch]).backward()
        opt.step()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ref")
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--tiles", default="0")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=0)
    ap.add_argument("--host-rows", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from train_rate import make_data, timed_fit

    from sparrowrecsys_amd import trainer_wide as TW
    if not torch.cuda.is_available():
        raise SystemExit("train_wide_rate.py measures on the device: no HIP device is visible")
    out = {"samples": a.samples, "batch": a.batch, "device": torch.cuda.get_device_name(0), "rows": []}
    steps = (a.samples + a.batch - 1) // a.batch

    def emit(row):
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
    for shape in a.shapes.split(","):
        fam = family(shape)                                            # (the shape alone: no 1.28 GB of host weights)
        w = device_weights(torch, fam, 1)
        data = make_data(torch, fam, a.samples, 7)
        n_params = sum(int(np.prod(s)) for s in TW.param_shapes(fam).values())
        for tile in [int(t) or TW.default_tile(fam) for t in a.tiles.split(",")]:       # 0: the default
            if TW.lds_bytes(fam, tile) > TW.LDS_BYTES:
                emit({"model": "wide", "shape": shape, "tile": tile, "lds_bytes": TW.lds_bytes(fam, tile), "skipped": "beyond the LDS"})
                continue
            small = tuple(t[:4 * a.batch] for t in data)
            timed_fit(torch, TW, fam, w, small, a.batch, tile, 1)                          # warm-up: code objects, allocator
            one, three = [], []
            for _ in range(a.repeat):
                one.append(timed_fit(torch, TW, fam, w, data, a.batch, tile, 1)[0])
                three.append(timed_fit(torch, TW, fam, w, data, a.batch, tile, 3)[0])
            step = (np.median(three) - np.median(one)) / (2 * steps)
            emit({"model": "wide", "shape": shape, "tile": tile, "lds_bytes": TW.lds_bytes(fam, tile), "steps_per_epoch": steps, "params": n_params,
                  "cross_floats": fam.cross_buckets * max(1, fam.cross_dim), "fit_1_epoch_s": sorted(one), "fit_3_epochs_s": sorted(three), "step_us": step * 1e6,
                  "epoch_s": step * steps, "setup_s": float(np.median(one) - step * steps), "samples_per_s": a.samples / (step * steps)})
        if a.torch_rows:
            n = min(a.torch_rows, a.samples)
            dt = torch_steps(fam, w, *(t[:n] for t in data), a.batch)
            emit({"model": "wide", "shape": shape, "torch_cpu_rows": n, "torch_cpu_s": dt, "torch_cpu_step_us": dt / ((n + a.batch - 1) // a.batch) * 1e6, "threads": 16})
        if a.host_rows:
            n = min(a.host_rows, a.samples)
            sl = tuple(t[:n] for t in data)
            hw = {k: v.cpu().numpy() for k, v in w.items()}
            t0 = time.perf_counter()
            want = TW.train_host(fam, hw, *(t.cpu().numpy() for t in sl), batch_size=a.batch, epochs=1)
            dt = time.perf_counter() - t0
            got = TW.train_device(fam, w, *sl, batch_size=a.batch, epochs=1)
            same = all(got.weights[k].cpu().numpy().tobytes() == want.weights[k].tobytes() and got.v[k].cpu().numpy().tobytes() == want.v[k].tobytes() for k in want.weights) \
                and got.p.cpu().numpy().tobytes() == want.p.tobytes()
            emit({"model": "wide", "shape": shape, "train_host_rows": n, "train_host_s": dt, "device_gives_the_host_bytes": bool(same)})
            if not same:
                raise SystemExit("the device's bytes differ from train_host's")
        del w, data
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def family(shape):
    """The trainer's family of a shape, built from the reference model's with the cross replaced (no weights are made)."""
    from sparrowrecsys_amd import models as M
    from sparrowrecsys_amd import trainer_wide as TW
    fam = TW.family_of(M.WideNDeep(seed=1))._replace(**SHAPES[shape])
    TW._check_family(fam)
    return fam


if __name__ == "__main__":
    main()
