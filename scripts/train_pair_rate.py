"""Rates of trainer_pair.fit on the device (trainer_pair.train_device / sprk_train_pair_fit), for docs/train_pair_results.md.  Needs a HIP device.

Shapes (--shapes): `ref` = DeepFM.py's (4 fields with its bucket counts, emb_dim 10, 4 pairs, deep 64-64 over the movieId and userId deep
tables and the 7 numerics); `c2` = BASELINE config 2's (synthetic.CONFIG2_FIELDS: 6 fields with the MovieLens-20M id ranges, emb_dim 16,
CONFIG2_PAIRS: 8 pairs, the same deep part).  `--shared` ties the deep tables to the FM tables.  Samples are generated on the device as
scripts/train_rate.py generates them (its make_data and timed_fit are used as they are).  batch_size 4096, packed device-resident arrays,
weights resident on the device.  Per tile:

* a host clock around synchronised fits of 1 and of 3 epochs (warmed up, repeated): time per step = the difference over the extra
  steps, set-up (the schedule: check, count, scan, scatter, sort; the copy of the weights) = the one-epoch fit less its steps;
* the same steps under torch on the host's CPU (torch.optim.Adam, dense gradients as Keras has them, 16 threads) on --torch-rows rows;
* train_host on the first --host-rows rows, one epoch, and whether the device gives its bytes there.

The split of a step over its three launches is read from a kernel trace of this script at one tile and few samples, e.g.
`rocprofv3 --kernel-trace --stats -- python scripts/train_pair_rate.py --shapes ref --samples 131072 --tiles 8 --repeat 1`.

    python scripts/train_pair_rate.py --shapes ref,c2 --samples 1000000 --tiles 2,4,8,16,32 --out train_pair_rate.json
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


def family(shape, shared=False):
    """The trainer's family of a shape (no weights are made)."""
    from sparrowrecsys_amd import models as M
    from sparrowrecsys_amd import synthetic as SY
    from sparrowrecsys_amd import trainer_pair as TP
    from sparrowrecsys_amd.schema import NUMERIC_KEYS
    if shape == "ref":
        return TP.make_family(M._default_fields(), M.DeepFM.DEFAULT_PAIRS, ("movieId", "userId"), shared, 10, (64, 64), list(NUMERIC_KEYS))
    if shape == "c2":
        return TP.make_family(SY.CONFIG2_FIELDS, SY.CONFIG2_PAIRS, ("movieId", "userId"), shared, 16, (64, 64), list(NUMERIC_KEYS))
    raise SystemExit("unknown shape %r" % shape)


def device_weights(torch, fam, seed):
    """Trained-like weights made where they are used: Glorot-sized kernels, small biases, unit-scale rows."""
    from sparrowrecsys_amd import trainer_pair as TP
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    w = {}
    for k, shape in TP.param_shapes(fam).items():
        if "emb/" in k:
            w[k] = torch.randn(shape, generator=g, device="cuda") / shape[1] ** 0.5
        elif k.endswith("/kernel"):
            lim = (6.0 / ((len(fam.pairs) + fam.hidden[-1] if k == "head/kernel" else shape[0]) + shape[1])) ** 0.5
            w[k] = (torch.rand(shape, generator=g, device="cuda") * 2 - 1) * lim
        else:
            w[k] = (torch.rand(shape, generator=g, device="cuda") * 2 - 1) * 0.1
    scale = torch.tensor([2000.0, 10000.0, 1.5, 5.0, 200.0, 5.0, 1.5], device="cuda")          # (the numerics are raw: rows scaled to their magnitudes)
    for k, (j, s) in enumerate(zip(fam.xsrc, fam.xsub)):
        if j < 0:
            w["deep0/kernel"][k] /= scale[s]
    return w


def torch_steps(fam, w, ids, dense, labels, batch):
    import torch
    import torch.nn.functional as Fn

    from tests import train_pair_cases as TPC
    torch.set_num_threads(16)
    p = {k: v.cpu().clone().requires_grad_(True) for k, v in w.items()}
    opt = torch.optim.Adam(list(p.values()), lr=0.001, eps=1e-7)
    ids, dense, labels = ids.cpu().numpy(), dense.cpu(), labels.cpu()
    t0 = time.perf_counter()
    for b0 in range(0, len(labels), batch):
        opt.zero_grad()
        Fn.binary_cross_entropy_with_logits(TPC.torch_logit(fam, p, ids[b0:b0 + batch], dense[b0:b0 + batch], torch.float32), labels[b0:b0 + batch]).backward()
        opt.step()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ref")
    ap.add_argument("--shared", action="store_true")
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

    from sparrowrecsys_amd import trainer_pair as TP
    if not torch.cuda.is_available():
        raise SystemExit("train_pair_rate.py measures on the device: no HIP device is visible")
    out = {"samples": a.samples, "batch": a.batch, "shared": a.shared, "device": torch.cuda.get_device_name(0), "rows": []}
    steps = (a.samples + a.batch - 1) // a.batch

    def emit(row):
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
    for shape in a.shapes.split(","):
        fam = family(shape, a.shared)
        w = device_weights(torch, fam, 1)
        data = make_data(torch, fam, a.samples, 7)
        n_params = sum(int(np.prod(s)) for s in TP.param_shapes(fam).values())
        for tile in [int(t) or TP.default_tile(fam) for t in a.tiles.split(",")]:       # 0: the default
            if TP.lds_bytes(fam, tile) > TP.LDS_BYTES:
                emit({"model": "pair", "shape": shape, "tile": tile, "lds_bytes": TP.lds_bytes(fam, tile), "skipped": "beyond the LDS"})
                continue
            small = tuple(t[:4 * a.batch] for t in data)
            timed_fit(torch, TP, fam, w, small, a.batch, tile, 1)                          # warm-up: code objects, allocator
            one, three = [], []
            for _ in range(a.repeat):
                one.append(timed_fit(torch, TP, fam, w, data, a.batch, tile, 1)[0])
                three.append(timed_fit(torch, TP, fam, w, data, a.batch, tile, 3)[0])
            step = (np.median(three) - np.median(one)) / (2 * steps)
            emit({"model": "pair", "shape": shape, "shared": a.shared, "tile": tile, "lds_bytes": TP.lds_bytes(fam, tile), "steps_per_epoch": steps, "params": n_params,
                  "fit_1_epoch_s": sorted(one), "fit_3_epochs_s": sorted(three), "step_us": step * 1e6, "epoch_s": step * steps,
                  "setup_s": float(np.median(one) - step * steps), "samples_per_s": a.samples / (step * steps)})
        if a.torch_rows:
            n = min(a.torch_rows, a.samples)
            dt = torch_steps(fam, w, *(t[:n] for t in data), a.batch)
            emit({"model": "pair", "shape": shape, "torch_cpu_rows": n, "torch_cpu_s": dt, "torch_cpu_step_us": dt / ((n + a.batch - 1) // a.batch) * 1e6, "threads": 16})
        if a.host_rows:
            n = min(a.host_rows, a.samples)
            sl = tuple(t[:n] for t in data)
            hw = {k: v.cpu().numpy() for k, v in w.items()}
            t0 = time.perf_counter()
            want = TP.train_host(fam, hw, *(t.cpu().numpy() for t in sl), batch_size=a.batch, epochs=1)
            dt = time.perf_counter() - t0
            got = TP.train_device(fam, w, *sl, batch_size=a.batch, epochs=1)
            same = all(got.weights[k].cpu().numpy().tobytes() == want.weights[k].tobytes() and got.v[k].cpu().numpy().tobytes() == want.v[k].tobytes() for k in want.weights) \
                and got.p.cpu().numpy().tobytes() == want.p.tobytes()
            emit({"model": "pair", "shape": shape, "train_host_rows": n, "train_host_s": dt, "device_gives_the_host_bytes": bool(same)})
            if not same:
                raise SystemExit("the device's bytes differ from train_host's")
        del w, data
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
