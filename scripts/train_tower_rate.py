"""Rates of trainer_tower on the device (train_device / sprk_train_tower_fit, tower_rows_device / sprk_tower_rows, towers(...).recommend_for_users),
for docs/train_tower_results.md.  Needs a HIP device.

The shape is the reference's neural_cf_model_2 (emb_dim 10, hidden (10, 10)) over tables of MovieLens-20M's size (131 263 movie rows, 138 494
user rows); the samples are generated on the device: users uniform, movies skewed towards small ids (floor(V u^3)), labels fair coins.
batch_size 4096, packed device-resident arrays, weights resident on the device.

* per tile: device events around fits of 1 and of 3 epochs (warmed up, repeated): time per step = the difference over the extra steps,
  set-up (the schedule: check, count, scan, scatter, sort; the copy of the weights) = the one-epoch fit less its steps;
* the same steps under torch on the host's CPU (torch.optim.Adam, dense gradients as Keras has them, 16 threads) on --torch-rows rows;
* train_host on the first --host-rows rows, one epoch, and whether the device gives its bytes there;
* --rows: tower_rows_device over both tables, and towers(...).recommend_for_users(k=10) for every user.

The split of a step over its three launches is read from a kernel trace of this script at one tile and few samples, e.g.
`rocprofv3 --kernel-trace --stats -- python scripts/train_tower_rate.py --samples 131072 --tiles 8 --repeat 1`.

    python scripts/train_tower_rate.py --samples 1000000 --tiles 1,2,4,8,16,32 --torch-rows 81920 --host-rows 8192 --rows --out train_tower_rate.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MOVIES, USERS = 131263, 138494


def device_weights(torch, fam, seed):
    """Trained-like weights made where they are used: Glorot-sized kernels, biases in [0, 0.2), unit-scale rows, a head of 1."""
    from sparrowrecsys_amd import trainer_tower as TT
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    w = {}
    for k, shape in TT.param_shapes(fam).items():
        if k.startswith("emb/"):
            w[k] = torch.randn(shape, generator=g, device="cuda") / shape[1] ** 0.5
        elif k == "head/kernel":
            w[k] = torch.ones(shape, device="cuda")
        elif k.endswith("/kernel"):
            w[k] = (torch.rand(shape, generator=g, device="cuda") * 2 - 1) * (6.0 / (shape[0] + shape[1])) ** 0.5
        else:
            w[k] = torch.rand(shape, generator=g, device="cuda") * 0.2
    return w


def make_data(torch, fam, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    movie = (torch.rand(n, generator=g, device="cuda") ** 3 * fam.columns[0][2]).to(torch.int32).clamp_(max=fam.columns[0][2] - 1)
    user = torch.randint(0, fam.columns[1][2], (n,), generator=g, device="cuda", dtype=torch.int32)
    labels = (torch.rand(n, generator=g, device="cuda") < 0.5).to(torch.float32)
    return torch.stack([movie, user], dim=1).contiguous(), labels


def timed_fit(torch, TT, fam, w, ids, labels, batch, tile, epochs):
    """-> the device time of one fit in seconds (events on the current stream around train_device)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    TT.train_device(fam, w, ids, None, labels, batch_size=batch, epochs=epochs, tile=tile)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def timed(torch, f, repeat):
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return sorted(out)


def torch_steps(fam, w, ids, labels, batch):
    import torch
    import torch.nn.functional as Fn

    from tests import train_tower_cases as TWC
    torch.set_num_threads(16)
    p = {k: v.cpu().clone().requires_grad_(True) for k, v in w.items()}
    opt = torch.optim.Adam(list(p.values()), lr=0.001, eps=1e-7)
    ids, labels = ids.cpu().numpy(), labels.cpu()
    t0 = time.perf_counter()
    for b0 in range(0, len(labels), batch):
        opt.zero_grad()
        Fn.binary_cross_entropy_with_logits(TWC.torch_logit(fam, p, ids[b0:b0 + batch]), labels[b0:b0 + batch]).backward()
        opt.step()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--tiles", default="0")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=0)
    ap.add_argument("--host-rows", type=int, default=0)
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from sparrowrecsys_amd import trainer_tower as TT
    if not torch.cuda.is_available():
        raise SystemExit("train_tower_rate.py measures on the device: no HIP device is visible")
    out = {"samples": a.samples, "batch": a.batch, "device": torch.cuda.get_device_name(0), "rows": []}
    steps = (a.samples + a.batch - 1) // a.batch

    def emit(row):
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
    fam = TT.make_family(MOVIES, USERS, 10, (10, 10))
    w = device_weights(torch, fam, 1)
    ids, labels = make_data(torch, fam, a.samples, 7)
    for tile in [int(t) or TT.default_tile(fam) for t in a.tiles.split(",")]:           # 0: the default
        if TT.lds_bytes(fam, tile) > TT.LDS_BYTES:
            emit({"model": "tower", "tile": tile, "lds_bytes": TT.lds_bytes(fam, tile), "skipped": "beyond the LDS"})
            continue
        timed_fit(torch, TT, fam, w, ids[:4 * a.batch], labels[:4 * a.batch], a.batch, tile, 1)      # warm-up: code objects, allocator
        one, three = [], []
        for _ in range(a.repeat):
            one.append(timed_fit(torch, TT, fam, w, ids, labels, a.batch, tile, 1))
            three.append(timed_fit(torch, TT, fam, w, ids, labels, a.batch, tile, 3))
        step = (np.median(three) - np.median(one)) / (2 * steps)
        emit({"model": "tower", "tile": tile, "lds_bytes": TT.lds_bytes(fam, tile), "steps_per_epoch": steps, "params": TT.n_params(fam),
              "fit_1_epoch_s": sorted(one), "fit_3_epochs_s": sorted(three), "step_us": step * 1e6, "epoch_s": step * steps,
              "setup_s": float(np.median(one) - step * steps), "samples_per_s": a.samples / (step * steps)})
    if a.torch_rows:
        n = min(a.torch_rows, a.samples)
        dt = torch_steps(fam, w, ids[:n], labels[:n], a.batch)
        emit({"model": "tower", "torch_cpu_rows": n, "torch_cpu_s": dt, "torch_cpu_step_us": dt / ((n + a.batch - 1) // a.batch) * 1e6, "threads": 16})
    if a.host_rows:
        n = min(a.host_rows, a.samples)
        hw = {k: v.cpu().numpy() for k, v in w.items()}
        t0 = time.perf_counter()
        want = TT.train_host(fam, hw, ids[:n].cpu().numpy(), None, labels[:n].cpu().numpy(), batch_size=a.batch, epochs=1)
        dt = time.perf_counter() - t0
        got = TT.train_device(fam, w, ids[:n], None, labels[:n], batch_size=a.batch, epochs=1)
        same = all(got.weights[k].cpu().numpy().tobytes() == want.weights[k].tobytes() and got.v[k].cpu().numpy().tobytes() == want.v[k].tobytes() for k in want.weights) \
            and got.p.cpu().numpy().tobytes() == want.p.tobytes()
        emit({"model": "tower", "train_host_rows": n, "train_host_s": dt, "device_gives_the_host_bytes": bool(same)})
        if not same:
            raise SystemExit("the device's bytes differ from train_host's")
    if a.rows:
        got = TT.train_device(fam, w, ids, None, labels, batch_size=a.batch, epochs=1)
        flat = TT._flat_view(fam, got.weights, ids.device)
        for side, vocab in (("item", MOVIES), ("user", USERS)):
            TT.tower_rows_device(fam, flat, side)
            t = timed(torch, lambda: TT.tower_rows_device(fam, flat, side), max(a.repeat, 3))
            emit({"model": "tower", "tower_rows": side, "table_rows": vocab, "tile": TT.default_rows_tile(fam), "seconds": t, "rows_per_s": vocab / float(np.median(t))})
        seen = {"movieId": ids[:, 0], "userId": ids[:, 1]}
        tm = TT.towers(got, seen)
        t = timed(torch, lambda: TT.towers(got, seen), max(a.repeat, 3))
        emit({"model": "tower", "towers_s": t, "users_seen": int(tm.user_has.sum()), "movies_seen": int(tm.item_has.sum()), "sign": tm.sign})
        tm.recommend_for_users(np.arange(1024), k=10)
        t = timed(torch, lambda: tm.recommend_for_users(k=10), 2)
        emit({"model": "tower", "recommend_for_users_k": 10, "queries": int(tm.user_has.sum()), "candidates": int(tm.item_has.sum()), "seconds": t})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
