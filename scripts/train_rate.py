"""Rates of model.fit on the device (trainer.train_device / sprk_train_fit), for docs/train_results.md.  Needs a HIP device.

The model shapes of NeuralCF.py and EmbeddingMLP.py (the reference's bucket counts and widths), samples shaped like MovieLens-20M as
the models see them: ids uniform over the buckets, a quarter of the genre slots empty, numerics at their raw magnitudes; everything is
generated on the device from a seed.  batch_size 4096, packed device-resident arrays.  Per model and tile:

* a host clock around synchronised fits of 1 and of 3 epochs (warmed up, repeated): time per step = the difference over the extra
  steps, set-up (the schedule: count, scan, scatter, sort) = the one-epoch fit less its steps;
* the same epoch under torch on the host's CPU (torch.optim.Adam, dense gradients as Keras has them, 16 threads) on --torch-rows rows;
* train_host on the first --host-rows rows, one epoch, and whether the device gives its bytes there.

    python scripts/train_rate.py --samples 1000000 --tiles 8,16,32,64 --out train_rate_1m.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_data(torch, fam, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    cols = []
    for _, kind, vocab in fam.columns:
        c = torch.randint(0, vocab, (n,), generator=g, device="cuda", dtype=torch.int32)
        if kind == "genre":
            c = torch.where(torch.rand(n, generator=g, device="cuda") < 0.25, torch.full_like(c, -1), c)
        cols.append(c)
    ids = torch.stack(cols, dim=1).contiguous()
    scale = torch.tensor([2000.0, 10000.0, 1.5, 5.0, 200.0, 5.0, 1.5][:fam.n_dense], device="cuda")
    dense = (torch.rand(n, fam.n_dense, generator=g, device="cuda") * scale).contiguous()
    labels = (torch.rand(n, generator=g, device="cuda") < 0.5).to(torch.float32)
    return ids, dense, labels


def timed_fit(torch, T, fam, w, data, batch, tile, epochs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = T.train_device(fam, w, *data, batch_size=batch, epochs=epochs, tile=tile)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, got


def torch_epoch(fam, w, ids, dense, labels, batch):
    import torch
    import torch.nn.functional as Fn
    torch.set_num_threads(16)
    p = {k: torch.tensor(np.array(v), requires_grad=True) for k, v in w.items()}
    opt = torch.optim.Adam(list(p.values()), lr=0.001, eps=1e-7)
    ids, dense, labels = ids.cpu().to(torch.int64), dense.cpu(), labels.cpu()
    t0 = time.perf_counter()
    for b0 in range(0, len(labels), batch):
        i, d = ids[b0:b0 + batch], dense[b0:b0 + batch]
        blocks = [Fn.embedding(i[:, c].clamp(min=0), p[tab]) * (i[:, c] >= 0).to(torch.float32)[:, None] for c, tab in enumerate(fam.tables)]
        x = torch.stack([d[:, s] if c < 0 else blocks[c][:, s] for c, s in zip(fam.xcol, fam.xsub)], dim=1)
        for name in fam.layers[:-1]:
            x = Fn.relu(Fn.linear(x, p[name + "/kernel"].t(), p[name + "/bias"]))
        logit = Fn.linear(x, p["head/kernel"].t(), p["head/bias"])[:, 0]
        opt.zero_grad()
        Fn.binary_cross_entropy_with_logits(logit, labels[b0:b0 + batch]).backward()
        opt.step()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--tiles", default="32")
    ap.add_argument("--models", default="neuralcf,embedding_mlp")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=0)
    ap.add_argument("--host-rows", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from sparrowrecsys_amd import models as M
    from sparrowrecsys_amd import trainer as T
    if not torch.cuda.is_available():
        raise SystemExit("train_rate.py measures on the device: no HIP device is visible")
    out = {"samples": a.samples, "batch": a.batch, "device": torch.cuda.get_device_name(0), "rows": []}
    for name in a.models.split(","):
        model = {"neuralcf": M.NeuralCF, "embedding_mlp": M.EmbeddingMLP}[name](seed=1)
        w = model.init_weights(1, trained_like=True)               # (the numerics are raw: rows scaled to their magnitudes)
        fam = T.family_of(model)
        data = make_data(torch, fam, a.samples, 7)
        steps = (a.samples + a.batch - 1) // a.batch
        n_table = sum(v * fam.emb_dim for _, _, v in fam.columns)
        n_params = sum(int(np.prod(s)) for s in T.param_shapes(fam).values())
        for tile in [int(t) or T.default_tile(fam) for t in a.tiles.split(",")]:       # 0: the default
            if T.lds_bytes(fam, tile) > T.LDS_BYTES:
                continue
            small = tuple(t[:4 * a.batch] for t in data)
            timed_fit(torch, T, fam, w, small, a.batch, tile, 1)                           # warm-up: code objects, allocator
            one, three = [], []
            for _ in range(a.repeat):                                                      # alternating, as the spread is the host's
                one.append(timed_fit(torch, T, fam, w, data, a.batch, tile, 1)[0])
                three.append(timed_fit(torch, T, fam, w, data, a.batch, tile, 3)[0])
            step = (np.median(three) - np.median(one)) / (2 * steps)
            row = {"model": name, "tile": tile, "steps_per_epoch": steps, "table_floats": n_table, "params": n_params,
                   "fit_1_epoch_s": sorted(one), "fit_3_epochs_s": sorted(three), "step_us": step * 1e6, "epoch_s": step * steps,
                   "setup_s": float(np.median(one) - step * steps), "samples_per_s": a.samples / (step * steps)}
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
        if a.torch_rows:
            n = min(a.torch_rows, a.samples)
            dt = torch_epoch(fam, w, *(t[:n] for t in data), a.batch)
            row = {"model": name, "torch_cpu_rows": n, "torch_cpu_s": dt, "torch_cpu_step_us": dt / ((n + a.batch - 1) // a.batch) * 1e6,
                   "torch_cpu_epoch_s_extrapolated": dt / n * a.samples, "threads": 16}
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
        if a.host_rows:
            n = min(a.host_rows, a.samples)
            sl = tuple(t[:n] for t in data)
            t0 = time.perf_counter()
            want = T.train_host(fam, w, *(t.cpu().numpy() for t in sl), batch_size=a.batch, epochs=1)
            dt = time.perf_counter() - t0
            got = T.train_device(fam, w, *sl, batch_size=a.batch, epochs=1)
            same = all(got.weights[k].cpu().numpy().tobytes() == want.weights[k].tobytes() and got.v[k].cpu().numpy().tobytes() == want.v[k].tobytes() for k in want.weights) \
                and got.p.cpu().numpy().tobytes() == want.p.tobytes()
            row = {"model": name, "train_host_rows": n, "train_host_s": dt, "device_gives_the_host_bytes": bool(same)}
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
            if not same:
                raise SystemExit("the device's bytes differ from train_host's")
        del data
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
