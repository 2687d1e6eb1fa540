"""Rates of trainer_dien.fit on the device (trainer_dien.train_device / sprk_train_dien_fit), for docs/train_dien_results.md.  Needs a HIP device.

The reference shape of DIEN.py (its bucket counts, T 5, emb_dim 10, att_hidden 32, tail (128, 64), 7 numerics), samples generated on the
device as scripts/train_rate.py generates them (its make_data and timed_fit are used as they are: every movie column uniform over the
movie buckets), then a fifth of the history ids set to 0 so that the GRU's mask is at work.  batch_size 4096, packed device-resident
arrays.  Per tile:

* a host clock around synchronised fits of 1 and of 3 epochs (warmed up, repeated): time per step = the difference over the extra
  steps, set-up (the schedule: count, scan, scatter, sort) = the one-epoch fit less its steps;
* the same steps under torch on the host's CPU (torch.optim.Adam, dense gradients as Keras has them, 16 threads) on --torch-rows rows;
* train_host on the first --host-rows rows, one epoch, and whether the device gives its bytes there.

The split by kernel comes from a run of its own under `rocprofv3 --kernel-trace --stats -- python scripts/train_dien_rate.py ...`.

    python scripts/train_dien_rate.py --samples 1000000 --tiles 1,2,4,8,16 --torch-rows 40960 --host-rows 8192 --out train_dien_rate_1m.json
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


def torch_steps(fam, w, ids, dense, labels, batch):
    import torch
    import torch.nn.functional as Fn

    from tests import train_dien_cases as TFC
    torch.set_num_threads(16)
    p = {k: torch.tensor(np.array(v), requires_grad=True) for k, v in w.items()}
    opt = torch.optim.Adam(list(p.values()), lr=0.001, eps=1e-7)
    ids, dense, labels = ids.cpu().to(torch.int64), dense.cpu(), labels.cpu()
    t0 = time.perf_counter()
    for b0 in range(0, len(labels), batch):
        opt.zero_grad()
        Fn.binary_cross_entropy_with_logits(TFC.torch_logit(fam, p, ids[b0:b0 + batch], dense[b0:b0 + batch], torch.float32), labels[b0:b0 + batch]).backward()
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from train_rate import make_data, timed_fit

    from sparrowrecsys_amd import models as M
    from sparrowrecsys_amd import trainer_dien as TF
    if not torch.cuda.is_available():
        raise SystemExit("train_dien_rate.py measures on the device: no HIP device is visible")
    out = {"samples": a.samples, "batch": a.batch, "device": torch.cuda.get_device_name(0), "rows": []}
    model = M.DIEN(seed=1)
    w = model.init_weights(1, trained_like=True)                   # (the numerics are raw: rows scaled to their magnitudes)
    fam = TF.family_of(model)
    data = make_data(torch, fam, a.samples, 7)
    hist = data[0][:, 1:fam.hist_len + 1]
    hist[torch.rand(hist.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8)) < 0.2] = 0
    steps = (a.samples + a.batch - 1) // a.batch
    n_params = sum(int(np.prod(s)) for s in TF.param_shapes(fam).values())
    n_table = sum(int(np.prod(TF.param_shapes(fam)[t])) for t in fam.tables)

    def emit(row):
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
    for tile in [int(t) or TF.default_tile(fam) for t in a.tiles.split(",")]:           # 0: the default
        if TF.lds_bytes(fam, tile) > TF.LDS_BYTES:
            emit({"model": "dien", "tile": tile, "lds_bytes": TF.lds_bytes(fam, tile), "skipped": "beyond the LDS"})
            continue
        small = tuple(t[:4 * a.batch] for t in data)
        timed_fit(torch, TF, fam, w, small, a.batch, tile, 1)                              # warm-up: code objects, allocator
        one, three = [], []
        for _ in range(a.repeat):
            one.append(timed_fit(torch, TF, fam, w, data, a.batch, tile, 1)[0])
            three.append(timed_fit(torch, TF, fam, w, data, a.batch, tile, 3)[0])
        step = (np.median(three) - np.median(one)) / (2 * steps)
        emit({"model": "dien", "tile": tile, "lds_bytes": TF.lds_bytes(fam, tile), "steps_per_epoch": steps, "table_floats": n_table, "params": n_params,
              "fit_1_epoch_s": sorted(one), "fit_3_epochs_s": sorted(three), "step_us": step * 1e6, "epoch_s": step * steps,
              "setup_s": float(np.median(one) - step * steps), "samples_per_s": a.samples / (step * steps)})
    if a.torch_rows:
        n = min(a.torch_rows, a.samples)
        dt = torch_steps(fam, w, *(t[:n] for t in data), a.batch)
        emit({"model": "dien", "torch_cpu_rows": n, "torch_cpu_s": dt, "torch_cpu_step_us": dt / ((n + a.batch - 1) // a.batch) * 1e6,
              "torch_cpu_epoch_s_extrapolated": dt / n * a.samples, "threads": 16})
    if a.host_rows:
        n = min(a.host_rows, a.samples)
        sl = tuple(t[:n] for t in data)
        t0 = time.perf_counter()
        want = TF.train_host(fam, w, *(t.cpu().numpy() for t in sl), batch_size=a.batch, epochs=1)
        dt = time.perf_counter() - t0
        got = TF.train_device(fam, w, *sl, batch_size=a.batch, epochs=1)
        same = all(got.weights[k].cpu().numpy().tobytes() == want.weights[k].tobytes() and got.v[k].cpu().numpy().tobytes() == want.v[k].tobytes() for k in want.weights) \
            and got.p.cpu().numpy().tobytes() == want.p.tobytes()
        emit({"model": "dien", "train_host_rows": n, "train_host_s": dt, "device_gives_the_host_bytes": bool(same)})
        if not same:
            raise SystemExit("the device's bytes differ from train_host's")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
