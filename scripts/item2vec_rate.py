#!/usr/bin/env python
"""Item2vec: the host experiment behind the default round, and the device's rate.

  python scripts/item2vec_rate.py --rounds [--seeds 5] [--jobs 5]
      host only (numpy; the same bits as the device): skipgram_host on tests/item2vec_cases.py's clustered corpus at round = 1 for
      --seeds seeds, and at every power of two up to 4 096 for seed 0, with and without the row cap.  Prints one JSON line per fit.
  python scripts/item2vec_rate.py --parity [--ratings 20000]
      device against the host definition (bytes) at a size the host finishes in about a minute, with both timings.
  python scripts/item2vec_rate.py --rate --ratings 1000000 [--iters 1] [--round 1024]
      device alone on ratings shaped like MovieLens (synthetic: users with log-normal activity, items by a power law).
Results are recorded by hand in docs/item2vec_results.md."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sparrowrecsys_amd import item2vec as IV  # noqa: E402


def movielens_like(n, seed=0):
    """n ratings: about n / 145 users, n / 750 items (MovieLens 20M: 138 k users, 27 k movies), half stars, timestamps in file order."""
    rng = np.random.default_rng(seed)
    n_users, n_items = max(n // 145, 2), max(n // 750, 20)
    w = rng.lognormal(0.0, 1.0, n_users)
    u = rng.choice(n_users, n, p=w / w.sum())
    m = np.minimum((rng.random(n) ** 3 * n_items).astype(np.int64), n_items - 1)
    r = (rng.integers(1, 11, n) * 0.5).astype(np.float32)
    r[rng.random(n) < 0.3] = 4.0
    t = (1_000_000_000 + rng.integers(0, 10 ** 8, n)).astype(np.int64)
    return {"userId": u.astype(np.int64), "movieId": m, "rating": r, "timestamp": t}, n_users, n_items


def _one(job):
    from tests import item2vec_cases as K
    round, cap, seed = job
    t = time.time()
    loss, pur, top = K.clustered_fit(round, cap, seed)
    return {"round": round, "row_cap": cap, "seed": seed, "loss": loss, "purity": pur, "max_abs_syn1": top, "seconds": round_(time.time() - t)}


def round_(x):
    return float("%.3g" % x)


def rounds(args):
    from concurrent.futures import ProcessPoolExecutor
    jobs = [(1, 32, s) for s in range(args.seeds)]
    jobs += [(1 << p, cap, 0) for p in range(12, 0, -1) for cap in (32, 1 << 30)]
    with ProcessPoolExecutor(args.jobs) as pool:
        for out in pool.map(_one, jobs):
            print(json.dumps(out), flush=True)


def device_fit(cols, n_users, n_items, **kw):
    import torch
    torch.cuda.synchronize()
    t = time.time()
    model = IV.fit(cols, n_users=n_users, n_items=n_items, **kw)
    torch.cuda.synchronize()
    return model, time.time() - t


def parity(args):
    cols, n_users, n_items = movielens_like(args.ratings)
    kw = dict(D=10, iters=args.iters, round=args.round)
    device_fit(cols, n_users, n_items, **dict(kw, iters=0))                       # (warm-up: the library, the allocator)
    model, dev_s = device_fit(cols, n_users, n_items, **kw)
    t = time.time()
    vocab, host = IV.item2vec_host(cols["userId"], cols["movieId"], cols["rating"], cols["timestamp"], n_users, n_items, **kw)
    host_s = time.time() - t
    got = model.to_host()
    same = bool(np.array_equal(got.vectors.view(np.uint32), host.vectors.view(np.uint32)) and np.array_equal(got.syn1.view(np.uint32), host.syn1.view(np.uint32))
                and np.float64(got.loss).tobytes() == np.float64(host.loss).tobytes())
    print(json.dumps({"mode": "parity", "ratings": args.ratings, "words": int(vocab.counts.sum()), "vocab": len(vocab.ids), "iters": args.iters, "round": args.round,
                      "same_bytes": same, "loss": host.loss, "device_seconds": round_(dev_s), "host_seconds": round_(host_s)}))
    return 0 if same else 1


def rate(args):
    cols, n_users, n_items = movielens_like(args.ratings)
    import torch
    dev = torch.device("cuda", 0)
    cols = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
    kw = dict(D=10, round=args.round)
    device_fit(cols, n_users, n_items, **dict(kw, iters=0))
    _, base_s = device_fit(cols, n_users, n_items, **dict(kw, iters=0))            # sequences, vocabulary, occurrence lists, loss
    model, dev_s = device_fit(cols, n_users, n_items, **dict(kw, iters=args.iters))
    words = int(model.vocab.counts.sum())
    print(json.dumps({"mode": "rate", "ratings": args.ratings, "words": words, "vocab": len(model.ids), "iters": args.iters, "round": args.round, "loss": model.loss,
                      "setup_seconds": round_(base_s), "fit_seconds": round_(dev_s),
                      "words_per_second_per_iteration": round_(words * args.iters / max(dev_s - base_s, 1e-9))}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", action="store_true")
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--rate", action="store_true")
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=5)
    ap.add_argument("--ratings", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--round", type=int, default=IV.DEFAULT_ROUND)
    args = ap.parse_args()
    if args.rounds:
        return rounds(args)
    if args.parity:
        return parity(args)
    if args.rate:
        return rate(args)
    ap.error("one of --rounds, --parity, --rate")


if __name__ == "__main__":
    sys.exit(main())
