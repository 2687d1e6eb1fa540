"""Embedding recall, EmbRanker.topk (sprk_emb_topk), against what the library could do before it existed.  Both paths run in one process,
alternating, warmed; one sample = --inner back-to-back calls between two device synchronisations, divided by --inner; median and spread
(min, max) of --repeats samples each.  Queries and table are device tensors: the times are the call's host code plus its kernels.

  a  serving shape    Q = 1,  N = 881,     D = 10, K = 800    baseline: score_many(q, arange(N)) with ordering (k_emb_rank_wave), cut to K
  b  catalogue shape  Q = 64, N = 131 073, D = 32, K = 1 024  baseline: score_many(..., want_order=False) over all rows, then torch.topk on
                                                             the device (for TIME only: its tie and NaN order is not the contract)

Condition: b -- the new median is faster than the baseline's by more than the larger of the two spreads (max - min); a -- not slower by more
than that spread.  There is no CPU figure: the script needs a HIP device.

    python scripts/emb_topk_rate.py [--repeats 12] [--inner 50] [--out profiles/r08/emb_topk_rate.json] [--only b]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "emb_topk_rate.json"))
    ap.add_argument("--only", default=None, help="run one case (a or b), new path only, and write nothing: for a profiler")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("emb_topk_rate.py needs a HIP device")
    from sparrowrecsys_amd.ranker import EmbRanker
    assert a.repeats >= 10 or a.only

    cases = [("a", 1, 881, 10, 800, "not_slower"), ("b", 64, 131073, 32, 1024, "faster")]
    result = {"repeats": a.repeats, "inner": a.inner, "device": torch.cuda.get_device_name(0), "cases": {}}
    all_ok = True
    for name, Q, N, D, K, cond in cases:
        if a.only and a.only != name:
            continue
        rng = np.random.default_rng(17)
        items = rng.normal(size=(N, D)).astype(np.float32)
        r = EmbRanker({i: items[i] for i in range(N)})
        q = torch.from_numpy(rng.normal(size=(Q, D)).astype(np.float32)).to(r.device)
        cand = torch.arange(N, dtype=torch.int32, device=r.device).repeat(Q, 1)

        def new():
            return r.topk(q, K)

        def old():
            if name == "a":
                s, o = r.score_many(q, cand)
                o = o[:, :K]
                return torch.gather(s, 1, o.long()), o
            s, _ = r.score_many(q, cand, want_order=False)
            v, i = torch.topk(s, K, dim=1)
            return v, i.int()

        def sample(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.inner):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.inner

        if a.only:
            for _ in range(max(3, a.repeats)):
                dt = sample(new)
            print(json.dumps({"case": name, "last_ms": round(dt * 1e3, 4)}))
            return
        for _ in range(2):                                           # warm both paths: code objects, workspace, allocator
            s_new, r_new = new()
            s_old, r_old = old()
            sample(new)
            sample(old)
        if name == "a":                                              # the same contract: identical bytes
            assert torch.equal(r_new, r_old) and torch.equal(s_new.view(torch.int64), s_old.view(torch.int64))
        else:                                                        # torch.topk: the same values (ties in its own order)
            assert torch.equal(s_new, s_old)
        t_new, t_old = [], []
        for _ in range(a.repeats):                                   # alternating
            t_new.append(sample(new))
            t_old.append(sample(old))
        med_new, med_old = statistics.median(t_new), statistics.median(t_old)
        spread = max(max(t_new) - min(t_new), max(t_old) - min(t_old))
        ok = (med_old - med_new > spread) if cond == "faster" else (med_new - med_old <= spread)
        all_ok &= ok
        ms = lambda v: round(v * 1e3, 4)                             # noqa: E731
        result["cases"][name] = {
            "shape": {"Q": Q, "N": N, "D": D, "K": K}, "condition": cond, "met": bool(ok),
            "topk_ms": {"median": ms(med_new), "min": ms(min(t_new)), "max": ms(max(t_new))},
            "baseline_ms": {"median": ms(med_old), "min": ms(min(t_old)), "max": ms(max(t_old))},
            "scored_rows_per_sec": round(Q * N / med_new), "speedup": round(med_old / med_new, 2)}
        print(name, json.dumps(result["cases"][name]), flush=True)
    result["all_conditions_met"] = bool(all_ok)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
