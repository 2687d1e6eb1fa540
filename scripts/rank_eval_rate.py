"""Ranking metrics on the device (rankeval.rank_eval_device: sprk_rank_eval), measured and written to docs/rank_eval_results.md.

Inputs shaped like MovieLens-20M's: users whose activity is log-normal (at least 20 ratings each), movies drawn by a Zipf-like popularity
over 26 744 ids, a tenth of every user's ratings held out as truth and the rest seen; one list of 100 popular movies per user.  Two
sizes: 138 493 queries with 2 M truth and 18 M seen pairs, and 10 000 queries with a fourteenth of the pairs.  Cut-offs 10 and 100.

  whole call          sprk_rank_eval between two events on the stream, the inputs device resident, the workspace allocated before
  truth segments      the same call with no seen pairs and no queries: check, count, scan, scatter and sort of the truth side
  seen segments       likewise with no truth pairs and no queries
  metrics and sums    the whole call less a call with both sides and no queries: k_re_users, k_re_eval, k_re_partial, k_re_total
  rank_eval_device    the Python call: its allocations, the copy of the gain table and its one synchronisation included (host clock)
  rank_eval_host      the definition, numpy and Python loops over the host copy (one run).  The parent commit has no device route,
                      so the definition is the baseline

Warmed, --repeats runs, the median.  The device result is compared with rank_eval_host byte for byte.  The figures are recorded, not
judged.  Needs a HIP device.

    python scripts/rank_eval_rate.py [--repeats 7] [--sizes 10000,138493] [--out docs/rank_eval_results.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ITEMS, LIST_LEN, KS = 26744, 100, (10, 100)


def inputs(np, n_users):
    """-> pred [n_users, 100], truth_user, truth_item, seen_user, seen_item: int32 numpy arrays, about 144 pairs a user."""
    rng = np.random.default_rng(n_users)
    counts = np.maximum(20, rng.lognormal(4.35, 1.1, n_users)).astype(np.int64)
    counts = np.minimum(counts, 9000)
    user = np.repeat(np.arange(n_users, dtype=np.int32), counts)
    pop = 1.0 / np.arange(1, N_ITEMS + 1) ** 0.9
    pop /= pop.sum()
    item = rng.choice(N_ITEMS, size=len(user), p=pop).astype(np.int32)
    held = rng.random(len(user)) < 0.1
    order = rng.permutation(len(user))                                        # a ratings file is not grouped by user
    user, item, held = user[order], item[order], held[order]
    pred = rng.choice(N_ITEMS, size=(n_users, LIST_LEN), p=pop).astype(np.int32)
    return pred, user[held], item[held], user[~held], item[~held]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="10000,138493")
    ap.add_argument("--out", default=os.path.join(ROOT, "docs", "rank_eval_results.md"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("rank_eval_rate.py needs a HIP device")
    from sparrowrecsys_amd import _lib as L
    from sparrowrecsys_amd import rankeval as RE
    lib = L.load_library()
    dev = torch.device("cuda", 0)
    p = lambda x: C.c_void_p(None if x is None or not x.numel() else x.data_ptr())
    gain, gain_sum = (torch.from_numpy(t).to(dev) for t in RE.gain_table())
    ks = (C.c_int32 * len(KS))(*KS)

    def call_timed(pred, tu, ti, su, si, n_users, Q):
        """sprk_rank_eval over the first Q lists between two events -> the median in ms"""
        n_truth, n_seen = (0 if tu is None else tu.numel()), (0 if su is None else su.numel())
        ws = torch.empty(lib.sprk_rank_eval_workspace_bytes(n_truth, n_seen, n_users, Q) // 8 + 2, dtype=torch.int64, device=dev)
        per_query = torch.empty((Q + 1, len(KS), 6), dtype=torch.float64, device=dev)
        n_relevant, n_ranked = torch.empty(Q + 1, dtype=torch.int32, device=dev), torch.empty(Q + 1, dtype=torch.int32, device=dev)
        sums, counts = torch.empty((len(KS), 6), dtype=torch.float64, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
        word = torch.full((1,), -1, dtype=torch.int64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ts = []
        for _ in range(a.repeats + 1):                      # the first run warms
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.check(lib.sprk_rank_eval(p(pred) if Q else None, Q, LIST_LEN, LIST_LEN, None, p(tu), p(ti), n_truth, p(su), p(si), n_seen, n_users, ks, len(KS), p(gain), p(gain_sum),
                                       p(per_query), p(n_relevant), p(n_ranked), p(sums), p(counts), p(word), p(ws), ws.numel() * 8, stream))
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        assert int(word.cpu()[0]) == -1
        return statistics.median(ts[1:])

    lines = ["# Ranking metrics on the device: measurements", "",
             "Written by `scripts/rank_eval_rate.py` on %s (HIP %s): %d runs after a warm-up, the median.  The first four timings lie between events on the stream;"
             " `rank_eval_device` and `rank_eval_host` are under a host clock (the first ends in the call's own synchronise)." % (torch.cuda.get_device_name(0), torch.version.hip, a.repeats),
             "Inputs shaped like MovieLens-20M's: log-normal user activity, Zipf-like movie popularity over %d ids, a tenth of the pairs held out as truth, lists of %d entries,"
             " cut-offs %s.  The parent commit has no device route: the definition is the baseline.  Nothing here is a bar; the figures are recorded." % (N_ITEMS, LIST_LEN, list(KS)), "",
             "| queries | truth pairs | seen pairs | whole call ms | truth segments ms | seen segments ms | metrics and sums ms | `rank_eval_device` ms | `rank_eval_host` ms | device = host |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for n_users in [int(s) for s in a.sizes.split(",")]:
        host = inputs(np, n_users)
        pred, tu, ti, su, si = (torch.from_numpy(x).to(dev) for x in host)
        whole = call_timed(pred, tu, ti, su, si, n_users, n_users)
        truth_ms = call_timed(pred, tu, ti, None, None, n_users, 0)
        seen_ms = call_timed(pred, None, None, su, si, n_users, 0)
        both_ms = call_timed(pred, tu, ti, su, si, n_users, 0)
        ts = []
        for _ in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = RE.rank_eval_device(pred, None, tu, ti, su, si, n_users=n_users, ks=KS)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = RE.rank_eval_host(*host[:1], None, *host[1:], n_users=n_users, ks=KS)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = got.to_host()
        for name in ("per_query", "n_relevant", "n_ranked", "sums", "counts"):
            assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), "the device result differs from the host definition: " + name
        lines.append("| %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.0f | yes |"
                     % (n_users, len(host[1]), len(host[3]), whole, truth_ms, seen_ms, whole - both_ms, statistics.median(ts[1:]), host_ms))
        print(lines[-1], flush=True)
        print("   mean over the queries with truth, %s at %s:" % (RE.METRICS, KS), want.mean("truth").tolist(), flush=True)
        del pred, tu, ti, su, si, got
        torch.cuda.empty_cache()
    lines += ["", "Reading the table.  `truth segments` and `seen segments` are calls with one side and no queries: the check, the counts per user, the scan, the scatter and the"
              " segment sort of that side.  `metrics and sums` is the whole call less a call with both sides and no queries: the one-wave-per-query kernel and the two"
              " levels of ordered sums.  The shares are differences of whole calls, not kernel times.  `rank_eval_device` adds the allocations of the outputs and the"
              " workspace, the copy of the gain table and the call's one synchronisation.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
