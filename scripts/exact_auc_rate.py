"""The exact ROC and PR areas (Spark's BinaryClassificationMetrics), the device route against the host:

  device        metrics.exact_auc_device over N device-resident float32 scores and labels: the whole call (allocations, the enqueue, the
                one synchronisation and the 64-byte copy; host clock), and the enqueued kernels alone (HIP events)
  host          metrics.exact_auc_host, the definition (numpy), over the same rows already on the host
  exact_roc_auc scores.cpu() and then metrics.exact_roc_auc: what a caller had before (the Python loop over sorted scores, ROC only)
  keras200      DeviceMetrics.update + result over the same device scores: the 200-threshold figures, for context
  bins          the enqueued kernels alone at other bin widths (SPRK_EXACT_AUC_BIN_BITS), next to the rule's own
  long rows     the share of rows that lie in bins longer than the LDS sort holds (they take the chunked sort and the merge passes)

at N = 2^20 and 2^24 for three inputs: `sigmoid` (sigmoid of a normal logit, labels drawn from the score), `uniform`, and `tied`
(the sigmoid scores rounded to 10^-3).  Then model level, NeuralCF on synthetic columns:

  evaluate_exact           the new route: one flat score buffer in device memory, one sprk_exact_auc
  evaluate + exact_roc_auc the route before it: model.evaluate (predict, every score to the host, numpy metrics), then exact_roc_auc

Every device result is checked against the host definition, word for word, at the size it is timed at.  Warmed; median, min and max of
--repeats runs (host legs that take tens of seconds run --host-repeats times).  The figures are recorded, not judged.  Needs a HIP device.

    python scripts/exact_auc_rate.py [--repeats 5] [--sizes 20,24] [--out docs/exact_auc_rate.json]
    python scripts/exact_auc_rate.py --only-device tied --sizes 24      # the device route alone, for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_input(np, kind, N, seed):
    rng = np.random.RandomState(seed)
    if kind == "uniform":
        p = rng.random_sample(N).astype(np.float32)
    else:
        p = (1.0 / (1.0 + np.exp(-1.5 * rng.standard_normal(N)))).astype(np.float32)
        if kind == "tied":
            p = (np.round(p.astype(np.float64) * 1000.0) / 1000.0).astype(np.float32)
    y = (rng.random_sample(N) < p).astype(np.float32)
    return y, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--sizes", default="20,24", help="log2 of the row counts")
    ap.add_argument("--bins", default="-4,-2,-1,1,2,4", help="bin widths to try, as offsets from the rule's bits")
    ap.add_argument("--only-device", default=None, help="one input (sigmoid / uniform / tied): the device route alone, --repeats times")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("exact_auc_rate.py needs a HIP device")
    from sparrowrecsys_amd import _lib as L
    from sparrowrecsys_amd import metrics as MT
    lib = L.load_library()

    def ms(v):
        return round(v * 1e3, 4)

    def stats(ts):
        return {"median": ms(statistics.median(ts)), "min": ms(min(ts)), "max": ms(max(ts))}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def enqueued(pd, yd):
        """The kernels of one call alone: events round the enqueue, the result read after them."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        call = MT._exact_auc_enqueue(pd, yd)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, call.result()

    sizes = [int(s) for s in a.sizes.split(",")]
    if a.only_device:
        for lg in sizes:
            y, p = make_input(np, a.only_device, 1 << lg, 100 + lg)
            pd, yd = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
            ts = [enqueued(pd, yd)[0] for _ in range(a.repeats + 1)][1:]
            print(a.only_device, "N=2^%d" % lg, json.dumps(stats(ts)), flush=True)
        return

    result = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "pr_run": MT.PR_RUN, "scores": {}, "model": {}}
    for lg in sizes:
        N = 1 << lg
        bits = lib.sprk_exact_auc_bin_bits(N)
        for kind in ("sigmoid", "uniform", "tied"):
            y, p = make_input(np, kind, N, 100 + lg)
            pd, yd = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
            t_host, want = [], None
            for _ in range(max(1, a.host_repeats)):
                t0 = time.perf_counter()
                want = MT.exact_auc_host(y, p)
                t_host.append(time.perf_counter() - t0)
            got = MT.exact_auc_device(pd, yd)                       # warm
            assert got.words() == want.words(), (kind, lg, got, want)
            t_call = [wall(lambda: MT.exact_auc_device(pd, yd))[0] for _ in range(a.repeats)]
            t_kern = [enqueued(pd, yd)[0] for _ in range(a.repeats)]
            t0 = time.perf_counter()
            on_host = pd.cpu().numpy()
            t_copy = time.perf_counter() - t0
            t0 = time.perf_counter()
            rank = MT.exact_roc_auc(y, on_host)
            t_rank = time.perf_counter() - t0
            assert abs(rank - want.area_under_roc) <= 1e-12
            dm = MT.DeviceMetrics(200)
            dm.update(pd, yd), dm.result()

            def keras():
                m = MT.DeviceMetrics(200)
                m.update(pd, yd)
                return m.result()
            t_keras = [wall(keras)[0] for _ in range(a.repeats)]
            k200 = keras()
            keys = MT.exact_score_keys(p) >> np.uint32(32 - bits)
            counts = np.bincount(keys.astype(np.int64))
            sweep = {}
            for off in [int(s) for s in a.bins.split(",")]:
                b = bits + off
                if not 1 <= b <= 24:
                    continue
                os.environ["SPRK_EXACT_AUC_BIN_BITS"] = str(b)
                try:
                    enqueued(pd, yd)
                    ts, res = zip(*[enqueued(pd, yd) for _ in range(a.repeats)])
                    assert all(r.words() == want.words() for r in res)
                    sweep[str(b)] = stats(list(ts))
                finally:
                    del os.environ["SPRK_EXACT_AUC_BIN_BITS"]
            med = statistics.median(t_call)
            res = {"rows": N, "n_thresholds": want.n_thresholds, "area_under_roc": want.area_under_roc, "area_under_pr": want.area_under_pr,
                   "keras200_roc": k200[2], "keras200_pr": k200[3], "bin_bits": bits, "workspace_mbytes": round(lib.sprk_exact_auc_workspace_bytes(N) / 1e6, 1),
                   "rows_in_long_bins_share": round(float(counts[counts > 4096].sum()) / N, 4), "longest_bin": int(counts.max()),
                   "device_call_ms": stats(t_call), "device_kernels_ms": stats(t_kern), "host_definition_ms": stats(t_host),
                   "copy_scores_to_host_ms": ms(t_copy), "exact_roc_auc_ms": ms(t_rank), "keras200_device_ms": stats(t_keras),
                   "host_definition_over_device_call": round(statistics.median(t_host) / med, 1),
                   "copy_plus_exact_roc_auc_over_device_call": round((t_copy + t_rank) / med, 1), "kernels_ms_at_other_bin_bits": sweep}
            result["scores"]["%s/N=2^%d" % (kind, lg)] = res
            print("%s/N=2^%d" % (kind, lg), json.dumps(res), flush=True)
            del pd, yd
    if not a.no_model:
        from sparrowrecsys_amd import models as M
        from sparrowrecsys_amd import synthetic as SY
        model = M.NeuralCF(seed=1)
        for lg in sizes:
            N = 1 << lg
            feats = SY.synth_fields(N, [(c.key, c.kind, c.vocab) for c in model.id_columns], seed=5)
            feats["label"] = (np.random.default_rng(6).random(N) < 0.56).astype(np.int64)
            got = model.evaluate_exact(feats, batch_size=65536)      # warm
            t_new = [wall(lambda: model.evaluate_exact(feats, batch_size=65536))[0] for _ in range(a.repeats)]
            model.evaluate({k: v[:65536] for k, v in feats.items()})
            t_old, t_old_rank = [], []
            for _ in range(max(1, a.host_repeats)):
                t0 = time.perf_counter()
                four = model.evaluate(feats, batch_size=65536)
                t1 = time.perf_counter()
                rank = MT.exact_roc_auc(feats["label"], model.predict(feats, batch_size=65536)[:, 0])
                t2 = time.perf_counter()
                t_old.append(t1 - t0)
                t_old_rank.append(t2 - t1)
            assert abs(rank - got.area_under_roc) <= 1e-12
            res = {"rows": N, "evaluate_exact_ms": stats(t_new), "evaluate_ms": stats(t_old), "predict_plus_exact_roc_auc_ms": stats(t_old_rank),
                   "area_under_roc": got.area_under_roc, "area_under_pr": got.area_under_pr, "n_thresholds": got.n_thresholds, "evaluate": four,
                   "old_route_over_evaluate_exact": round((statistics.median(t_old) + statistics.median(t_old_rank)) / statistics.median(t_new), 1)}
            result["model"]["NeuralCF/N=2^%d" % lg] = res
            print("NeuralCF/N=2^%d" % lg, json.dumps(res), flush=True)
            del feats
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
