"""model.evaluate's four numbers, two routes over the same rows and the same model:

  evaluate          model.evaluate(feats): predict -> every score back to the host -> metrics.evaluate_scores (numpy sorts)
  evaluate_device   model.evaluate_device(feats): the same packing and forward, the metrics accumulated in device memory
                    (sprk_metrics_update), one copy of a few KB at the end

for NeuralCF and DeepFM_v2 on synthetic columns at N = 2^20 and 2^24, plus

  update      sprk_metrics_update alone over N device-resident scores, for float32 / uint8 / int64 labels (HIP events), as bytes/s
              against the 4 + 4 / 1 / 8 bytes it reads per sample
  forward     the forward those scores come from, alone, over the packed device arrays (HIP events)
  evaluate_csv  over the file scripts/bench_predict_csv.py generates (tests/golden/test_samples_512.csv repeated to ~1 M rows),
              next to predict_csv on the same file

Both routes of a case run in one process, alternating, warmed; median, min and max of --repeats runs each (synchronise,
perf_counter around the call).  The figures are recorded, not judged.  Needs a HIP device.

    python scripts/evaluate_rate.py [--repeats 5] [--sizes 20,24] [--out docs/evaluate_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="20,24", help="log2 of the row counts")
    ap.add_argument("--csv-rows", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("evaluate_rate.py needs a HIP device")
    from sparrowrecsys_amd import metrics as MT
    from sparrowrecsys_amd import models as M
    from sparrowrecsys_amd import synthetic as SY
    assert a.repeats >= 5

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

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    result = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "evaluate": {}, "update": {}, "forward": {}}
    for name, model in (("NeuralCF", M.NeuralCF(seed=1)), ("DeepFM_v2", M.DeepFMv2(seed=1))):
        for lg in [int(s) for s in a.sizes.split(",")]:
            N = 1 << lg
            feats = SY.synth_fields(N, [(c.key, c.kind, c.vocab) for c in model.id_columns], seed=5)
            feats["label"] = (np.random.default_rng(6).random(N) < 0.56).astype(np.int64)
            host, dev = model.evaluate(feats, batch_size=65536), model.evaluate_device(feats, batch_size=65536)     # warm both
            assert host[1:] == dev[1:] and abs(host[0] - dev[0]) <= max(N, 64) * 2.0 ** -50 * host[0], (host, dev)
            t_host, t_dev = [], []
            for _ in range(a.repeats):                                # alternating
                t_dev.append(wall(lambda: model.evaluate_device(feats, batch_size=65536))[0])
                t_host.append(wall(lambda: model.evaluate(feats, batch_size=65536))[0])
            scores = model.predict(feats, batch_size=65536)[:, 0]
            t_metrics = [wall(lambda: MT.evaluate_scores(feats["label"], scores))[0] for _ in range(2)]     # the host half alone
            key = "%s/N=2^%d" % (name, lg)
            res = {"rows": N, "evaluate_ms": stats(t_host), "evaluate_device_ms": stats(t_dev), "host_metrics_alone_ms": ms(min(t_metrics)),
                   "evaluate_over_evaluate_device": round(statistics.median(t_host) / statistics.median(t_dev), 2), "result": dev}
            result["evaluate"][key] = res
            print(key, json.dumps(res), flush=True)
            # the forward alone, over the packed device arrays, in groups as evaluate_device runs it
            ids, dense = model.pack_device({k: v for k, v in feats.items() if k != "label"})
            out = torch.empty(N, dtype=torch.float32, device=ids.device)
            sl = [(lo, lo + 65536) for lo in range(0, N, 65536)]

            def forward():
                for g in range(0, len(sl), model.MANY_GROUP):
                    grp = sl[g:g + model.MANY_GROUP]
                    model.predict_device_many([ids[x:y] for x, y in grp], [dense[x:y] for x, y in grp], [out[x:y] for x, y in grp])
            forward()
            t_fwd = [events(forward) for _ in range(a.repeats)]
            result["forward"][key] = {"rows": N, "ms": stats(t_fwd), "rows_per_sec": round(N / statistics.median(t_fwd))}
            print("forward", key, json.dumps(result["forward"][key]), flush=True)
            if name == "NeuralCF":                                    # the update alone: the scores of this forward, every label storage
                for dtype, nbytes in (("float32", 4), ("uint8", 1), ("int64", 8)):
                    lab = torch.from_numpy(feats["label"]).cuda().to(getattr(torch, dtype))
                    dm = MT.DeviceMetrics(200)
                    dm.update(out, lab)
                    t_up = [events(lambda: dm.update(out, lab)) for _ in range(a.repeats)]
                    med = statistics.median(t_up)
                    k2 = "N=2^%d/%s labels" % (lg, dtype)
                    result["update"][k2] = {"rows": N, "ms": stats(t_up), "rows_per_sec": round(N / med), "bytes_per_sample": 4 + nbytes,
                                            "gbytes_per_sec": round(N * (4 + nbytes) / med / 1e9, 1)}
                    print("update", k2, json.dumps(result["update"][k2]), flush=True)
            del feats, ids, dense, out
    # evaluate_csv over the file of scripts/bench_predict_csv.py
    base = open(os.path.join(ROOT, "tests", "golden", "test_samples_512.csv"), "rb").read()
    head, body = base.split(b"\n", 1)
    reps = max(1, a.csv_rows // 512)
    with tempfile.NamedTemporaryFile(suffix=".csv", delete=False) as f:
        f.write(head + b"\n" + body * reps)
        big = f.name
    try:
        model = M.DeepFMv2(seed=1)
        model.evaluate_csv(base), model.predict_csv(base)
        got = model.evaluate_csv(big)
        t_eval, t_pred = [], []
        for _ in range(a.repeats):
            t_eval.append(wall(lambda: model.evaluate_csv(big))[0])
            t_pred.append(wall(lambda: model.predict_csv(big))[0])
        result["evaluate_csv"] = {"model": "DeepFM_v2", "rows": 512 * reps, "text_mbytes": round(os.path.getsize(big) / 1e6, 1), "evaluate_csv_ms": stats(t_eval),
                                  "predict_csv_ms": stats(t_pred), "rows_per_sec": round(512 * reps / statistics.median(t_eval)), "result": got}
        print("evaluate_csv", json.dumps(result["evaluate_csv"]), flush=True)
    finally:
        os.unlink(big)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
