"""model.predict(features_dict), host dict -> scores on the host, B = 65 536: the native column packers (device native -> host native ->
Python, CTRModel.pack_device) against the Python packer alone (SPRK_PACK_NATIVE=0: schema.pack_ids / pack_dense, the route before the
native packers existed).  Both routes run in one process, alternating, warmed; median and spread (min, max) of --repeats runs each.

  a1  config 2 synthetic columns, all numeric, DeepFMv2          a2  config 3 synthetic columns with the [B, 50] history matrix, DIN
  b   the sample file's columns tiled to B, typed int32 / float32 with S genre columns: DeepFMv2, DIN, EmbeddingMLP
  c   the same as object-string columns (what read_samples_csv hands over)
  d   a1 and a2 as CUDA tensors

Condition per case: a2, b, c, d -- the new route's median is faster than the forced route's by more than the larger of the two spreads
(max - min); a1 -- not slower by more than that spread.  There is no CPU figure: the script needs a HIP device.

    python scripts/predict_dict_rate.py [--rows 65536] [--repeats 12] [--out profiles/r07/predict_dict_rate.json] [--only b/EmbeddingMLP]
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
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "predict_dict_rate.json"))
    ap.add_argument("--only", default=None, help="run one case (e.g. b/EmbeddingMLP), new route only, and write nothing: for a profiler")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("predict_dict_rate.py needs a HIP device")
    from sparrowrecsys_amd import ingest, models as M, schema as S, synthetic as SY
    B = a.rows
    assert a.repeats >= 10 or a.only

    def tiled(f):
        n = len(next(iter(f.values())))
        return {k: np.tile(v, (B + n - 1) // n)[:B] for k, v in f.items()}

    def typed(f):
        out = {}
        for k, v in f.items():
            if "Genre" in k:
                out[k] = np.asarray(v).astype(str).astype("S")
            elif k in S.FLOAT_KEYS or k == "rating":
                out[k] = S.to_float_column(v)
            else:
                out[k] = S.to_int_column(v).astype(np.int32)
        return out

    def cuda(f):
        return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in f.items()}

    strings = tiled(S.read_samples_csv(os.path.join(ROOT, "tests", "golden", "test_samples_512.csv")))
    f2 = SY.synth_fields(B, SY.CONFIG2_FIELDS, seed=1)
    f3 = SY.synth_din(B, 50, 5000, 7000, seed=3)
    m2 = lambda: M.DeepFMv2(seed=2, emb_dim=16, fields=SY.CONFIG2_FIELDS, proj_dim=16)                      # noqa: E731
    m3 = lambda: M.DIN(seed=4, emb_dim=32, hist_len=50, movie_buckets=5000, user_buckets=7000)              # noqa: E731
    sample_models = [("DeepFMv2", lambda: M.DeepFMv2(seed=1)), ("DIN", lambda: M.DIN(seed=1)), ("EmbeddingMLP", lambda: M.EmbeddingMLP(seed=1))]
    cases = [("a1/DeepFMv2", m2, f2, "not_slower"), ("a2/DIN", m3, f3, "faster")]
    cases += [("b/" + n, mk, typed(strings), "faster") for n, mk in sample_models]
    cases += [("c/" + n, mk, strings, "faster") for n, mk in sample_models]
    cases += [("d1/DeepFMv2", m2, cuda(f2), "faster"), ("d2/DIN", m3, cuda(f3), "faster")]

    def run(model, feats, forced):
        if forced:
            os.environ["SPRK_PACK_NATIVE"] = "0"
        else:
            os.environ.pop("SPRK_PACK_NATIVE", None)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scores = model.predict(feats)                            # ends in the device -> host copy of the scores
            dt = time.perf_counter() - t0
            return dt, scores, ingest.last_pack_route()
        finally:
            os.environ.pop("SPRK_PACK_NATIVE", None)

    if a.only:
        name, mk, feats, _ = [c for c in cases if c[0] == a.only][0]
        model = mk()
        for _ in range(max(3, a.repeats)):
            dt, _, route = run(model, feats, False)
        print(json.dumps({"case": name, "route": route, "last_ms": round(dt * 1e3, 3)}))
        return

    result = {"rows": B, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "host_threads": ingest.default_threads(), "cases": {}}
    all_ok = True
    for name, mk, feats, cond in cases:
        model = mk()
        for _ in range(2):                                           # warm both routes: engine, staging buffers, allocator
            _, s_new, _ = run(model, feats, False)
            _, s_old, _ = run(model, feats, True)
        assert np.array_equal(s_new, s_old), name
        t_new, t_old, route = [], [], None
        for _ in range(a.repeats):                                   # alternating
            dt, _, route = run(model, feats, False)
            t_new.append(dt)
            dt, _, r_old = run(model, feats, True)
            assert r_old == "python"
            t_old.append(dt)
        med_new, med_old = statistics.median(t_new), statistics.median(t_old)
        spread = max(max(t_new) - min(t_new), max(t_old) - min(t_old))
        ok = (med_old - med_new > spread) if cond == "faster" else (med_new - med_old <= spread)
        all_ok &= ok
        ms = lambda v: round(v * 1e3, 3)                             # noqa: E731
        result["cases"][name] = {
            "route": route, "condition": cond, "met": bool(ok),
            "native_ms": {"median": ms(med_new), "min": ms(min(t_new)), "max": ms(max(t_new))},
            "python_ms": {"median": ms(med_old), "min": ms(min(t_old)), "max": ms(max(t_old))},
            "native_rows_per_sec": round(B / med_new), "python_rows_per_sec": round(B / med_old), "speedup": round(med_old / med_new, 2)}
        print(name, json.dumps(result["cases"][name]), flush=True)
    result["all_conditions_met"] = bool(all_ok)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
