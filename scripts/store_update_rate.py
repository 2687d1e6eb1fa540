"""New ratings applied to a feature store in HBM (FeatureStore.update, sprk_store_update) against rebuilding the store from all ratings
(FeatureStore.from_ratings, sprk_feature_eng), on the ratings of scripts/feature_eng_rate.py shaped like MovieLens-20M, sorted by
timestamp so that later batches are later in time:

  build     empty + update(all --ratings rows)  against  from_ratings on the same device-resident columns
  update    --repeats successive batches of 100 000, of 1 000 and of 1 rating onto that store, each against from_ratings on the
            concatenation of everything applied so far (the columns concatenated beforehand, outside the timing)
  state     the bytes an updatable store keeps next to its tables

After the build and after the first batch of each size the updated tables are compared with the rebuilt ones byte for byte.  Timings:
synchronise, perf_counter around the call, warmed, median / min / max of --repeats runs; they include the call's own allocations
(workspace; for the builds also tables and state).  The figures are recorded, not judged.  Needs a HIP device.

    python scripts/store_update_rate.py [--repeats 5] [--out docs/store_update_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

BATCHES = [100_000, 1_000, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ratings", type=int, default=20_000_000)
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("store_update_rate.py needs a HIP device")
    from feature_eng_rate import synth
    from sparrowrecsys_amd import featurestore as FS

    def ms(v):
        return round(v * 1e3, 3)

    def stats(ts):
        return {"median": ms(statistics.median(ts)), "min": ms(min(ts)), "max": ms(max(ts))}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def same(x, y):
        return all(torch.equal(p, q) for p, q in zip(x.tensors(), y.tensors()))

    assert a.repeats >= 5
    extra = a.repeats * sum(BATCHES)
    t0 = time.perf_counter()
    ratings, table, lens = synth(a.ratings + extra, a.users)
    order = np.argsort(ratings["timestamp"], kind="stable")
    n_users, n_movies = a.users, len(table.year)
    print("generated %d + %d ratings in time order, %d users, %d movie rows in %.1f s" % (a.ratings, extra, n_users, n_movies, time.perf_counter() - t0), flush=True)
    dev = {k: torch.from_numpy(v[order]).cuda() for k, v in ratings.items()}
    cut = lambda lo, hi: {k: v[lo:hi] for k, v in dev.items()}
    base = cut(0, a.ratings)
    rebuild = lambda cols: FS.FeatureStore.from_ratings(cols, table, 5, n_users=n_users, n_movies=n_movies)
    def incremental(cols):
        store = FS.FeatureStore.empty(table, n_users, n_movies, 5)
        store.update(cols)
        return store
    store, built = incremental(base), rebuild(base)             # warm
    result = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "ratings": a.ratings, "users": n_users, "movie_rows": n_movies,
              "state_bytes": store._state.state_bytes(), "table_bytes": store.table_bytes(), "build_equals_rebuild": bool(same(store, built))}
    del built
    t_inc, t_reb = [], []
    for _ in range(a.repeats):
        t, s = wall(lambda: incremental(base)); t_inc.append(t); del s
        t, s = wall(lambda: rebuild(base)); t_reb.append(t); del s
    result["build"] = {"empty_plus_update_ms": stats(t_inc), "from_ratings_ms": stats(t_reb)}
    print("build", json.dumps(result), flush=True)
    at = a.ratings
    result["update"] = []
    for size in BATCHES:
        t_up, t_reb, equal = [], [], None
        for r in range(a.repeats):
            t, _ = wall(lambda: store.update(cut(at, at + size)))
            t_up.append(t)
            at += size
            if r == 0:                                          # everything applied so far, rebuilt
                whole = {k: v[:at].clone() for k, v in dev.items()}
                rebuilt = rebuild(whole)
                equal = bool(same(store, rebuilt))
                del rebuilt
                t_reb = [wall(lambda: rebuild(whole))[0] for _ in range(a.repeats)]
                del whole
        row = {"batch": size, "update_ms": stats(t_up), "rebuild_ms": stats(t_reb), "rebuild_over_update": round(statistics.median(t_reb) / statistics.median(t_up), 1),
               "update_equals_rebuild": equal}
        result["update"].append(row)
        print("update", json.dumps(row), flush=True)
    assert result["build_equals_rebuild"] and all(r["update_equals_rebuild"] for r in result["update"]), "the updated store differs from the rebuilt one"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
