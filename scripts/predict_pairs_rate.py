"""(userId, movieId) pairs on the host -> scores on the host, two routes over the same feature store and the same pairs:

  join   model.predict_pairs(store, users, movies): the ids go to the device, sprk_join_features assembles the packed rows there
  host   what there was before the store: numpy fancy-indexing of host copies of the store's columns into a typed feature dict
         (int32 ids and genre indices, float32 numerics), then model.predict(dict) -- the native column packer and the forward

for DeepFMv2, DIN and EmbeddingMLP at B = 800 (one user x 800 candidates, the Jetty request) and B = 65 536 (random pairs), plus

  recommend   model.recommend(store, 64 users, [64, 800] candidates, 10)   against   predict_pairs + a stable host argsort per user

Both routes of a case run in one process, alternating, warmed; median, min and max of --repeats runs each (timed as
scripts/predict_dict_rate.py times: synchronise, perf_counter around the call that ends in the device -> host copy).  The figures are
recorded, not judged: nothing is asserted about which route is faster.  Needs a HIP device.

    python scripts/predict_pairs_rate.py [--repeats 12] [--out profiles/r09/predict_pairs_rate.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "predict_pairs_rate.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("predict_pairs_rate.py needs a HIP device")
    from sparrowrecsys_amd import models as M
    from sparrowrecsys_amd.featurestore import FeatureStore
    assert a.repeats >= 10
    store = FeatureStore.from_samples(os.path.join(ROOT, "tests", "golden", "test_samples_512.csv"))
    im = store.images
    users, movies = np.flatnonzero(im.user_has), np.flatnonzero(im.movie_has)
    # host copies of the store's columns, one contiguous typed array each
    host_cols = {}
    for rows, layout in ((im.user_rows, store.user_layout), (im.movie_rows, store.movie_layout)):
        for k, (off, role) in layout.items():
            col = np.ascontiguousarray(rows[:, off])
            host_cols[k] = (col.view(np.float32) if role == "dense" else col, rows is im.user_rows)

    def host_route(model, keys, u, m):
        d = {"userId": u, "movieId": m}
        for k in keys:
            col, of_user = host_cols[k]
            d[k] = col[u if of_user else m]
        return model.predict(d)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def compare(name, rows, new, old, same):
        for _ in range(3):                                           # warm both routes: engine, staging buffers, allocator
            r_new, r_old = new(), old()
        assert same(r_new, r_old), name
        t_new, t_old = [], []
        for _ in range(a.repeats):                                   # alternating
            t_new.append(timed(new)[0])
            t_old.append(timed(old)[0])
        ms = lambda v: round(v * 1e3, 4)                             # noqa: E731
        med_new, med_old = statistics.median(t_new), statistics.median(t_old)
        res = {"rows": rows,
               "join_ms": {"median": ms(med_new), "min": ms(min(t_new)), "max": ms(max(t_new))},
               "host_ms": {"median": ms(med_old), "min": ms(min(t_old)), "max": ms(max(t_old))},
               "join_rows_per_sec": round(rows / med_new), "host_rows_per_sec": round(rows / med_old), "host_over_join": round(med_old / med_new, 2)}
        print(name, json.dumps(res), flush=True)
        return res

    result = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "store": {"users": int(users.size), "movies": int(movies.size),
              "table_bytes": store.table_bytes()}, "predict_pairs": {}, "recommend": {}}
    rng = np.random.default_rng(1)
    models = [("DeepFMv2", M.DeepFMv2(seed=1)), ("DIN", M.DIN(seed=1)), ("EmbeddingMLP", M.EmbeddingMLP(seed=1))]
    for name, model in models:
        keys = [c.key for c in model.id_columns if c.key not in ("userId", "movieId")] + list(model.numeric_keys)
        for B in (800, 65536):
            u = np.full(B, users[7], dtype=np.int64) if B == 800 else users[rng.integers(0, users.size, B)]
            m = movies[rng.integers(0, movies.size, B)]
            result["predict_pairs"]["%s/B=%d" % (name, B)] = compare(
                "%s/B=%d" % (name, B), B, lambda: model.predict_pairs(store, u, m), lambda: host_route(model, keys, u, m), np.array_equal)
    for name, model in models[:2]:
        Q, Cn, size = 64, 800, 10
        u = users[rng.integers(0, users.size, Q)]
        cand = movies[rng.integers(0, movies.size, (Q, Cn))]

        def host_sort():
            s = model.predict_pairs(store, np.repeat(u, Cn), cand.reshape(-1)).reshape(Q, Cn)
            order = np.argsort(-s, axis=1, kind="stable")[:, :size]
            return [cand[q][order[q]].tolist() for q in range(Q)]
        result["recommend"]["%s/64x800" % name] = compare("recommend/%s/64x800" % name, Q * Cn, lambda: model.recommend(store, u, cand, size), host_sort,
                                                        lambda x, y: x == y)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
