"""ratings -> samples + feature store, two routes over the same ratings:

  device   featureeng.build(...) from device-resident rating columns (sprk_feature_eng: histogram, scan, scatter, per-user sort,
           movie aggregates, windows, store rows), one host synchronisation at the end
  host     featureeng.samples_host(...) + featurestore.row_images_from_samples(...), the definition, in numpy

on synthetic ratings shaped like MovieLens-20M: --ratings rows (default 20 M) of --users users (138 493) with a long-tailed length
distribution, at least 20 each, one user of 10 000; 26 744 movies with ids up to 131 262 and a Zipf-like popularity; half-star ratings;
timestamps over twenty years.  The device route runs on the whole set; the host route on the ratings of the first users that make up
--host-ratings rows (default 1 M: the whole set would take the host several minutes and tens of GB), where the device route runs as
well and the two results are compared byte for byte.  Device timings: synchronise, perf_counter around the call, warmed, median /
min / max of --repeats runs; they include the call's own allocations (outputs, workspace, store tables) and the upload of the movie
table.  The figures are recorded, not judged.  Needs a HIP device.

    python scripts/feature_eng_rate.py [--repeats 5] [--out docs/feature_eng_rate.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/feature_eng_rate.py --once      # the per-stage kernel times
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(n_ratings, n_users, seed=7):
    import numpy as np
    from sparrowrecsys_amd import featureeng as FE
    from sparrowrecsys_amd import schema as S
    rng = np.random.default_rng(seed)
    big = min(10_000, n_ratings // 4)
    raw = rng.lognormal(4.1, 1.2, n_users)
    lens = np.maximum(20, (raw * ((n_ratings - big) / raw.sum())).astype(np.int64))
    lens = np.minimum(lens, big - 1)
    lens[n_users // 2] = big
    while lens.sum() != n_ratings:                          # spread the remainder over random users, keeping the floor of 20
        diff = int(n_ratings - lens.sum())
        at = rng.integers(0, n_users, size=min(abs(diff), n_users))
        at = at[(at != n_users // 2) & ((diff > 0) | (lens[at] > 20))]
        np.add.at(lens, at, 1 if diff > 0 else -1)
        lens = np.maximum(lens, 20)
    n_movies_present, max_movie = 26_744, 131_262
    movie_ids = np.sort(rng.choice(max_movie, n_movies_present - 1, replace=False) + 1)
    movie_ids = np.unique(np.concatenate([movie_ids, [max_movie]]))
    pop = 1.0 / (np.arange(len(movie_ids)) + 10.0)
    order = rng.permutation(n_ratings)
    ratings = {
        "userId": np.repeat(np.arange(n_users, dtype=np.int64), lens)[order],
        "movieId": movie_ids[rng.choice(len(movie_ids), n_ratings, p=pop / pop.sum())][order],
        "rating": (rng.choice(np.arange(1, 11), n_ratings, p=[.012, .034, .014, .072, .044, .215, .110, .278, .077, .144]) / 2.0).astype(np.float32),
        "timestamp": rng.integers(789_652_009, 1_427_784_002, n_ratings),
    }
    names = S.GENRE_VOCAB + ["(no genres listed)"]
    movies = {"movieId": movie_ids.tolist(), "title": ["Movie %d (%d)" % (m, 1900 + m % 116) for m in movie_ids.tolist()],
              "genres": ["|".join(rng.choice(names, size=1 + int(k) % 4, replace=False)) for k in rng.integers(0, 4, len(movie_ids))]}
    return ratings, FE.movie_table(movies), lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ratings", type=int, default=20_000_000)
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--host-ratings", type=int, default=1_000_000)
    ap.add_argument("--once", action="store_true", help="generate, run the device build twice, exit (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("feature_eng_rate.py needs a HIP device")
    from sparrowrecsys_amd import featureeng as FE
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

    t0 = time.perf_counter()
    ratings, table, lens = synth(a.ratings, a.users)
    n_users, n_movies = a.users, len(table.year)
    print("generated %d ratings, %d users (longest %d, median %d), %d movie rows in %.1f s" % (a.ratings, n_users, lens.max(), int(np.median(lens)), n_movies,
                                                                                                time.perf_counter() - t0), flush=True)
    dev = {k: torch.from_numpy(v).cuda() for k, v in ratings.items()}
    device_build = lambda cols: FE.build(cols, table, 5, n_users=n_users, n_movies=n_movies)
    built = device_build(dev)                                # warm
    kept = built.n_samples
    assert kept == int(np.maximum(lens - 2, 0).sum())
    if a.once:
        del built
        device_build(dev)
        print("once: %d samples" % kept)
        return
    assert a.repeats >= 5
    del built
    t_dev = []
    for _ in range(a.repeats):
        t, built = wall(lambda: device_build(dev))
        t_dev.append(t)
        del built
    med = statistics.median(t_dev)
    result = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "ratings": a.ratings, "users": n_users, "movie_rows": n_movies,
              "longest_user": int(lens.max()), "samples": kept, "sort_cap": int(os.environ.get("SPRK_FE_SORT_CAP", 4096)),
              "device_build_ms": stats(t_dev), "device_ratings_per_sec": round(a.ratings / med)}
    print("device", json.dumps(result), flush=True)
    # the host definition, and the device against it, on the first users' ratings
    upto = int(np.searchsorted(np.cumsum(lens), a.host_ratings)) + 1
    sel = ratings["userId"] < upto
    sub = {k: v[sel] for k, v in ratings.items()}
    n_sub = int(sel.sum())
    t_host, host = wall(lambda: (lambda s: (s, FS.row_images_from_samples(s, 5, upto, n_movies)))(FE.samples_host(sub, table, 5)))
    sub_dev = {k: torch.from_numpy(v).cuda() for k, v in sub.items()}
    sub_build = lambda: FE.build(sub_dev, table, 5, n_users=upto, n_movies=n_movies)
    got = sub_build()
    cols = got.to_host()
    same = all(cols[k].tobytes() == host[0][k].tobytes() for k in host[0]) and all(
        t.cpu().numpy()[:-1].tobytes() == w.tobytes() for t, w in zip(got.store().tensors(), host[1][:4]))
    del got
    t_sub = [wall(sub_build)[0] for _ in range(a.repeats)]
    result["subset"] = {"ratings": n_sub, "users": upto, "samples": len(host[0]["userId"]), "host_ms": ms(t_host), "host_ratings_per_sec": round(n_sub / t_host),
                        "device_build_ms": stats(t_sub), "device_ratings_per_sec": round(n_sub / statistics.median(t_sub)), "device_equals_host": bool(same)}
    print("subset", json.dumps(result["subset"]), flush=True)
    assert same, "the device result differs from the host definition"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
