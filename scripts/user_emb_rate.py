"""ratings + item embeddings -> user embeddings -> recommendations, two routes over the same ratings:

  device   userembedding.build(...) from device-resident rating columns (sprk_user_emb: count, scan, and for input that is not grouped
           by user scatter + per-user sort by input row, then the ordered float32 sum), one host synchronisation at the end
  host     userembedding.user_emb_host(...), the definition, in numpy (np.add.at)

on synthetic ratings shaped like MovieLens-20M (scripts/feature_eng_rate.py's generator: a long-tailed length distribution, one user
of 10 000, 26 744 movies with a Zipf-like popularity), fully shuffled, at --ratings rows (default 1 M and 20 M; users in proportion,
138 493 at 20 M) with item embeddings of D = 10 for every movie.  At each size the device result is compared with the host's byte for
byte.  Device timings: warmed, --repeats runs, each between two events on the stream and under a host clock that ends in a synchronise;
median / min / max.  `shuffled` is the input as generated; `grouped` the same ratings sorted by user, which skips the scatter and the
sort, so the difference of the two is what those cost and `grouped` is count + scan + sum.  Then recommend() for ALL users at
size = 10.  The figures are recorded, not judged.  Needs a HIP device.

    python scripts/user_emb_rate.py [--repeats 5] [--out docs/user_emb_rate.json]
    rocprofv3 --kernel-trace --stats -d DIR -o ue -- python scripts/user_emb_rate.py --once --ratings 20000000
                                                   # the per-kernel times: three builds, shuffled (warm), grouped, shuffled
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ratings", type=int, nargs="+", default=[1_000_000, 20_000_000])
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--size", type=int, default=10)
    ap.add_argument("--once", action="store_true", help="the first size only: generate, build shuffled, grouped, shuffled, exit (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("user_emb_rate.py needs a HIP device")
    from feature_eng_rate import synth
    from sparrowrecsys_amd import ranker as R
    from sparrowrecsys_amd import userembedding as UE

    def ms(v):
        return round(v * 1e3, 3)

    def stats(ts):
        return {"median": ms(statistics.median(ts)), "min": ms(min(ts)), "max": ms(max(ts))}

    def timed(fn):
        """-> (host seconds around fn + synchronise, seconds between two events on the stream, fn's result)"""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        out = fn()
        stop.record()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, start.elapsed_time(stop) / 1e3, out

    assert a.repeats >= 5 or a.once
    result = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "D": a.dim, "size": a.size,
              "sort_cap": int(os.environ.get("SPRK_FE_SORT_CAP", 4096)), "runs": []}
    for n in a.ratings:
        n_users = max(4, round(138_493 * n / 20_000_000))
        t0 = time.perf_counter()
        ratings, table, lens = synth(n, n_users)
        movie_ids = np.flatnonzero(table.has)
        rng = np.random.default_rng(11)
        item_emb = rng.standard_normal((len(movie_ids), a.dim)).astype(np.float32)
        ranker = R.EmbRanker({int(m): item_emb[i] for i, m in enumerate(movie_ids)})
        print("generated %d ratings, %d users (longest %d, median %d), %d movies with an embedding of D = %d in %.1f s"
              % (n, n_users, lens.max(), int(np.median(lens)), len(movie_ids), a.dim, time.perf_counter() - t0), flush=True)
        cols = {k: torch.from_numpy(ratings[k]).cuda() for k in ("userId", "movieId")}
        by_user = np.argsort(ratings["userId"], kind="stable")
        cols_grouped = {k: torch.from_numpy(ratings[k][by_user]).cuda() for k in ("userId", "movieId")}
        build = lambda c: UE.build(c, ranker, n_users=n_users)
        built = build(cols)                                   # warm
        build(cols_grouped)
        if a.once:
            build(cols)
            print("once: %d users with an embedding" % int(built.has.sum()))
            return
        run = {"ratings": n, "users": n_users, "longest_user": int(lens.max()), "movies": len(movie_ids)}
        for name, c in (("shuffled", cols), ("grouped", cols_grouped)):
            ts = [timed(lambda: build(c))[:2] for _ in range(a.repeats)]
            run["device_%s_ms" % name] = {"host_clock": stats([t[0] for t in ts]), "events": stats([t[1] for t in ts])}
        run["device_ratings_per_sec"] = round(n / (run["device_shuffled_ms"]["host_clock"]["median"] / 1e3))
        # the host definition on the same columns, and the device against it
        rows = ranker.rows(movie_ids)
        lut = np.full(int(movie_ids.max()) + 1, -1, dtype=np.int32)
        lut[movie_ids] = rows
        emb_host, has_host = ranker.table.cpu().numpy(), ranker.has.cpu().numpy()
        t0 = time.perf_counter()
        want = UE.user_emb_host(ratings["userId"], lut[ratings["movieId"]], emb_host, has_host, n_users)
        t_host = time.perf_counter() - t0
        same = all(g.tobytes() == w.tobytes() for g, w in zip(built.to_host(), want))
        same_grouped = all(g.tobytes() == w.tobytes() for g, w in zip(build(cols_grouped).to_host(), want))
        run.update({"host_ms": ms(t_host), "host_ratings_per_sec": round(n / t_host), "device_equals_host": bool(same and same_grouped)})
        users = np.arange(n_users)
        built.recommend(ranker, users[:1024], a.size)         # warm
        ts = [timed(lambda: built.recommend(ranker, users, a.size))[0] for _ in range(a.repeats)]
        run["recommend_all_users_ms"] = stats(ts)
        run["recommend_users_per_sec"] = round(n_users / statistics.median(ts))
        print("run", json.dumps(run), flush=True)
        assert same and same_grouped, "the device result differs from the host definition"
        result["runs"].append(run)
        del cols, cols_grouped, built
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
