"""ratings + movies.csv -> the movie catalogue -> similar movies for every movie, two routes over the same inputs:

  device   catalog.build(...) from device-resident rating columns (sprk_catalog_build: count, scan, and for input that is not grouped by
           movie scatter + per-movie sort by input row, then the recurrence of the average and the 2 (G + 1) sorted lists), one host
           synchronisation at the end; Catalog.similar_device(...) (sprk_catalog_similar, one workgroup per query)
  host     catalog.catalog_host(...) and catalog.similar_host(...), the definition, in numpy

on synthetic ratings shaped like MovieLens-20M (scripts/feature_eng_rate.py's generator: 26 744 movies with a Zipf-like popularity, one to
four of 20 genres each), fully shuffled, at --ratings rows (default 1 M and 20 M).  At each size the device bytes are compared with the
host's before anything is reported.  Device timings: warmed, --repeats runs, each between two events on the stream and under a host
clock that ends in a synchronise; median / min / max.  `shuffled` is the input as generated; `grouped` the same ratings stably sorted by
movie, which skips the scatter and the sort.  The recurrence's floor: the most-rated movie's count times the time per step of a lone
dependent multiply / add / divide chain, measured as the difference of two builds of ONE movie of --chain and of 2 x --chain ratings
(grouped input) divided by --chain; that difference also holds the count kernel's --chain atomics on one address, so it is an upper
estimate, and k_cat_avg_wave's own two durations in a kernel trace of --chain-only give the step alone.  Then the default similar movies
of EVERY movie, modes 0 and 1, and of one movie alone (the request latency).  The figures are recorded, not judged.  Needs a HIP device.

    python scripts/catalog_rate.py [--repeats 5] [--out docs/catalog_rate.json] [--md TABLES.md]     # docs/catalog_results.md's tables
    rocprofv3 --kernel-trace --stats -d DIR -o cat -- python scripts/catalog_rate.py --once --ratings 20000000
                                                   # the per-kernel times: builds shuffled (warm), grouped, shuffled; then mode 0, mode 1
    rocprofv3 --kernel-trace --stats -d DIR -o chain -- python scripts/catalog_rate.py --chain-only
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


def synth_catalog(n_ratings, n_users):
    """feature_eng_rate.synth's ratings with the movie columns it draws (the same generator state): -> ratings, movies columns."""
    import feature_eng_rate as FR
    from sparrowrecsys_amd import featureeng as FE
    kept = {}
    real = FE.movie_table
    FE.movie_table = lambda movies: kept.setdefault("movies", movies)          # (the generator ends in movie_table(columns): keep the columns)
    try:
        ratings, _, _ = FR.synth(n_ratings, n_users)
    finally:
        FE.movie_table = real
    return {"movieId": ratings["movieId"], "rating": ratings["rating"]}, kept["movies"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ratings", type=int, nargs="+", default=[1_000_000, 20_000_000])
    ap.add_argument("--size", type=int, default=10)
    ap.add_argument("--chain", type=int, default=50_000)
    ap.add_argument("--once", action="store_true", help="the first size only: build shuffled, grouped, shuffled, similar in both modes, exit (for a kernel trace)")
    ap.add_argument("--chain-only", action="store_true", help="the two one-movie builds only, then exit (under a kernel trace: k_cat_avg_wave's two durations)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("catalog_rate.py needs a HIP device")
    from sparrowrecsys_amd import catalog as CT

    ms = lambda v: round(v * 1e3, 3)
    stats = lambda ts: {"median": ms(statistics.median(ts)), "min": ms(min(ts)), "max": ms(max(ts))}

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

    def both(fn):
        ts = [timed(fn)[:2] for _ in range(a.repeats)]
        return {"host_clock": stats([t[0] for t in ts]), "events": stats([t[1] for t in ts])}

    assert a.repeats >= 5 or a.once or a.chain_only
    result = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "size": a.size,
              "sort_cap": int(os.environ.get("SPRK_FE_SORT_CAP", 4096)), "runs": []}

    # the time per step of a lone chain: one movie, grouped input, two lengths
    one = {"movieId": [1], "title": ["One (1999)"], "genres": ["Drama"]}
    chain = {}
    for n in (a.chain, 2 * a.chain):
        cols = {"movieId": torch.ones(n, dtype=torch.int64, device="cuda"), "rating": torch.full((n,), 3.5, device="cuda")}
        CT.build(cols, one)
        chain[n] = statistics.median(timed(lambda: CT.build(cols, one))[1] for _ in range(max(a.repeats, 5)))
    step_ns = (chain[2 * a.chain] - chain[a.chain]) / a.chain * 1e9
    result["chain"] = {"ratings": [a.chain, 2 * a.chain], "build_ms": [ms(chain[a.chain]), ms(chain[2 * a.chain])], "ns_per_step": round(step_ns, 2)}
    print("chain", json.dumps(result["chain"]), flush=True)
    if a.chain_only:
        return

    for n in a.ratings:
        n_users = max(4, round(138_493 * n / 20_000_000))
        t0 = time.perf_counter()
        ratings, movies = synth_catalog(n, n_users)
        table = CT.catalog_table(movies)
        held = np.flatnonzero(table.has)
        per_movie = np.bincount(ratings["movieId"], minlength=len(table.has))
        print("generated %d ratings over %d movies (most-rated %d, median %d) in %.1f s"
              % (n, len(held), per_movie.max(), int(np.median(per_movie[held])), time.perf_counter() - t0), flush=True)
        cols = {k: torch.from_numpy(v).cuda() for k, v in ratings.items()}
        by_movie = np.argsort(ratings["movieId"], kind="stable")
        cols_grouped = {k: torch.from_numpy(v[by_movie]).cuda() for k, v in ratings.items()}
        build = lambda c: CT.build(c, table)
        cat = build(cols)                                     # warm
        build(cols_grouped)
        queries = cat._queries(held)
        similar = lambda q, mode: cat.similar_device(q, mode, CT._heads(None, mode), 100, 1, a.size, a.size)
        if a.once:
            build(cols)
            for mode in (0, 1):
                similar(queries, mode)
            torch.cuda.synchronize()
            print("once: %d movies held" % len(held))
            return
        run = {"ratings": n, "movies": len(held), "genres": len(table.dictionary), "most_rated": int(per_movie.max()), "list_entries": CT.list_total(table)}
        for name, c in (("shuffled", cols), ("grouped", cols_grouped)):
            run["device_%s_ms" % name] = both(lambda: build(c))
        run["device_ratings_per_sec"] = round(n / (run["device_shuffled_ms"]["host_clock"]["median"] / 1e3))
        run["chain_floor_ms"] = round(int(per_movie.max()) * step_ns / 1e6, 3)
        t0 = time.perf_counter()
        want = CT.catalog_host(ratings, table)
        t_host = time.perf_counter() - t0
        same = all(np.asarray(g[k]).tobytes() == np.asarray(want[k]).tobytes() for g in (cat.to_host(), build(cols_grouped).to_host()) for k in CT.HOST_KEYS)
        run.update({"host_ms": ms(t_host), "host_ratings_per_sec": round(n / t_host), "device_equals_host": bool(same)})
        for mode in (0, 1):
            similar(queries, mode)                            # warm
            run["similar_all_mode%d_ms" % mode] = both(lambda: similar(queries, mode))
            t0 = time.perf_counter()
            host = CT.similar_host(want, held, size=a.size, mode=mode)
            run["similar_all_mode%d_host_ms" % mode] = ms(time.perf_counter() - t0)
            ids, scores, counts = similar(queries, mode)
            ok = all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip((ids, scores, counts), host))
            run["similar_mode%d_equals_host" % mode] = bool(ok)
            same = same and ok
            run["similar_one_mode%d_ms" % mode] = both(lambda: similar(queries[:1], mode))
        run["similar_movies_call_one_ms"] = stats([timed(lambda: cat.similar_movies([int(held[0])], a.size))[0] for _ in range(a.repeats)])
        print("run", json.dumps(run), flush=True)
        assert same, "the device result differs from the host definition"
        result["runs"].append(run)
        del cols, cols_grouped, cat
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print("wrote", a.out)
    if a.md:
        f3 = lambda d: "%.2f ms (%.2f – %.2f)" % (d["host_clock"]["median"], d["host_clock"]["min"], d["host_clock"]["max"])
        lines = ["<!-- the tables below are written by scripts/catalog_rate.py --md; the text around them is in docs/catalog_results.md -->", "",
                 "Device: %s, HIP %s; %d runs each, median (minimum – maximum) under a host clock that ends in a synchronise." % (result["device"], result["hip"], a.repeats), "",
                 "| ratings | movies | most-rated | input | device build | ratings / s | host definition | bytes equal |", "|---|---|---|---|---|---|---|---|"]
        for r in result["runs"]:
            for name in ("shuffled", "grouped"):
                d = r["device_%s_ms" % name]
                lines.append("| %d | %d | %d | %s | %s | %.0f M | %s | %s |" % (r["ratings"], r["movies"], r["most_rated"], name, f3(d), r["ratings"] / d["host_clock"]["median"] / 1e3,
                                                                               "%.0f ms" % r["host_ms"] if name == "shuffled" else "", "yes" if r["device_equals_host"] else "NO"))
        lines += ["", "Lone chain: %.2f ns per step (one movie of %d and of %d ratings: %.3f and %.3f ms between events)."
                  % (result["chain"]["ns_per_step"], a.chain, 2 * a.chain, result["chain"]["build_ms"][0], result["chain"]["build_ms"][1]), "",
                  "| ratings | most-rated movie | its chain's floor |", "|---|---|---|"]
        lines += ["| %d | %d | %.3f ms |" % (r["ratings"], r["most_rated"], r["chain_floor_ms"]) for r in result["runs"]]
        lines += ["", "| ratings | queries | mode | similar movies of every movie | queries / s | host definition | bytes equal | one query (events) | one query (host clock) |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in result["runs"]:
            for mode in (0, 1):
                d, o = r["similar_all_mode%d_ms" % mode], r["similar_one_mode%d_ms" % mode]
                lines.append("| %d | %d | %d | %s | %.2f M | %.0f ms | %s | %.3f ms | %.3f ms |" % (r["ratings"], r["movies"], mode, f3(d), r["movies"] / d["host_clock"]["median"] / 1e3,
                                                                                               r["similar_all_mode%d_host_ms" % mode], "yes" if r["similar_mode%d_equals_host" % mode] else "NO",
                                                                                               o["events"]["median"], o["host_clock"]["median"]))
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", a.md)


if __name__ == "__main__":
    main()
