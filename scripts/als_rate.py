"""ratings -> ALS factors -> scores and a top 10 for every user, two routes over the same ratings:

  device   als.als_device(...) on device-resident rating columns (sprk_als_fit: count, scans, scatter into per-movie and per-user
           segments, the two sorts, then 2 x iters half-sweeps), als.predict_device and ALSModel.recommend_for_users
  host     als.als_host(...), the definition, in numpy

on synthetic ratings shaped like MovieLens-20M (scripts/feature_eng_rate.py's generator: a long-tailed length distribution, one user of
10 000, 26 744 movies with ids up to 131 262 and a Zipf-like popularity), fully shuffled, at --ratings rows (default 1 M and 20 M; users
in proportion, 138 493 at 20 M), rank 10, reg 0.01, 5 iterations.  At the sizes up to --host-full the host runs all iterations and the
six outputs are compared byte for byte (asserted); above, the host runs ONE iteration (said in the output) and the device's one-iteration
result is compared with it.  Device timings: warmed, --repeats runs, each under a host clock that starts after and ends in a
synchronise; median / min / max.  What is reported besides the whole fit:
  * the fit at iters = 0 (everything before the sweeps) and, by difference, one iteration = two half-sweeps;
  * one half-sweep alone: the fit at iters = 1 minus the fit at iters = 0 on the ratings of the most rated movie only -- there the movie
    half-sweep is ONE row's dependent chain and the user half-sweep rows of one rating --, which is the floor that row sets for every
    movie half-sweep of the full set, and its share of the full set's iteration;
  * predict at 2^20 random pairs; the top 10 for all users.
The figures are recorded, not judged.  Needs a HIP device.

    python scripts/als_rate.py [--repeats 5] [--out docs/als_rate.json] [--doc docs/als_results.md]
    rocprofv3 --kernel-trace --stats -d DIR -o als -- python scripts/als_rate.py --once --ratings 20000000     # the per-kernel times
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def fmt(s):
    return "%.2f ms (%.2f – %.2f)" % (s["median"], s["min"], s["max"])


def write_doc(path, result):
    lines = ["# ALS collaborative filtering: the device route against the host definition, measured", "",
             "Written by `python scripts/als_rate.py --repeats %d --doc %s` on %s; commit `%s`%s; device \"%s\", HIP runtime %s." % (
                 result["repeats"], os.path.relpath(path, ROOT), result["date"], result["commit"], " plus uncommitted changes" if result["dirty"] else "",
                 result["device"], result["hip"]),
             "Rank %d, reg %g, %d iterations; synthetic ratings shaped like MovieLens-20M (`scripts/feature_eng_rate.py`'s generator), shuffled." % (
                 result["rank"], result["reg"], result["iters"]),
             "Device times: warmed, %d runs, median (minimum – maximum) under a host clock that ends in a synchronise; the rating columns and the"
             % result["repeats"],
             "initial factors are already device tensors, the call's own allocations (outputs, workspace) are inside.", "",
             "## The fit", "",
             "| ratings | users | item rows | longest movie | device fit | ratings x iterations / s | before the sweeps (iters = 0) | one iteration | host definition | equal |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in result["runs"]:
        lines.append("| %d | %d | %d | %d | %s | %.0f M | %s | %.2f ms | %.1f s (%d iteration%s) | %s |" % (
            r["ratings"], r["users"], r["item_rows"], r["longest_movie"], fmt(r["fit_ms"]), r["ratings"] * result["iters"] / r["fit_ms"]["median"] / 1e3,
            fmt(r["fit_iters0_ms"]), r["iteration_ms"], r["host_s"], r["host_iters"], "" if r["host_iters"] == 1 else "s",
            "byte for byte" if r["device_equals_host"] else "NO"))
    lines += ["", "`one iteration` = (fit − fit at iters = 0) / iterations: a movie half-sweep and a user half-sweep.  Where the host ran one iteration only,",
              "the device's one-iteration result is what was compared.", "",
              "## The longest row's chain", "",
              "The fit on the ratings of the most rated movie ALONE, iters = 1 minus iters = 0: its movie half-sweep is one row, one dependent chain of",
              "chunks on one lane group, and no movie half-sweep of the full set can end sooner.", "",
              "| ratings | longest movie | its half-sweep alone | per rating of the chain | share of one full iteration |", "|---|---|---|---|---|"]
    for r in result["runs"]:
        lines.append("| %d | %d | %.2f ms | %.0f ns | %.0f %% |" % (r["ratings"], r["longest_movie"], r["longest_row_ms"], 1e6 * r["longest_row_ms"] / r["longest_movie"],
                                                                  100.0 * r["longest_row_ms"] / r["iteration_ms"]))
    lines += ["", "## Scores and recommendations", "",
              "| ratings | predict, 2^20 pairs | pairs / s | top 10 for all users | users / s |", "|---|---|---|---|---|"]
    for r in result["runs"]:
        lines.append("| %d | %s | %.0f M | %s | %.0f k |" % (r["ratings"], fmt(r["predict_ms"]), (1 << 20) / r["predict_ms"]["median"] / 1e3,
                                                             fmt(r["top10_ms"]), r["users_with_factors"] / r["top10_ms"]["median"]))
    lines += ["", "The top 10 runs over every row of the item table (row = movieId, so %d rows of which %d have factors)." % (
        result["runs"][-1]["item_rows"], result["runs"][-1]["movies"]), ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ratings", type=int, nargs="+", default=[1_000_000, 20_000_000])
    ap.add_argument("--rank", type=int, default=10)
    ap.add_argument("--reg", type=float, default=0.01)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-full", type=int, default=1_000_000, help="the host runs every iteration up to this many ratings, one iteration above")
    ap.add_argument("--once", action="store_true", help="the first size only: generate, fit twice, exit (for a kernel trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--doc", default=None)
    ap.add_argument("--commit", default=None, help="the commit to name in --doc where the tree is no git checkout")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("als_rate.py needs a HIP device")
    from feature_eng_rate import synth
    from sparrowrecsys_amd import als as A

    def ms(v):
        return round(v * 1e3, 3)

    def stats(ts):
        return {"median": ms(statistics.median(ts)), "min": ms(min(ts)), "max": ms(max(ts))}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def git(*args):
        try:
            return subprocess.run(["git", "-C", ROOT] + list(args), capture_output=True, text=True).stdout.strip()
        except OSError:
            return ""

    assert a.repeats >= 5 or a.once
    result = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "rank": a.rank, "reg": a.reg, "iters": a.iters,
              "commit": a.commit or git("rev-parse", "--short", "HEAD") or "unknown", "dirty": bool(git("status", "--porcelain", "--untracked-files=no")),
              "date": time.strftime("%Y-%m-%d"), "runs": []}
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    for n in a.ratings:
        n_users = max(4, round(138_493 * n / 20_000_000))
        t0 = time.perf_counter()
        ratings, _, lens = synth(n, n_users)
        n_items = int(ratings["movieId"].max()) + 1
        per_movie = np.bincount(ratings["movieId"], minlength=n_items)
        print("generated %d ratings, %d users (longest %d), %d movies in %d item rows (longest %d) in %.1f s"
              % (n, n_users, lens.max(), int((per_movie > 0).sum()), n_items, per_movie.max(), time.perf_counter() - t0), flush=True)
        u, m, r = up(ratings["userId"], np.int32), up(ratings["movieId"], np.int32), up(ratings["rating"], np.float32)
        init_host = A.init_factors(n_users, a.rank, 0)
        init = up(init_host, np.float32)
        fit = lambda iters: A.als_device(u, m, r, n_users, n_items, a.rank, a.reg, iters, init)
        out = fit(a.iters)                                     # warm
        assert int(out[6].cpu()[0]) == -1
        if a.once:
            fit(a.iters)
            torch.cuda.synchronize()
            print("once: %d users with factors" % int(out[2].sum()))
            return
        run = {"ratings": n, "users": n_users, "item_rows": n_items, "movies": int((per_movie > 0).sum()), "longest_movie": int(per_movie.max()),
               "longest_user": int(lens.max())}
        run["fit_ms"] = stats([timed(lambda: fit(a.iters))[0] for _ in range(a.repeats)])
        fit(0)
        run["fit_iters0_ms"] = stats([timed(lambda: fit(0))[0] for _ in range(a.repeats)])
        run["iteration_ms"] = round((run["fit_ms"]["median"] - run["fit_iters0_ms"]["median"]) / max(a.iters, 1), 3)
        # the most rated movie alone
        top = int(per_movie.argmax())
        only = np.flatnonzero(ratings["movieId"] == top)
        u1, m1, r1 = up(ratings["userId"][only], np.int32), up(ratings["movieId"][only], np.int32), up(ratings["rating"][only], np.float32)
        fit1 = lambda iters: A.als_device(u1, m1, r1, n_users, n_items, a.rank, a.reg, iters, init)
        fit1(1); fit1(0)
        t1 = statistics.median([timed(lambda: fit1(1))[0] for _ in range(a.repeats)])
        t0_ = statistics.median([timed(lambda: fit1(0))[0] for _ in range(a.repeats)])
        run["longest_row_ms"] = ms(t1 - t0_)
        print("device", json.dumps(run), flush=True)
        # the host definition
        host_iters = a.iters if n <= a.host_full else 1
        if host_iters != a.iters:
            print("the host definition runs ONE iteration at %d ratings; the device's one-iteration result is compared with it" % n, flush=True)
        t0 = time.perf_counter()
        want = A.als_host(ratings["userId"], ratings["movieId"], ratings["rating"], n_users, n_items, rank=a.rank, reg=a.reg, iters=host_iters, init_user=init_host)
        run["host_s"], run["host_iters"] = round(time.perf_counter() - t0, 2), host_iters
        got = out if host_iters == a.iters else fit(host_iters)
        same = all(np.ascontiguousarray(g.cpu().numpy()).tobytes() == w.tobytes() for g, w in zip(got[:6], want))
        run["device_equals_host"] = bool(same)
        print("host %.1f s for %d iteration(s); device equals host: %s" % (run["host_s"], host_iters, same), flush=True)
        # scores and recommendations, on the full fit
        model = A.ALSModel(*out[:6])
        rng = np.random.default_rng(5)
        pu, pm = up(rng.integers(0, n_users, 1 << 20), np.int32), up(ratings["movieId"][rng.integers(0, n, 1 << 20)], np.int32)
        predict = lambda: A.predict_device(pu, pm, model.user_factors, model.user_has, model.item_factors, model.item_has)
        predict()
        run["predict_ms"] = stats([timed(predict)[0] for _ in range(a.repeats)])
        run["users_with_factors"] = int(model.user_has.sum())
        model.recommend_for_users(list(range(min(n_users, 1024))), k=10)
        run["top10_ms"] = stats([timed(lambda: model.recommend_for_users(k=10))[0] for _ in range(a.repeats)])
        print("run", json.dumps(run), flush=True)
        assert same, "the device result differs from the host definition"
        result["runs"].append(run)
        del u, m, r, out, model, got
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print("wrote", a.out)
    if a.doc:
        write_doc(os.path.abspath(a.doc), result)
        print("wrote", a.doc)


if __name__ == "__main__":
    main()
