"""Embedding LSH on the device (sparrowrecsys_amd/lsh.py, sprk_lsh_hash / sprk_lsh_build / sprk_lsh_query), measured and written to
docs/lsh_results.md:

  build           LSHIndex.build (hash + index) at 26 744 x 10 and at 2^22 x 64, the reference's settings (bucket_length 0.1, 3 tables)
  approx_nearest  1, 1 024 and 26 744 queries (rows of the table) at K = 10 on the 26 744-row table, next to
                    EmbRanker.topk on the same table and queries: the exact search.  It ranks by COSINE, so this is a comparison of
                                    times only;
                    approx_nearest_host, the definition in numpy (1 and 1 024 queries)
                  and 1 and 1 024 queries on the 2^22-row table, device only
  candidates      the median / least / greatest candidate count of the queries
  recall          the share of the exact Euclidean top 10 (brute force on the host, 1 024 queries) that the approximate top 10 holds

Tables are unit-normal float32 rows times --scale (default 0.4 at D = 10, as tests/test_gpu_lsh.py's movie table; 1.0 at D = 64).  Device
timings: warmed, --repeats runs, each under a host clock that ends in a synchronise; the median.  The device result is compared with the
host definition byte for byte where both are computed.  The figures are recorded, not judged.  Needs a HIP device.

    python scripts/lsh_rate.py [--repeats 5] [--out docs/lsh_results.md]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "docs", "lsh_results.md"))
    ap.add_argument("--scale", type=float, default=0.4)
    ap.add_argument("--large-log2", type=int, default=22)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("lsh_rate.py needs a HIP device")
    from sparrowrecsys_amd import lsh
    from sparrowrecsys_amd import ranker as R

    def timed(fn):
        ts = []
        for _ in range(a.repeats + 1):                      # the first run warms
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[1:]) * 1e3, out

    K, LENGTH, T = 10, 0.1, 3
    lines = ["# Embedding LSH on the device: measurements", "",
             "Written by `scripts/lsh_rate.py` on %s (HIP %s), %d runs after a warm-up, the median, host clock around the call and a synchronise."
             % (torch.cuda.get_device_name(0), torch.version.hip, a.repeats),
             "Settings: `bucket_length %.1f`, `%d` hash tables, `K = %d` (Embedding.embeddingLSH's configuration).  Nothing here is a bar; the figures are recorded." % (LENGTH, T, K), ""]

    # ---- the catalogue-sized table ----
    n, D = 26_744, 10
    emb = (np.random.default_rng(0).standard_normal((n, D)) * a.scale).astype(np.float32)
    ranker = R.EmbRanker({i: emb[i] for i in range(n)})
    build_ms, index = timed(lambda: lsh.LSHIndex.build(ranker.table, ranker.has, bucket_length=LENGTH, num_hash_tables=T))
    lines += ["## %d x %d (unit-normal rows x %.1f)" % (n, D, a.scale), "", "`LSHIndex.build`: %.3f ms" % build_ms, "",
              "| queries | `approx_nearest` ms | `EmbRanker.topk` ms (exact, cosine) | `approx_nearest_host` ms | device = host |", "|---|---|---|---|---|"]
    slower = []
    for Q in (1, 1024, n):
        q = ranker.table[:Q]
        dev_ms, got = timed(lambda: index.approx_nearest(q, K))
        exact_ms, _ = timed(lambda: ranker.topk(q, K))
        host_ms, same = None, None
        if Q <= 1024:
            t0 = time.perf_counter()
            want = lsh.approx_nearest_host(emb, None, index.vectors, LENGTH, emb[:Q], K)
            host_ms = (time.perf_counter() - t0) * 1e3
            same = all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip(got, want))
            assert same, "the device result differs from the host definition"
        if dev_ms >= exact_ms:
            slower.append(Q)
        lines.append("| %d | %.3f | %.3f | %s | %s |" % (Q, dev_ms, exact_ms, "%.1f" % host_ms if host_ms is not None else "not run", {None: "not compared", True: "yes"}[same]))
        print(lines[-1], flush=True)
    count = got[2].cpu().numpy()
    lines += ["", "Candidates per query (all %d rows as queries): median %d, least %d, greatest %d." % (n, int(np.median(count)), count.min(), count.max())]
    # recall of the approximate top 10 against the exact Euclidean top 10, the first 1024 rows as queries
    rows = got[1].cpu().numpy()[:1024]
    x = emb.astype(np.float64)
    hit = 0
    for qi in range(1024):
        d = ((x - x[qi]) ** 2).sum(axis=1)
        exact = np.lexsort((np.arange(n), d))[:K]
        hit += len(set(exact.tolist()) & set(rows[qi].tolist()))
    lines += ["Recall of the approximate top %d against the exact Euclidean top %d (host brute force, 1 024 queries): %.3f." % (K, K, hit / (1024.0 * K)), ""]
    if slower:
        lines += ["At this table the device query is NOT faster than the exact scan at a query count of %s: the exact search reads 1 MB of rows for a query,"
                  " the index walks three bucket ranges and sorts its candidates.  The index is for large tables." % ", ".join(str(s) for s in slower), ""]
    else:
        lines += ["At this table the device query is faster than the exact scan at every query count measured.", ""]
    del ranker, index

    # ---- the large table: build, and the query against the exact scan ----
    n, D = 1 << a.large_log2, 64
    emb = np.random.default_rng(1).standard_normal((n, D), dtype=np.float32)
    table = torch.from_numpy(emb).cuda()
    build_ms, index = timed(lambda: lsh.LSHIndex.build(table, bucket_length=LENGTH, num_hash_tables=T))
    hash_ms, _ = timed(lambda: lsh.LSHIndex.build(table[:1], bucket_length=LENGTH, num_hash_tables=T))
    lines += ["## 2^%d x %d (unit-normal rows)" % (a.large_log2, D), "", "`LSHIndex.build`: %.3f ms (a one-row build, the call's fixed cost: %.3f ms)" % (build_ms, hash_ms), "",
              "| queries | `approx_nearest` ms | candidates: median | least | greatest |", "|---|---|---|---|---|"]
    for Q in (1, 1024):
        dev_ms, got = timed(lambda: index.approx_nearest(table[:Q], K))
        count = got[2].cpu().numpy()
        lines.append("| %d | %.3f | %d | %d | %d |" % (Q, dev_ms, int(np.median(count)), count.min(), count.max()))
        print(lines[-1], flush=True)
    lines += ["", "The exact search reads all %.1f GB of this table for every query; the index reads the rows of the query's three buckets -- with unit-normal"
              " rows and `bucket_length 0.1` about 4 %% of the table each near the centre, so the candidate counts above are large: a table of this size wants a"
              " bucket length chosen for it." % (n * D * 4 / 1e9), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
