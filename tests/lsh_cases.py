"""Inputs that tests/test_lsh.py (CPU) and tests/test_gpu_lsh.py share: the hand-worked example, the synthetic tables, the edge rows,
and a brute force over Python floats that is independent of lsh.py's numpy."""
import math

import numpy as np

from sparrowrecsys_amd import lsh

NO = lsh.NO_BUCKET

# ---- the hand-worked example: D = 2, T = 2, axis-aligned vectors, bucket_length 1.0, six rows ----
HAND_VECTORS = np.array([[1.0, 0.0], [0.0, 1.0]])
HAND_LENGTH = 1.0
HAND_EMB = np.array([[0.5, 0.5], [0.25, 1.5], [1.5, 0.75], [-0.5, 0.25], [0.75, 0.25], [2.5, 2.5]], dtype=np.float32)
HAND_BUCKETS = [[0, 0], [0, 1], [1, 0], [-1, 0], [0, 0], [2, 2]]
# query (0.5, 0.25) has buckets (0, 0): table 0 gives rows 0, 1, 4, table 1 rows 0, 2, 3, 4 -- five candidates, rows 0 and 4 tie at 0.25 and
# go by row; query (2.75, -0.5) has buckets (2, -1): table 0 gives row 5, table 1 nothing; query (9, 9) shares no bucket
HAND_QUERIES = np.array([[0.5, 0.25], [2.75, -0.5], [9.0, 9.0]], dtype=np.float32)
HAND_K = 3
HAND_ROWS = [[0, 4, 3], [5, -1, -1], [-1, -1, -1]]
HAND_DIST = [[0.25, 0.25, 1.0], [math.sqrt(0.0625 + 9.0), math.nan, math.nan], [math.nan] * 3]
HAND_COUNT = [5, 1, 0]
HAND_ALL_ROWS_QUERY0 = [0, 4, 3, 2, 1]                       # every candidate of query 0, in order: 0.25, 0.25, 1, sqrt(1.25), sqrt(1.625)


def table(n, D, seed=0, scale=1.0):
    """Unit-normal float32 rows (times `scale`) from default_rng(seed)."""
    return (np.random.default_rng(seed).standard_normal((n, D)) * scale).astype(np.float32)


def edge_rows():
    """D = 2 rows for vectors e_0, e_1 and bucket_length 0.25 -> (emb, has, the buckets sprk_lsh_hash gives).  Bucket edges (0.5 -> 2,
    -0.5 -> -2, -0.0 -> 0), the clamp on both sides and the largest unclamped power of two, subnormals, non-finite coordinates
    (NO_BUCKET in EVERY table: inf * 0 is NaN), a row without an embedding."""
    inf, nan = np.inf, np.nan
    rows = [([0.5, -0.5], 1, [2, -2]), ([-0.0, 0.0], 1, [0, 0]), ([0.2499, -0.2501], 1, [0, -2]),
            ([1e30, -1e30], 1, [1 << 62, -(1 << 62)]), ([2.0 ** 59, -2.0 ** 59], 1, [1 << 61, -(1 << 61)]), ([2.0 ** 60, -2.0 ** 61], 1, [1 << 62, -(1 << 62)]),
            ([1e-40, -1e-40], 1, [0, -1]), ([1.5e-45, 0.75], 1, [0, 3]),
            ([inf, 1.0], 1, [NO, NO]), ([1.0, -inf], 1, [NO, NO]), ([nan, 0.5], 1, [NO, NO]), ([3.4e38, 3.4e38], 1, [1 << 62, 1 << 62]),
            ([0.5, -0.5], 0, [NO, NO]), ([0.6, -0.4], 1, [2, -2]), ([0.5, 0.75], 1, [2, 3])]
    emb = np.array([r[0] for r in rows], dtype=np.float32)
    return emb, np.array([r[1] for r in rows], dtype=np.uint8), np.array([r[2] for r in rows], dtype=np.int64)


EDGE_VECTORS = np.array([[1.0, 0.0], [0.0, 1.0]])
EDGE_LENGTH = 0.25


def loop_hash(emb, vectors, bucket_length):
    """hash_host over Python floats, one operation at a time."""
    out = []
    for x in np.asarray(emb, dtype=np.float32).tolist():
        line = []
        for r in np.asarray(vectors, dtype=np.float64).tolist():
            dot = 0.0
            for a, b in zip(x, r):
                dot = dot + a * b
            if not math.isfinite(dot):
                line.append(NO)
                continue
            q = dot / bucket_length
            line.append(max(-(1 << 62), min(1 << 62, math.floor(q))) if math.isfinite(q) else (1 << 62 if q > 0 else -(1 << 62)))
        out.append(line)
    return np.array(out, dtype=np.int64).reshape(len(out), len(vectors))


def brute_force(emb, has, vectors, bucket_length, queries, k, query_has=None):
    """approx_nearest_host by sets: a dict bucket -> set of rows per table, the union over the tables, Python's sorted on (dist, row)."""
    emb, queries = np.asarray(emb, dtype=np.float32), np.asarray(queries, dtype=np.float32)
    b, qb = loop_hash(emb, vectors, bucket_length), loop_hash(queries, vectors, bucket_length)
    T = len(vectors)
    tables = [{} for _ in range(T)]
    for i in range(len(emb)):
        if has is not None and not has[i]:
            continue
        for t in range(T):
            if b[i, t] != NO:
                tables[t].setdefault(int(b[i, t]), set()).add(i)
    x, y = emb.tolist(), queries.tolist()
    dist, rows, count = [], [], []
    for q in range(len(queries)):
        cand = set()
        if query_has is None or query_has[q]:
            for t in range(T):
                if qb[q, t] != NO:
                    cand |= tables[t].get(int(qb[q, t]), set())
        scored = []
        for i in cand:
            s = 0.0
            for a, c in zip(x[i], y[q]):
                d = a - c
                s = s + d * d
            scored.append((math.sqrt(s), i))
        scored = sorted(scored)[:k]
        dist.append([d for d, _ in scored] + [math.nan] * (k - len(scored)))
        rows.append([i for _, i in scored] + [-1] * (k - len(scored)))
        count.append(len(cand))
    return (np.array(dist, dtype=np.float64).reshape(len(queries), k), np.array(rows, dtype=np.int32).reshape(len(queries), k), np.array(count, dtype=np.int32))


def same(got, want):
    """(dist, rows, count) byte for byte: the NaN padding is 0x7ff8000000000000 on both sides."""
    for g, w, name in zip(got, want, ("dist", "rows", "count")):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, np.flatnonzero((g.reshape(len(g), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(axis=1))[:8])
