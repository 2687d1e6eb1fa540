"""Embedding LSH without Spark: random-projection buckets and the approximate nearest neighbours found through them.

The reference's embedding job ends with ``embeddingLSH`` (Embedding.scala:230-252, and its PySpark twin): a
``BucketedRandomProjectionLSH`` with ``bucketLength 0.1`` and ``numHashTables 3``, its ``transform`` and
``approxNearestNeighbors(movieEmbDF, sampleEmb, 5)``.  This module is that function.  :func:`hash_host` and
:func:`approx_nearest_host` are the DEFINITION, in numpy with a fixed operation order; :class:`LSHIndex` computes the same bits on
the device (``sprk_lsh_hash`` / ``sprk_lsh_build`` / ``sprk_lsh_query``, csrc/k_lsh.h).  The rules:

* The projection vectors ``[T, D]`` float64 are an INPUT.  :func:`random_unit_vectors` draws them from numpy's generator; Spark draws
  ``java.util.Random.nextGaussian`` from a seed made of the class name, which is not reproduced (deviation 1: the generator).
* ``bucket = floor(dot(x, r_t) / bucket_length)``: the row widened from float32 to double, ``dot = ((+0.0 + x_0 r_t0) + x_1 r_t1) + ...``
  in index order, every product and sum rounded on its own, no fused multiply-add.  The bucket is an int64 clamped to ``[-2^62, 2^62]``
  where Spark keeps the double (deviation 2: the clamp).  A ``dot`` that is not finite gives :data:`NO_BUCKET`: the row is in no bucket
  of that table.  A row with a non-finite coordinate therefore has no bucket in any table (``inf * 0`` is NaN, and neither NaN nor an
  infinity sums back to a finite number).
* The candidates of a query are the rows with ``has != 0`` whose bucket equals the query's in AT LEAST ONE table, each once: Spark's
  single-probe ``approxNearestNeighbors``.  ``dist = sqrt(sum_i (x_i - y_i)^2)`` in double, difference, square and sum in index order
  from ``+0.0``, the square root correctly rounded.  Candidates are ordered by ``(dist, row)`` ascending: Spark leaves ties open
  (deviation 3: the tie order).  ``count`` is the number of candidates and may exceed ``k``; places past it hold ``NaN`` and ``-1``.

Multi-probe search and ``approxSimilarityJoin`` are out of scope: the reference uses neither.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

NO_BUCKET = -(1 << 63)
CLAMP = 1 << 62
MAX_D, MAX_T, MAX_K = 1024, 16, 1024
_ROW_LIMIT = (1 << 31) - 1


def _bucket_length(bucket_length) -> float:
    b = float(bucket_length)
    if not (np.isfinite(b) and b > 0):
        raise ValueError("bucket_length = %r must be finite and > 0" % (bucket_length,))
    return b


def _k(k) -> int:
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k = %d outside [1, %d]" % (k, MAX_K))
    return k


def _table_shape(shape, what: str):
    if len(shape) != 2 or not 1 <= shape[1] <= MAX_D or shape[0] >= _ROW_LIMIT:
        raise ValueError("%s must be [n, D] with 1 <= D <= %d and n < 2^31 - 1" % (what, MAX_D))


def _vectors(vectors, D: int) -> np.ndarray:
    v = np.ascontiguousarray(np.asarray(vectors, dtype=np.float64))
    if v.ndim != 2 or v.shape[1] != D or not 1 <= v.shape[0] <= MAX_T:
        raise ValueError("vectors must be [T, %d] with 1 <= T <= %d" % (D, MAX_T))
    return v


def random_unit_vectors(dim: int, num_hash_tables: int, seed: int = 0) -> np.ndarray:
    """``[T, D]`` float64: ``numpy.random.default_rng(seed).standard_normal((T, D))``, every row divided by the square root of its sum of
    squares, taken in index order.  Not Spark's vectors (module docstring, deviation 1)."""
    dim, T = int(dim), int(num_hash_tables)
    if not 1 <= dim <= MAX_D or not 1 <= T <= MAX_T:
        raise ValueError("need 1 <= dim <= %d and 1 <= num_hash_tables <= %d" % (MAX_D, MAX_T))
    v = np.random.default_rng(seed).standard_normal((T, dim))
    s = np.zeros(T)
    for i in range(dim):
        s = s + v[:, i] * v[:, i]
    return v / np.sqrt(s)[:, None]


def hash_host(emb, vectors, bucket_length) -> np.ndarray:
    """The buckets of every row in every table (module docstring): ``emb [n, D]`` float32, ``vectors [T, D]`` float64 -> ``[n, T]`` int64."""
    b = _bucket_length(bucket_length)
    x = np.asarray(emb, dtype=np.float32)
    _table_shape(x.shape, "emb")
    r = _vectors(vectors, x.shape[1])
    x = x.astype(np.float64)
    with np.errstate(all="ignore"):
        dot = np.zeros((x.shape[0], r.shape[0]))
        for i in range(x.shape[1]):
            dot = dot + x[:, i:i + 1] * r[None, :, i]                     # two ufuncs: the product is rounded before the sum
        ok = np.isfinite(dot)
        h = np.clip(np.floor(np.where(ok, dot, 0.0) / b), -float(CLAMP), float(CLAMP))
    return np.where(ok, h.astype(np.int64), np.int64(NO_BUCKET))


def approx_nearest_host(emb, has, vectors, bucket_length, queries, k: int, query_has=None):
    """The definition of the search (module docstring).  ``emb [n, D]`` float32, ``has [n]`` or None (every row), ``queries [Q, D]``
    float32, ``query_has [Q]`` or None -> ``(dist [Q, k] float64, rows [Q, k] int32, count [Q] int32)``."""
    k = _k(k)
    x = np.asarray(emb, dtype=np.float32)
    y = np.asarray(queries, dtype=np.float32)
    _table_shape(x.shape, "emb")
    if y.ndim != 2 or y.shape[1] != x.shape[1]:
        raise ValueError("queries must be [Q, %d]" % x.shape[1])
    n, Q = x.shape[0], y.shape[0]
    has = np.ones(n, np.uint8) if has is None else np.asarray(has)
    qh = np.ones(Q, np.uint8) if query_has is None else np.asarray(query_has)
    if has.shape != (n,) or qh.shape != (Q,):
        raise ValueError("has must be [n] and query_has [Q]")
    buckets = hash_host(x, vectors, bucket_length)
    qb = hash_host(y, vectors, bucket_length)
    live = has != 0
    dist = np.full((Q, k), np.nan)
    rows = np.full((Q, k), -1, dtype=np.int32)
    count = np.zeros(Q, dtype=np.int32)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    for q in range(Q):
        if not qh[q]:
            continue
        match = ((buckets == qb[q][None, :]) & (qb[q] != NO_BUCKET)[None, :]).any(axis=1) & live
        cand = np.flatnonzero(match)
        count[q] = len(cand)
        if not len(cand):
            continue
        d = xd[cand] - yd[q][None, :]
        s = np.zeros(len(cand))
        for i in range(d.shape[1]):
            s = s + d[:, i] * d[:, i]
        s = np.sqrt(s)
        order = np.lexsort((cand, s))[:k]                                  # by (dist, row) ascending
        dist[q, :len(order)] = s[order]
        rows[q, :len(order)] = cand[order]
    return dist, rows, count


class LSHIndex:
    """What :meth:`build` returns.  ``buckets [n, T]`` int64 (``transform``; :data:`NO_BUCKET` in every table of a row with ``has == 0``),
    ``vectors [T, D]`` float64 (numpy) and ``bucket_length``; ``table`` / ``has`` as given, and on the device the sorted index
    ``idx_bucket [T, n]`` / ``idx_row [T, n]``.  Device tensors from a device build, numpy arrays from ``device="cpu"``."""

    def __init__(self, table, has, vectors, bucket_length, buckets, idx_bucket=None, idx_row=None, vectors_dev=None):
        self.table, self.has, self.vectors, self.bucket_length, self.buckets = table, has, vectors, bucket_length, buckets
        self.idx_bucket, self.idx_row, self._vectors_dev = idx_bucket, idx_row, vectors_dev
        self.n, self.D, self.T = int(table.shape[0]), int(table.shape[1]), int(vectors.shape[0])
        self.on_device = idx_bucket is not None

    @classmethod
    def build(cls, table, has=None, bucket_length: float = 0.1, num_hash_tables: int = 3, seed: int = 0, vectors=None, device=None) -> "LSHIndex":
        """The index over ``table [n, D]`` float32 (``has [n]``: rows without an embedding are in no bucket), a numpy array or a device
        tensor; a tensor on the device is used where it is.  ``vectors`` None: :func:`random_unit_vectors` ``(D, num_hash_tables, seed)``.
        ``device="cpu"`` runs the host definition; any other device needs a HIP device and raises ``RuntimeError`` without one.
        Enqueued on the current stream, no synchronisation."""
        b = _bucket_length(bucket_length)
        _table_shape(tuple(table.shape), "table")
        n, D = int(table.shape[0]), int(table.shape[1])
        vec = random_unit_vectors(D, num_hash_tables, seed) if vectors is None else _vectors(vectors, D)
        if has is not None and tuple(has.shape) != (n,):
            raise ValueError("has must be [n]")
        if device is not None and str(device) == "cpu":
            from . import featureeng as FE
            x = np.ascontiguousarray(FE._host_column(table), dtype=np.float32)
            h = None if has is None else np.ascontiguousarray(FE._host_column(has))
            buckets = hash_host(x, vec, b)
            if h is not None:
                buckets[h == 0] = NO_BUCKET
            return cls(x, h, vec, b, buckets)
        import ctypes as C

        import torch

        from . import _lib as L
        if not torch.cuda.is_available():
            raise RuntimeError("lsh.LSHIndex.build needs a HIP device: no HIP device is visible (approx_nearest_host is the host definition)")
        lib = L.load_library()
        if hasattr(table, "detach") and table.is_cuda and device is None:
            dev = table.device
        else:
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        t = _rows_on(table, dev)
        h = None if has is None else torch.as_tensor(has).to(dev).to(torch.uint8).contiguous()
        v = torch.from_numpy(vec).to(dev)
        with torch.cuda.device(dev):
            buckets = torch.empty((n, len(vec)), dtype=torch.int64, device=dev)
            idx_bucket = torch.empty((len(vec), n), dtype=torch.int64, device=dev)
            idx_row = torch.empty((len(vec), n), dtype=torch.int32, device=dev)
            ws_bytes = int(lib.sprk_lsh_build_workspace_bytes(n, len(vec)))
            ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)      # (torch's allocations are 512-byte aligned)
            p = lambda x: C.c_void_p(x.data_ptr() if x is not None and x.numel() else None)
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            L.check(lib.sprk_lsh_hash(p(t), p(h), n, D, int(t.stride(0)) if n else D, p(v), len(vec), b, p(buckets), stream))
            L.check(lib.sprk_lsh_build(p(buckets), n, len(vec), p(idx_bucket), p(idx_row), p(ws), ws.numel() * 8, stream))
        return cls(t, h, vec, b, buckets, idx_bucket, idx_row, v)

    def approx_nearest(self, queries, k: int, query_has=None):
        """Spark's ``approxNearestNeighbors`` for every row of ``queries [Q, D]`` float32 (numpy or a device tensor, used where it is):
        ``(dist [Q, k] float64, rows [Q, k] int32, count [Q] int32)`` -- :func:`approx_nearest_host`'s result, bit for bit; device
        tensors from a device index.  ``1 <= k <= 1024``.  Enqueued on the current stream, no synchronisation."""
        k = _k(k)
        if len(queries.shape) != 2 or int(queries.shape[1]) != self.D:
            raise ValueError("queries must be [Q, %d]" % self.D)
        Q = int(queries.shape[0])
        if query_has is not None and tuple(query_has.shape) != (Q,):
            raise ValueError("query_has must be [Q]")
        if not self.on_device:
            from . import featureeng as FE
            qh = None if query_has is None else FE._host_column(query_has)
            return approx_nearest_host(self.table, self.has, self.vectors, self.bucket_length, FE._host_column(queries), k, qh)
        import ctypes as C

        import torch

        from . import _lib as L
        lib = L.load_library()
        dev = self.table.device
        y = _rows_on(queries, dev)
        qh = None if query_has is None else torch.as_tensor(query_has).to(dev).to(torch.uint8).contiguous()
        with torch.cuda.device(dev):
            dist = torch.empty((Q, k), dtype=torch.float64, device=dev)
            rows = torch.empty((Q, k), dtype=torch.int32, device=dev)
            count = torch.empty(Q, dtype=torch.int32, device=dev)
            p = lambda x: C.c_void_p(x.data_ptr() if x is not None and x.numel() else None)
            L.check(lib.sprk_lsh_query(p(self.table), p(self.has), self.n, self.D, int(self.table.stride(0)) if self.n else self.D, p(self._vectors_dev), self.T,
                                       self.bucket_length, p(self.buckets), p(self.idx_bucket), p(self.idx_row), p(y), p(qh), Q,
                                       int(y.stride(0)) if Q else self.D, k, p(dist), p(rows), p(count), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return dist, rows, count


def _rows_on(a, dev):
    """``a [n, D]`` as a float32 tensor on ``dev`` whose rows are contiguous (a row stride above D is kept: the library takes it)."""
    import torch
    t = a.detach() if hasattr(a, "detach") else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    t = t.to(dev).to(torch.float32)
    if t.shape[1] > 0 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.data_ptr() % 4 == 0:
        return t
    return t.contiguous()
