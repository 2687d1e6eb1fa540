"""ALS collaborative filtering from ratings, without Spark: factors, scores and a top-K for every user and movie.

The reference's ``offline/spark/model/CollaborativeFiltering.scala`` (PySpark twin ``CollaborativeFiltering.py``) fits Spark ALS
(``maxIter 5``, ``regParam 0.01``, rank 10) on ``ratings.csv``, scores held-out pairs, prints the RMSE and calls
``recommendForAllUsers(10)`` / ``recommendForAllItems(10)``.  :func:`als_host` is the DEFINITION of that fit, in numpy;
:func:`als_device` / :func:`fit` compute the same bits on the device (``sprk_als_fit``, csrc/k_als.h).  DESIGN.md section 5.10 has
the rules and the deviations from Spark; in short:

* Explicit feedback, no non-negativity.  Every iteration recomputes the item factors from the user factors, then the user factors
  from the new item factors, so only the initial USER factors are an input (:func:`init_factors` by default).
* One destination row (a movie, then a user) walks its ratings in ascending order of the other side's id, a repeated (user, movie)
  pair by ascending input row, both counting.  With ``x`` = the other side's factor row widened to double it accumulates, in doubles
  from ``+0.0``, the packed upper triangle ``ata[i, j] += x[i] * x[j]`` (entry (i, j), i <= j, at ``j (j + 1) / 2 + i``; skipped when
  ``x[j] == 0``) and ``atb[i] += rating * x[i]`` (skipped when ``rating == 0``): the product is rounded, then the sum; then
  ``n * reg`` (``n`` = the row's ratings) is added to the diagonal.
* ``U^T U = A`` by columns (netlib's ``dpptrf``), then the forward and the back substitution of ``dpptrs``, in the operation order
  :func:`cholesky_solve_host` spells out; the row's factor is the solution rounded to float32.  A row whose ``d = A[j, j] - sum``
  is not ``> 0`` fails: the fit stops after that half-sweep and names the smallest such id (error kind 5 = user, 6 = movie).
* A row without a rating gets ``has = 0`` and zeros; its prediction is NaN (Spark's cold start).
"""
from __future__ import annotations

from collections import namedtuple
from typing import Mapping, Optional

import numpy as np

from . import featureeng as FE

MAX_RANK = 16
MAX_K = 1024
_ID_LIMIT = (1 << 31) - 1
ERR_USER, ERR_MOVIE, ERR_RATING, ERR_USER_SOLVE, ERR_MOVIE_SOLVE, ERR_INIT = 1, 2, 3, 5, 6, 7

Recommendations = namedtuple("Recommendations", "query ids scores")


def _error_message(kind: int, at: int) -> str:
    if kind in (ERR_USER, ERR_MOVIE):
        return FE._error_message(kind, at)
    if kind == ERR_RATING:
        return "ratings row %d: rating is not finite" % at
    if kind == ERR_USER_SOLVE:
        return "userId %d: the normal equations are not positive definite" % at
    if kind == ERR_MOVIE_SOLVE:
        return "movieId %d: the normal equations are not positive definite" % at
    if kind == ERR_INIT:
        return "init_user row %d: a value is not finite" % at
    return "error kind %d at %d" % (kind, at)


def _check_params(rank, reg, iters):
    if not 1 <= int(rank) <= MAX_RANK:
        raise ValueError("rank = %r outside [1, %d]" % (rank, MAX_RANK))
    if int(iters) < 0:
        raise ValueError("iters = %r is negative" % (iters,))
    if not (np.isfinite(reg) and reg >= 0):
        raise ValueError("reg = %r must be finite and >= 0" % (reg,))


def init_factors(n_users: int, rank: int, seed: int = 0) -> np.ndarray:
    """The default initial user factors: ``numpy.random.default_rng(seed).standard_normal`` as float32, every row divided by its
    float32 L2 norm.  (Spark's own generator is not reproduced.)"""
    x = np.random.default_rng(seed).standard_normal((int(n_users), int(rank))).astype(np.float32)
    norm = np.sqrt((x * x).sum(axis=1, dtype=np.float32)).astype(np.float32)
    return (x / norm[:, None]).astype(np.float32)


def tri_index(rank: int):
    """-> (I, J): the (i, j) of every entry of the packed upper triangle, in storage order (entry (i, j) at ``j (j + 1) / 2 + i``)."""
    I = np.array([i for j in range(rank) for i in range(j + 1)], dtype=np.int64)
    J = np.array([j for j in range(rank) for i in range(j + 1)], dtype=np.int64)
    return I, J


def normal_equations_host(dst, other, rating, n_dst: int, src, reg: float, descending: bool = False):
    """The accumulation of one half-sweep: ``dst`` / ``other`` the destination's and the other side's id of every rating, ``src
    [*, rank]`` float32 the other side's factors.  -> ``(ata [n_dst, rank (rank + 1) / 2], atb [n_dst, rank], count [n_dst])``,
    float64, regularised.  It steps "the t-th rating of every row that has one" as array operations: the rows are independent
    chains, so this is the per-row loop bit for bit.  ``descending`` walks every row backwards (tests: the order matters)."""
    dst, other = np.asarray(dst, dtype=np.int64), np.asarray(other, dtype=np.int64)
    rating, src = np.asarray(rating, dtype=np.float32), np.asarray(src, dtype=np.float32)
    rank = src.shape[1]
    I, J = tri_index(rank)
    order = np.lexsort((np.arange(len(dst)), other, dst))
    count = np.bincount(dst, minlength=n_dst).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(count)])
    o, r = other[order], rating[order]
    by_len = np.argsort(-count, kind="stable")
    neg_sorted = -count[by_len]
    ata, atb = np.zeros((n_dst, len(I))), np.zeros((n_dst, rank))
    with np.errstate(all="ignore"):
        for t in range(int(count.max()) if n_dst and len(dst) else 0):
            rows = by_len[:np.searchsorted(neg_sorted, -t, side="left")]         # the rows of more than t ratings
            at = off[rows] + (count[rows] - 1 - t if descending else t)
            x = src[o[at]].astype(np.float64)
            p = x[:, I] * x[:, J]                                                # rounded, then added
            ata[rows] = ata[rows] + np.where(x[:, J] != 0, p, 0.0)               # dspr's skip (acc + 0.0 is acc: acc is never -0.0)
            rt = r[at].astype(np.float64)[:, None]
            atb[rows] = atb[rows] + np.where(rt != 0, rt * x, 0.0)               # daxpy's skip
        lam = count.astype(np.float64) * np.float64(reg)
        diag = np.arange(rank) * (np.arange(rank) + 1) // 2 + np.arange(rank)
        ata[:, diag] = ata[:, diag] + lam[:, None]
    return ata, atb, count


def cholesky_solve_host(ata, atb):
    """``dpptrf`` + ``dpptrs`` on every row of the packed systems at once.  -> ``(y [n, rank] float64, ok [n] bool)``; a row that is
    not ``ok`` (some ``d`` not ``> 0``) holds nothing of use."""
    U, y = np.array(ata, dtype=np.float64), np.array(atb, dtype=np.float64)
    rank = y.shape[1]
    ix = lambda i, j: j * (j + 1) // 2 + i
    ok = np.ones(len(U), dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(rank):
            for i in range(j):
                s = U[:, ix(i, j)].copy()
                for p in range(i):
                    s = s - U[:, ix(p, i)] * U[:, ix(p, j)]
                U[:, ix(i, j)] = s / U[:, ix(i, i)]
            t = np.zeros(len(U))
            for p in range(j):
                t = t + U[:, ix(p, j)] * U[:, ix(p, j)]
            d = U[:, ix(j, j)] - t
            ok &= d > 0
            U[:, ix(j, j)] = np.sqrt(d)
        for j in range(rank):                                                    # U^T z = b
            t = y[:, j].copy()
            for i in range(j):
                t = t - U[:, ix(i, j)] * y[:, i]
            y[:, j] = t / U[:, ix(j, j)]
        for j in range(rank - 1, -1, -1):                                        # U y = z
            nz = y[:, j] != 0
            y[:, j] = np.where(nz, y[:, j] / U[:, ix(j, j)], y[:, j])
            for i in range(j - 1, -1, -1):
                y[:, i] = np.where(nz, y[:, i] - y[:, j] * U[:, ix(i, j)], y[:, i])
    return y, ok


def half_sweep_host(dst, other, rating, n_dst: int, src, reg: float, descending: bool = False):
    """-> ``(factors [n_dst, rank] float32, count, failed ids)``: zeros for a row without ratings and for a failed one."""
    ata, atb, count = normal_equations_host(dst, other, rating, n_dst, src, reg, descending)
    y, ok = cholesky_solve_host(ata, atb)
    rated = count > 0
    with np.errstate(all="ignore"):
        f = np.where((rated & ok)[:, None], y, 0.0).astype(np.float32)
    return f, count, np.flatnonzero(rated & ~ok)


def _check_columns(user_id, movie_id, rating, n_users, n_items):
    u, m = np.asarray(user_id).astype(np.int64), np.asarray(movie_id).astype(np.int64)
    r = np.asarray(rating, dtype=np.float32)
    if u.ndim != 1 or u.shape != m.shape or u.shape != r.shape:
        raise ValueError("the ratings columns differ in length")
    if not 0 <= n_users < _ID_LIMIT or not 0 <= n_items < _ID_LIMIT:
        raise ValueError("n_users / n_items outside [0, 2^31 - 1)")
    for kind, bad in ((ERR_USER, (u < 0) | (u >= n_users)), (ERR_MOVIE, (m < 0) | (m >= n_items)), (ERR_RATING, ~np.isfinite(r))):
        if bad.any():
            raise ValueError(_error_message(kind, int(np.flatnonzero(bad)[0])))
    return u, m, r


def als_host(user_id, movie_id, rating, n_users: int, n_items: int, rank: int = 10, reg: float = 0.01, iters: int = 5,
             init_user=None, seed: int = 0, descending: bool = False):
    """The definition (module docstring).  -> ``(user_factors [n_users, rank] float32, item_factors [n_items, rank] float32, user_has
    uint8, item_has uint8, user_count int32, item_count int32)``.  ``iters = 0`` gives ``init_user``, zero item factors and the
    counts.  Errors raise ``ValueError`` with the message of the device's error word."""
    _check_params(rank, reg, iters)
    n_users, n_items, rank = int(n_users), int(n_items), int(rank)
    u, m, r = _check_columns(user_id, movie_id, rating, n_users, n_items)
    uf = init_factors(n_users, rank, seed) if init_user is None else np.array(init_user, dtype=np.float32)
    if uf.shape != (n_users, rank):
        raise ValueError("init_user must be [n_users, rank]")
    bad = ~np.isfinite(uf).all(axis=1)
    if bad.any():
        raise ValueError(_error_message(ERR_INIT, int(np.flatnonzero(bad)[0])))
    itf = np.zeros((n_items, rank), dtype=np.float32)
    ucount, icount = np.bincount(u, minlength=n_users).astype(np.int32), np.bincount(m, minlength=n_items).astype(np.int32)
    for _ in range(int(iters)):
        itf, _, failed = half_sweep_host(m, u, r, n_items, uf, reg, descending)
        if len(failed):
            raise ValueError(_error_message(ERR_MOVIE_SOLVE, int(failed[0])))
        uf, _, failed = half_sweep_host(u, m, r, n_users, itf, reg, descending)
        if len(failed):
            raise ValueError(_error_message(ERR_USER_SOLVE, int(failed[0])))
    return uf, itf, (ucount > 0).astype(np.uint8), (icount > 0).astype(np.uint8), ucount, icount


def predict_host(users, movies, user_factors, user_has, item_factors, item_has) -> np.ndarray:
    """``ALSModel``'s score on the host: the float32 dot in index order, ``acc = acc + u[d] * v[d]`` unfused from ``0.0f``; NaN
    when either id is out of range or has no factor."""
    users, movies = np.asarray(users, dtype=np.int64), np.asarray(movies, dtype=np.int64)
    uf, itf = np.asarray(user_factors, dtype=np.float32), np.asarray(item_factors, dtype=np.float32)
    ok = (users >= 0) & (users < len(uf)) & (movies >= 0) & (movies < len(itf))
    us, ms = np.where(ok, users, 0), np.where(ok, movies, 0)
    acc = np.zeros(len(users), dtype=np.float32)
    if len(uf) and len(itf):
        ok &= (np.asarray(user_has)[us] != 0) & (np.asarray(item_has)[ms] != 0)
        with np.errstate(all="ignore"):
            for d in range(uf.shape[1]):
                acc = acc + uf[us, d] * itf[ms, d]
    else:
        ok &= False
    return np.where(ok, acc, np.float32(np.nan)).astype(np.float32)


def topk_host(query, query_has, table, table_has, k: int):
    """The definition of ``sprk_als_topk``: per query row the ``k`` rows of ``table`` with the largest :func:`predict_host` dot,
    descending, equal scores by ascending row, rows with ``has == 0`` left out; ``-1`` / NaN past the rows available (all of them for a
    query without factors).  -> ``(rows [n, k] int32, scores [n, k] float32)``."""
    query, table = np.asarray(query, dtype=np.float32), np.asarray(table, dtype=np.float32)
    rows = np.full((len(query), k), -1, dtype=np.int32)
    scores = np.full((len(query), k), np.nan, dtype=np.float32)
    live = np.flatnonzero(np.asarray(table_has) != 0)
    for q in range(len(query)):
        if not query_has[q] or not len(live):
            continue
        acc = np.zeros(len(live), dtype=np.float32)
        with np.errstate(all="ignore"):
            for d in range(table.shape[1]):
                acc = acc + query[q, d] * table[live, d]
        order = np.lexsort((live, -acc.astype(np.float64)))[:k]
        rows[q, :len(order)], scores[q, :len(order)] = live[order], acc[order]
    return rows, scores


def split(ratings: Mapping, weights=(0.8, 0.2), seed: int = 0) -> list:
    """A random split of the rating columns by ``numpy.random.default_rng(seed).permutation`` -- not Spark's ``randomSplit``: part i
    holds the rows the permutation places in its share, in input order.  -> one dict of numpy columns per weight."""
    cols = {k: FE._host_column(v) for k, v in ratings.items()}
    n = len(next(iter(cols.values())))
    w = np.asarray(weights, dtype=np.float64)
    if len(w) < 1 or (w < 0).any() or not w.sum() > 0:
        raise ValueError("weights must be non-negative and sum to more than 0")
    cuts = np.floor(np.cumsum(w) / w.sum() * n + 0.5).astype(np.int64)
    cuts[-1] = n
    perm = np.random.default_rng(seed).permutation(n)
    out, lo = [], 0
    for hi in cuts.tolist():
        at = np.sort(perm[lo:hi])
        out.append({k: v[at] for k, v in cols.items()})
        lo = hi
    return out


# ---------------------------------------------------------------- the device

def _need(t, dt, dev, what):
    if t.dtype != dt or not t.is_contiguous() or t.device != dev:
        raise ValueError("%s must be a contiguous %s tensor on %s" % (what, dt, dev))


def als_device(user_id, movie_id, rating, n_users: int, n_items: int, rank: int = 10, reg: float = 0.01, iters: int = 5, init_user=None,
               user_stride: Optional[int] = None, item_stride: Optional[int] = None):
    """``sprk_als_fit`` on device tensors, enqueued on the current stream; no synchronisation.  ``user_id`` / ``movie_id`` int32 ``[n]``,
    ``rating`` float32 ``[n]``, ``init_user [n_users, >= rank]`` float32 (its row stride is passed on).  -> ``(user_factors [n_users,
    user_stride], item_factors [n_items, item_stride], user_has, item_has, user_count, item_count, error word)``: tensors; the error
    word (int64, -1 = none) is the caller's to read."""
    import ctypes as C

    import torch

    from . import _lib as L
    _check_params(rank, reg, iters)
    lib = L.load_library()
    dev = rating.device
    n, rank = int(user_id.numel()), int(rank)
    user_stride = rank if user_stride is None else int(user_stride)
    item_stride = rank if item_stride is None else int(item_stride)
    _need(user_id, torch.int32, dev, "user_id"); _need(movie_id, torch.int32, dev, "movie_id"); _need(rating, torch.float32, dev, "rating")
    if init_user.dtype != torch.float32 or init_user.device != dev or init_user.ndim != 2 or init_user.shape[0] != n_users or \
            init_user.shape[1] < rank or (n_users and init_user.stride(1) != 1):
        raise ValueError("init_user must be a float32 [n_users, >= rank] tensor on %s with unit column stride" % (dev,))
    with torch.cuda.device(dev):
        # (one spare row each: an empty table still has an address)
        uf = torch.zeros((n_users + 1, max(user_stride, 1)), dtype=torch.float32, device=dev)
        itf = torch.zeros((n_items + 1, max(item_stride, 1)), dtype=torch.float32, device=dev)
        uh, ih = torch.zeros(n_users + 1, dtype=torch.uint8, device=dev), torch.zeros(n_items + 1, dtype=torch.uint8, device=dev)
        uc, ic = torch.zeros(n_users + 1, dtype=torch.int32, device=dev), torch.zeros(n_items + 1, dtype=torch.int32, device=dev)
        word = torch.full((1,), -1, dtype=torch.int64, device=dev)
        ws_bytes = lib.sprk_als_workspace_bytes(n, n_users, n_items, rank)
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        init_stride = int(init_user.stride(0)) if n_users else rank
        L.check(lib.sprk_als_fit(p(user_id), p(movie_id), p(rating), n, n_users, n_items, rank, float(reg), int(iters),
                                 p(init_user) if n_users else p(uf), max(init_stride, rank), p(uf), user_stride, p(itf), item_stride, p(uh), p(ih), p(uc), p(ic),
                                 p(word), p(ws), ws.numel() * 8, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return uf[:n_users], itf[:n_items], uh[:n_users], ih[:n_items], uc[:n_users], ic[:n_items], word


def predict_device(users, movies, user_factors, user_has, item_factors, item_has, rank: Optional[int] = None):
    """``sprk_als_predict`` on device tensors (ids int32), enqueued on the current stream.  -> float32 ``[n]``."""
    import ctypes as C

    import torch

    from . import _lib as L
    lib = L.load_library()
    dev = user_factors.device
    _need(users, torch.int32, dev, "users"); _need(movies, torch.int32, dev, "movies")
    rank = int(user_factors.shape[1]) if rank is None else int(rank)
    n = int(users.numel())
    with torch.cuda.device(dev):
        out = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        L.check(lib.sprk_als_predict(p(users), p(movies), n, p(user_factors), int(user_factors.stride(0)) if user_factors.shape[0] else rank, p(user_has),
                                     p(item_factors), int(item_factors.stride(0)) if item_factors.shape[0] else rank, p(item_has),
                                     int(user_factors.shape[0]), int(item_factors.shape[0]), rank, p(out),
                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out[:n]


def topk_device(query, query_has, table, table_has, k: int, rank: Optional[int] = None):
    """``sprk_als_topk`` on device tensors, enqueued on the current stream.  -> ``(rows [n, k] int32, scores [n, k] float32)``."""
    import ctypes as C

    import torch

    from . import _lib as L
    lib = L.load_library()
    dev = table.device
    rank = int(table.shape[1]) if rank is None else int(rank)
    nq, nt, k = int(query.shape[0]), int(table.shape[0]), int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k = %d outside [1, %d]" % (k, MAX_K))
    with torch.cuda.device(dev):
        rows = torch.empty((max(nq, 1), k), dtype=torch.int32, device=dev)
        scores = torch.empty((max(nq, 1), k), dtype=torch.float32, device=dev)
        ws_bytes = lib.sprk_als_topk_workspace_bytes(nt, nq, k)
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        L.check(lib.sprk_als_topk(p(table), p(table_has), nt, rank, int(table.stride(0)) if nt else rank, p(query), p(query_has), nq,
                                  int(query.stride(0)) if nq else rank, k, p(scores), p(rows), p(ws), ws.numel() * 8,
                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return rows[:nq], scores[:nq]


def _columns(ratings, dev, with_rating=True):
    """-> userId, movieId (int32, an id beyond int32 as -1) and rating (float32) as device tensors."""
    import torch

    from . import userembedding as UE
    if isinstance(ratings, str):
        ratings = FE._read_csv_columns(ratings, ["userId", "movieId", "rating"])
    u, m = UE._id_columns(ratings, dev)
    narrow = lambda t: torch.where((t < 0) | (t >= _ID_LIMIT), torch.full_like(t, -1), t).to(torch.int32).contiguous()
    if not with_rating:
        return narrow(u), narrow(m), None
    if "rating" not in ratings:
        raise KeyError("ratings needs the column 'rating'")
    col = ratings["rating"]
    if hasattr(col, "detach"):
        r = col.detach().to(dev).to(torch.float32)
    else:
        a = np.asarray(col)
        a = a.astype(np.float32) if a.dtype.kind in "fiub" else np.array([float(v) for v in a.tolist()], dtype=np.float32)
        r = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if r.ndim != 1 or r.numel() != u.numel():
        raise ValueError("the ratings columns differ in length")
    return narrow(u), narrow(m), r.contiguous()


def _ids(ids, dev):
    import torch
    if hasattr(ids, "detach"):
        t = ids.detach().to(dev).to(torch.int64)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(ids, dtype=np.int64))).to(dev)
    return torch.where((t < 0) | (t >= _ID_LIMIT), torch.full_like(t, -1), t).to(torch.int32).contiguous()


class ALSModel:
    """What :func:`fit` returns: ``user_factors [n_users, rank]`` / ``item_factors [n_items, rank]`` float32, ``user_has`` /
    ``item_has`` uint8 and ``user_count`` / ``item_count`` int32, row = id, as device tensors."""

    def __init__(self, user_factors, item_factors, user_has, item_has, user_count, item_count):
        self.user_factors, self.item_factors = user_factors, item_factors
        self.user_has, self.item_has, self.user_count, self.item_count = user_has, item_has, user_count, item_count
        self.n_users, self.n_items, self.rank = int(user_factors.shape[0]), int(item_factors.shape[0]), int(user_factors.shape[1])
        self.device = user_factors.device

    def to_host(self):
        """:func:`als_host`'s six arrays, bit for bit."""
        return tuple(np.ascontiguousarray(FE._host_column(x)) for x in
                     (self.user_factors, self.item_factors, self.user_has, self.item_has, self.user_count, self.item_count))

    def predict(self, users, movies):
        """The score of every (user, movie) pair, a float32 device tensor; NaN for an id outside the tables or without a factor."""
        return predict_device(_ids(users, self.device), _ids(movies, self.device), self.user_factors, self.user_has, self.item_factors, self.item_has)

    def rmse(self, ratings) -> float:
        """The evaluator of the reference with ``coldStartStrategy = "drop"``: rows whose prediction is NaN are dropped, the squared
        float32 errors are averaged in float64, then the square root.  Computed with torch on the device; not promised bit for bit."""
        import torch
        u, m, r = _columns(ratings, self.device)
        pred = predict_device(u, m, self.user_factors, self.user_has, self.item_factors, self.item_has)
        keep = ~torch.isnan(pred)
        e = (pred[keep] - r[keep])
        return float(torch.sqrt((e * e).to(torch.float64).mean())) if int(keep.sum()) else float("nan")

    def _recommend(self, query, query_has, table, table_has, ids, k):
        import torch
        if ids is None:
            at = torch.nonzero(query_has, as_tuple=False)[:, 0]
            q, qh = query[at].contiguous(), query_has[at].contiguous()
        else:
            at = _ids(ids, self.device).to(torch.int64)
            inside = (at >= 0) & (at < query.shape[0])
            safe = torch.where(inside, at, torch.zeros_like(at))
            if query.shape[0]:
                q, qh = query[safe].contiguous(), (query_has[safe] * inside.to(query_has.dtype)).contiguous()
            else:
                q, qh = torch.zeros((at.numel(), self.rank), dtype=torch.float32, device=self.device), torch.zeros(at.numel(), dtype=torch.uint8, device=self.device)
        rows, scores = topk_device(q, qh, table, table_has, k, rank=self.rank)
        return Recommendations(at, rows, scores)

    def recommend_for_users(self, users=None, k: int = 10) -> Recommendations:
        """``recommendForAllUsers(k)`` / ``recommendForUserSubset``: for every user of ``users`` (None: every user that has factors) the
        ``k`` movies with the largest score, best first, equal scores by ascending movie id.  -> ``(query, ids [n, k] int32, scores
        [n, k] float32)`` device tensors; ``-1`` / NaN past the movies that have factors and for a user without factors."""
        return self._recommend(self.user_factors, self.user_has, self.item_factors, self.item_has, users, k)

    def recommend_for_items(self, items=None, k: int = 10) -> Recommendations:
        """``recommendForAllItems(k)``: the same with the sides exchanged."""
        return self._recommend(self.item_factors, self.item_has, self.user_factors, self.user_has, items, k)

    def evaluate_ranking(self, test, train=None, ks=(10,), list_len: Optional[int] = None, min_rating: float = 3.5):
        """The ranking metrics of this model's recommendations against held-out ratings (``rankeval.evaluate``): for every user with a
        ``test`` row of ``rating >= min_rating``, the ``list_len`` best movies (default ``min(1024, n_items)``) by
        :meth:`recommend_for_users`, cleared of the movies the user rated in ``train``, against the user's truth at the cut-offs ``ks``.
        ``test`` / ``train``: a CSV path or rating columns, numpy arrays or device tensors.  -> ``rankeval.RankEval`` of device tensors,
        one query per such user in ascending user id; no list leaves HBM."""
        import torch

        from . import rankeval as RE
        u, m, r = _columns(test, self.device)
        held_out = {"userId": u, "movieId": m, "rating": r}
        users = torch.unique(u[(r >= float(min_rating)) & (u >= 0)])
        k = min(MAX_K, self.n_items) if list_len is None else int(list_len)
        lists = self.recommend_for_users(users, k).ids
        return RE.evaluate(lists, users, held_out, train, ks=ks, min_rating=min_rating, device=self.device)


def fit(ratings, rank: int = 10, reg: float = 0.01, iters: int = 5, seed: int = 0, init_user=None, device=None,
        n_users: Optional[int] = None, n_items: Optional[int] = None) -> ALSModel:
    """ALS on the device.  ``ratings``: a CSV path or columns ``{userId, movieId, rating, ..}``, numpy arrays or device tensors.  The
    tables are sized by the greatest ids + 1 unless given.  Errors are the ``ValueError`` of :func:`als_host`, naming kind and row or
    id.  One host synchronisation, the error word (and the reductions that find the greatest ids)."""
    import torch
    _check_params(rank, reg, iters)
    if not torch.cuda.is_available():
        raise RuntimeError("als.fit needs a HIP device: no HIP device is visible (als_host is the host definition)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    u, m, r = _columns(ratings, dev)
    if n_users is None:
        n_users = max(int(u.max()) + 1, 0) if u.numel() else 0
    if n_items is None:
        n_items = max(int(m.max()) + 1, 0) if m.numel() else 0
    if not 0 <= n_users < _ID_LIMIT or not 0 <= n_items < _ID_LIMIT:
        raise ValueError("n_users / n_items outside [0, 2^31 - 1)")
    if init_user is None:
        init_user = init_factors(n_users, rank, seed)
    init = (init_user.detach() if hasattr(init_user, "detach") else torch.from_numpy(np.ascontiguousarray(init_user, dtype=np.float32))).to(dev).to(torch.float32).contiguous()
    if tuple(init.shape) != (n_users, int(rank)):
        raise ValueError("init_user must be [n_users, rank]")
    out = als_device(u, m, r, int(n_users), int(n_items), rank, reg, iters, init)
    err = int(out[6].cpu()[0])                                                     # the one synchronisation
    if err != -1:
        raise ValueError(_error_message((err >> 32) & 0xffffffff, err & 0xffffffff))
    return ALSModel(*out[:6])
