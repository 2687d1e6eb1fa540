"""Ranking metrics of top-K lists against held-out ratings: Spark's ``RankingMetrics`` (``precisionAt``, ``recallAt``, ``ndcgAt``,
``meanAveragePrecisionAt``) plus hit rate and reciprocal rank, with the movies a user has already rated dropped from the lists.

:func:`rank_eval_host` is the definition: numpy and Python loops, float64, every operation rounded on its own, in a fixed order.
:func:`rank_eval_device` computes the same bytes from HBM (``sprk_rank_eval``, csrc/k_rank_eval.h); DESIGN.md section 5.18 has the rules.

Per query ``q`` of user ``u``: ``T`` = the distinct truth items of ``u``, ``R = |T|``; ``E`` = ``pred[q]`` in order without negative
entries and without the entries in ``seen(u)``, ``L = len(E)``.  A truth item that is also seen stays in ``T`` (its list entry is
dropped all the same); duplicate entries of ``pred`` each count.  For a cut-off ``k`` with ``n = min(L, k)``, the hits are the places
``i < n`` with ``E[i]`` in ``T``:

=========  =====================================================================================================
precision  ``hits / k``
recall     ``hits / R``
ndcg       ``dcg / gain_sum[min(R, k)]``, ``dcg`` = the sum of ``gain[i]`` over the hits, in list order, from ``+0.0``
ap         ``(sum over the hits, in order, of cnt_i / (i + 1)) / min(R, k)``, ``cnt_i`` = the running hit count
hit        ``1.0`` where ``hits > 0``
rr         ``1 / (i0 + 1)`` for the first hit ``i0``, else ``0.0``
=========  =====================================================================================================

A query with ``R == 0`` scores ``+0.0`` six times (Spark's rule) and is not counted in ``n_with_truth``.  ``gain`` and ``gain_sum``
come from :func:`gain_table` on the host for both routes: no logarithm is taken on the device.

``recall@K`` of approximate lists against exact ones is the same computation with the exact lists as the truth::

    _, exact = ranker.topk(queries, 10)                                   # rows [Q, 10], an EmbRanker's exact search
    _, approx, _ = ranker.lsh_index().approx_nearest(queries, 10)         # rows [Q, 10], what approx_similar_movies ranks by
    truth_user, truth_item = lists_as_truth(exact)
    recall = rank_eval_device(approx, None, truth_user, truth_item, ks=(10,)).mean("all")[0, RECALL]
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

MAX_K, MAX_KS, MAX_LIST, CHUNK = 1024, 8, 65536, 256
_ID_LIMIT = 2**31 - 1
PRECISION, RECALL, NDCG, AP, HIT, RR = range(6)
METRICS = ("precision", "recall", "ndcg", "ap", "hit", "rr")
ERR_TRUTH, ERR_SEEN, ERR_QUERY = 1, 2, 3


def gain_table():
    """``(gain [1024], gain_sum [1025])`` float64: ``gain[i] = 1.0 / log(i + 2)`` and ``gain_sum[c]`` = the sum of ``gain[:c]``, added
    in order from ``+0.0``."""
    gain = np.array([1.0 / math.log(i + 2) for i in range(MAX_K)], dtype=np.float64)
    gain_sum = np.zeros(MAX_K + 1, dtype=np.float64)
    s = 0.0
    for c in range(MAX_K):
        s = s + float(gain[c])
        gain_sum[c + 1] = s
    return gain, gain_sum


def _error_message(kind: int, at: int) -> str:
    what = {ERR_TRUTH: "truth row %d: user outside [0, n_users) or item < 0", ERR_SEEN: "seen row %d: user outside [0, n_users) or item < 0",
            ERR_QUERY: "query %d: user outside [0, n_users)"}.get(kind, "row %d")
    return "rank_eval: error kind %d, " % kind + what % at


def _check_ks(ks) -> list:
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= MAX_KS:
        raise ValueError("ks holds %d cut-offs: 1 to %d" % (len(ks), MAX_KS))
    for k in ks:
        if not 1 <= k <= MAX_K:
            raise ValueError("k = %d outside [1, %d]" % (k, MAX_K))
    return ks


def _check_tables(gain, gain_sum):
    if gain is None and gain_sum is None:
        return gain_table()
    if gain is None or gain_sum is None or tuple(gain.shape) != (MAX_K,) or tuple(gain_sum.shape) != (MAX_K + 1,):
        raise ValueError("gain must be [%d] and gain_sum [%d], both given or neither" % (MAX_K, MAX_K + 1))
    return gain, gain_sum


class RankEval:
    """What both routes return.  ``per_query [Q, n_ks, 6]`` float64 (metric order :data:`METRICS`), ``n_relevant [Q]`` (= R) and
    ``n_ranked [Q]`` (= L) int32, ``sums [n_ks, 6]`` float64 and ``counts [2]`` int64 = ``(Q, n_with_truth)``: numpy arrays from the
    definition, device tensors from the device.  ``ks`` is the tuple of cut-offs."""

    def __init__(self, ks, per_query, n_relevant, n_ranked, sums, counts):
        self.ks = tuple(ks)
        self.per_query, self.n_relevant, self.n_ranked, self.sums, self.counts = per_query, n_relevant, n_ranked, sums, counts

    def to_host(self) -> "RankEval":
        from . import featureeng as FE
        return RankEval(self.ks, *(np.ascontiguousarray(FE._host_column(x)) for x in (self.per_query, self.n_relevant, self.n_ranked, self.sums, self.counts)))

    def mean(self, over: str = "truth") -> np.ndarray:
        """``sums`` divided by the number of queries -- ``over="all"``, Spark's ``.mean()`` -- or by the number of queries that have
        truth, ``over="truth"``.  -> numpy ``[n_ks, 6]`` float64; NaN where the divisor is 0."""
        if over not in ("truth", "all"):
            raise ValueError("over = %r ('truth' or 'all')" % (over,))
        from . import featureeng as FE
        sums, counts = FE._host_column(self.sums).astype(np.float64), FE._host_column(self.counts)
        n = int(counts[0] if over == "all" else counts[1])
        return sums / np.float64(n) if n else np.full_like(sums, np.nan)


def _pairs(user, item, what):
    if user is None and item is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if user is None or item is None:
        raise ValueError("%s_user and %s_item go together" % (what, what))
    u, i = np.asarray(user), np.asarray(item)
    if u.ndim != 1 or u.shape != i.shape or u.dtype.kind not in "iu" or i.dtype.kind not in "iu":
        raise ValueError("%s_user and %s_item must be integer columns of one length" % (what, what))
    return u.astype(np.int64), i.astype(np.int64)


def ordered_sums(per_query: np.ndarray, n_relevant: np.ndarray):
    """``(sums [n_ks, 6], counts [2])`` of ``per_query``: per (k, metric), partial sums over :data:`CHUNK` consecutive queries from
    ``+0.0`` in query order, then the partials in order from ``+0.0``."""
    Q, n_ks = per_query.shape[0], per_query.shape[1]
    sums = np.zeros((n_ks, 6), dtype=np.float64)
    for j in range(n_ks):
        for m in range(6):
            total = 0.0
            for c0 in range(0, Q, CHUNK):
                part = 0.0
                for v in per_query[c0:c0 + CHUNK, j, m].tolist():
                    part = part + v
                total = total + part
            sums[j, m] = total
    return sums, np.array([Q, int((n_relevant > 0).sum())], dtype=np.int64)


def rank_eval_host(pred, query_user, truth_user, truth_item, seen_user=None, seen_item=None, n_users: Optional[int] = None, ks: Sequence[int] = (10,),
                   gain=None, gain_sum=None) -> RankEval:
    """The definition (the module's docstring has the rules).  ``pred [Q, Lp]`` integer, best first, a negative entry is no entry;
    ``query_user [Q]`` or None for ``u = q``; the truth and the seen pairs in any order, duplicates allowed; ``n_users`` (None: the
    greatest user + 1 of the three).  Errors are ``ValueError`` naming kind and row, the smallest ``(kind << 32 | row)``: kind 1 a
    truth row and kind 2 a seen row whose user lies outside ``[0, n_users)`` or whose item is negative, kind 3 a query's user
    outside ``[0, n_users)``."""
    ks = _check_ks(ks)
    gain, gain_sum = _check_tables(gain, gain_sum)
    pred = np.asarray(pred)
    if pred.ndim != 2 or pred.dtype.kind not in "iu" or not 1 <= pred.shape[1] <= MAX_LIST:
        raise ValueError("pred must be an integer [Q, 1 .. %d] array" % MAX_LIST)
    Q = pred.shape[0]
    qu = np.arange(Q, dtype=np.int64) if query_user is None else np.asarray(query_user).astype(np.int64)
    if qu.shape != (Q,):
        raise ValueError("query_user must be [Q]")
    tu, ti = _pairs(truth_user, truth_item, "truth")
    su, si = _pairs(seen_user, seen_item, "seen")
    if n_users is None:
        n_users = max([int(a.max()) + 1 for a in (qu, tu, su) if len(a)] + [0])
    n_users = int(n_users)
    if not 0 <= n_users < _ID_LIMIT or len(tu) >= _ID_LIMIT or len(su) >= _ID_LIMIT:
        raise ValueError("n_users, n_truth and n_seen must each be in [0, 2^31 - 1)")
    for kind, bad in ((ERR_TRUTH, (tu < 0) | (tu >= n_users) | (ti < 0)), (ERR_SEEN, (su < 0) | (su >= n_users) | (si < 0)), (ERR_QUERY, (qu < 0) | (qu >= n_users))):
        if bad.any():
            raise ValueError(_error_message(kind, int(np.flatnonzero(bad)[0])))
    truth, seen = {}, {}
    for u, i in zip(tu.tolist(), ti.tolist()):
        truth.setdefault(u, set()).add(i)
    for u, i in zip(su.tolist(), si.tolist()):
        seen.setdefault(u, set()).add(i)
    g, gs = [float(v) for v in np.asarray(gain, dtype=np.float64)], [float(v) for v in np.asarray(gain_sum, dtype=np.float64)]
    per_query = np.zeros((Q, len(ks), 6), dtype=np.float64)
    n_relevant, n_ranked = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32)
    none = frozenset()
    for q in range(Q):
        u = int(qu[q])
        T, S = truth.get(u, none), seen.get(u, none)
        E = [i for i in pred[q].tolist() if i >= 0 and i not in S]
        R, L = len(T), len(E)
        n_relevant[q], n_ranked[q] = R, L
        if R == 0:
            continue
        for j, k in enumerate(ks):
            hits, dcg, ap, first = 0, 0.0, 0.0, 0
            for i in range(min(L, k)):
                if E[i] in T:
                    hits += 1
                    dcg = dcg + g[i]
                    ap = ap + float(hits) / float(i + 1)
                    if not first:
                        first = i + 1
            m = min(R, k)
            per_query[q, j] = (float(hits) / float(k), float(hits) / float(R), dcg / gs[m], ap / float(m), 1.0 if hits else 0.0,
                               1.0 / float(first) if first else 0.0)
    sums, counts = ordered_sums(per_query, n_relevant)
    return RankEval(ks, per_query, n_relevant, n_ranked, sums, counts)


# ---------------------------------------------------------------- the device

def _i32(t, dev, what):
    """An id column or matrix as a contiguous int32 tensor on ``dev``; an id beyond int32 becomes -1 (no entry / an error row)."""
    import torch
    if t is None:
        return None
    if hasattr(t, "detach"):
        t = t.detach()
        if t.dtype.is_floating_point:
            raise TypeError("%s must hold integers" % what)
    else:
        a = np.asarray(t)
        if a.dtype.kind not in "iu":
            raise TypeError("%s must hold integers" % what)
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64) if a.dtype != np.int32 else a))
    t = t.to(dev)
    if t.dtype != torch.int32:
        t = t.to(torch.int64)
        t = torch.where((t < 0) | (t > _ID_LIMIT), torch.full_like(t, -1), t).to(torch.int32)
    return t


def rank_eval_device(pred, query_user, truth_user, truth_item, seen_user=None, seen_item=None, n_users: Optional[int] = None,
                     ks: Sequence[int] = (10,), gain=None, gain_sum=None, device=None) -> RankEval:
    """:func:`rank_eval_host`'s five outputs, byte for byte, as device tensors (``sprk_rank_eval``).  The inputs are numpy arrays or
    tensors; a tensor on the device is used where it is, and a ``pred`` whose rows are contiguous keeps its row stride.  ``n_users``
    None costs one reduction per column.  One host synchronisation, the error word; the errors are the definition's.
    ``device="cpu"`` runs the definition; any other device needs a HIP device and raises ``RuntimeError`` without one."""
    ks = _check_ks(ks)
    gain, gain_sum = _check_tables(gain, gain_sum)
    if device is not None and str(device) == "cpu":
        from . import featureeng as FE
        h = lambda x: None if x is None else FE._host_column(x)
        return rank_eval_host(h(pred), h(query_user), h(truth_user), h(truth_item), h(seen_user), h(seen_item), n_users, ks, h(gain), h(gain_sum))
    import ctypes as C

    import torch

    from . import _lib as L
    if not torch.cuda.is_available():
        raise RuntimeError("rankeval.rank_eval_device needs a HIP device: no HIP device is visible (rank_eval_host is the host definition)")
    lib = L.load_library()
    if hasattr(pred, "detach") and pred.is_cuda and device is None:
        dev = pred.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if len(pred.shape) != 2 or not 1 <= int(pred.shape[1]) <= MAX_LIST:
        raise ValueError("pred must be an integer [Q, 1 .. %d] array" % MAX_LIST)
    if (truth_user is None) != (truth_item is None) or (seen_user is None) != (seen_item is None):
        raise ValueError("the user and the item column of the truth, and of the seen pairs, go together")
    p_ = _i32(pred, dev, "pred")
    if p_.shape[0] and (p_.stride(1) != 1 or p_.stride(0) < p_.shape[1]):
        p_ = p_.contiguous()
    Q, Lp = int(p_.shape[0]), int(p_.shape[1])
    col = lambda x, what: None if x is None else _i32(x, dev, what).contiguous()
    qu, tu, ti, su, si = (col(x, w) for x, w in ((query_user, "query_user"), (truth_user, "truth_user"), (truth_item, "truth_item"),
                                                 (seen_user, "seen_user"), (seen_item, "seen_item")))
    for a, b, w in ((tu, ti, "truth"), (su, si, "seen")):
        if a is not None and (a.ndim != 1 or a.shape != b.shape):
            raise ValueError("%s_user and %s_item must be integer columns of one length" % (w, w))
    if qu is not None and tuple(qu.shape) != (Q,):
        raise ValueError("query_user must be [Q]")
    n_truth, n_seen = (0 if tu is None else int(tu.numel())), (0 if su is None else int(su.numel()))
    if n_users is None:
        n_users = max([int(a.max()) + 1 for a in (qu, tu, su) if a is not None and a.numel()] + [Q if qu is None else 0, 0])
    n_users = int(n_users)
    if not 0 <= n_users < _ID_LIMIT or n_truth >= _ID_LIMIT or n_seen >= _ID_LIMIT:
        raise ValueError("n_users, n_truth and n_seen must each be in [0, 2^31 - 1)")
    as_f64 = lambda x: (x.detach() if hasattr(x, "detach") else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).to(dev).to(torch.float64).contiguous()
    g, gs = as_f64(gain), as_f64(gain_sum)
    with torch.cuda.device(dev):
        # (one spare row each: an empty output still has an address)
        per_query = torch.empty((Q + 1, len(ks), 6), dtype=torch.float64, device=dev)
        n_relevant = torch.empty(Q + 1, dtype=torch.int32, device=dev)
        n_ranked = torch.empty(Q + 1, dtype=torch.int32, device=dev)
        sums = torch.empty((len(ks), 6), dtype=torch.float64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        word = torch.full((1,), -1, dtype=torch.int64, device=dev)
        ws_bytes = int(lib.sprk_rank_eval_workspace_bytes(n_truth, n_seen, n_users, Q))
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)          # (torch's allocations are 512-byte aligned)
        p = lambda x: C.c_void_p(x.data_ptr() if x is not None and x.numel() else None)
        L.check(lib.sprk_rank_eval(p(p_), Q, Lp, int(p_.stride(0)) if Q else Lp, p(qu), p(tu), p(ti), n_truth, p(su), p(si), n_seen, n_users,
                                   (C.c_int32 * len(ks))(*ks), len(ks), p(g), p(gs), C.c_void_p(per_query.data_ptr()), C.c_void_p(n_relevant.data_ptr()),
                                   C.c_void_p(n_ranked.data_ptr()), p(sums), p(counts), p(word), p(ws), ws.numel() * 8,
                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        err = int(word.cpu()[0])                                                           # the one synchronisation
    if err != -1:
        raise ValueError(_error_message((err >> 32) & 0xffffffff, err & 0xffffffff))
    return RankEval(ks, per_query[:Q], n_relevant[:Q], n_ranked[:Q], sums, counts)


def lists_as_truth(lists):
    """The ``(query, item)`` pairs of one set of lists ``[Q, K]`` as truth columns ``(truth_user, truth_item)``, query ``q`` standing
    for user ``q``; negative entries are left out.  numpy in, numpy out; a device tensor in, device tensors out."""
    if hasattr(lists, "detach"):
        import torch
        t = lists.detach()
        keep = t >= 0
        q = torch.arange(t.shape[0], device=t.device, dtype=torch.int32)[:, None].expand(t.shape)
        return q[keep].contiguous(), t[keep].to(torch.int32).contiguous()
    a = np.asarray(lists)
    if a.ndim != 2:
        raise ValueError("lists must be [Q, K]")
    keep = a >= 0
    q = np.broadcast_to(np.arange(a.shape[0], dtype=np.int32)[:, None], a.shape)
    return np.ascontiguousarray(q[keep]), np.ascontiguousarray(a[keep].astype(np.int32))


def evaluate(lists, users, test, train=None, ks: Sequence[int] = (10,), min_rating: float = 3.5, n_users: Optional[int] = None, device=None) -> RankEval:
    """The ranking metrics of ``lists [Q, Lp]`` (item ids, best first) for ``users [Q]`` (None: list ``q`` is user ``q``'s) against
    the held-out ratings ``test``: the truth is its rows with ``rating >= min_rating``, the reference's label rule.  ``train``, when
    given, is what the users have already rated: those movies are dropped from the lists.  ``test`` / ``train`` are rating columns
    ``{userId, movieId, rating, ..}`` -- numpy arrays or device tensors, any mapping that holds them, or a CSV path (``train`` needs
    no ``rating``).  On the device unless ``device="cpu"``; no list leaves HBM."""
    import torch

    from . import als as A
    if device is not None and str(device) == "cpu":
        dev = torch.device("cpu")
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("rankeval.evaluate needs a HIP device: no HIP device is visible (device=\"cpu\" runs the host definition)")
        if hasattr(lists, "detach") and lists.is_cuda and device is None:
            dev = lists.device
        else:
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    tu, ti, tr = A._columns(test, dev)
    keep = tr >= float(min_rating)
    tu, ti = tu[keep].contiguous(), ti[keep].contiguous()
    su = si = None
    if train is not None:
        su, si, _ = A._columns(train, dev, with_rating=False)
    return rank_eval_device(lists, users, tu, ti, su, si, n_users=n_users, ks=ks, device=dev)
