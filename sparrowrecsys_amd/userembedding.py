"""User embeddings from ratings and item embeddings, and recommendations from them, without Spark.

The reference's embedding route has three stages: item embeddings (``item2vecEmb.csv``), user embeddings built from those and the
ratings (``Embedding.generateUserEmb``, Embedding.scala:53-101, which writes ``userEmb.csv``), and the "emb" ranker and recall over
them (``ranker.EmbRanker``).  This module is the second stage: :func:`user_emb_host` is the DEFINITION, in numpy, and :func:`build`
computes the same bits on the device (``sprk_user_emb``, csrc/k_user_emb.h).  The rules:

* Per user, ``movieCount`` is the number of the user's rating rows, whether or not the movie has an embedding; ``rating`` and
  ``timestamp`` are not read and nothing is filtered.
* ``acc`` is a float32 vector that starts at ``+0.0``.  The Scala folds with ``foldRight`` over the user's rows in file order, so the
  sum runs from the user's LAST row in the input to the first: ``acc = acc + emb[movie]``, one float32 add per element per row.  The
  sum is not associative in float32: the order is part of the definition.
* A row whose movie has no embedding, or lies outside the table, is skipped -- no zero row is added; a table row with ``has == 0`` may
  hold anything -- but still counts in ``movieCount``.
* ``userEmb = acc / (float)movieCount``, an IEEE float32 division.  A user with at least one rating gets a vector, all zeros if none
  of the movies has an embedding (the ranker then gives NaN, as Java does); a user with no rating gets none.

``mode="sum"`` is the PySpark twin (Embedding.py:166-183): it inner-joins on the movies that have an embedding, sums and does not
divide, and writes nothing for a user with no such movie; ``count`` is then the number of joined rows.  Its ``reduceByKey`` leaves the
order open: it is defined here to be the Scala's.  In both modes ``has = count > 0``.

Parity with the reference: it ships no ``ratings.csv``, so the result is pinned by this definition and a hand-worked user
(tests/userembedding_cases.py), as for feature engineering.  Java's text form of a float is not reproduced: :meth:`UserEmbeddings.save`
writes numpy's shortest round-trip form, which ``ranker.load_emb_file`` reads back to the same bits.
"""
from __future__ import annotations

from typing import Mapping, Optional

import numpy as np

from . import featureeng as FE

MODES = {"mean": 0, "sum": 1}
MAX_D = 1024
_ID_LIMIT = (1 << 31) - 1


def _mode(mode) -> int:
    if mode not in MODES:
        raise ValueError("mode = %r (\"mean\" = the Scala, \"sum\" = the PySpark twin)" % (mode,))
    return MODES[mode]


def user_emb_host(user_id, movie_row, item_emb, item_has, n_users: int, mode: str = "mean"):
    """The definition (module docstring).  ``user_id`` and ``movie_row`` (the item table's row of the rated movie; outside
    ``[0, n_items)`` = no embedding) are integer columns of one length, in file order; ``item_emb [n_items, D]`` float32, ``item_has
    [n_items]``.  -> ``(emb [n_users, D] float32, has [n_users] uint8, count [n_users] int32)``.  A ``user_id`` outside ``[0, n_users)``
    raises ``ValueError`` naming the first such row."""
    m = _mode(mode)
    u, r = np.asarray(user_id).astype(np.int64), np.asarray(movie_row).astype(np.int64)
    emb, has = np.asarray(item_emb, dtype=np.float32), np.asarray(item_has)
    if u.ndim != 1 or u.shape != r.shape:
        raise ValueError("the ratings columns differ in length")
    if emb.ndim != 2 or has.shape != emb.shape[:1] or not 1 <= emb.shape[1] <= MAX_D:
        raise ValueError("item_emb must be [n_items, D] with 1 <= D <= %d and item_has [n_items]" % MAX_D)
    if not 0 <= n_users < _ID_LIMIT:
        raise ValueError("n_users outside [0, 2^31 - 1)")
    bad = (u < 0) | (u >= n_users)
    if bad.any():
        raise ValueError(FE._error_message(FE.ERR_USER, int(np.flatnonzero(bad)[0])))
    inside = (r >= 0) & (r < len(has))
    ok = inside & (has[np.where(inside, r, 0)] != 0) if len(has) else np.zeros(len(r), dtype=bool)
    uo, ro = u[ok][::-1], r[ok][::-1]
    acc = np.zeros((n_users, emb.shape[1]), dtype=np.float32)
    np.add.at(acc, uo, emb[ro])                              # unbuffered: one float32 add per row, in the order given
    count = np.bincount(u if m == 0 else u[ok], minlength=n_users).astype(np.int32)
    if m == 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = np.where(count[:, None] > 0, acc / count.astype(np.float32)[:, None], np.float32(0)).astype(np.float32)
    return acc, (count > 0).astype(np.uint8), count


def _format_row(v) -> str:
    return " ".join(str(x) for x in np.asarray(v, dtype=np.float32))


class UserEmbeddings:
    """What :func:`build` returns: ``table [n_users, D]`` float32, ``has [n_users]`` uint8 and ``count [n_users]`` int32, row = userId --
    device tensors from :func:`build`, numpy arrays when made from :func:`user_emb_host`'s result."""

    def __init__(self, table, has, count, mode: str = "mean"):
        self.table, self.has, self.count, self.mode = table, has, count, mode
        self.n_users, self.D = int(table.shape[0]), int(table.shape[1])

    def to_host(self):
        """``(emb, has, count)`` as numpy arrays: :func:`user_emb_host`'s result, bit for bit."""
        return tuple(np.ascontiguousarray(FE._host_column(x)) for x in (self.table, self.has, self.count))

    def vector(self, user_id: int) -> Optional[np.ndarray]:
        """The user's vector, or None for a user without one (``DataManager.getUserById(..).getEmb() == null``)."""
        u = int(user_id)
        if not 0 <= u < self.n_users or not int(self.has[u]):
            return None
        return np.array(FE._host_column(self.table[u]), dtype=np.float32)

    def save(self, path: str) -> int:
        """``userEmb.csv``: one ``id:f f f ...`` line per user with ``has``, in id order; -> the number of lines.  Every float is numpy's
        shortest form that reads back to the same float32 (``ranker.load_emb_file`` returns the bits written)."""
        emb, has, _ = self.to_host()
        users = np.flatnonzero(has)
        with open(path, "w") as f:
            for u in users.tolist():
                f.write("%d:%s\n" % (u, _format_row(emb[u])))
        return len(users)

    def recommend(self, ranker, users, size: int, largest: bool = True) -> list:
        """The reference's "emb" recommendation for many users at once: for every id of ``users`` the ``size`` movie ids of the whole
        table closest to the user's vector, best first (``largest=False``: the least similar first) -- one ``ranker.topk`` call on
        ``table[users]`` / ``has[users]`` where they lie, and one copy of the rows to the host.  A user without an embedding (no rating,
        or an id outside the table) gets ``[]``; ``size`` is clamped to the table and to topk's 1024."""
        import torch
        ids = np.asarray(list(users), dtype=np.int64)
        k = max(0, min(int(size), len(ranker.ids), 1024))
        if len(ids) == 0 or k == 0 or self.n_users == 0:
            return [[] for _ in ids]
        dev = ranker.device
        at = torch.from_numpy(ids).to(dev)
        inside = (at >= 0) & (at < self.n_users)
        at = torch.where(inside, at, torch.zeros_like(at))
        table, has = torch.as_tensor(self.table).to(dev), torch.as_tensor(self.has).to(dev)
        q_has = has[at] * inside.to(has.dtype)
        _, rows = ranker.topk(table[at], k, query_has=q_has, largest=largest)
        got = torch.cat([rows.to(torch.int64), q_has.to(torch.int64)[:, None]], dim=1).cpu().numpy()     # the one copy
        return [ranker.ids[row[:k]].tolist() if row[k] else [] for row in got]


def _id_columns(ratings, dev):
    """-> userId, movieId as int64 device tensors (tensors on the device are used where they are)."""
    import torch
    if isinstance(ratings, str):
        ratings = FE._read_csv_columns(ratings, ["userId", "movieId"])
    if not isinstance(ratings, Mapping) or "userId" not in ratings or "movieId" not in ratings:
        raise KeyError("ratings needs the columns 'userId' and 'movieId'")
    out = []
    for key in ("userId", "movieId"):
        col = ratings[key]
        if hasattr(col, "detach"):
            if col.dtype.is_floating_point:
                raise TypeError("userId and movieId must be integer tensors")
            t = col.detach().to(dev).to(torch.int64)
        else:
            a = np.asarray(col)
            a = a.astype(np.int64) if a.dtype.kind in "iub" else np.array([int(v) for v in a.tolist()], dtype=np.int64)
            t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        if t.ndim != 1:
            raise ValueError("%s must be a column" % key)
        out.append(t)
    if out[0].numel() != out[1].numel():
        raise ValueError("the ratings columns differ in length")
    if out[0].numel() >= _ID_LIMIT:
        raise ValueError("at most 2^31 - 2 ratings")
    return out


def user_emb_device(user_id, item_row, item_emb, item_has, n_users: int, mode: str = "mean", D: Optional[int] = None, user_stride: Optional[int] = None):
    """``sprk_user_emb`` on device tensors, enqueued on the current stream; no synchronisation.  ``user_id`` / ``item_row`` int32 ``[n]``,
    ``item_emb [n_items, item_stride]`` float32 of which ``D`` (default: all) columns are read, ``item_has [n_items]`` uint8.
    -> ``(emb [n_users, user_stride], has, count, error word)``: tensors; the error word (int64, -1 = none) is the caller's to read."""
    import ctypes as C

    import torch

    from . import _lib as L
    lib = L.load_library()
    dev = item_emb.device
    D = int(item_emb.shape[1]) if D is None else int(D)
    user_stride = D if user_stride is None else int(user_stride)
    n, n_items = int(user_id.numel()), int(item_emb.shape[0])
    for t, dt in ((user_id, torch.int32), (item_row, torch.int32), (item_emb, torch.float32), (item_has, torch.uint8)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError("user_emb_device takes contiguous int32 / int32 / float32 / uint8 tensors on one device")
    with torch.cuda.device(dev):
        # (one spare row each: an empty table still has an address)
        emb = torch.zeros((n_users + 1, max(user_stride, 1)), dtype=torch.float32, device=dev)
        has = torch.zeros(n_users + 1, dtype=torch.uint8, device=dev)
        count = torch.zeros(n_users + 1, dtype=torch.int32, device=dev)
        word = torch.full((1,), -1, dtype=torch.int64, device=dev)                 # the error word, ~0
        ws_bytes = lib.sprk_user_emb_workspace_bytes(n, n_users)
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)   # (torch's allocations are 512-byte aligned)
        p = lambda x: C.c_void_p(x.data_ptr())
        L.check(lib.sprk_user_emb(p(user_id), p(item_row), n, n_users, p(item_emb), p(item_has), n_items, D, int(item_emb.stride(0)) if n_items else D,
                                  _mode(mode), p(emb), user_stride, p(has), p(count), p(word), p(ws), ws.numel() * 8,
                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return emb[:n_users], has[:n_users], count[:n_users], word


def build(ratings, ranker, n_users: Optional[int] = None, mode: str = "mean", device=None) -> UserEmbeddings:
    """User embeddings on the device.  ``ratings``: a CSV path or columns ``{userId, movieId, ..}``, numpy arrays or device tensors
    (``rating`` and ``timestamp`` are not read); ``ranker``: the :class:`~sparrowrecsys_amd.ranker.EmbRanker` that holds the item
    embeddings -- ``movieId`` becomes its table row on the device, through a dense lookup table built once from ``ranker.ids``
    (a movie the ranker does not know has no embedding).  ``n_users`` sizes the table (default: the greatest id + 1, one reduction).
    Errors are the ``ValueError`` of :func:`user_emb_host`.  One host synchronisation, the error word -- and a second, the reduction
    that finds the greatest id, when ``n_users`` is not given."""
    import torch
    _mode(mode)
    if not torch.cuda.is_available():
        raise RuntimeError("userembedding.build needs a HIP device: no HIP device is visible (user_emb_host is the host definition)")
    dev = ranker.device if device is None else torch.device(device)
    u, m = _id_columns(ratings, dev)
    # (an id beyond int32 must not wrap into range: it becomes -1, which the kernel reports)
    u32 = torch.where((u < 0) | (u >= _ID_LIMIT), torch.full_like(u, -1), u).to(torch.int32).contiguous()
    if n_users is None:
        n_users = max(int(u32.max()) + 1, 0) if u32.numel() else 0
    if not 0 <= n_users < _ID_LIMIT:
        raise ValueError("n_users outside [0, 2^31 - 1)")
    lut = ranker.row_lut().to(dev)                                                  # [greatest movie id + 2] int32, -1 = not in the table
    rows = lut[torch.where((m < 0) | (m >= lut.numel() - 1), torch.full_like(m, lut.numel() - 1), m)].contiguous()
    table = ranker.table.to(dev)
    emb, has, count, word = user_emb_device(u32, rows, table, ranker.has.to(dev), int(n_users), mode, D=ranker.D)
    err = int(word.cpu()[0])                                                        # the one synchronisation
    if err != -1:
        raise ValueError(FE._error_message((err >> 32) & 0xffffffff, err & 0xffffffff))
    return UserEmbeddings(emb, has, count, mode)
