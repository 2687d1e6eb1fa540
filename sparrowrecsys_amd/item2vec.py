"""Item2vec from ratings, without Spark: rating sequences, random walks and a skip-gram trainer with hierarchical softmax.

The reference's ``offline/spark/embedding/Embedding.scala`` builds per-user item sequences (``processItemSequence``), optionally
random walks over their transition graph (``generateTransitionMatrix`` / ``randomWalk``) and trains Spark ``Word2Vec`` on either
(``trainItem2vec``); the result is ``item2vecEmb.csv``.  Spark's trainer is one sequential SGD chain with a generator of its own and
cannot be reproduced bit for bit, so -- as for ALS -- the project defines its own trainer: :func:`skipgram_host` is the DEFINITION, in
numpy, and ``sprk_skipgram_fit`` (csrc/k_item2vec.h) computes the same bits on the device.  DESIGN.md section 5.11 has the rules, the
deviations from Spark and the experiment behind the row cap; in short:

* :func:`sequences_host` / ``sprk_item_sequences``: rows with ``rating >= 3.5f``, per user in ascending ``(timestamp, input row)``.
  (Scala sorts the timestamps as strings; here they are integers, and equal timestamps go by input row.)
* :func:`vocabulary_host`: the items of at least ``min_count`` occurrences by descending count then ascending id, and Spark's Huffman
  tables over that order.  On the host: one device -> host copy of the counts.
* :func:`transitions_host` / :func:`walks_host` / ``sprk_item_walks``: the graph route, in integers only.  (A counter-based generator,
  ascending-id order in place of Scala's hash-map order, integer thresholds in place of accumulated doubles.)
* :func:`skipgram_host`: an iteration walks the corpus in rounds of ``round`` consecutive positions; every position of a round reads
  the model as it stood when the round began, and the round's updates of one row are added in a fixed order and scaled by
  ``row_cap / n`` when more than ``row_cap`` of them meet.  ``round = 1`` is Spark's update order, except that a word repeated
  inside one window reads the snapshot.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Mapping, Optional

import numpy as np

from . import featureeng as FE

MAX_CODE = 40
MAX_D = 64
MAX_WINDOW = 16
EXP_TABLE_SIZE = 1000
MAX_EXP = 6.0
LOSS_CHUNK = 1024
DEFAULT_ROUND = 512
_ID_LIMIT = (1 << 31) - 1
ERR_USER, ERR_MOVIE, ERR_RATING, ERR_CORPUS = 1, 2, 3, 4
_M64 = (1 << 64) - 1

Vocabulary = namedtuple("Vocabulary", "ids counts code_len codes points")
Corpus = namedtuple("Corpus", "word lo hi")
SkipGram = namedtuple("SkipGram", "vectors syn1 loss")


def _error_message(kind: int, at: int) -> str:
    if kind in (ERR_USER, ERR_MOVIE):
        return FE._error_message(kind, at)
    if kind == ERR_RATING:
        return "ratings row %d: rating is not finite" % at
    if kind == ERR_CORPUS:
        return "the corpus holds %d words, not the number the vocabulary's counts give" % at
    return "error kind %d at %d" % (kind, at)


# ---------------------------------------------------------------- sequences

def sequences_host(user_id, movie_id, rating, timestamp, n_users: int, n_items: int):
    """-> ``(seq_offsets [n_users + 1] int32, seq_items [n_kept] int32, item_count [n_items] int32)``: the rows with ``rating >=
    3.5f``, per user in ascending ``(timestamp, input row)``; ``item_count`` = an item's occurrences among them.  Errors (an id out of
    range, a rating that is not finite; the first such row) raise ``ValueError``."""
    u, m = np.asarray(user_id).astype(np.int64), np.asarray(movie_id).astype(np.int64)
    r, t = np.asarray(rating, dtype=np.float32), np.asarray(timestamp).astype(np.int64)
    if u.ndim != 1 or not (u.shape == m.shape == r.shape == t.shape):
        raise ValueError("the ratings columns differ in length")
    n_users, n_items = int(n_users), int(n_items)
    if not 0 <= n_users < _ID_LIMIT or not 0 <= n_items < _ID_LIMIT:
        raise ValueError("n_users / n_items outside [0, 2^31 - 1)")
    kind = np.where((u < 0) | (u >= n_users), ERR_USER, np.where((m < 0) | (m >= n_items), ERR_MOVIE, np.where(~np.isfinite(r), ERR_RATING, 0)))
    if kind.any():
        keys = (kind[kind != 0].astype(np.int64) << 32) | np.flatnonzero(kind)
        k = int(keys.min())
        raise ValueError(_error_message(k >> 32, k & 0xffffffff))
    keep = np.flatnonzero(r >= np.float32(3.5))
    order = keep[np.lexsort((keep, t[keep], u[keep]))]
    off = np.concatenate([[0], np.cumsum(np.bincount(u[keep], minlength=n_users))]).astype(np.int32)
    return off, m[order].astype(np.int32), np.bincount(m[keep], minlength=n_items).astype(np.int32)


# ---------------------------------------------------------------- vocabulary

def vocabulary_host(item_count, min_count: int = 5) -> Vocabulary:
    """The items of at least ``min_count`` occurrences by descending count then ascending id (vocabulary index = that rank), and
    Spark's ``createBinaryTree`` over that order: ``code_len [V]`` int32, ``codes [V, 40]`` uint8 and ``points [V, 40]`` int32 (the
    inner nodes of the word's path from the root, root = ``V - 2``), unused entries 0.  A code longer than 40 raises."""
    cnt = np.asarray(item_count).astype(np.int64)
    ids = np.flatnonzero(cnt >= max(int(min_count), 1))
    ids = ids[np.lexsort((ids, -cnt[ids]))]
    V = len(ids)
    code_len = np.zeros(V, dtype=np.int32)
    codes = np.zeros((V, MAX_CODE), dtype=np.uint8)
    points = np.zeros((V, MAX_CODE), dtype=np.int32)
    if V >= 2:
        count = [int(c) for c in cnt[ids]] + [10 ** 9] * (V + 1)
        binary, parent = [0] * (2 * V + 1), [0] * (2 * V + 1)
        pos1, pos2 = V - 1, V
        for a in range(V - 1):
            pick = []
            for _ in range(2):
                if pos1 >= 0 and count[pos1] < count[pos2]:
                    pick.append(pos1); pos1 -= 1
                else:
                    pick.append(pos2); pos2 += 1
            count[V + a] = count[pick[0]] + count[pick[1]]
            parent[pick[0]] = parent[pick[1]] = V + a
            binary[pick[1]] = 1
        for a in range(V):
            code, point, b = [], [], a
            while b != 2 * V - 2:
                code.append(binary[b]); point.append(b); b = parent[b]
            i = len(code)
            if i > MAX_CODE:
                raise ValueError("item %d: its Huffman code has %d bits, more than %d" % (int(ids[a]), i, MAX_CODE))
            code_len[a] = i
            path = [V - 2] + [p - V for p in point[::-1]]           # root first; the last entry is the word itself and is not a node
            codes[a, :i] = code[::-1]
            points[a, :i] = path[:i]
    return Vocabulary(ids.astype(np.int64), cnt[ids].astype(np.int64), code_len, codes, points)


# ---------------------------------------------------------------- the graph route (host definition)

def mix64(x):
    """The 64-bit finaliser every counter-based draw here goes through (splitmix64's), on uint64 arrays."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _counter(seed: int, a, b):
    """``mix64(mix64(seed + 0x9E3779B97F4A7C15 * (a + 1)) ^ b)`` (mod 2^64)."""
    with np.errstate(over="ignore"):
        s = np.uint64(int(seed) & _M64) + np.uint64(0x9E3779B97F4A7C15) * (np.asarray(a, dtype=np.uint64) + np.uint64(1))
        return mix64(mix64(s) ^ np.asarray(b, dtype=np.uint64))


def mulhi64(w, n):
    """floor(w * n / 2^64) for uint64 ``w`` and a non-negative integer ``n`` < 2^63."""
    return np.array([(int(x) * int(n)) >> 64 for x in np.atleast_1d(w)], dtype=np.int64)


def transitions_host(seq_offsets, seq_items, n_items: int):
    """Adjacent pairs ``(prev, next)`` of every sequence, counted by value, as CSR over ``prev``: -> ``(row_offsets [n_items + 1],
    next_id (ascending in a row), pair_count, row_total [n_items], total)``, int64."""
    off, items = np.asarray(seq_offsets, dtype=np.int64), np.asarray(seq_items, dtype=np.int64)
    inner = np.ones(max(len(items) - 1, 0), dtype=bool)
    ends = off[1:-1]
    inner[ends[(ends > 0) & (ends < len(items))] - 1] = False          # a pair does not span two sequences
    prev, nxt = items[:-1][inner], items[1:][inner]
    key, cnt = np.unique(prev * (int(n_items) + 1) + nxt, return_counts=True)
    p, q = key // (int(n_items) + 1), key % (int(n_items) + 1)
    row_total = np.bincount(p, weights=cnt, minlength=int(n_items)).astype(np.int64)
    row_off = np.concatenate([[0], np.cumsum(np.bincount(p, minlength=int(n_items)))]).astype(np.int64)
    return row_off, q.astype(np.int64), cnt.astype(np.int64), row_total, int(cnt.sum())


def walk_word(seed: int, walk, step):
    """The word walk ``walk`` draws at ``step`` (0 = its start)."""
    return _counter(seed, walk, step)


def walks_host(transitions, sample_count: int = 20000, sample_length: int = 10, seed: int = 0, words=None):
    """``sample_count`` walks of at most ``sample_length`` items.  Walk ``i`` starts at the first item, in ascending id, whose
    cumulative ``row_total`` exceeds ``mulhi64(word(i, 0), total)``; step ``s`` moves to the first ``next`` of the current item whose
    cumulative ``pair_count`` exceeds ``mulhi64(word(i, s), row_total[cur])``; an item without successors ends the walk.  ``words``
    (tests) replaces the generator: ``words(walk, step) -> uint64``.  -> ``(offsets [sample_count + 1] int32, items int32)``."""
    row_off, nxt, cnt, row_total, total = transitions
    draw = (lambda i, s: int(walk_word(seed, i, s))) if words is None else (lambda i, s: int(words(i, s)) & _M64)
    cum_rows = np.cumsum(row_total)
    cum_pairs = np.cumsum(cnt)
    out, offs = [], [0]
    for i in range(int(sample_count)) if total > 0 and sample_length > 0 else []:
        cur = int(np.searchsorted(cum_rows, (draw(i, 0) * total) >> 64, side="right"))
        out.append(cur)
        for s in range(1, int(sample_length)):
            if row_total[cur] == 0:
                break
            lo, hi = int(row_off[cur]), int(row_off[cur + 1])
            base = int(cum_pairs[lo - 1]) if lo else 0
            t = (draw(i, s) * int(row_total[cur])) >> 64
            cur = int(nxt[lo + int(np.searchsorted(cum_pairs[lo:hi] - base, t, side="right"))])
            out.append(cur)
        offs.append(len(out))
    if len(offs) == 1:
        offs = [0] * (int(sample_count) + 1)
    return np.asarray(offs, dtype=np.int32), np.asarray(out, dtype=np.int32)


# ---------------------------------------------------------------- the trainer's inputs

def init_vectors(V: int, D: int, seed: int = 0) -> np.ndarray:
    """``(default_rng(seed).random(float32) - 0.5) / D`` (Spark's generator is not reproduced)."""
    x = np.random.default_rng(seed).random((int(V), int(D)), dtype=np.float32)
    return ((x - np.float32(0.5)) / np.float32(D)).astype(np.float32)


def exp_table() -> np.ndarray:
    """Spark's table: ``float32(e / (e + 1))``, ``e = exp((2 i / 1000 - 1) * 6)`` in doubles."""
    e = np.exp((2.0 * np.arange(EXP_TABLE_SIZE) / EXP_TABLE_SIZE - 1.0) * MAX_EXP)
    return (e / (e + 1.0)).astype(np.float32)


def loss_table() -> np.ndarray:
    """``[2, 1000]`` float64: row 0 = ``-log s``, row 1 = ``-log(1 - s)`` with ``s`` = :func:`exp_table`'s entry widened: the loss of a
    term whose code bit is 0 / 1 and whose ``f`` falls on that entry."""
    s = exp_table().astype(np.float64)
    return np.stack([-np.log(s), -np.log1p(-s)])


def table_index(f: np.ndarray) -> np.ndarray:
    """``(int)((f + 6) * 83)`` in float32 -- 83 is Spark's ``EXP_TABLE_SIZE / MAX_EXP / 2.0`` with its integer division, 1000 / 6 =
    166.  Only meaningful where ``-6 < f < 6``; 0 elsewhere."""
    ok = (f > -MAX_EXP) & (f < MAX_EXP)
    with np.errstate(all="ignore"):
        v = (np.where(ok, f, np.float32(0)).astype(np.float32) + np.float32(MAX_EXP)) * np.float32(83.0)
    return np.where(ok, v.astype(np.int64), 0)


def corpus_host(seq_offsets, seq_items, vocab: Vocabulary, n_items: int, max_sentence: int = 1000) -> Corpus:
    """Out-of-vocabulary items dropped, every sequence cut into sentences of at most ``max_sentence`` words.  -> per global position
    its vocabulary index ``word`` and the bounds ``[lo, hi)`` of its sentence."""
    off, items = np.asarray(seq_offsets, dtype=np.int64), np.asarray(seq_items, dtype=np.int64)
    if ((items < 0) | (items >= int(n_items))).any():
        at = int(np.flatnonzero((items < 0) | (items >= int(n_items)))[0])
        raise ValueError(_error_message(ERR_MOVIE, at))
    lut = np.full(int(n_items) + 1, -1, dtype=np.int64)
    lut[vocab.ids] = np.arange(len(vocab.ids))
    v = lut[items]
    kept = v >= 0
    pos = np.concatenate([[0], np.cumsum(kept)])                     # the position of every kept item; pos[-1] = N
    seq = np.searchsorted(off, np.arange(len(items)), side="right") - 1
    fs, fe = pos[off[seq]], pos[off[seq + 1]]
    q = pos[:-1] - fs
    lo = fs + q // int(max_sentence) * int(max_sentence)
    hi = np.minimum(fe, lo + int(max_sentence))
    return Corpus(v[kept].astype(np.int32), lo[kept].astype(np.int64), hi[kept].astype(np.int64))


def shrink(seed: int, iteration: int, k, window: int) -> np.ndarray:
    """The window shrink ``b`` in ``[0, window)`` of position ``k`` in ``iteration``: ``(word >> 33) % window``."""
    return ((_counter(seed, iteration, k) >> np.uint64(33)) % np.uint64(window)).astype(np.int64)


def round_alpha(lr: float, done: int, N: int, iters: int) -> np.float32:
    return np.float32(max(float(lr) * (1.0 - float(done) / float(N * iters + 1)), float(lr) * 1e-4))


def _dot(x, s):
    """The float32 dot of the rows of ``x`` and ``s`` in index order from ``0.0f``, every product and sum rounded on its own."""
    p = np.zeros((x.shape[0], x.shape[1] + 1), dtype=np.float32)
    p[:, 1:] = x * s
    return np.add.accumulate(p, axis=1, dtype=np.float32)[:, -1]


def _check_fit(D, window, iters, lr, round, row_cap, max_sentence):
    if not 1 <= int(D) <= MAX_D:
        raise ValueError("D = %r outside [1, %d]" % (D, MAX_D))
    if not 1 <= int(window) <= MAX_WINDOW:
        raise ValueError("window = %r outside [1, %d]" % (window, MAX_WINDOW))
    if int(iters) < 0:
        raise ValueError("iters = %r is negative" % (iters,))
    if not (np.isfinite(lr) and lr > 0):
        raise ValueError("lr = %r must be finite and > 0" % (lr,))
    if int(round) < 1 or int(row_cap) < 1 or int(max_sentence) < 1:
        raise ValueError("round, row_cap and max_sentence must be >= 1")


def skipgram_host(corpus: Corpus, vocab: Vocabulary, D: int = 10, window: int = 5, iters: int = 10, lr: float = 0.025,
                  round: int = DEFAULT_ROUND, row_cap: int = 32, seed: int = 0, init=None, trace: Optional[list] = None) -> SkipGram:
    """The definition (module docstring).  -> ``(vectors [V, D] float32, syn1 [V, D] float32 (row = inner node;
    the last row is no node and stays zero), loss float64)``.  ``trace`` (tests): a list that receives the table indices of the terms
    that were not skipped, one array per (round, context offset, depth)."""
    _check_fit(D, window, iters, lr, round, row_cap, 1)
    word, lo, hi = np.asarray(corpus.word, dtype=np.int64), np.asarray(corpus.lo, dtype=np.int64), np.asarray(corpus.hi, dtype=np.int64)
    V, N, D, W, R, C = len(vocab.ids), len(word), int(D), int(window), int(round), int(row_cap)
    syn0 = init_vectors(V, D, seed) if init is None else np.array(init, dtype=np.float32)
    if syn0.shape != (V, D):
        raise ValueError("init must be [V, D]")
    syn1 = np.zeros((V, D), dtype=np.float32)
    table = exp_table()
    code_len, codes, points = vocab.code_len.astype(np.int64), vocab.codes, vocab.points.astype(np.int64)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        for it in range(int(iters)):
            for r0 in range(0, N, R):
                k = np.arange(r0, min(N, r0 + R))
                live = k[hi[k] - lo[k] >= 2]                               # a position without contexts emits nothing
                if not len(live):
                    continue
                alpha = round_alpha(lr, it * N + r0, N, iters)
                w, L = word[live], code_len[word[live]]
                reach = W - shrink(seed, it, live, W)
                inc1 = np.zeros((len(live), int(L.max()) if len(L) else 0, D), dtype=np.float32)
                base1 = syn1[points[w][:, :inc1.shape[1]]]                 # the path rows of the snapshot
                rec0 = []                                                  # (row, centre, context, emission)
                for o in [o for o in range(-W, W + 1) if o]:
                    c = live + o
                    ok = (np.abs(o) <= reach) & (c >= lo[live]) & (c < hi[live])
                    at = np.flatnonzero(ok)
                    if not len(at):
                        continue
                    x = syn0[word[c[at]]]
                    neu = np.zeros((len(at), D), dtype=np.float32)
                    for d in range(int(L[at].max())):
                        s = base1[at, d] + inc1[at, d]
                        f = _dot(x, s)
                        on = (d < L[at]) & (f > -MAX_EXP) & (f < MAX_EXP)
                        if trace is not None:
                            trace.append(table_index(f)[on])
                        g = ((one - codes[w[at], d].astype(np.float32)) - table[table_index(f)]) * alpha
                        g = g.astype(np.float32)[:, None]
                        neu = np.where(on[:, None], neu + g * s, neu)
                        inc1[at, d] = np.where(on[:, None], inc1[at, d] + g * x, inc1[at, d])
                    rec0.append((word[c[at]], live[at], c[at], neu))
                rows0 = np.concatenate([r[0] for r in rec0]); k0 = np.concatenate([r[1] for r in rec0])
                c0 = np.concatenate([r[2] for r in rec0]); e0 = np.concatenate([r[3] for r in rec0])
                _apply(syn0, rows0, k0, c0, e0, C)
                dd = np.arange(inc1.shape[1])
                sel = dd[None, :] < L[:, None]
                _apply(syn1, points[w][:, :inc1.shape[1]][sel], np.broadcast_to(live[:, None], sel.shape)[sel],
                       np.broadcast_to(dd[None, :], sel.shape)[sel], inc1[sel], C)
        loss = loss_host(corpus, vocab, syn0, syn1, W)
    return SkipGram(syn0, syn1, loss)


def _apply(table, rows, major, minor, emission, C):
    """Applies one round's emissions: per row they are added left to right from ``+0.0f`` in ascending ``(major, minor)``; ``row +=
    total`` for ``n <= C`` emissions, else ``row += total * ((float)C / (float)n)``."""
    order = np.lexsort((minor, major, rows))
    rows, emission = rows[order], emission[order]
    first = np.flatnonzero(np.concatenate([[True], rows[1:] != rows[:-1]]))
    n = np.diff(np.concatenate([first, [len(rows)]]))
    total = np.zeros((len(first), emission.shape[1]), dtype=np.float32)
    by_len = np.argsort(-n, kind="stable")
    neg = -n[by_len]
    for t in range(int(n.max())):
        sel = by_len[:np.searchsorted(neg, -t, side="left")]               # the rows of more than t emissions
        total[sel] = total[sel] + emission[first[sel] + t]
    scale = (np.float32(C) / n.astype(np.float32)).astype(np.float32)[:, None]
    ids = rows[first]
    table[ids] = np.where((n <= C)[:, None], table[ids] + total, table[ids] + total * scale)


def loss_host(corpus: Corpus, vocab: Vocabulary, syn0, syn1, window: int = 5) -> float:
    """The mean of ``-log sigma(+-f)`` over every (position, context at the full window, depth) term under ``(syn0, syn1)``: a term's
    loss is :func:`loss_table`'s entry at the term's table index (index 0 for ``f <= -6`` or NaN, 999 for ``f >= 6``); a position's
    terms are added in doubles by ascending (context, depth), the positions of each chunk of 1 024 in ascending order, then the chunks."""
    word, lo, hi = np.asarray(corpus.word, dtype=np.int64), np.asarray(corpus.lo, dtype=np.int64), np.asarray(corpus.hi, dtype=np.int64)
    N, W = len(word), int(window)
    if N == 0:
        return 0.0
    lt = loss_table()
    code_len, codes, points = vocab.code_len.astype(np.int64), vocab.codes, vocab.points.astype(np.int64)
    k = np.arange(N)
    L = code_len[word]
    pos_loss, terms = np.zeros(N), 0
    with np.errstate(all="ignore"):
        for o in [o for o in range(-W, W + 1) if o]:
            c = k + o
            at = np.flatnonzero((c >= lo) & (c < hi))
            if not len(at):
                continue
            x = syn0[word[c[at]]]
            for d in range(int(L[at].max()) if len(at) else 0):
                f = _dot(x, syn1[points[word[at], d]])
                idx = np.where(f >= MAX_EXP, EXP_TABLE_SIZE - 1, table_index(f))
                on = d < L[at]
                pos_loss[at] = pos_loss[at] + np.where(on, lt[codes[word[at], d].astype(np.int64), idx], 0.0)
                terms += int(on.sum())
    if terms == 0:
        return 0.0
    pad = np.zeros((N + LOSS_CHUNK - 1) // LOSS_CHUNK * LOSS_CHUNK)
    pad[:N] = pos_loss
    pad = pad.reshape(-1, LOSS_CHUNK)
    chunk = np.zeros(len(pad))
    for i in range(LOSS_CHUNK):
        chunk = chunk + pad[:, i]
    total = 0.0
    for v in chunk.tolist():
        total = total + v
    return float(total / float(terms))


def item2vec_host(user_id, movie_id, rating, timestamp, n_users: int, n_items: int, D: int = 10, window: int = 5, iters: int = 10,
                  lr: float = 0.025, round: int = DEFAULT_ROUND, row_cap: int = 32, seed: int = 0, min_count: int = 5,
                  max_sentence: int = 1000, init=None, graph: bool = False, sample_count: int = 20000, sample_length: int = 10):
    """The whole host chain: sequences (-> walks) -> vocabulary -> corpus -> :func:`skipgram_host`.  -> ``(vocab, SkipGram)``."""
    off, items, count = sequences_host(user_id, movie_id, rating, timestamp, n_users, n_items)
    if graph:
        off, items = walks_host(transitions_host(off, items, n_items), sample_count, sample_length, seed)
        count = np.bincount(items, minlength=int(n_items))
    vocab = vocabulary_host(count, min_count)
    corpus = corpus_host(off, items, vocab, n_items, max_sentence)
    return vocab, skipgram_host(corpus, vocab, D, window, iters, lr, round, row_cap, seed, init)


# ---------------------------------------------------------------- the device

def _need(t, dt, dev, what):
    if t.dtype != dt or not t.is_contiguous() or t.device != dev:
        raise ValueError("%s must be a contiguous %s tensor on %s" % (what, dt, dev))


def sequences_device(user_id, movie_id, rating, timestamp, n_users: int, n_items: int):
    """``sprk_item_sequences`` on device tensors (ids int32, rating float32, timestamp int64), enqueued on the current stream; no
    synchronisation.  -> ``(seq_offsets [n_users + 1] int32, seq_items [n] int32 of which seq_offsets[-1] are written, item_count
    [n_items] int32, error word)``."""
    import ctypes as C

    import torch

    from . import _lib as L
    lib = L.load_library()
    dev = rating.device
    n = int(user_id.numel())
    _need(user_id, torch.int32, dev, "user_id"); _need(movie_id, torch.int32, dev, "movie_id")
    _need(rating, torch.float32, dev, "rating"); _need(timestamp, torch.int64, dev, "timestamp")
    with torch.cuda.device(dev):
        off = torch.zeros(n_users + 1, dtype=torch.int32, device=dev)
        items = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        count = torch.zeros(n_items + 1, dtype=torch.int32, device=dev)
        word = torch.full((1,), -1, dtype=torch.int64, device=dev)
        ws_bytes = lib.sprk_item_sequences_workspace_bytes(n, n_users, n_items)
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        L.check(lib.sprk_item_sequences(p(user_id), p(movie_id), p(rating), p(timestamp), n, n_users, n_items, p(off), p(items), p(count),
                                        p(word), p(ws), ws.numel() * 8, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return off, items[:n], count[:n_items], word


def walks_device(seq_offsets, seq_items, n_items: int, sample_count: int = 20000, sample_length: int = 10, seed: int = 0,
                 n_seq_items: Optional[int] = None):
    """``sprk_item_walks`` on device tensors (int32), enqueued on the current stream; no synchronisation.  -> ``(walk_offsets
    [sample_count + 1] int32, walk_items [sample_count * sample_length] int32 of which walk_offsets[-1] are written, error word)``."""
    import ctypes as C

    import torch

    from . import _lib as L
    lib = L.load_library()
    dev = seq_items.device
    _need(seq_offsets, torch.int32, dev, "seq_offsets"); _need(seq_items, torch.int32, dev, "seq_items")
    if int(sample_count) < 0 or int(sample_length) < 1:
        raise ValueError("sample_count must be >= 0 and sample_length >= 1")
    n_seq = int(seq_offsets.numel()) - 1
    n = int(seq_items.numel()) if n_seq_items is None else int(n_seq_items)
    with torch.cuda.device(dev):
        woff = torch.zeros(int(sample_count) + 1, dtype=torch.int32, device=dev)
        items = torch.zeros(int(sample_count) * int(sample_length) + 1, dtype=torch.int32, device=dev)
        word = torch.full((1,), -1, dtype=torch.int64, device=dev)
        ws_bytes = lib.sprk_item_walks_workspace_bytes(n, n_seq, int(n_items), int(sample_count), int(sample_length))
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        L.check(lib.sprk_item_walks(p(seq_offsets), p(seq_items), n, n_seq, int(n_items), int(sample_count), int(sample_length), int(seed) & _M64,
                                    p(woff), p(items), p(word), p(ws), ws.numel() * 8, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return woff, items[:int(sample_count) * int(sample_length)], word


def skipgram_device(seq_offsets, seq_items, vocab: Vocabulary, n_items: int, D: int = 10, window: int = 5, iters: int = 10, lr: float = 0.025,
                    round: int = DEFAULT_ROUND, row_cap: int = 32, seed: int = 0, max_sentence: int = 1000, init=None,
                    stride: Optional[int] = None, n_seq_items: Optional[int] = None):
    """``sprk_skipgram_fit`` on device tensors, enqueued on the current stream; no synchronisation.  ``seq_offsets [n_seq + 1]`` /
    ``seq_items`` int32 (``n_seq_items`` of them; default all), ``init [V, >= D]`` float32 (numpy or tensor; default
    :func:`init_vectors`).  -> ``(vectors [V, stride], syn1 [V, D], loss [1] float64, error word)``: device tensors."""
    import ctypes as C

    import torch

    from . import _lib as L
    _check_fit(D, window, iters, lr, round, row_cap, max_sentence)
    lib = L.load_library()
    dev = seq_items.device
    _need(seq_offsets, torch.int32, dev, "seq_offsets"); _need(seq_items, torch.int32, dev, "seq_items")
    V, D = len(vocab.ids), int(D)
    n_seq = int(seq_offsets.numel()) - 1
    n = int(seq_items.numel()) if n_seq_items is None else int(n_seq_items)
    N = int(vocab.counts.sum())
    stride = D if stride is None else int(stride)
    if init is None:
        init = init_vectors(V, D, seed)
    init = (init.detach() if hasattr(init, "detach") else torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32))).to(dev)
    if init.dtype != torch.float32 or init.ndim != 2 or init.shape[0] != V or init.shape[1] < D or (V and init.stride(1) != 1):
        raise ValueError("init must be a float32 [V, >= D] table with unit column stride")
    lut = np.full(int(n_items) + 1, -1, dtype=np.int32)
    lut[vocab.ids] = np.arange(V, dtype=np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with torch.cuda.device(dev):
        t_lut, t_len, t_codes, t_points = up(lut), up(np.append(vocab.code_len, 0).astype(np.int32)), up(np.vstack([vocab.codes, np.zeros((1, MAX_CODE), np.uint8)])), \
            up(np.vstack([vocab.points, np.zeros((1, MAX_CODE), np.int32)]).astype(np.int32))
        t_exp, t_loss = up(exp_table()), up(loss_table())
        vectors = torch.zeros((V + 1, max(stride, 1)), dtype=torch.float32, device=dev)
        syn1 = torch.zeros((V + 1, D), dtype=torch.float32, device=dev)
        loss = torch.zeros(1, dtype=torch.float64, device=dev)
        word = torch.full((1,), -1, dtype=torch.int64, device=dev)
        ws_bytes = lib.sprk_skipgram_workspace_bytes(n, n_seq, V, N, D, int(window), int(round))
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        L.check(lib.sprk_skipgram_fit(p(seq_offsets), p(seq_items), n, n_seq, p(t_lut), int(n_items), V, N, p(t_len), p(t_codes), p(t_points),
                                      p(init) if V else p(vectors), int(init.stride(0)) if V else D, p(t_exp), p(t_loss),
                                      D, int(window), int(iters), float(lr), int(round), int(row_cap), int(seed) & _M64, int(max_sentence),
                                      p(vectors), stride, p(syn1), p(loss), p(word), p(ws), ws.numel() * 8,
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return vectors[:V], syn1[:V], loss, word


def _raise(word):
    err = int(word.cpu()[0])
    if err != -1:
        raise ValueError(_error_message((err >> 32) & 0xffffffff, err & 0xffffffff))


class Item2VecModel:
    """What :func:`fit` returns: ``ids [V]`` (numpy int64, the item of every row), ``vectors [V, D]`` / ``syn1 [V, D]`` float32 device
    tensors, ``loss`` (float) and the vocabulary."""

    def __init__(self, vocab: Vocabulary, vectors, syn1, loss: float):
        self.vocab, self.ids, self.vectors, self.syn1, self.loss = vocab, vocab.ids, vectors, syn1, float(loss)
        self.device = vectors.device
        self._ranker = None

    def to_host(self) -> SkipGram:
        return SkipGram(np.ascontiguousarray(FE._host_column(self.vectors)), np.ascontiguousarray(FE._host_column(self.syn1)), self.loss)

    def save(self, path: str) -> int:
        """``item2vecEmb.csv``: one ``id:v v v`` line per item, in vocabulary order.  -> the number of lines."""
        v = self.to_host().vectors
        with open(path, "w") as f:
            for i, row in zip(self.ids.tolist(), v):
                f.write("%d:%s\n" % (i, " ".join(str(x) for x in row)))               # (a float32's str round-trips)
        return len(v)

    def ranker(self):
        """An :class:`~sparrowrecsys_amd.ranker.EmbRanker` over the trained table."""
        if self._ranker is None:
            from .ranker import EmbRanker
            v = self.to_host().vectors
            self._ranker = EmbRanker({int(i): v[r] for r, i in enumerate(self.ids.tolist())}, device=str(self.device))
        return self._ranker

    def similar(self, ids, k: int = 10):
        """``findSynonyms``: for every item of ``ids`` the ``k`` items most similar to it by ``EmbRanker.topk``, the item itself left
        out.  -> a list of lists of item ids; an item outside the vocabulary gives an empty list."""
        rk = self.ranker()
        rows = rk.rows(ids)
        known = rows >= 0
        out = [[] for _ in rows]
        if known.any():
            kk = min(int(k) + 1, len(rk.ids))
            got = rk.topk(rk.table[rows[known].tolist()], kk)
            top = FE._host_column(got[1])                                            # (scores, rows)
            for at, r, line in zip(np.flatnonzero(known).tolist(), rows[known].tolist(), np.asarray(top)):
                out[at] = [int(rk.ids[j]) for j in line.tolist() if j >= 0 and j != r][:int(k)]
        return out

    def user_embeddings(self, ratings, n_users: Optional[int] = None, mode: str = "mean"):
        """:func:`sparrowrecsys_amd.userembedding.build` over the trained table."""
        from . import userembedding
        return userembedding.build(ratings, self.ranker(), n_users=n_users, mode=mode)


def _columns(ratings, dev):
    import torch

    from . import als
    if isinstance(ratings, str):
        ratings = FE._read_csv_columns(ratings, ["userId", "movieId", "rating", "timestamp"])
    u, m, r = als._columns(ratings, dev)
    if "timestamp" not in ratings:
        raise KeyError("ratings needs the column 'timestamp'")
    col = ratings["timestamp"]
    if hasattr(col, "detach"):
        t = col.detach().to(dev).to(torch.int64)
    else:
        a = np.asarray(col)
        a = a.astype(np.int64) if a.dtype.kind in "iub" else np.array([int(v) for v in a.tolist()], dtype=np.int64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if t.ndim != 1 or t.numel() != u.numel():
        raise ValueError("the ratings columns differ in length")
    return u, m, r, t.contiguous()


def fit(ratings, D: int = 10, window: int = 5, iters: int = 10, lr: float = 0.025, round: int = DEFAULT_ROUND, row_cap: int = 32,
        seed: int = 0, min_count: int = 5, max_sentence: int = 1000, init=None, graph: bool = False, sample_count: int = 20000,
        sample_length: int = 10, device=None, n_users: Optional[int] = None, n_items: Optional[int] = None) -> Item2VecModel:
    """Item2vec on the device.  ``ratings``: a CSV path or columns ``{userId, movieId, rating, timestamp}``, numpy arrays or device
    tensors.  ``graph = True`` trains on ``sample_count`` random walks of ``sample_length`` over the sequences' transition graph (the
    reference's ``graphEmb``) in place of the sequences.  Two host synchronisations: the item counts (the vocabulary and its Huffman tree are built on the host) and the error
    word with the loss.  Errors are the ``ValueError`` of the host definitions."""
    import torch
    _check_fit(D, window, iters, lr, round, row_cap, max_sentence)
    if not torch.cuda.is_available():
        raise RuntimeError("item2vec.fit needs a HIP device: no HIP device is visible (item2vec_host is the host definition)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    u, m, r, t = _columns(ratings, dev)
    if n_users is None:
        n_users = max(int(u.max()) + 1, 0) if u.numel() else 0
    if n_items is None:
        n_items = max(int(m.max()) + 1, 0) if m.numel() else 0
    if not 0 <= n_users < _ID_LIMIT or not 0 <= n_items < _ID_LIMIT:
        raise ValueError("n_users / n_items outside [0, 2^31 - 1)")
    off, items, count, word = sequences_device(u, m, r, t, int(n_users), int(n_items))
    host_count = count.cpu().numpy()                                               # the first synchronisation
    _raise(word)
    if graph:
        off, items, word = walks_device(off, items, int(n_items), sample_count, sample_length, seed, n_seq_items=int(host_count.sum()))
        total = int(off[-1].cpu())
        _raise(word)
        host_count = torch.bincount(items[:total].to(torch.int64), minlength=int(n_items)).cpu().numpy()   # (plumbing: the walks' item counts)
    vocab = vocabulary_host(host_count, min_count)
    vectors, syn1, loss, word = skipgram_device(off, items, vocab, int(n_items), D, window, iters, lr, round, row_cap, seed, max_sentence, init,
                                                n_seq_items=int(host_count.sum()))
    _raise(word)                                                                   # the second
    return Item2VecModel(vocab, vectors, syn1, float(loss.cpu()[0]))
