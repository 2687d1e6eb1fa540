"""The host definitions of sparrowrecsys_amd/item2vec.py (sequences, vocabulary, walks, the skip-gram trainer) and the argument checks
of the C ABI; no GPU.  The device is held to these definitions in tests/test_gpu_item2vec.py."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import item2vec as IV
from tests import item2vec_cases as K

F = np.float32


def _words(a):
    return [hex(w) for w in np.asarray(a, dtype=np.float32).view(np.uint32).ravel().tolist()]


def test_a_hand_worked_round():
    """Corpus A B A, one sentence, D = 2, window 1 (so no shrink), lr 0.5, one round of 3: V = 2, both codes one bit (A = 1, B = 0),
    one node.  syn1 starts at zero, so every first term has f = 0, table entry 498; the second context of the middle position meets
    the increment of the first."""
    vocab = IV.vocabulary_host([2, 1], 1)
    assert vocab.ids.tolist() == [0, 1] and vocab.code_len.tolist() == [1, 1] and vocab.codes[:, 0].tolist() == [1, 0] and vocab.points[:, 0].tolist() == [0, 0]
    corpus = IV.corpus_host([0, 3], [0, 1, 0], vocab, 2)
    xa, xb = np.array([0.5, -0.25], dtype=F), np.array([1.0, 0.75], dtype=F)
    got = IV.skipgram_host(corpus, vocab, D=2, window=1, iters=1, lr=0.5, round=3, init=np.stack([xa, xb]))
    table = IV.exp_table()
    alpha = F(0.5)                                                               # done = 0
    t0 = table[int((F(0.0) + F(6.0)) * F(83.0))]
    assert int((F(0.0) + F(6.0)) * F(83.0)) == 498
    g_a, g_b = ((F(1) - F(1)) - t0) * alpha, ((F(1) - F(0)) - t0) * alpha
    e0 = g_a * xb                                                                # position 0: centre A, context B; neu = g * (0 + 0) = 0
    inc = g_b * xa                                                               # position 1: centre B, context 0 (A) ...
    s = F(0) + inc                                                               # ... context 2 (A): syn1 + inc1
    f = (F(0) + xa[0] * s[0]) + xa[1] * s[1]
    assert -6 < f < 6
    g2 = ((F(1) - F(0)) - table[int((f + F(6.0)) * F(83.0))]) * alpha
    neu2 = F(0) + g2 * s
    e1 = inc + g2 * xa
    e2 = g_a * xb                                                                # position 2: as position 0
    node = F(0) + (((F(0) + e0) + e1) + e2)
    a_new = xa + ((np.zeros(2, dtype=F) + np.zeros(2, dtype=F)) + neu2)          # emissions (1, 0) = 0 and (1, 2) = neu2
    assert got.vectors[0].tobytes() == a_new.tobytes() and got.vectors[1].tobytes() == xb.tobytes()
    assert got.syn1[0].tobytes() == node.tobytes() and not got.syn1[1].any()
    assert _words(got.vectors[0]) == ["0x3f07e6d8", "0xbe87e6d8"] and _words(got.syn1[0]) == ["0xbe7b644c", "0xbefd4fee"]


def _sequential(corpus, vocab, D, window, iters, lr, seed, init, row_cap=32):
    """round = 1 as a plain loop over positions, scalars only."""
    word, lo, hi = corpus
    syn0, syn1, table, N = np.array(init, dtype=F), np.zeros((len(vocab.ids), D), dtype=F), IV.exp_table(), len(word)
    for it in range(iters):
        for k in range(N):
            if hi[k] - lo[k] < 2:
                continue
            alpha = IV.round_alpha(lr, it * N + k, N, iters)
            w = int(word[k])
            reach = window - int(IV.shrink(seed, it, np.array([k]), window)[0])
            inc1 = {}
            add0 = {}
            for c in range(max(int(lo[k]), k - reach), min(int(hi[k]) - 1, k + reach) + 1):
                if c == k:
                    continue
                x = syn0[word[c]].copy()
                neu = np.zeros(D, dtype=F)
                for d in range(int(vocab.code_len[w])):
                    node = int(vocab.points[w, d])
                    s = syn1[node] + inc1.get(d, np.zeros(D, dtype=F))
                    f = F(0)
                    for i in range(D):
                        f = f + x[i] * s[i]
                    if -6 < f < 6:
                        g = ((F(1) - F(vocab.codes[w, d])) - table[int((f + F(6)) * F(83))]) * alpha
                        neu = neu + g * s
                        inc1[d] = inc1.get(d, np.zeros(D, dtype=F)) + g * x
                add0.setdefault(int(word[c]), []).append(neu)
            for row, parts in add0.items():
                total = np.zeros(D, dtype=F)
                for e in parts:
                    total = total + e
                syn0[row] = syn0[row] + total
            for d in range(int(vocab.code_len[w])):
                syn1[int(vocab.points[w, d])] = syn1[int(vocab.points[w, d])] + (np.zeros(D, dtype=F) + inc1.get(d, np.zeros(D, dtype=F)))
    return syn0, syn1


def test_round_one_is_the_sequential_loop():
    off, items = K.sequences([9, 1, 14, 2, 30, 6], 7, seed=2)
    vocab = IV.vocabulary_host(np.bincount(items, minlength=7), 5)
    corpus = IV.corpus_host(off, items, vocab, 7, max_sentence=10)
    init = IV.init_vectors(len(vocab.ids), 3, 4) * F(8)
    with np.errstate(all="ignore"):
        want0, want1 = _sequential(corpus, vocab, 3, 2, 2, 0.05, 9, init)
    got = IV.skipgram_host(corpus, vocab, D=3, window=2, iters=2, lr=0.05, round=1, seed=9, init=init)
    assert got.vectors.tobytes() == want0.tobytes() and got.syn1.tobytes() == want1.tobytes()
    assert IV.skipgram_host(corpus, vocab, D=3, window=2, iters=2, lr=0.05, round=5, seed=9, init=init).vectors.tobytes() != want0.tobytes()


def test_huffman_tables_of_a_hand_built_tree():
    """Counts 5 3 2 1 (items 3 0 2 1): 1 + 2 -> node 0 (3); node 0 + 3 -> node 1 (6), the tie going to the node; 5 + node 1 -> the root."""
    v = IV.vocabulary_host([3, 1, 2, 5, 0], 1)
    assert v.ids.tolist() == [3, 0, 2, 1] and v.counts.tolist() == [5, 3, 2, 1] and v.code_len.tolist() == [1, 2, 3, 3]
    assert v.codes[0, :1].tolist() == [0] and v.codes[1, :2].tolist() == [1, 1] and v.codes[2, :3].tolist() == [1, 0, 1] and v.codes[3, :3].tolist() == [1, 0, 0]
    assert v.points[0, :1].tolist() == [2] and v.points[1, :2].tolist() == [2, 1] and v.points[2, :3].tolist() == [2, 1, 0] and v.points[3, :3].tolist() == [2, 1, 0]
    assert IV.vocabulary_host([4, 9, 9, 5], 5).ids.tolist() == [1, 2, 3]              # min_count, then equal counts by ascending id
    assert len(IV.vocabulary_host([7], 5).ids) == 1 and IV.vocabulary_host([7], 5).code_len.tolist() == [0]


def test_a_code_longer_than_40_bits_is_an_error():
    fib = [1, 1]
    while len(fib) < 42:
        fib.append(fib[-1] + fib[-2])
    assert IV.vocabulary_host(fib[:41], 1).code_len.max() == 40
    with pytest.raises(ValueError, match="41 bits"):
        IV.vocabulary_host(fib, 1)


def test_sequences_keep_good_ratings_in_timestamp_then_input_order():
    user = [1, 0, 1, 1, 0, 1, 1]
    movie = [5, 4, 3, 2, 1, 0, 6]
    rating = [4.0, 3.5, 5.0, 3.0, 3.49, 4.5, 3.5]
    ts = [20, 7, 10, 5, 1, 10, 10]
    off, items, count = IV.sequences_host(user, movie, rating, ts, 3, 7)
    assert off.tolist() == [0, 1, 5, 5] and items.tolist() == [4, 3, 0, 6, 5] and count.tolist() == [1, 0, 0, 1, 1, 1, 1]
    with pytest.raises(ValueError, match="row 2"):
        IV.sequences_host(user, [5, 4, 7, 2, 1, 0, 6], rating, ts, 3, 7)
    with pytest.raises(ValueError, match="row 3.*not finite"):
        IV.sequences_host(user, movie, [4.0, 3.5, 5.0, np.nan, 3.49, 4.5, 3.5], ts, 3, 7)


def test_walk_thresholds_and_a_dead_end():
    """Sequences 1 2 1 3 | 2 4: pairs 1->2, 2->1, 1->3, 2->4; rows 1: {2: 1, 3: 1}, 2: {1: 1, 4: 1}; total 4; 3 and 4 have no successor."""
    tr = IV.transitions_host([0, 4, 6], [1, 2, 1, 3, 2, 4], 5)
    assert tr[0].tolist() == [0, 0, 2, 4, 4, 4] and tr[1].tolist() == [2, 3, 1, 4] and tr[2].tolist() == [1, 1, 1, 1] and tr[3].tolist() == [0, 2, 2, 0, 0] and tr[4] == 4
    top = (1 << 64) - 1
    assert IV.mulhi64(np.array([0, top, 1 << 63], dtype=np.uint64), 4).tolist() == [0, 3, 2]
    low = IV.walks_host(tr, 1, 4, words=lambda i, s: 0)                           # t = 0 everywhere: 1 -> 2 -> 1 -> 2
    high = IV.walks_host(tr, 1, 4, words=lambda i, s: top)                        # t = total - 1: starts at 2, takes its last next, 4: a dead end
    mid = IV.walks_host(tr, 2, 4, words=lambda i, s: (1 << 63) if s == 0 else (top if i else 0))   # t = 2: the first pair of row 2
    assert low[1].tolist() == [1, 2, 1, 2] and high[0].tolist() == [0, 2] and high[1].tolist() == [2, 4]
    assert mid[0].tolist() == [0, 4, 6] and mid[1].tolist() == [2, 1, 2, 1, 2, 4]
    again = IV.walks_host(tr, 50, 6, seed=3)
    assert IV.walks_host(tr, 50, 6, seed=3)[1].tolist() == again[1].tolist() != IV.walks_host(tr, 50, 6, seed=4)[1].tolist()
    assert IV.walks_host(IV.transitions_host([0, 1, 2], [1, 2], 3), 5, 4)[0].tolist() == [0] * 6   # no pair at all: empty walks


# docs/item2vec_results.md: round = 1 on the clustered corpus, seeds 0 .. 4
R1_LOSS = 0.49078331490936905                                                       # seed 0
R1_SPREAD = 0.4914841292493983 - 0.49029651846301786                                # the greatest less the least of the five


def test_the_default_round_stays_within_the_spread_of_round_one():
    loss, purity, top = K.clustered_fit(IV.DEFAULT_ROUND)
    assert IV.DEFAULT_ROUND == 512 and abs(loss - R1_LOSS) <= R1_SPREAD and purity >= 0.99 and top < 6


def test_plain_summing_at_4096_does_not():
    """Without the row cap the 4 096 updates of the root node in a round add up: its weights pass the table's range and stop learning."""
    loss, purity, top = K.clustered_fit(4096, row_cap=1 << 30)
    assert abs(loss - R1_LOSS) > 100 * R1_SPREAD and purity < 0.9 and top > 6
    assert K.clustered_fit(4096)[2] < 6                                             # the same rounds with the cap stay inside


# ---------------------------------------------------------------- the C ABI's checks (before any device call: host memory will do)

def _buf(n_bytes=256):
    a = np.zeros(n_bytes // 8 + 2, dtype=np.int64)
    return a, a.ctypes.data + (-a.ctypes.data) % 16


def _skip_args(**over):
    keep = [_buf(1 << 16) for _ in range(14)]
    a = [b[1] for b in keep]
    v = dict(off=a[0], items=a[1], n=6, n_seq=2, lut=a[2], n_items=4, V=3, N=5, code_len=a[3], codes=a[4], points=a[5], init=a[6], init_stride=4, exp=a[7], loss_t=a[8],
             D=4, window=2, iters=1, lr=0.025, round=3, row_cap=32, seed=0, max_sentence=1000, vectors=a[9], stride=4, syn1=a[10], loss=a[11], err=a[12], ws=a[13],
             ws_bytes=1 << 16, stream=None)
    v.update(over)
    return keep, list(v.keys()), list(v.values())


def test_skipgram_arguments_are_checked_before_any_device_call(lib):
    need = lib.sprk_skipgram_workspace_bytes(6, 2, 3, 5, 4, 2, 3)
    assert 0 < need <= 1 << 16 and need % 16 == 0
    bad = [dict(D=0), dict(D=65), dict(window=0), dict(window=17), dict(iters=-1), dict(lr=0.0), dict(lr=float("nan")), dict(lr=float("inf")), dict(round=0),
           dict(row_cap=0), dict(max_sentence=0), dict(n=-1), dict(n=1 << 31), dict(n_seq=0), dict(n_seq=-1), dict(V=-1), dict(V=0), dict(N=7), dict(N=-1),
           dict(n_items=-1), dict(stride=3), dict(init_stride=3), dict(off=None), dict(items=None), dict(lut=None), dict(code_len=None), dict(codes=None),
           dict(points=None), dict(init=None), dict(exp=None), dict(loss_t=None), dict(vectors=None), dict(syn1=None), dict(loss=None), dict(err=None), dict(ws=None),
           dict(ws_bytes=need - 1)]
    for over in bad:
        keep, names, args = _skip_args(**over)
        assert lib.sprk_skipgram_fit(*args) == L.EINVAL, over
        assert lib.sprk_last_error()
    for key, off in (("off", 2), ("items", 1), ("lut", 2), ("code_len", 1), ("points", 2), ("init", 2), ("exp", 1), ("loss_t", 4), ("vectors", 2), ("syn1", 1),
                     ("loss", 4), ("err", 4), ("ws", 8)):
        keep, names, args = _skip_args()
        args[names.index(key)] += off
        assert lib.sprk_skipgram_fit(*args) == L.EINVAL, key
    keep, names, args = _skip_args(ws_bytes=16)
    assert lib.sprk_skipgram_fit(*args) == L.EINVAL and (b"%d bytes" % need) in lib.sprk_last_error()
    for sizes in ((-1, 2, 3, 5, 4, 2, 3), (6, 0, 3, 5, 4, 2, 3), (6, 2, -1, 5, 4, 2, 3), (6, 2, 3, 7, 4, 2, 3), (6, 2, 3, 5, 0, 2, 3), (6, 2, 3, 5, 65, 2, 3),
                  (6, 2, 3, 5, 4, 17, 3), (6, 2, 3, 5, 4, 2, 0), (1 << 31, 2, 3, 5, 4, 2, 3), (1 << 30, 2, 3, 1 << 30, 4, 2, 3)):
        assert lib.sprk_skipgram_workspace_bytes(*sizes) == 0, sizes


def test_sequences_and_walks_arguments_are_checked_before_any_device_call(lib):
    keep = [_buf(4096) for _ in range(9)]
    a = [b[1] for b in keep]
    names = ("user", "movie", "rating", "ts", "n", "nu", "ni", "off", "items", "count", "err", "ws", "ws_bytes", "stream")
    base = dict(zip(names, (a[0], a[1], a[2], a[3], 5, 3, 4, a[4], a[5], a[6], a[7], a[8], 4096, None)))
    need = lib.sprk_item_sequences_workspace_bytes(5, 3, 4)
    assert 0 < need <= 4096 and need % 16 == 0
    for over in (dict(n=-1), dict(n=1 << 31), dict(nu=-1), dict(ni=-1), dict(user=None), dict(movie=None), dict(rating=None), dict(ts=None), dict(off=None), dict(items=None),
                 dict(count=None), dict(err=None), dict(ws=None), dict(ws_bytes=need - 1), dict(user=a[0] + 2), dict(ts=a[3] + 4), dict(off=a[4] + 1), dict(err=a[7] + 4),
                 dict(ws=a[8] + 8)):
        assert lib.sprk_item_sequences(*dict(base, **over).values()) == L.EINVAL, over
        assert lib.sprk_last_error()
    assert lib.sprk_item_sequences_workspace_bytes(-1, 3, 4) == 0 and lib.sprk_item_sequences_workspace_bytes(5, -1, 4) == 0
    names = ("off", "items", "n", "n_seq", "ni", "count", "length", "seed", "woff", "witems", "err", "ws", "ws_bytes", "stream")
    base = dict(zip(names, (a[0], a[1], 5, 2, 4, 6, 3, 0, a[2], a[3], a[7], a[8], 4096, None)))
    need = lib.sprk_item_walks_workspace_bytes(5, 2, 4, 6, 3)
    assert 0 < need <= 4096 and need % 16 == 0
    for over in (dict(n=-1), dict(n_seq=0), dict(ni=-1), dict(count=-1), dict(length=0), dict(count=1 << 30, length=4), dict(off=None), dict(items=None), dict(woff=None),
                 dict(witems=None), dict(err=None), dict(ws=None), dict(ws_bytes=need - 1), dict(items=a[1] + 2), dict(woff=a[2] + 1), dict(err=a[7] + 4), dict(ws=a[8] + 8)):
        assert lib.sprk_item_walks(*dict(base, **over).values()) == L.EINVAL, over
        assert lib.sprk_last_error()
    assert lib.sprk_item_walks_workspace_bytes(5, 2, 4, 6, 0) == 0 and lib.sprk_item_walks_workspace_bytes(5, 0, 4, 6, 3) == 0


def test_fit_checks_its_parameters_and_needs_a_device():
    for kw in (dict(D=0), dict(D=65), dict(window=0), dict(iters=-1), dict(lr=0.0), dict(round=0), dict(row_cap=0), dict(max_sentence=0)):
        with pytest.raises(ValueError):
            IV.fit({}, **kw)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            IV.fit(K.ratings())
