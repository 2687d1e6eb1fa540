"""Item2vec on the device (sprk_item_sequences / sprk_item_walks / sprk_skipgram_fit, csrc/k_item2vec.h) against its definitions in
sparrowrecsys_amd/item2vec.py: sequences, walks, vectors, syn1 and the loss byte for byte, with error word -1.  The host corpora hold
at most about 1 500 words and run 2 iterations; every host result is computed once per module."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import item2vec as IV
from tests import item2vec_cases as K

pytestmark = pytest.mark.gpu

FILL, GUARD_BYTES, GUARD_ROWS = 0xA5, 4096, 3
NU, NI = 40, 30


def _up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _is_fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def _dev_sequences(cols, n_users=NU, n_items=NI):
    off, items, cnt, word = IV.sequences_device(_up(cols["userId"], np.int32), _up(cols["movieId"], np.int32), _up(cols["rating"], np.float32),
                                                _up(cols["timestamp"], np.int64), n_users, n_items)
    off = off.cpu().numpy()
    return off, items.cpu().numpy()[:off[-1]], cnt.cpu().numpy(), int(word.cpu()[0])


def _host_sequences(cols, n_users=NU, n_items=NI):
    return IV.sequences_host(cols["userId"], cols["movieId"], cols["rating"], cols["timestamp"], n_users, n_items)


def _same(got, want, name):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (name, np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))[:8])


_HOST = {}


def _host_fit(key, off, items, n_items, min_count=5, max_sentence=1000, **kw):
    """skipgram_host on (off, items), once per key."""
    if key not in _HOST:
        vocab = IV.vocabulary_host(np.bincount(items, minlength=n_items), min_count)
        corpus = IV.corpus_host(off, items, vocab, n_items, max_sentence)
        _HOST[key] = (vocab, corpus, IV.skipgram_host(corpus, vocab, **kw))
    return _HOST[key]


def _dev_fit(off, items, vocab, n_items, **kw):
    D = kw.get("D", 10)
    vectors, syn1, loss, word = IV.skipgram_device(_up(off, np.int32), _up(items, np.int32), vocab, n_items, **kw)
    return np.ascontiguousarray(vectors.cpu().numpy()[:, :D]), syn1.cpu().numpy(), float(loss.cpu()[0]), int(word.cpu()[0])


def _check_fit(key, off, items, n_items, min_count=5, max_sentence=1000, **kw):
    vocab, corpus, want = _host_fit(key, off, items, n_items, min_count, max_sentence, **kw)
    vectors, syn1, loss, err = _dev_fit(off, items, vocab, n_items, max_sentence=max_sentence, **kw)
    assert err == -1
    _same(vectors, want.vectors, "vectors")
    _same(syn1, want.syn1, "syn1")
    assert np.float64(loss).tobytes() == np.float64(want.loss).tobytes(), (loss, want.loss)
    return vocab, corpus, want


@pytest.fixture(scope="module")
def base(lib):
    """The sequences of tests/item2vec_cases.py ratings(): 564 kept rows of 40 users over 30 items."""
    off, items, cnt = _host_sequences(K.ratings())
    return off, items, cnt


# ---------------------------------------------------------------- sequences and walks

@pytest.mark.parametrize("sort_cap", [None, 64])
@pytest.mark.parametrize("grouped", [False, True])
def test_sequences_equal_the_host_definition(lib, monkeypatch, grouped, sort_cap):
    """Shuffled and user-grouped input, timestamps with many ties (input row decides), a user of more than 64 kept rows with the LDS sort
    capped at 64 (chunks and merge passes)."""
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    cols = K.ratings(seed=1, long_user=7, long_len=260, grouped=grouped)
    want = _host_sequences(cols)
    assert np.diff(want[0]).max() > 64
    off, items, cnt, err = _dev_sequences(cols)
    assert err == -1
    _same(off, want[0], "seq_offsets"); _same(items, want[1], "seq_items"); _same(cnt, want[2], "item_count")


@pytest.mark.parametrize("sort_cap", [None, 64])
def test_walks_equal_the_host_definition(lib, base, monkeypatch, sort_cap):
    """Items with more than 64 outgoing pairs (with the sort capped: the long path), and item 29 made a dead end (a last item)."""
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    off, items, _ = base
    items = items.copy()
    ends = off[1:][np.diff(off) > 0] - 1
    items[(items == 29) & ~np.isin(np.arange(len(items)), ends)] = 3              # 29 is never a `prev` ...
    items[ends[:4]] = 29                                                           # ... but is reached
    tr = IV.transitions_host(off, items, NI)
    assert tr[3][29] == 0 and tr[3].max() > 64
    want = IV.walks_host(tr, 300, 10, seed=5)
    assert (np.diff(want[0]) < 10).any() and (np.diff(want[0]) == 10).any()
    woff, witems, word = IV.walks_device(_up(off, np.int32), _up(items, np.int32), NI, 300, 10, seed=5)
    assert int(word.cpu()[0]) == -1
    woff = woff.cpu().numpy()
    _same(woff, want[0], "walk_offsets"); _same(witems.cpu().numpy()[:woff[-1]], want[1], "walk_items")


# ---------------------------------------------------------------- the trainer

@pytest.mark.parametrize("D", [1, 10, 16, 17, 64])
def test_every_lane_grouping(lib, base, D):
    """D = 1, 10, 16 in groups of 16 lanes, 17 and 64 in a wave; rounds of 7 over 564 words (not a multiple)."""
    off, items, _ = base
    _, corpus, _ = _check_fit(("D", D), off, items, NI, D=D, iters=2, round=7)
    assert len(corpus.word) % 7


@pytest.mark.parametrize("round", [1, 564, 600])
def test_round_sizes(lib, base, round):
    """R = 1 (Spark's order), R = N and R > N (one round an iteration)."""
    off, items, _ = base
    _, corpus, _ = _check_fit(("R", round), off, items, NI, D=10, iters=2, round=round)
    assert len(corpus.word) == 564


@pytest.mark.parametrize("row_cap", [6, 7])
def test_a_row_hit_exactly_cap_and_cap_plus_one_times(lib, row_cap):
    """Every sentence has two words or more, so the root node collects one emission per position: 7 in every full round of 7 -- exactly
    row_cap = 7 (added as it is) and row_cap + 1 for 6 (scaled by 6 / 7)."""
    off, items = K.sequences([9, 2, 30, 17, 5, 40, 3, 11, 50, 23, 2, 8], 12, seed=3)
    _, corpus, _ = _check_fit(("cap", row_cap), off, items, 12, D=10, iters=2, round=7, row_cap=row_cap)
    assert (corpus.hi - corpus.lo >= 2).all() and len(corpus.word) % 7


def test_sentences_cut_short_and_lonely(lib):
    """max_sentence = 8 cuts a sequence of 17 into 8 + 8 + 1: the last word is a sentence of its own and emits nothing; sequences of 3
    and 2 are shorter than the window; a sequence of 1."""
    off, items = K.sequences([17, 3, 1, 2, 30, 8, 9, 16, 40], 9, seed=4)
    _, corpus, _ = _check_fit("cut", off, items, 9, max_sentence=8, D=10, iters=2, round=5)
    assert (corpus.hi - corpus.lo == 1).sum() >= 2 and (corpus.hi - corpus.lo).max() == 8


def test_items_below_min_count_are_dropped(lib, base):
    off, items, cnt = base
    vocab, corpus, _ = _check_fit("min_count", off, items, NI, min_count=12, D=10, iters=2, round=16)
    assert 0 < len(vocab.ids) < (cnt > 0).sum() and len(corpus.word) < len(items)


def test_a_large_init_saturates_the_sigmoid(lib, base):
    """Vectors of size about 10: after the first rounds a third of the (word, node) pairs have |f| >= 6 and their terms are skipped, the
    others fall anywhere on the table -- on its first entry, 0, and on 995, the last one an f below 6 reaches (but for the one f whose
    f + 6 rounds to 12)."""
    off, items, _ = base
    init = IV.init_vectors(30, 10, 1) * np.float32(200.0)
    vocab, corpus, want = _check_fit("large", off, items, NI, D=10, iters=2, round=7, init=init)
    f = (want.vectors[:, None, :] * want.syn1[None, :-1, :]).sum(-1)
    assert (np.abs(f) >= 6).mean() > 0.1 and (np.abs(f) < 6).any() and np.isfinite(want.loss)
    trace = []
    IV.skipgram_host(corpus, vocab, D=10, iters=2, round=7, init=init, trace=trace)
    used = np.concatenate(trace)
    assert used.min() == 0 and used.max() == 995


def test_no_iterations(lib, base):
    off, items, _ = base
    vocab, _, want = _check_fit("iters0", off, items, NI, D=10, iters=0, round=7)
    _same(want.vectors, IV.init_vectors(len(vocab.ids), 10, 0), "init")
    assert not want.syn1.any() and want.loss > 0


def test_empty_inputs(lib):
    empty = {"userId": np.zeros(0, np.int64), "movieId": np.zeros(0, np.int64), "rating": np.zeros(0, np.float32), "timestamp": np.zeros(0, np.int64)}
    for nu, ni in ((0, 0), (5, 4)):
        off, items, cnt, err = _dev_sequences(empty, nu, ni)
        assert err == -1 and not off.any() and len(off) == nu + 1 and len(items) == 0 and not cnt.any()
    off, items = K.sequences([4, 6], 5)
    for min_count in (1000, 1):                                                     # no vocabulary at all; then no sequence items
        o, it = (off, items) if min_count == 1000 else (np.zeros(3, np.int32), np.zeros(0, np.int32))
        vocab = IV.vocabulary_host(np.bincount(it if min_count == 1 else items, minlength=5), min_count)
        vectors, syn1, loss, err = _dev_fit(o, it, vocab, 5, D=10, iters=2)
        assert err == -1 and loss == 0.0 and vectors.shape == (len(vocab.ids), 10)
    woff, witems, word = IV.walks_device(_up(np.zeros(3, np.int32), np.int32), _up(np.zeros(0, np.int32), np.int32), 5, 7, 4)
    assert int(word.cpu()[0]) == -1 and not woff.cpu().numpy().any()


def test_error_words(lib, base):
    cols = K.ratings()
    bad = dict(cols, userId=cols["userId"].copy()); bad["userId"][[700, 30]] = [NU, -1]
    assert _dev_sequences(bad)[3] == 1 << 32 | 30
    bad = dict(cols, movieId=cols["movieId"].copy()); bad["movieId"][[12, 500]] = [NI, 1 << 20]
    assert _dev_sequences(bad)[3] == 2 << 32 | 12
    bad = dict(cols, rating=cols["rating"].copy()); bad["rating"][[800, 45]] = [np.inf, np.nan]
    assert _dev_sequences(bad)[3] == 3 << 32 | 45
    with pytest.raises(ValueError, match="row 45"):
        _host_sequences(bad)
    off, items, cnt = base
    vocab = IV.vocabulary_host(cnt, 5)
    wrong = items.copy(); wrong[[400, 17]] = [NI, -3]
    assert _dev_fit(off, wrong, vocab, NI, iters=1)[3] == 2 << 32 | 17
    short = vocab._replace(counts=vocab.counts - (np.arange(len(vocab.ids)) == 0))   # n_words one less than the corpus holds
    assert _dev_fit(off, items, short, NI, iters=1)[3] == 4 << 32 | len(items)
    _, _, word = IV.walks_device(_up(off, np.int32), _up(wrong, np.int32), NI, 10, 5)
    assert int(word.cpu()[0]) == 2 << 32 | 17


def test_nothing_is_written_outside_the_outputs_or_the_workspace(lib, base):
    """Guard bands of a fill pattern after every output of the trainer, between D and the stride of every row of `vectors`, and on both
    sides of a workspace of exactly the advertised length keep their fill; the floats past D of an init row (NaN) are not read."""
    import torch
    off, items, _ = base
    D, stride, ins, R = 10, 13, 11, 7
    vocab, corpus, want = _host_fit(("D", 10), off, items, NI, D=10, iters=2, round=7)
    V, N, n, n_seq = len(vocab.ids), len(corpus.word), len(items), len(off) - 1
    dev = torch.device("cuda", torch.cuda.current_device())
    def filled(shape, dtype):
        n_bytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        return torch.full((n_bytes,), FILL, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)
    init = np.full((V, ins), np.nan, dtype=np.float32)
    init[:, :D] = IV.init_vectors(V, D, 0)
    lut = np.full(NI, -1, dtype=np.int32); lut[vocab.ids] = np.arange(V)
    t = [_up(off, np.int32), _up(items, np.int32), _up(lut, np.int32), _up(vocab.code_len, np.int32), _up(vocab.codes, np.uint8), _up(vocab.points, np.int32),
         _up(init, np.float32), _up(IV.exp_table(), np.float32), _up(IV.loss_table(), np.float64)]
    o_vec, o_syn1, o_loss = filled((V + GUARD_ROWS, stride), torch.float32), filled((V + GUARD_ROWS, D), torch.float32), filled((4,), torch.float64)
    word = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ws_bytes = lib.sprk_skipgram_workspace_bytes(n, n_seq, V, N, D, 5, R)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    arena = torch.full((GUARD_BYTES + ws_bytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    L.check(lib.sprk_skipgram_fit(p(t[0]), p(t[1]), n, n_seq, p(t[2]), NI, V, N, p(t[3]), p(t[4]), p(t[5]), p(t[6]), ins, p(t[7]), p(t[8]), D, 5, 2, 0.025, R, 32, 0, 1000,
                                  p(o_vec), stride, p(o_syn1), p(o_loss), p(word), C.c_void_p(arena.data_ptr() + GUARD_BYTES), ws_bytes,
                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    assert int(word.cpu()[0]) == -1
    arena, vec, syn1, loss = arena.cpu().numpy(), o_vec.cpu().numpy(), o_syn1.cpu().numpy(), o_loss.cpu().numpy()
    assert _is_fill(arena[:GUARD_BYTES]) and _is_fill(arena[GUARD_BYTES + ws_bytes:])
    assert _is_fill(vec[V:]) and _is_fill(vec[:V, D:]) and _is_fill(syn1[V:]) and _is_fill(loss[1:])
    _same(vec[:V, :D], want.vectors, "vectors"); _same(syn1[:V], want.syn1, "syn1")
    assert loss[:1].tobytes() == np.float64(want.loss).tobytes()


def test_guard_bands_of_sequences_and_walks(lib):
    import torch
    cols = K.ratings(seed=1, long_user=7, long_len=260)
    want = _host_sequences(cols)
    n, kept = len(cols["userId"]), int(want[0][-1])
    dev = torch.device("cuda", torch.cuda.current_device())
    filled = lambda count: torch.full((count * 4,), FILL, dtype=torch.uint8, device=dev).view(torch.int32)
    p = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    t = [_up(cols["userId"], np.int32), _up(cols["movieId"], np.int32), _up(cols["rating"], np.float32), _up(cols["timestamp"], np.int64)]
    o_off, o_items, o_cnt = filled(NU + 1 + 8), filled(n + 8), filled(NI + 8)
    word = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ws_bytes = lib.sprk_item_sequences_workspace_bytes(n, NU, NI)
    arena = torch.full((GUARD_BYTES + ws_bytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device=dev)
    L.check(lib.sprk_item_sequences(p(t[0]), p(t[1]), p(t[2]), p(t[3]), n, NU, NI, p(o_off), p(o_items), p(o_cnt), p(word), C.c_void_p(arena.data_ptr() + GUARD_BYTES),
                                    ws_bytes, stream))
    assert int(word.cpu()[0]) == -1
    a, off, items, cnt = arena.cpu().numpy(), o_off.cpu().numpy(), o_items.cpu().numpy(), o_cnt.cpu().numpy()
    assert _is_fill(a[:GUARD_BYTES]) and _is_fill(a[GUARD_BYTES + ws_bytes:]) and _is_fill(off[NU + 1:]) and _is_fill(items[kept:]) and _is_fill(cnt[NI:])
    _same(off[:NU + 1], want[0], "seq_offsets"); _same(items[:kept], want[1], "seq_items"); _same(cnt[:NI], want[2], "item_count")
    walks = IV.walks_host(IV.transitions_host(want[0], want[1], NI), 100, 6, seed=2)
    total = int(walks[0][-1])
    w_off, w_items = filled(100 + 1 + 8), filled(100 * 6 + 8)
    ws_bytes = lib.sprk_item_walks_workspace_bytes(kept, NU, NI, 100, 6)
    arena = torch.full((GUARD_BYTES + ws_bytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device=dev)
    L.check(lib.sprk_item_walks(p(o_off), p(o_items), kept, NU, NI, 100, 6, 2, p(w_off), p(w_items), p(word), C.c_void_p(arena.data_ptr() + GUARD_BYTES), ws_bytes, stream))
    assert int(word.cpu()[0]) == -1
    a, woff, witems = arena.cpu().numpy(), w_off.cpu().numpy(), w_items.cpu().numpy()
    assert _is_fill(a[:GUARD_BYTES]) and _is_fill(a[GUARD_BYTES + ws_bytes:]) and _is_fill(woff[101:]) and _is_fill(witems[total:])
    _same(woff[:101], walks[0], "walk_offsets"); _same(witems[:total], walks[1], "walk_items")


def test_caller_strides(lib, base):
    off, items, _ = base
    vocab, _, want = _host_fit(("D", 10), off, items, NI, D=10, iters=2, round=7)
    wide = np.full((len(vocab.ids), 12), np.nan, dtype=np.float32)
    wide[:, :10] = IV.init_vectors(len(vocab.ids), 10, 0)
    vectors, syn1, loss, word = IV.skipgram_device(_up(off, np.int32), _up(items, np.int32), vocab, NI, D=10, iters=2, round=7, init=_up(wide, np.float32)[:, :11], stride=16)
    assert int(word.cpu()[0]) == -1 and vectors.shape[1] == 16
    v = vectors.cpu().numpy()
    _same(v[:, :10], want.vectors, "vectors")
    assert not v[:, 10:].any()                                                     # (the wrapper's zeros: untouched)


def test_two_runs_give_the_same_bytes(lib, base):
    off, items, cnt = base
    vocab = IV.vocabulary_host(cnt, 5)
    runs = [_dev_fit(off, items, vocab, NI, D=10, iters=2, round=64) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][2] == runs[1][2]


def test_side_stream(lib, base):
    import torch
    off, items, _ = base
    vocab, _, want = _host_fit(("D", 10), off, items, NI, D=10, iters=2, round=7)
    args = (_up(off, np.int32), _up(items, np.int32))
    torch.cuda.synchronize()
    side, done = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(side):
        out = IV.skipgram_device(*args, vocab, NI, D=10, iters=2, round=7)
        done.record(side)
    done.synchronize()
    assert int(out[3].cpu()[0]) == -1
    _same(out[0].cpu().numpy(), want.vectors, "vectors"); _same(out[1].cpu().numpy(), want.syn1, "syn1")


@pytest.mark.parametrize("graph", [False, True])
def test_fit_end_to_end(lib, graph, tmp_path):
    """fit -> similar -> user_embeddings against the host chain: the vectors byte for byte, the neighbours those of the host's vectors,
    the user embeddings userembedding.user_emb_host's."""
    from sparrowrecsys_amd import userembedding as UE
    cols = K.ratings()
    kw = dict(D=10, iters=2, round=32, graph=graph, sample_count=120, sample_length=8)
    model = IV.fit(cols, n_users=NU, n_items=NI, **kw)
    vocab, want = IV.item2vec_host(cols["userId"], cols["movieId"], cols["rating"], cols["timestamp"], NU, NI, **kw)
    got = model.to_host()
    assert list(model.ids) == list(vocab.ids)
    _same(got.vectors, want.vectors, "vectors"); _same(got.syn1, want.syn1, "syn1")
    assert np.float64(model.loss).tobytes() == np.float64(want.loss).tobytes()
    from sparrowrecsys_amd.ranker import load_emb_file
    assert model.save(str(tmp_path / "item2vecEmb.csv")) == len(vocab.ids)
    back = load_emb_file(str(tmp_path / "item2vecEmb.csv"))
    assert sorted(back) == sorted(vocab.ids.tolist()) and all(np.asarray(back[int(i)], np.float32).tobytes() == want.vectors[r].tobytes() for r, i in enumerate(vocab.ids))
    order = np.argsort(vocab.ids)                                                   # the ranker's rows: ascending id
    table = want.vectors[order]
    query = [int(vocab.ids[0]), 10 ** 6, int(vocab.ids[3])]
    near = model.similar(query, 4)
    import torch
    twin = IV.Item2VecModel(vocab, torch.from_numpy(want.vectors).cuda(), torch.from_numpy(want.syn1).cuda(), want.loss)
    assert near == twin.similar(query, 4)
    assert near[1] == [] and len(near[0]) == 4 and query[0] not in near[0] and set(near[0]) <= set(vocab.ids.tolist())
    ue = model.user_embeddings(cols, n_users=NU)
    row_of = np.full(NI, -1); row_of[vocab.ids[order]] = np.arange(len(order))
    emb, has, count = UE.user_emb_host(cols["userId"], row_of[cols["movieId"]], table, np.ones(len(table), np.uint8), NU)
    g = ue.to_host()
    _same(g[0], emb, "user_emb"); _same(g[1], has, "user_has"); _same(g[2], count, "user_count")
