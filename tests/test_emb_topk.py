"""Embedding recall (sprk_emb_topk, EmbRanker.topk / retrieve / similar_movies): the argument contract and the workspace size on
the CPU; on the GPU the HIP path against the ranker oracle over the whole table cut to K -- rows exactly, scores bit for bit, no
tolerance and no excluded case."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import emb_rank_oracle as EO
from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import ranker as R
from tests.conftest import GOLDEN


# ---------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=4)
def _case(Q, N, D, seed, first_query_has=False):
    """test_emb_rank.py's _case without the candidate list: normal rows, ~2 % zero rows (NaN), ~10 % exact duplicates (at a small
    chunk length they land in different chunks), ~5 % rows and ~10 % queries without an embedding."""
    rng = np.random.default_rng(seed)
    items = rng.normal(size=(N, D)).astype(np.float32)
    items[rng.integers(0, N, size=max(1, N // 50))] = 0
    dup = rng.integers(0, N, size=(max(1, N // 10), 2))
    items[dup[:, 0]] = items[dup[:, 1]]
    has = (rng.random(N) > 0.05).astype(np.uint8)
    q = rng.normal(size=(Q, D)).astype(np.float32)
    qh = (rng.random(Q) > 0.1).astype(np.uint8)
    if first_query_has:
        qh[0] = 1
    return items, has, q, qh


def _ascending(s):
    """Ascending Double.compareTo order, ties by position: the oracle's key map restated, stable argsort of the key itself."""
    b = np.asarray(s, dtype=np.float64).view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    k = np.where(neg, ~b, b | np.uint64(1 << 63))
    k = np.where(np.isnan(s), np.uint64(0xFFFFFFFFFFFFFFFF), k)
    return np.argsort(k, axis=1, kind="stable").astype(np.int32)


_FULL = {}


def _oracle(items, has, q, qh, K, largest):
    """The ranker oracle over the whole table, cut to K.  The full ranking of one input set is computed once and shared (read-only)."""
    key = (id(items), id(has), id(q), id(qh))
    if key not in _FULL:
        N = len(items)
        full = EO.scores(items, has, q, qh, np.tile(np.arange(N), (len(q), 1)))
        down, up = EO.rank(full), _ascending(full)
        for a in (full, down, up):
            a.setflags(write=False)
        if len(_FULL) > 8:
            _FULL.clear()
        _FULL[key] = (full, down, up, items, has, q, qh)                # (inputs kept alive: id() keys stay unique)
    full, down, up = _FULL[key][:3]
    order = (down if largest else up)[:, :K]
    return np.take_along_axis(full, order, axis=1), order


def _same(got_scores, got_rows, want_scores, want_rows):
    gs, gr = got_scores.cpu().numpy(), got_rows.cpu().numpy()
    assert gr.dtype == np.int32 and gs.dtype == np.float64 and gs.shape == want_scores.shape
    assert np.array_equal(gr, want_rows)
    nan = np.isnan(want_scores)
    assert np.array_equal(np.isnan(gs), nan)
    assert np.array_equal(gs[~nan].view(np.uint64), want_scores[~nan].view(np.uint64))


def _ranker(items, has=None):
    import torch
    r = R.EmbRanker({i: items[i] for i in range(len(items))})
    if has is not None:
        r.has = torch.from_numpy(has).to(r.device)
    return r


class _chunk:
    """SPRK_EMB_TOPK_CHUNK for the calls inside."""
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        if self.n:
            os.environ["SPRK_EMB_TOPK_CHUNK"] = str(self.n)

    def __exit__(self, *a):
        os.environ.pop("SPRK_EMB_TOPK_CHUNK", None)


# ---------------------------------------------------------------- CPU: symbols, argument contract, workspace size, host logic
def test_both_symbols_load(lib):
    assert hasattr(lib, "sprk_emb_topk") and hasattr(lib, "sprk_emb_topk_workspace_bytes")
    assert "sprk_emb_topk" in L.EXPORTED_SYMBOLS and "sprk_emb_topk_workspace_bytes" in L.EXPORTED_SYMBOLS
    assert lib.sprk_emb_topk_workspace_bytes.restype is C.c_size_t


def _call(lib, **kw):
    """sprk_emb_topk with made-up non-NULL addresses: every argument check happens before any device call, nothing is dereferenced."""
    a = dict(item_emb=0x1000, item_has=None, n_items=100000, D=10, item_stride=10, query_emb=0x2000, query_has=None, n_queries=2,
             query_stride=10, K=100, largest=1, scores=0x3000, items=0x4000, workspace=0x5000, workspace_bytes=1 << 40, stream=None)
    a.update(kw)
    return lib.sprk_emb_topk(a["item_emb"], a["item_has"], a["n_items"], a["D"], a["item_stride"], a["query_emb"], a["query_has"],
                             a["n_queries"], a["query_stride"], a["K"], a["largest"], a["scores"], a["items"], a["workspace"],
                             a["workspace_bytes"], a["stream"])


@pytest.mark.parametrize("bad", [
    dict(K=0), dict(K=-3), dict(K=1025), dict(K=101, n_items=100), dict(K=1, n_items=0), dict(n_items=-1),
    dict(D=0), dict(D=1025, item_stride=2048, query_stride=2048), dict(item_stride=9), dict(query_stride=9), dict(n_queries=-1),
    dict(largest=2), dict(largest=-1),
    dict(item_emb=None), dict(query_emb=None), dict(scores=None), dict(items=None),
    dict(workspace=None), dict(workspace_bytes=0), dict(workspace=0x5004),
], ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_every_invalid_argument_is_einval_without_a_device(lib, bad):
    assert _call(lib, **bad) == L.EINVAL
    assert lib.sprk_last_error().startswith(b"emb_topk:")


def test_workspace_too_small_names_the_bytes_and_zero_queries_do_nothing(lib):
    need = lib.sprk_emb_topk_workspace_bytes(100000, 2, 100)
    assert need > 0
    assert _call(lib, workspace_bytes=need - 1) == L.EINVAL
    assert str(need).encode() in lib.sprk_last_error()
    assert _call(lib, workspace=None) == L.EINVAL and str(need).encode() in lib.sprk_last_error()
    assert _call(lib, n_queries=0) == L.OK                                  # valid arguments, no query: nothing to do, no device touched
    assert _call(lib, n_queries=0, workspace=None, workspace_bytes=0) == L.OK
    assert _call(lib, n_queries=0, K=0) == L.EINVAL                         # ... but the arguments are still checked


def test_workspace_bytes_properties(lib):
    ws = lib.sprk_emb_topk_workspace_bytes
    os.environ.pop("SPRK_EMB_TOPK_CHUNK", None)
    assert ws(881, 1, 800) == 0 and ws(4096, 64, 1024) == 0 and ws(1, 5, 1) == 0      # one chunk
    assert ws(4097, 1, 1) > 0
    assert ws(4097, 0, 1) == 0
    prev = 0
    for n in (4097, 8192, 8193, 20011, 131073, 1 << 20, 27_000_000):                    # monotone in N
        cur = ws(n, 3, 1024)
        assert cur >= prev and cur > 0
        prev = cur
    assert ws(27_000_000, 1, 1024) < 128 << 20                                          # the project's largest table: ~101 MB per query
    for q in range(1, 6):                                                               # linear (so monotone) in Q
        assert ws(20011, q, 100) == q * ws(20011, 1, 100)
    assert ws(20011, 2, 1) <= ws(20011, 2, 100) <= ws(20011, 2, 1024)
    assert ws(100, 1, 101) == 0 and ws(100, 1, 0) == 0 and ws(100, 1, 1025) == 0        # outside the limits: nothing to size
    with _chunk(64):                                                                    # the hook shortens the chunk for both functions
        assert ws(64, 1, 64) == 0 and ws(65, 1, 1) > 0
        assert ws(881, 1, 800) > 0
        small = ws(5003, 3, 100)
    with _chunk(48):                                                                    # not a power of two in [64, 4096]: ignored
        assert ws(881, 1, 800) == 0
    with _chunk(8192):
        assert ws(4097, 1, 1) > 0 and ws(4096, 1, 1) == 0
    assert small > ws(5003, 3, 100) > 0


def test_retrieve_size_follows_the_java(lib):
    """retrieve's host decisions, reachable without a device: null for a missing / wrong-length query, subList's clamp."""
    q = np.ones(10, dtype=np.float32)
    assert R._retrieve_size(None, 5, 10, 881) is None
    assert R._retrieve_size(np.ones(9, dtype=np.float32), 5, 10, 881) is None
    assert R._retrieve_size(np.ones((1, 10), dtype=np.float32), 5, 10, 881) is None
    assert R._retrieve_size(q, 5, 10, 881) == 5
    assert R._retrieve_size(q, 881, 10, 881) == 881 and R._retrieve_size(q, 10000, 10, 881) == 881
    assert R._retrieve_size(q, 0, 10, 881) == 0 and R._retrieve_size(q, -2, 10, 881) == 0
    for name in ("topk", "retrieve", "similar_movies"):
        assert callable(getattr(R.EmbRanker, name))


# ---------------------------------------------------------------- GPU: against the oracle
_DEFAULT = [(1, 881, 10, 800), (5, 3, 10, 1), (5, 3, 10, 3), (3, 20011, 32, 1024), (2, 131073, 16, 1024), (16, 1001, 7, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("Q,N,D,K", _DEFAULT)
def test_topk_default_chunk_bit_exact(Q, N, D, K, largest):
    items, has, q, qh = _case(Q, N, D, seed=Q * 131 + N)
    r = _ranker(items, has)
    want_s, want_r = _oracle(items, has, q, qh, K, largest)
    s, rows = r.topk(q, K, qh, largest=largest)
    _same(s, rows, want_s, want_r)


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("N", [63, 64, 65, 127, 129, 1000, 5003])
def test_topk_chunk_64_every_boundary(N, largest):
    """One chunk, the exact boundary, a last chunk shorter than K, K above the chunk length, three and more merge levels: the oracle's
    answer, and the very bytes of the same call at the default chunk."""
    Q, D = 3, 10
    items, has, q, qh = _case(Q, N, D, seed=N, first_query_has=True)
    r = _ranker(items, has)
    for K in (1, 17, 64, 100, 1024):
        if K > N:
            continue
        want_s, want_r = _oracle(items, has, q, qh, K, largest)
        with _chunk(64):
            s64, r64 = r.topk(q, K, qh, largest=largest)
        s0, r0 = r.topk(q, K, qh, largest=largest)
        _same(s64, r64, want_s, want_r)
        assert np.array_equal(s64.cpu().numpy().view(np.uint64), s0.cpu().numpy().view(np.uint64))
        assert np.array_equal(r64.cpu().numpy(), r0.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("Q,N,D,K", [(4, 881, 10, 800), (3, 300, 16, 300), (2, 4096, 10, 1024), (5, 1000, 7, 1), (2, 3000, 32, 257)])
def test_topk_agrees_with_the_shipped_ranker(Q, N, D, K):
    """N <= 4096: topk(q, K) IS score_many(q, arange(N)) cut to K -- order and gathered scores, every bit (NaN payloads included)."""
    import torch
    items, has, q, qh = _case(Q, N, D, seed=7 * N + K)
    r = _ranker(items, has)
    scores, order = r.score_many(q, np.tile(np.arange(N, dtype=np.int32), (Q, 1)), qh)
    want_r = order[:, :K]
    want_s = torch.gather(scores, 1, want_r.long())
    s, rows = r.topk(q, K, qh)
    assert torch.equal(rows, want_r)
    assert torch.equal(s.view(torch.int64), want_s.view(torch.int64))
    with _chunk(64):
        s, rows = r.topk(q, K, qh)
    assert torch.equal(rows, want_r) and torch.equal(s.view(torch.int64), want_s.view(torch.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [0, 64])
def test_topk_near_ties(chunk):
    """test_emb_rank's (1, k 1e-7) fixture: 300 scores within 1e-9, many sharing the upper 52 bits of their keys -- full keys decide."""
    N = 300
    items = np.zeros((N, 2), dtype=np.float32)
    items[:, 0] = 1.0
    items[:, 1] = (1e-7 * np.arange(N, 0, -1)).astype(np.float32)
    q = np.array([[1.0, 0.0], [0.5, 0.0]], dtype=np.float32)
    full = EO.scores(items, None, q, None, np.tile(np.arange(N), (2, 1)))
    assert len(np.unique(full[0])) > N // 2 and np.ptp(full[0]) < 1e-9 and EO.rank(full)[0, 0] != 0
    r = _ranker(items)
    for K in (10, 300):
        for largest in (True, False):
            want_s, want_r = _oracle(items, None, q, None, K, largest)
            with _chunk(chunk):
                s, rows = r.topk(q, K, largest=largest)
            _same(s, rows, want_s, want_r)


@pytest.mark.gpu
def test_topk_nan_rows_and_padding():
    """N = 100 is no power of two: the sort is padded.  Ascending, K = N: NaN rows come last in row order and no padding entry shows."""
    N, D = 100, 6
    rng = np.random.default_rng(5)
    q = rng.normal(size=(2, D)).astype(np.float32)
    zero = np.zeros((N, D), dtype=np.float32)
    some = rng.normal(size=(N, D)).astype(np.float32)
    nan_rows = [3, 50, 51, 99]
    some[nan_rows] = 0
    for items in (zero, some):
        r = _ranker(items)
        for chunk in (0, 64):
            for largest in (False, True):
                with _chunk(chunk):
                    s, rows = r.topk(q, N, largest=largest)
                want_s, want_r = _oracle(items, None, q, None, N, largest)
                _same(s, rows, want_s, want_r)
                got = rows.cpu().numpy()
                assert all(sorted(g.tolist()) == list(range(N)) for g in got)          # a permutation of the rows: no padding entry
    assert rows.cpu().numpy()[0, :4].tolist() == nan_rows                               # (last loop: `some`, descending: NaN first)
    with _chunk(64):
        s, rows = _ranker(some).topk(q, N, largest=False)
    assert rows.cpu().numpy()[1, -4:].tolist() == nan_rows and bool(np.isnan(s.cpu().numpy()[:, -4:]).all())
    s, rows = _ranker(zero).topk(q, N, largest=False)
    assert rows.cpu().numpy().tolist() == [list(range(N))] * 2 and bool(np.isnan(s.cpu().numpy()).all())


@pytest.mark.gpu
def test_topk_reference_embeddings_fixture():
    """tests/golden/emb_rank.npz, 256 of the reference's movies x 32 of its users with the stored scores / order."""
    z = np.load(os.path.join(GOLDEN, "emb_rank.npz"))
    r = R.EmbRanker({i: z["item_emb"][i] for i in range(len(z["item_ids"]))})          # table rows = fixture positions, which `order` holds
    for K in (1, 100, 256):
        s, rows = r.topk(z["user_emb"], K)
        want_r = z["order"][:, :K]
        assert np.array_equal(rows.cpu().numpy(), want_r)
        assert np.array_equal(s.cpu().numpy().view(np.uint64), np.take_along_axis(z["scores"], want_r.astype(np.int64), axis=1).view(np.uint64))


@pytest.mark.gpu
def test_retrieve_and_similar_movies():
    rng = np.random.default_rng(11)
    ids = [int(m) for m in rng.choice(100000, size=500, replace=False)]
    emb = {m: rng.normal(size=8).astype(np.float32) for m in ids}
    r = R.EmbRanker(emb)
    table_ids = np.array(sorted(ids))
    items = np.stack([emb[m] for m in table_ids])
    q = rng.normal(size=8).astype(np.float32)
    full = EO.scores(items, None, q[None], None, np.arange(500)[None])
    best = table_ids[EO.rank(full)[0]].tolist()
    worst = table_ids[_ascending(full)[0]].tolist()
    assert r.retrieve(q, 20) == best[:20]                                               # best first
    assert r.retrieve(q, 20, reference_order=True) == worst[:20]                        # the Java to the letter: the other end of the list
    assert worst[:20] == best[::-1][:20]                                                # (no ties in this table)
    assert r.retrieve(None, 20) is None and r.retrieve(np.ones(7, dtype=np.float32), 20) is None
    assert r.retrieve(q, 10000) == best and len(best) == 500                            # size above the table clamps
    assert r.retrieve(q, 0) == []
    with pytest.raises(L.SparrowHipError):
        R.EmbRanker({i: np.ones(2, dtype=np.float32) for i in range(2000)}).retrieve(np.ones(2, dtype=np.float32), 1025)
    # similar movies: the movie's own row is the query
    m = int(table_ids[123])
    sim = r.similar_movies(m, 30)
    full = EO.scores(items, None, items[123][None], None, np.arange(500)[None])
    want = [int(x) for x in table_ids[EO.rank(full)[0]].tolist() if x != m][:30]
    assert sim == want and m not in sim and len(sim) == 30
    assert len(r.similar_movies(m, 499)) == 499 and len(r.similar_movies(m, 5000)) == 499
    assert r.similar_movies(-5, 30) == [] and r.similar_movies(m, 0) == []
    # argument errors of topk
    with pytest.raises(ValueError):
        r.topk(np.zeros((2, 9), dtype=np.float32), 5)
    with pytest.raises(ValueError):
        r.topk(np.zeros(8, dtype=np.float32), 5)
    for k in (0, 501, 1025, -1):
        with pytest.raises(L.SparrowHipError):
            r.topk(q[None], k)


@pytest.mark.gpu
def test_topk_is_deterministic_and_takes_device_queries():
    import torch
    Q, N, D, K = 3, 20011, 32, 1024
    items, has, q, qh = _case(Q, N, D, seed=Q * 131 + N)
    r = _ranker(items, has)
    s1, r1 = r.topk(q, K, qh)
    s2, r2 = r.topk(q, K, qh)
    wide = torch.zeros((Q, 2 * D), dtype=torch.float32, device=r.device)
    wide[:, ::2] = torch.from_numpy(q).to(r.device)
    s3, r3 = r.topk(wide[:, ::2], K, torch.from_numpy(qh).to(r.device))                 # a non-contiguous device tensor
    assert not wide[:, ::2].is_contiguous()
    for s, rows in ((s2, r2), (s3, r3)):
        assert torch.equal(s.view(torch.int64), s1.view(torch.int64)) and torch.equal(rows, r1)
    r.TOPK_WORKSPACE_BYTES = 1                                                          # (this object only) one query per tile: the walk over tiles
    s4, r4 = r.topk(q, K, qh)
    assert torch.equal(s4.view(torch.int64), s1.view(torch.int64)) and torch.equal(r4, r1)
