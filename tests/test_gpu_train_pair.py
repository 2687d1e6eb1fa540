"""``trainer_pair.train_device`` (``sprk_train_pair_fit``, csrc/k_train_pair.h) against its definition ``trainer_pair.train_host``: every
weight, every ``m``, every ``v``, every ``p`` of the last epoch, accuracy and both AUCs of every epoch byte for byte, the loss within
``max(N, 64) 2^-50`` relative (``-m gpu``).  Tiny vocabularies and tens to a few hundred rows, the one table that has to exceed a capped grid
and the end-to-end test's few thousand ratings, then the step shape ``trainer_pair.fit`` ships with: batch 4096 at the default tile, every
stated maximum, and tables, Dense parameters and schedules beyond one round of a grid (docs/train_shapes_results.md)."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_pair as TP
from tests import metrics_cases as MC
from tests import train_pair_cases as TPC

pytestmark = pytest.mark.gpu
F = np.float32
same = TPC.same_bits
SHARED = [False, True]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


def host_of(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def both(fam, w, ids, dense, y, **kw):
    """Host and device fits of one input: asserts the equalities of the module docstring, -> the host's result."""
    want = TP.train_host(fam, w, ids, dense, y, **kw)
    got = TP.train_device(fam, w, ids, dense, y, **kw)
    assert got.step == want.step and len(got.history) == len(want.history)
    for name, g, h in (("weight", got.weights, want.weights), ("m", got.m, want.m), ("v", got.v, want.v)):
        g = host_of(g)
        for k in TP.param_names(fam):
            assert same(g[k], h[k]), (name, k, np.flatnonzero(g[k].reshape(-1).view(np.uint32) != h[k].reshape(-1).view(np.uint32))[:8])
    p = got.p.cpu().numpy()
    assert same(p, want.p), np.flatnonzero(p.view(np.uint32) != want.p.view(np.uint32))[:8]
    for e, (a, b) in enumerate(zip(got.history, want.history)):
        assert a[1:] == b[1:] or (np.isnan(a[2:]).all() and np.isnan(b[2:]).all() and a[1] == b[1]), (e, a, b)
        assert abs(a[0] - b[0]) <= MC.loss_bound(len(y)) * abs(b[0]) or (np.isnan(a[0]) and np.isnan(b[0])), (e, a[0], b[0])
    return want


def moved(got, w, keys):
    return all(not same(got.weights[k], w[k]) for k in keys)


# ---------------------------------------------------------------- rows and batches

@pytest.mark.parametrize("shared", SHARED)
@pytest.mark.parametrize("n,batch,tile", [(1, 4, 8), (7, 16, 8), (8, 16, 8), (9, 16, 8), (50, 12, 8), (23, 1, 8), (40, 12, 32), (33, 32, 32)])
def test_row_counts_and_batching(torch, n, batch, tile, shared):
    """N = 1, tile - 1, tile, tile + 1; B no multiple of the tile; a short last batch; B = 1; one batch only; three epochs; both table forms."""
    fam, w, ids, dense, y = TPC.small(n, seed=n, shared=shared)
    want = both(fam, w, ids, dense, y, batch_size=batch, epochs=3, tile=tile)
    assert want.step == 3 * ((n + batch - 1) // batch)
    assert moved(want, w, ["emb/movieId", "head/kernel", "head/bias", "deep0/kernel"] + ([] if shared else ["deep_emb/userId"]))


@pytest.mark.parametrize("as_tensor", [False, True])
def test_order(torch, as_tensor):
    fam, w, ids, dense, y = TPC.small(50, seed=4)
    order = np.random.default_rng(1).permutation(50)
    want = TP.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8, order=order)
    plain = TP.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8)
    assert not same(want.weights["head/kernel"], plain.weights["head/kernel"])
    dev = lambda a: torch.from_numpy(a).cuda()
    got = TP.train_device(fam, w, dev(ids), dev(dense), dev(y), batch_size=12, epochs=3, tile=8, order=dev(order) if as_tensor else order)
    assert all(same(host_of(got.weights)[k], want.weights[k]) for k in want.weights)
    assert same(got.p.cpu().numpy(), want.p) and [h[1:] for h in got.history] == [h[1:] for h in want.history]
    with pytest.raises(ValueError, match="permutation"):
        TP.train_device(fam, w, ids, dense, y, order=dev(np.zeros(50, dtype=np.int64)) if as_tensor else np.zeros(50, dtype=np.int64))


# ---------------------------------------------------------------- the graph's shapes

@pytest.mark.parametrize("shared", SHARED)
@pytest.mark.parametrize("emb_dim", [1, 3, 4, 10, 16, 64])
def test_row_widths(torch, emb_dim, shared):
    fam, w, ids, dense, y = TPC.small(40, seed=20 + emb_dim, emb_dim=emb_dim, shared=shared)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


PAIR_SETS = {
    "one": dict(pairs=[("movieId", "userId")]),
    "reference": dict(),
    "config2": dict(fields=TPC.SIX, pairs=TPC.SIX_PAIRS),
    "all28": dict(fields=TPC.EIGHT, pairs=TPC.EIGHT_PAIRS, deep_emb=("f0", "f2")),
    "self": dict(pairs=[("movieId", "movieId"), ("movieId", "userId"), ("userGenre1", "userGenre1")]),
    "thrice": dict(pairs=[("movieId", "userId"), ("movieGenre1", "movieId"), ("movieId", "userGenre1"), ("movieId", "movieId")]),
}


@pytest.mark.parametrize("shared", SHARED)
@pytest.mark.parametrize("name", sorted(PAIR_SETS))
def test_pair_lists(torch, name, shared):
    """One pair, the reference's four, config 2's eight over six fields, all 28 pairs of eight fields, pairs ``(a, a)``, one table in four pairs."""
    fam, w, ids, dense, y = TPC.small(40, seed=len(name), shared=shared, **PAIR_SETS[name])
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert moved(got, w, ["emb/" + fam.fields[a][0] for a, _ in fam.pairs])


@pytest.mark.parametrize("shared", SHARED)
def test_a_field_in_no_pair(torch, shared):
    """``movieGenre1`` is in no pair and is no deep key: its table receives ``g = +0`` on every step and keeps its bits with zero moments, while
    its first-order rows move.  ``userGenre1`` is in no pair but is a deep key: its ``emb/`` table moves only when the tables are shared."""
    fam, w, ids, dense, y = TPC.small(40, seed=31, pairs=[("movieId", "userId")], deep_emb=("userGenre1",), shared=shared)
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert same(got.weights["emb/movieGenre1"], w["emb/movieGenre1"]) and not got.m["emb/movieGenre1"].any() and not got.v["emb/movieGenre1"].any()
    off = fam.fo_off[3]
    assert not same(got.weights["head/kernel"][off:off + 3], w["head/kernel"][off:off + 3])
    assert same(got.weights["emb/userGenre1"], w["emb/userGenre1"]) != shared
    assert shared or moved(got, w, ["deep_emb/userGenre1"])


@pytest.mark.parametrize("shared", SHARED)
@pytest.mark.parametrize("deep_emb", [(), ("userId",), ("movieGenre1", "movieId")])
def test_deep_keys(torch, deep_emb, shared):
    """No deep table (the deep stack reads the numerics only), one, and two of which one is a genre field named out of field order."""
    fam, w, ids, dense, y = TPC.small(40, seed=33 + len(deep_emb), deep_emb=deep_emb, shared=shared)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


@pytest.mark.parametrize("hidden", [(1,), (256,), (256, 256), (7, 200, 3)])
def test_hidden_widths(torch, hidden):
    fam, w, ids, dense, y = TPC.small(40, seed=35, hidden=hidden)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


@pytest.mark.parametrize("shared", SHARED)
def test_no_numerics(torch, shared):
    fam, w, ids, dense, y = TPC.small(40, seed=36, n_dense=0, shared=shared)
    assert dense.shape == (40, 0)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


# ---------------------------------------------------------------- ids

@pytest.mark.parametrize("shared", SHARED)
def test_one_id_in_every_field(torch, shared):
    """Every sample carries id 2 in every field: one run per field, as long as the batch; every other row keeps its bits."""
    fam, w, ids, dense, y = TPC.small(48, seed=2, shared=shared)
    ids[:] = 2
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    for f, (k, _, vocab) in enumerate(fam.fields):
        keep = np.arange(vocab) != 2
        assert same(got.weights["emb/" + k][keep], w["emb/" + k][keep]) and not same(got.weights["emb/" + k][2], w["emb/" + k][2])
        rows = fam.fo_off[f] + np.arange(vocab)
        assert same(got.weights["head/kernel"][rows[keep]], w["head/kernel"][rows[keep]]) and not same(got.weights["head/kernel"][rows[2]], w["head/kernel"][rows[2]])


@pytest.mark.parametrize("shared", SHARED)
def test_every_genre_id_none(torch, shared):
    """Both genre fields -1 throughout, in pairs and (``movieGenre1``) in the deep part: no row, no first-order term, no schedule entry."""
    fam, w, ids, dense, y = TPC.small(40, seed=3, deep_emb=("movieGenre1", "userId"), shared=shared)
    ids[:, 2:] = -1
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    for k in ("emb/userGenre1", "emb/movieGenre1") + (() if shared else ("deep_emb/movieGenre1",)):
        assert same(got.weights[k], w[k]) and not got.v[k].any()
    for f in (2, 3):
        rows = slice(fam.fo_off[f], fam.fo_off[f] + fam.fields[f][2])
        assert same(got.weights["head/kernel"][rows], w["head/kernel"][rows])
    assert moved(got, w, ["emb/userId", "emb/movieId"])


@pytest.mark.parametrize("shared", SHARED)
def test_a_vocabulary_of_one(torch, shared):
    fields = [("movieId", "id", 1), ("userId", "id", 5), ("userGenre1", "genre", 1), ("movieGenre1", "genre", 3)]
    fam, w, ids, dense, y = TPC.small(40, seed=5, fields=fields, shared=shared)
    assert (ids[:, 0] == 0).all() and set(ids[:, 2].tolist()) == {-1, 0}
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


# ---------------------------------------------------------------- arithmetic edges

@pytest.mark.parametrize("bias", [100.0, -100.0])
def test_a_saturated_head(torch, bias):
    fam, w, ids, dense, y = TPC.small(40, seed=7)
    w["head/bias"][0] = bias
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert set(np.unique(got.p).tolist()) == ({1.0} if bias > 0 else {0.0}) and set(y.tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("shared", SHARED)
@pytest.mark.parametrize("scale", [1e-20, 1e-39])
def test_tiny_and_subnormal_rows(torch, scale, shared):
    fam, w, ids, dense, y = TPC.small(40, seed=8, hidden=(6, 4), shared=shared)
    w = {k: (v.astype(np.float64) * scale).astype(F) for k, v in w.items()}
    tiny = np.finfo(F).tiny
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    sub = lambda d: any(((np.abs(a) > 0) & (np.abs(a) < tiny)).any() for a in d.values())
    assert sub(got.m) if scale == 1e-20 else sub(w)


def test_a_dot_that_overflows(torch):
    """Finite rows of +-1e20: ``movieId . userId`` adds ``+inf`` and ``-inf``, the dot is NaN, and so are the logit and ``p``: every ``p`` is the
    quiet NaN ``0x7fc00000`` on both sides, and so is every NaN the weights, ``m`` and ``v`` then hold."""
    fam, w, ids, dense, y = TPC.small(16, seed=6, emb_dim=4)
    w["emb/movieId"][:] = F(1e20)
    w["emb/userId"][:] = np.array([1e20, -1e20, 1e20, -1e20], dtype=F)
    assert all(np.isfinite(a).all() for a in w.values())
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert (got.p.view(np.uint32) == 0x7fc00000).all()
    for d in (got.weights, got.m, got.v):
        for a in d.values():
            assert (a.view(np.uint32)[np.isnan(a)] == 0x7fc00000).all()
    assert np.isnan(got.weights["head/bias"]).all() and np.isnan(got.weights["emb/movieId"]).any()


# ---------------------------------------------------------------- grids and the sort

@pytest.mark.parametrize("shared", SHARED)
@pytest.mark.parametrize("grid", ["3", "1"])
def test_grids_capped(torch, monkeypatch, grid, shared):
    """SPRK_FE_MAX_GRID 3 and 1 at 300 rows, six fields of 30 rows in all, hidden (64, 64), emb_dim 32: every grid-stride loop of the schedule
    (1 800 entries) and of the two Adam kernels goes round (more than 3 x 256 Dense parameters and ``emb/`` elements)."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", grid)
    fam, w, ids, dense, y = TPC.small(300, seed=10, fields=TPC.SIX, pairs=TPC.SIX_PAIRS, emb_dim=32, hidden=(64, 64), shared=shared)
    assert len(y) > 256 and ids.size > 3 * 256 and sum(v for _, _, v in fam.fields) * 32 > 3 * 256
    both(fam, w, ids, dense, y, batch_size=128, epochs=1, tile=8)


@pytest.mark.parametrize("shared", SHARED)
def test_table_adam_grid_goes_past_one_round(torch, monkeypatch, shared):
    """A field of 2 000 rows x 10: 20 000 ``emb/`` elements (and as many of ``deep_emb/``, and 2 000 first-order rows behind them) under a grid
    capped at 64 workgroups of 256 threads: the table Adam's grid-stride loop goes round.  Rows on both sides of the round's end are hit."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", "64")
    fields = [("movieId", "id", 2000), ("userId", "id", 5), ("userGenre1", "genre", 4), ("movieGenre1", "genre", 3)]
    fam, w, ids, dense, y = TPC.small(40, seed=26, fields=fields, emb_dim=10, shared=shared)
    assert 2000 * 10 > 64 * 256 and 1638 * 10 < 64 * 256 <= 1639 * 10
    ids[:16, 0] = np.array([0, 1638, 1639, 1999])[np.arange(16) % 4]
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    for row in (0, 1638, 1639, 1999):
        assert not same(got.weights["emb/movieId"][row], w["emb/movieId"][row])
        assert not same(got.weights["head/kernel"][fam.fo_off[0] + row], w["head/kernel"][fam.fo_off[0] + row])
        assert shared or not same(got.weights["deep_emb/movieId"][row], w["deep_emb/movieId"][row])
    never = np.ones(2000, dtype=bool)
    never[ids[:, 0]] = False
    assert never.sum() > 1900 and same(got.weights["emb/movieId"][never], w["emb/movieId"][never])
    assert same(got.weights["head/kernel"][fam.fo_off[0]:fam.fo_off[0] + 2000][never], w["head/kernel"][fam.fo_off[0]:fam.fo_off[0] + 2000][never])


@pytest.mark.parametrize("shared", SHARED)
def test_batches_beyond_the_lds_sort_capacity(torch, monkeypatch, shared):
    """SPRK_FE_SORT_CAP=64: a batch's 40 x 4 entries take the chunked sort and the merge passes."""
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    fam, w, ids, dense, y = TPC.small(100, seed=9, shared=shared)
    both(fam, w, ids, dense, y, batch_size=40, epochs=2, tile=8)


@pytest.mark.parametrize("batch", [56, 64, 72, 136])
def test_tile_counts_around_the_unrolled_partial_sum(torch, batch):
    """Tile 8: 7, 8, 9 and 17 tiles -- k_tp_dense_adam adds eight partials at a time, then the rest -- and a last batch of 5 rows."""
    fam, w, ids, dense, y = TPC.small(batch + 5, seed=batch)
    both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=8)


def test_a_step_of_more_than_48_kb_of_lds(torch):
    """Six fields x 64, hidden (256, 256) at tile 8: above the 48 KB a kernel gets without asking; the first tile beyond 160 KB is refused in
    words."""
    fam, w, ids, dense, y = TPC.small(40, seed=14, fields=TPC.SIX, pairs=TPC.SIX_PAIRS, emb_dim=64, hidden=(256, 256))
    assert 48 * 1024 < TP.lds_bytes(fam, 8) <= TP.LDS_BYTES
    both(fam, w, ids, dense, y, batch_size=40, epochs=2, tile=8)
    top = TP.LDS_BYTES // TP.lds_bytes(fam, 1)
    assert TP.lds_bytes(fam, top) <= TP.LDS_BYTES < TP.lds_bytes(fam, top + 1)
    with pytest.raises(ValueError, match="tile = %d needs %d bytes of LDS" % (top + 1, TP.lds_bytes(fam, top + 1))):
        TP.train_device(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=top + 1)


def test_a_tile_wider_than_the_workgroup(torch):
    """Tile 300 > 256 threads: every per-sample loop of k_tp_step goes round; N = batch = 300 is one tile."""
    fam, w, ids, dense, y = TPC.small(300, seed=24)
    assert TP.lds_bytes(fam, 300) <= TP.LDS_BYTES
    both(fam, w, ids, dense, y, batch_size=300, epochs=2, tile=300)


# ---------------------------------------------------------------- the C ABI: errors, memory, streams

GUARD = 64


def raw_fit(torch, fam, w, ids, dense, y, batch, tile, epochs, stream=None):
    """``sprk_train_pair_fit`` itself: parameters, moments, p and the workspace each inside guard bands of a fixed pattern, the workspace
    exactly as large as ``sprk_train_pair_workspace_bytes`` reports.  -> (rc, params, m, v, p, error word, guards intact)."""
    lib = L.load_library()
    dev = torch.device("cuda")
    n = len(y)
    flat = TP._flatten(fam, w, dev)
    ms = TP._model_struct(fam)
    need = int(lib.sprk_train_pair_workspace_bytes(C.byref(ms), n, batch, tile))
    assert need > 0 and need % 16 == 0

    def banded(count, dtype, fill=None):
        buf = torch.full((count + 2 * GUARD,), 0x5A if dtype == torch.uint8 else -7, dtype=dtype, device=dev)
        if fill is not None:
            buf[GUARD:GUARD + count] = fill
        return buf
    params, m, v = banded(flat.numel(), torch.float32, flat), banded(flat.numel(), torch.float32, 0.0), banded(flat.numel(), torch.float32, 0.0)
    p = banded(max(epochs, 1) * n, torch.float32, 0.0)
    ws = banded(need, torch.uint8)
    steps = (n + batch - 1) // batch
    alphas = torch.from_numpy(np.array([T.adam_alpha(0.001, t + 1) for t in range(epochs * steps)] + [0.0], dtype=F)).to(dev)
    word = torch.full((1,), -1, dtype=torch.int64, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_ids, t_dense, t_y = up(ids), up(dense), up(y)
    c1, c2, eps = T.adam_constants()
    at = lambda b, size: C.c_void_p(b.data_ptr() + GUARD * size)
    rc = lib.sprk_train_pair_fit(C.byref(ms), C.c_void_p(t_ids.data_ptr()), C.c_void_p(t_dense.data_ptr()), C.c_void_p(t_y.data_ptr()), None,
                                 n, batch, tile, epochs, C.c_void_p(alphas.data_ptr()), float(c1), float(c2), float(eps), at(params, 4), at(m, 4), at(v, 4), at(p, 4),
                                 C.c_void_p(word.data_ptr()), at(ws, 1), need, C.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream))
    (stream or torch.cuda.current_stream()).synchronize()
    intact = all(bool((b[:GUARD] == b[0]).all()) and bool((b[-GUARD:] == b[0]).all()) and (float(b[0]) in (-7.0, 90.0)) for b in (params, m, v, p, ws))
    cut = lambda b: b[GUARD:-GUARD].cpu().numpy()
    return rc, cut(params), cut(m), cut(v), cut(p), int(word.cpu()[0]), intact


@pytest.mark.parametrize("shared", SHARED)
def test_guard_bands_side_stream_exact_workspace(torch, shared):
    fam, w, ids, dense, y = TPC.small(50, seed=10, shared=shared)
    want = TP.train_host(fam, w, ids, dense, y, batch_size=12, epochs=2, tile=8)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 12, 8, 2, stream=side)
    assert rc == 0 and word == -1 and intact
    flat = lambda d: np.concatenate([d[k].reshape(-1) for k in TP.param_names(fam)])
    assert same(params, flat(want.weights)) and same(m, flat(want.m)) and same(v, flat(want.v))
    assert same(p[50:], want.p)
    lib = L.load_library()
    ms = TP._model_struct(fam)
    need = int(lib.sprk_train_pair_workspace_bytes(C.byref(ms), 50, 12, 8))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    word_t = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    f = torch.zeros(TP._flatten(fam, w, torch.device("cuda")).numel(), device="cuda")
    z = C.c_void_p(f.data_ptr())
    rc = lib.sprk_train_pair_fit(C.byref(ms), z, z, z, None, 50, 12, 8, 1, z, 0.1, 0.001, 1e-7, z, z, z, z, C.c_void_p(word_t.data_ptr()), C.c_void_p(ws.data_ptr()), need - 1, None)
    assert rc == L.EINVAL and b"sprk_train_pair_workspace_bytes" in lib.sprk_last_error()


@pytest.mark.parametrize("shared", SHARED)
def test_each_error_word_and_no_parameter_moves(torch, shared):
    fam, w, ids, dense, y = TPC.small(40, seed=11, shared=shared)
    flat0 = np.concatenate([w[k].reshape(-1) for k in TP.param_names(fam)])

    def check(kind, row, message, ids=ids, dense=dense, y=y):
        rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 16, 8, 2)
        assert rc == 0 and intact and word == (kind << 32 | row), (word >> 32, word & 0xffffffff)
        assert same(params, flat0) and not m.any() and not v.any() and not p.any()
        for fit in (TP.train_device, TP.train_host):
            with pytest.raises(ValueError, match=message):
                fit(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    bad = ids.copy(); bad[30, 0] = 7; bad[12, 0] = -1; bad[20, 2] = -2     # an id column takes no -1, a genre column no -2
    check(T.ERR_ID, 12, "samples row 12: an id outside", ids=bad)
    bad = ids.copy(); bad[25, 3] = 3                                        # == the genre field's vocabulary
    check(T.ERR_ID, 25, "samples row 25: an id outside", ids=bad)
    bad = dense.copy(); bad[9, 1] = np.inf; bad[3, 0] = np.nan
    check(T.ERR_NUMERIC, 3, "samples row 3: a numeric", dense=bad)
    bad = y.copy(); bad[7] = np.nan; bad[39] = -np.inf
    check(T.ERR_LABEL, 7, "samples row 7: the label", y=bad)
    bad_y = y.copy(); bad_y[5] = np.inf
    bad = ids.copy(); bad[30, 1] = 5
    check(T.ERR_ID, 30, "samples row 30: an id outside", ids=bad, y=bad_y)  # the least key: kind 1 at row 30 before kind 3 at row 5


@pytest.mark.parametrize("shared", SHARED)
def test_two_fits_give_the_same_bytes_and_a_fit_continues(torch, shared):
    fam, w, ids, dense, y = TPC.small(200, seed=12, hidden=(65, 7), shared=shared)
    a = TP.train_device(fam, w, ids, dense, y, batch_size=48, epochs=2, tile=8)
    b = TP.train_device(fam, w, ids, dense, y, batch_size=48, epochs=2, tile=8)
    for x, z in ((a.weights, b.weights), (a.m, b.m), (a.v, b.v)):
        assert all(same(x[k].cpu().numpy(), z[k].cpu().numpy()) for k in x)
    assert same(a.p.cpu().numpy(), b.p.cpu().numpy()) and a.history == b.history
    one = TP.train_device(fam, w, ids, dense, y, batch_size=48, epochs=1, tile=8)
    two = TP.train_device(fam, one.weights, ids, dense, y, batch_size=48, epochs=1, tile=8, state=(one.m, one.v, one.step))
    assert two.step == a.step and all(same(two.weights[k].cpu().numpy(), a.weights[k].cpu().numpy()) and same(two.v[k].cpu().numpy(), a.v[k].cpu().numpy()) for k in w)
    none = TP.train_device(fam, w, ids, dense, y, epochs=0)
    assert none.step == 0 and none.history == [] and all(same(none.weights[k].cpu().numpy(), w[k]) for k in w)


# ---------------------------------------------------------------- trainer_pair.fit

def _ratings_model(shared=False):
    from tests import featureeng_cases as cases
    fields = [("movieId", "id", cases.N_MOVIES), ("userId", "id", cases.N_USERS), ("userGenre1", "genre", 19), ("movieGenre1", "genre", 19)]
    return M.DeepFM(seed=3, fields=fields, hidden=(32, 16), share_deep_tables=shared)


@pytest.mark.parametrize("shared", SHARED)
def test_ratings_to_recommendations(torch, shared):
    """3 000 structured ratings (tests/train_wide_cases.py): featureeng.build -> split(mode="time") -> trainer_pair.fit(train.columns) ->
    evaluate_device(test.columns) -> recommend.  The weights are ``train_host``'s and the held-out AUC of the last epoch's weights exceeds that
    of the untrained weights.  A second fit continues; ``DeepFM.fit`` itself still refuses."""
    from sparrowrecsys_amd import featureeng as FE
    from tests import featureeng_cases as cases
    built = FE.build(TPC.structured_ratings(), cases.synthetic_movies(), 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    train, test = built.split(mode="time", sample=1.0)
    model, other = _ratings_model(shared), _ratings_model(shared)
    start = {k: v.copy() for k, v in model.weights.items()}
    auc_before = model.evaluate_device(test.columns)[2]
    history = TP.fit(model, train.columns, batch_size=128, epochs=3, learning_rate=0.01)
    tcols = train.to_host()
    ids, dense = other.pack(tcols)
    y = np.asarray(tcols["label"], dtype=F)
    fam = TP.family_of(other)
    want = TP.train_host(fam, start, ids, dense, y, batch_size=128, epochs=3, learning_rate=0.01)
    assert len(y) > 2000 and all(same(model.weights[k], want.weights[k]) for k in want.weights)
    assert not same(model.weights["head/kernel"], start["head/kernel"]) and not same(model.weights["emb/movieId"], start["emb/movieId"])
    assert [h[1:] for h in history] == [h[1:] for h in want.history] and len(history) == 3
    other.set_weights(want.weights)
    after = model.evaluate_device(test.columns)
    print("held-out AUC %.4f -> %.4f over %d training rows" % (auc_before, after[2], len(y)))
    assert after == other.evaluate_device(test.columns) and after[2] > auc_before
    store = built.store()
    users, cand = np.array([30, 12, 8, 1, 17]), np.arange(1, 116, 2)
    got = model.recommend(store, users, cand, 10)
    assert got == other.recommend(store, users, cand, 10) and len(got[0]) == 10
    again = TP.fit(model, train.columns, batch_size=128, epochs=1, learning_rate=0.01)
    cont = TP.train_host(fam, want.weights, ids, dense, y, batch_size=128, epochs=1, learning_rate=0.01, state=(want.m, want.v, want.step))
    assert all(same(model.weights[k], cont.weights[k]) for k in cont.weights) and again[0][1:] == cont.history[0][1:]
    with pytest.raises(NotImplementedError, match=r"NeuralCF\(arch=1\) and EmbeddingMLP"):
        model.fit(tcols)


# ---------------------------------------------------------------- the step shape trainer_pair.fit ships with (docs/train_shapes_results.md)

ROUND = 2048 * 256                                                     # FE_MAX_GRID workgroups of 256 threads: what one trip of a strided loop covers
MORE_PAIRS = TPC.EIGHT_PAIRS + [("f0", "f0"), ("f3", "f3"), ("f7", "f1"), ("f5", "f5")]      # 32: all 28, then a reversed one and three (a, a)


def strides(items):
    """A loop over ``items`` elements, launched with fe_grid_capped(items) workgroups, makes a second trip (tests/test_gpu_grid_rounds.py)."""
    return items > L.load_library().sprk_segments_grid(items) * 256


@pytest.mark.parametrize("shared", SHARED)
@pytest.mark.parametrize("kw", [dict(), dict(fields=TPC.SIX, pairs=TPC.SIX_PAIRS, emb_dim=10)], ids=["reference", "config2"])
def test_batch_4096_at_the_default_tile(torch, kw, shared):
    """The reference's four pairs and config 2's eight over six fields x 10, N = 4096 + 77, one epoch: one full batch of ``DEFAULT_BATCH`` rows
    (512 tiles of 8: 64 trips of k_tp_dense_adam's unrolled partial sum) and a short one of 10 tiles."""
    fam, w, ids, dense, y = TPC.small(TP.DEFAULT_BATCH + 77, seed=21, shared=shared, **kw)
    assert TP.default_tile(fam) == TP.DEFAULT_TILE == 8
    want = both(fam, w, ids, dense, y, epochs=1)
    assert want.step == 2


@pytest.mark.parametrize("shared", SHARED)
def test_tile_one(torch, shared):
    """Tile 1 on 23 rows in batches of 7: every tile's partial sum is one sample's term."""
    fam, w, ids, dense, y = TPC.small(23, seed=23, shared=shared)
    both(fam, w, ids, dense, y, batch_size=7, epochs=2, tile=1)


@pytest.mark.parametrize("shared", SHARED)
def test_thirty_two_pairs(torch, shared):
    """``MAX_PAIRS`` = 32 over eight small fields: all 28 pairs, one of them again in reverse, three of the form ``(a, a)``."""
    fam, w, ids, dense, y = TPC.small(40, seed=37, fields=TPC.EIGHT, pairs=MORE_PAIRS, deep_emb=("f0", "f2"), shared=shared)
    assert len(fam.pairs) == TP.MAX_PAIRS and len(fam.fields) == TP.MAX_FIELDS
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


def test_every_maximum_at_once(torch):
    """Eight fields, 32 pairs, ``emb_dim`` 64 and eight hidden layers of 256 units at the default tile: 104 672 B of LDS, and no wider legal
    shape exists, so ``default_tile`` never falls below 8 for this trainer (docs/train_shapes_results.md).  28 rows, no tile named."""
    fam, w, ids, dense, y = TPC.small(28, seed=38, fields=TPC.EIGHT, pairs=MORE_PAIRS, deep_emb=("f0", "f2"), emb_dim=TP.MAX_DIM, hidden=(TP.MAX_WIDTH,) * TP.MAX_LAYERS)
    assert TP.default_tile(fam) == TP.DEFAULT_TILE and 48 * 1024 < TP.lds_bytes(fam, TP.DEFAULT_TILE) <= TP.LDS_BYTES
    both(fam, w, ids, dense, y, batch_size=16, epochs=2)


def test_dense_parameters_beyond_one_round_of_the_grid(torch):
    """Four deep tables of ``emb_dim`` 62 and seven numerics -- 255 of the 256 deep inputs -- under eight layers of 256: 526 341 floats in
    k_tp_dense_adam's loop, the hole of the first-order rows among them, so it goes past one round of its grid.  28 rows."""
    fam, w, ids, dense, y = TPC.small(28, seed=39, deep_emb=("movieId", "userId", "userGenre1", "movieGenre1"), emb_dim=62, hidden=(TP.MAX_WIDTH,) * TP.MAX_LAYERS)
    assert len(fam.xsrc) == 255 and strides(TPC.dense_floats(fam)) and TP.lds_bytes(fam, 8) <= TP.LDS_BYTES
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


@pytest.mark.parametrize("shared", SHARED)
def test_a_table_beyond_one_real_round_of_the_grid(torch, shared):
    """60 000 movies x 10: 600 000 floats of ``emb/movieId`` at the head of the parameter vector, more than the 524 288 one round of
    k_tp_table_adam's grid covers; ``deep_emb/movieId`` and the first-order rows of ``head/kernel`` lie wholly beyond it.  Step 1 hits rows 0,
    52 428, 52 429 and 59 999: elements 524 280 .. 524 299 lie on both sides of the round's end.  Those rows move in all three places; rows
    never hit keep their bits and zero moments; a row hit in step 1 only still moves in step 3."""
    fields = [("movieId", "id", 60000), ("userId", "id", 5), ("userGenre1", "genre", 4), ("movieGenre1", "genre", 3)]
    fam, w, ids, dense, y = TPC.small(40, seed=26, fields=fields, emb_dim=10, shared=shared)
    assert TP.param_names(fam)[0] == "emb/movieId" and strides(TPC.table_floats(fam)) and 52428 * 10 < ROUND <= 52429 * 10
    places = [("emb/movieId", 0), ("head/kernel", fam.fo_off[0])] + ([] if shared else [("deep_emb/movieId", 0)])
    first = np.array([0, 52428, 52429, 59999])
    ids[:16, 0] = first[np.arange(16) % 4]
    ids[16:, 0] = np.random.default_rng(26).integers(100, 50000, 24)
    one = both(fam, w, ids[:16], dense[:16], y[:16], batch_size=16, epochs=1, tile=8)
    two = both(fam, w, ids[:32], dense[:32], y[:32], batch_size=16, epochs=1, tile=8)
    three = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert three.step == 3
    never = np.ones(60000, dtype=bool)
    never[ids[:, 0]] = False
    rest = np.setdiff1d(np.arange(60000), first)
    assert never.sum() > 59900
    for name, r0 in places:
        for row in first:
            assert not same(one.weights[name][r0 + row], w[name][r0 + row]), (name, row)
            assert not same(three.weights[name][r0 + row], two.weights[name][r0 + row]), (name, row)    # hit in step 1 only: still moving
        rows = slice(r0, r0 + 60000)
        assert same(three.weights[name][rows][never], w[name][rows][never]) and not three.m[name][rows][never].any() and not three.v[name][rows][never].any()
        assert same(one.weights[name][r0 + rest], w[name][r0 + rest])


@pytest.mark.parametrize("batch,tile", [(4096, 32), (66000, 128)])
def test_the_schedule_beyond_one_round_of_the_grid(torch, batch, tile):
    """Eight fields, N = 66 000: 528 000 entries, so k_tr_count and k_tr_scatter make a second trip; in batches of 4 096 and as one batch,
    whose positions pass 65 535."""
    fam, w, ids, dense, y = TPC.small(66000, seed=27, fields=TPC.EIGHT, pairs=TPC.EIGHT_PAIRS, deep_emb=("f0", "f2"))
    assert strides(ids.size) and TP.lds_bytes(fam, tile) <= TP.LDS_BYTES and (batch == 4096 or batch == len(y) > 65536)
    both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=tile)


def test_the_error_word_beyond_one_round_of_the_grid(torch):
    """N = 524 288 + 600: bad labels at rows 524 300 and 524 500, both in k_tr_check's second trip.  The library and both routes name row
    524 300 and no parameter moves."""
    fam, w, ids, dense, y = TPC.small(ROUND + 600, seed=28)
    assert strides(len(y))
    y[524500], y[524300] = np.nan, np.inf
    flat0 = np.concatenate([w[k].reshape(-1) for k in TP.param_names(fam)])
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 65536, 16, 1)
    assert rc == 0 and intact and word == (T.ERR_LABEL << 32 | 524300), (word >> 32, word & 0xffffffff)
    assert same(params, flat0) and not m.any() and not v.any() and not p.any()
    for fit in (TP.train_device, TP.train_host):
        with pytest.raises(ValueError, match="samples row 524300: the label"):
            fit(fam, w, ids, dense, y, batch_size=65536, epochs=1, tile=16)
