"""``trainer_dien.train_device`` (``sprk_train_dien_fit``, csrc/k_train_dien.h) against its definition ``trainer_dien.train_host``: every
weight, every ``m``, every ``v``, every ``p`` of the last epoch, accuracy and both AUCs of every epoch byte for byte, the loss within
``max(N, 64) 2^-50`` relative (``-m gpu``).  Tiny vocabularies and tens to a few hundred rows with about a third of the history ids 0, then
the step shape ``trainer_dien.fit`` ships with: batch 4096 at the default tile, the tiles below it and a tile wider than the workgroup, the
stated maxima, a table, Dense parameters and schedules beyond one round of a grid (docs/train_dien_results.md section 4), and the chain from
ratings to recommendations."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_dien as TE
from tests import metrics_cases as MC
from tests import train_dien_cases as TEC

pytestmark = pytest.mark.gpu
F = np.float32
same = TEC.same_bits


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


def host_of(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def both(fam, w, ids, dense, y, **kw):
    """Host and device fits of one input: asserts the equalities of the module docstring, -> the host's result."""
    want = TE.train_host(fam, w, ids, dense, y, **kw)
    got = TE.train_device(fam, w, ids, dense, y, **kw)
    assert got.step == want.step and len(got.history) == len(want.history)
    for name, g, h in (("weight", got.weights, want.weights), ("m", got.m, want.m), ("v", got.v, want.v)):
        g = host_of(g)
        for k in TE.param_names(fam):
            assert same(g[k], h[k]), (name, k, np.flatnonzero(g[k].reshape(-1).view(np.uint32) != h[k].reshape(-1).view(np.uint32))[:8])
    p = got.p.cpu().numpy()
    assert same(p, want.p), np.flatnonzero(p.view(np.uint32) != want.p.view(np.uint32))[:8]
    for e, (a, b) in enumerate(zip(got.history, want.history)):
        assert a[1:] == b[1:] or (np.isnan(a[2:]).all() and np.isnan(b[2:]).all() and a[1] == b[1]), (e, a, b)
        assert abs(a[0] - b[0]) <= MC.loss_bound(len(y)) * abs(b[0]), (e, a[0], b[0])
    return want


# ---------------------------------------------------------------- rows and batches

@pytest.mark.parametrize("n,batch,tile", [(1, 4, 8), (7, 16, 8), (8, 16, 8), (9, 16, 8), (50, 12, 8), (23, 1, 8), (33, 32, 32)])
def test_row_counts_and_batching(torch, n, batch, tile):
    """N = 1, tile - 1, tile, tile + 1; B no multiple of the tile; a short last batch; B = 1; three epochs."""
    fam, w, ids, dense, y = TEC.small(n, seed=n)
    want = both(fam, w, ids, dense, y, batch_size=batch, epochs=3, tile=tile)
    assert want.step == 3 * ((n + batch - 1) // batch)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_order(torch, as_tensor):
    fam, w, ids, dense, y = TEC.small(50, seed=4)
    order = np.random.default_rng(1).permutation(50)
    want = TE.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8, order=order)
    plain = TE.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8)
    assert not same(want.weights["fc0/kernel"], plain.weights["fc0/kernel"])
    dev = lambda a: torch.from_numpy(a).cuda()
    got = TE.train_device(fam, w, dev(ids), dev(dense), dev(y), batch_size=12, epochs=3, tile=8, order=dev(order) if as_tensor else order)
    assert all(same(host_of(got.weights)[k], want.weights[k]) for k in want.weights)
    assert same(got.p.cpu().numpy(), want.p) and [h[1:] for h in got.history] == [h[1:] for h in want.history]
    with pytest.raises(ValueError, match="permutation"):
        TE.train_device(fam, w, ids, dense, y, order=dev(np.zeros(50, dtype=np.int64)) if as_tensor else np.zeros(50, dtype=np.int64))


# ---------------------------------------------------------------- widths

@pytest.mark.parametrize("kw", [dict(hist_len=1), dict(hist_len=5), dict(hist_len=12), dict(emb_dim=1), dict(emb_dim=10), dict(emb_dim=16), dict(emb_dim=17),
                                dict(emb_dim=64, others=False), dict(att_hidden=1), dict(att_hidden=31), dict(att_hidden=32), dict(att_hidden=33), dict(att_hidden=64),
                                dict(hidden=(1,)), dict(hidden=(64, 65)), dict(hidden=(128, 64)), dict(hidden=(7, 6, 5)), TEC.REFERENCE_SHAPE])
def test_slots_widths_and_tails(torch, kw):
    """T 1, 3 (the other cases), 5 and 12; D 1, 3, 10, 16 (the widest whose recurrent weights are staged in LDS), 17 (the first read from
    L2) and 64 (a family without the user and genre columns: ``fc0`` has 256 input rows at most); H 1, 5, 31, 32, 33 and 64; tails (1,),
    (64, 65), (128, 64) and (7, 6, 5); the reference shape."""
    fam, w, ids, dense, y = TEC.small(40, seed=sum(map(ord, repr(sorted(kw.items())))) % 97, **kw)
    assert (fam.emb_dim <= TE.STAGE_EMB) == (TE.lds_bytes(fam, 0) > 0)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=4 if fam.emb_dim == 64 else 8)


# ---------------------------------------------------------------- masks

def test_all_slots_masked(torch):
    fam, w, ids, dense, y = TEC.small(40, seed=31)
    ids[:, 1:4] = 0
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    for k in ("gru/kernel", "gru_rec/kernel", "gru/bias"):
        assert same(got.weights[k], w[k]) and not got.m[k].any() and not got.v[k].any(), k
    assert (ids[:, 0] == 0).any() and not same(got.weights["emb/movie"][0], w["emb/movie"][0])
    ids[:, 0] = 1 + ids[:, 0] % 6
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert same(got.weights["emb/movie"][0], w["emb/movie"][0]) and not got.v["emb/movie"][0].any()


@pytest.mark.parametrize("hist", [(0, 2, 3), (2, 0, 3), (0, 0, 3), (3, 0, 0)])
def test_mask_patterns(torch, hist):
    """Only the first slot 0; a 0 between two movies; only the last slot non-zero; only the first: every sample carries the pattern, the
    movies themselves vary."""
    fam, w, ids, dense, y = TEC.small(40, seed=32)
    ids[:, 1:4] = np.where(np.array(hist) == 0, 0, 1 + (ids[:, 1:4] + np.array(hist)) % 6)
    assert ((ids[:, 1:4] == 0) == (np.array(hist) == 0)).all()
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert got.m["gru/kernel"].any()


# ---------------------------------------------------------------- ids

def test_every_genre_id_none(torch):
    fam, w, ids, dense, y = TEC.small(40, seed=3)
    ids[:, 5:] = -1
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    for k in ("emb/userGenre1", "emb/movieGenre1"):
        assert same(got.weights[k], w[k]) and not got.v[k].any()
    assert not same(got.weights["emb/userId"], w["emb/userId"])


def test_one_movie_in_every_column_of_every_sample(torch):
    """All samples carry movie 3 in all T + 1 columns: one run of (T + 1) B entries per batch, and every other movie row never hit."""
    fam, w, ids, dense, y = TEC.small(48, seed=2, hist_len=5)
    ids[:, :6] = 3
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    keep = np.arange(7) != 3
    assert same(got.weights["emb/movie"][keep], w["emb/movie"][keep]) and not same(got.weights["emb/movie"][3], w["emb/movie"][3])


def test_a_candidate_that_is_also_in_two_slots(torch):
    fam, w, ids, dense, y = TEC.small(48, seed=5)
    ids[:, :4] %= 4
    ids[9, :4] = np.array([2, 2, 1, 2])
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


def test_vocabularies_of_one(torch):
    """One movie, one user, one genre: every history id is 0 (masked) and so is every candidate."""
    fam, w, ids, dense, y = TEC.small(40, seed=33, movies=1, users=1, genres=1)
    assert not ids[:, :5].any()
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert not got.m["gru/kernel"].any() and got.m["emb/movie"].any()


# ---------------------------------------------------------------- arithmetic edges

@pytest.mark.parametrize("scale", [100.0, -100.0])
def test_saturated_gates_and_tanh_at_one(torch, scale):
    """Large recurrent weights: the GRU's and the AUGRU's sigmoids at 0 and 1 and ``tanh_def`` at -1 and 1 exactly."""
    fam, w, ids, dense, y = TEC.small(40, seed=34)
    for k in ("gru/bias", "augru_r_out/bias", "augru_z_out/bias", "augru_h_out/bias"):
        w[k][...] = scale
    keep = {}
    TE.forward_host(fam, w, ids, dense, keep)
    assert set(np.unique(keep["hc"]).tolist()) == {1.0 if scale > 0 else -1.0} and set(np.unique(keep["rt"]).tolist()) <= {0.0, 1.0}
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


@pytest.mark.parametrize("bias", [100.0, -100.0])
def test_a_saturated_attention_gate_and_head(torch, bias):
    fam, w, ids, dense, y = TEC.small(40, seed=8)
    w["att1/bias"][0] = bias
    got = both(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    for k in ("att0/kernel", "att0/bias", "att1/kernel", "att1/bias"):
        assert same(got.weights[k], w[k]) and not got.m[k].any(), k
    w["att1/bias"][0] = 0.0
    w["head/bias"][0] = bias
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert set(np.unique(got.p).tolist()) <= ({1.0} if bias > 0 else {0.0})


def test_prelu_at_exactly_zero(torch):
    fam, w, ids, dense, y = TEC.small(40, seed=6, hidden=(4, 3))
    w["fc0/kernel"][:, 0] = 0.0
    w["fc0/bias"][0] = 0.0
    got = both(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    assert not got.m["fc0/kernel"][:, 0].any() and not got.m["fc0/bias"][0] and not got.m["fc0_prelu/alpha"][0] and not got.m["fc1/kernel"][0].any()


@pytest.mark.parametrize("scale", [1e-20, 1e-39])
def test_tiny_and_subnormal_weights(torch, scale):
    fam, w, ids, dense, y = TEC.small(40, seed=8)
    w = {k: (v.astype(np.float64) * scale).astype(F) for k, v in w.items()}
    tiny = np.finfo(F).tiny
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    sub = lambda d: any(((np.abs(a) > 0) & (np.abs(a) < tiny)).any() for a in d.values())
    assert sub(got.m) if scale == 1e-20 else sub(w)


def test_batches_beyond_the_lds_sort_capacity(torch, monkeypatch):
    """SPRK_FE_SORT_CAP=64: a batch's 40 x 7 entries take the chunked sort and the merge passes."""
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    fam, w, ids, dense, y = TEC.small(100, seed=9)
    both(fam, w, ids, dense, y, batch_size=40, epochs=2, tile=8)


@pytest.mark.parametrize("grid", ["3", "1"])
def test_grids_capped(torch, monkeypatch, grid):
    """SPRK_FE_MAX_GRID 3 and 1: every grid-stride loop of the schedule and of the two Adam kernels goes round."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", grid)
    fam, w, ids, dense, y = TEC.small(300, seed=10, **TEC.REFERENCE_SHAPE)
    assert ids.size > 3 * 256 and sum(a.size for a in w.values()) > 3 * 256
    both(fam, w, ids, dense, y, batch_size=128, epochs=1, tile=8)


# ---------------------------------------------------------------- the C ABI: errors, memory, streams

GUARD = 64


def raw_fit(torch, fam, w, ids, dense, y, batch, tile, epochs, stream=None):
    """``sprk_train_dien_fit`` itself: parameters, moments, p and the workspace each inside guard bands of a fixed pattern, the workspace
    exactly as large as ``sprk_train_dien_workspace_bytes`` reports.  -> (rc, params, m, v, p, error word, guards intact)."""
    lib = L.load_library()
    dev = torch.device("cuda")
    n = len(y)
    flat = TE._flatten(fam, w, dev)
    ms = TE._model_struct(fam)
    need = int(lib.sprk_train_dien_workspace_bytes(C.byref(ms), n, batch, tile))
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
    rc = lib.sprk_train_dien_fit(C.byref(ms), C.c_void_p(t_ids.data_ptr()), C.c_void_p(t_dense.data_ptr()), C.c_void_p(t_y.data_ptr()), None,
                                 n, batch, tile, epochs, C.c_void_p(alphas.data_ptr()), float(c1), float(c2), float(eps), at(params, 4), at(m, 4), at(v, 4), at(p, 4),
                                 C.c_void_p(word.data_ptr()), at(ws, 1), need, C.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream))
    (stream or torch.cuda.current_stream()).synchronize()
    intact = all(bool((b[:GUARD] == b[0]).all()) and bool((b[-GUARD:] == b[0]).all()) and (float(b[0]) in (-7.0, 90.0)) for b in (params, m, v, p, ws))
    cut = lambda b: b[GUARD:-GUARD].cpu().numpy()
    return rc, cut(params), cut(m), cut(v), cut(p), int(word.cpu()[0]), intact


def test_guard_bands_side_stream_exact_workspace(torch):
    fam, w, ids, dense, y = TEC.small(50, seed=10)
    want = TE.train_host(fam, w, ids, dense, y, batch_size=12, epochs=2, tile=8)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 12, 8, 2, stream=side)
    assert rc == 0 and word == -1 and intact
    flat = lambda d: np.concatenate([d[k].reshape(-1) for k in TE.param_names(fam)])
    assert same(params, flat(want.weights)) and same(m, flat(want.m)) and same(v, flat(want.v))
    assert same(p[50:], want.p)


def test_each_error_word_and_no_parameter_moves(torch):
    fam, w, ids, dense, y = TEC.small(40, seed=11)
    flat0 = np.concatenate([w[k].reshape(-1) for k in TE.param_names(fam)])

    def check(kind, row, message, ids=ids, dense=dense, y=y):
        rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 16, 8, 2)
        assert rc == 0 and intact and word == (kind << 32 | row), (word >> 32, word & 0xffffffff)
        assert same(params, flat0) and not m.any() and not v.any()
        for fit in (TE.train_device, TE.train_host):
            with pytest.raises(ValueError, match=message):
                fit(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    bad = ids.copy(); bad[30, 0] = 7; bad[12, 2] = -1; bad[20, 5] = -2
    check(T.ERR_ID, 12, "samples row 12: an id outside", ids=bad)
    bad = dense.copy(); bad[9, 1] = np.inf; bad[3, 0] = np.nan
    check(T.ERR_NUMERIC, 3, "samples row 3: a numeric", dense=bad)
    bad = y.copy(); bad[7] = np.nan; bad[39] = -np.inf
    check(T.ERR_LABEL, 7, "samples row 7: the label", y=bad)


def test_a_fit_continues(torch):
    fam, w, ids, dense, y = TEC.small(120, seed=12)
    a = TE.train_device(fam, w, ids, dense, y, batch_size=48, epochs=2, tile=8)
    one = TE.train_device(fam, w, ids, dense, y, batch_size=48, epochs=1, tile=8)
    two = TE.train_device(fam, one.weights, ids, dense, y, batch_size=48, epochs=1, tile=8, state=(one.m, one.v, one.step))
    assert two.step == a.step and all(same(two.weights[k].cpu().numpy(), a.weights[k].cpu().numpy()) and same(two.v[k].cpu().numpy(), a.v[k].cpu().numpy()) for k in w)
    none = TE.train_device(fam, w, ids, dense, y, epochs=0)
    assert none.step == 0 and none.history == [] and all(same(none.weights[k].cpu().numpy(), w[k]) for k in w)


def test_lds_refusal_in_words_and_a_step_of_more_than_48_kb(torch):
    fam, w, ids, dense, y = TEC.small(40, seed=13, **TEC.REFERENCE_SHAPE)
    once = TE.lds_bytes(fam, 0)
    top = (TE.LDS_BYTES - once) // (TE.lds_bytes(fam, 1) - once)
    with pytest.raises(ValueError, match="tile = %d needs %d bytes of LDS" % (top + 1, TE.lds_bytes(fam, top + 1))):
        TE.train_device(fam, w, ids, dense, y, batch_size=20, epochs=1, tile=top + 1)
    assert 48 * 1024 < TE.lds_bytes(fam, 8) <= TE.LDS_BYTES
    both(fam, w, ids, dense, y, batch_size=40, epochs=2, tile=8)


# ---------------------------------------------------------------- the step shape trainer_dien.fit ships with

def test_batch_4096_at_the_default_tile(torch):
    """The reference shape, N = 4096 + 37, one epoch: one full batch of ``DEFAULT_BATCH`` rows and a short one."""
    fam, w, ids, dense, y = TEC.small(TE.DEFAULT_BATCH + 37, seed=21, **TEC.REFERENCE_SHAPE)
    assert TE.default_tile(fam) == TE.DEFAULT_TILE
    want = both(fam, w, ids, dense, y, epochs=1)
    assert want.step == 2


ROUND = 2048 * 256                                                     # FE_MAX_GRID workgroups of 256 threads: what one trip of a strided loop covers


def strides(items):
    """A loop over ``items`` elements, launched with fe_grid_capped(items) workgroups, makes a second trip (tests/test_gpu_grid_rounds.py)."""
    return items > L.load_library().sprk_segments_grid(items) * 256


def top_tile(fam):
    """The largest tile whose ``lds_bytes`` fit the LDS."""
    once = TE.lds_bytes(fam, 0)
    return (TE.LDS_BYTES - once) // (TE.lds_bytes(fam, 1) - once)


def test_batch_4096_at_the_default_tile_with_twelve_slots(torch):
    """The reference shape with T = 12, N = 4096 + 37, one epoch: ``default_tile`` is still 8 (143 312 B of LDS; 9 is the largest tile that
    fits), 512 tiles and then 5."""
    fam, w, ids, dense, y = TEC.small(TE.DEFAULT_BATCH + 37, seed=41, **dict(TEC.REFERENCE_SHAPE, hist_len=12))
    assert TE.default_tile(fam) == TE.DEFAULT_TILE == 8 and TE.lds_bytes(fam, 8) == 143312 <= TE.LDS_BYTES and top_tile(fam) == 9
    want = both(fam, w, ids, dense, y, epochs=1)
    assert want.step == 2


@pytest.mark.parametrize("tile", [None, 3])
def test_the_default_tile_falls_to_what_the_lds_holds(torch, tile):
    """T = 12, H = 256, D = 16 (the recurrent weights still staged): tiles 1, 2 and 3 fit the LDS (3 takes 145 032 B) and 4 does not, so
    ``default_tile`` halves from 8 to 2.  A fit that names no tile, and tile 3, the largest that fits."""
    fam, w, ids, dense, y = TEC.small(40, seed=42, hist_len=12, att_hidden=256, emb_dim=16)
    assert [TE.lds_bytes(fam, t) <= TE.LDS_BYTES for t in (1, 2, 3, 4, 8)] == [True, True, True, False, False] and TE.lds_bytes(fam, 3) == 145032
    assert TE.default_tile(fam) == 2 < TE.DEFAULT_TILE and top_tile(fam) == 3
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=tile)


def test_the_default_tile_falls_to_one(torch):
    """D = 64 at T = 12 and H = 256 (the movie columns alone): one sample takes 95 768 B and two do not fit, so a fit that names no tile
    runs at tile 1, its recurrent weights read from L2."""
    fam, w, ids, dense, y = TEC.small(40, seed=43, emb_dim=64, hist_len=12, att_hidden=256, others=False)
    assert [TE.lds_bytes(fam, t) <= TE.LDS_BYTES for t in (1, 2, 4, 8)] == [True, False, False, False] and TE.lds_bytes(fam, 1) == 95768
    assert TE.default_tile(fam) == 1 and TE.lds_bytes(fam, 0) == 0
    both(fam, w, ids, dense, y, batch_size=16, epochs=2)


def test_tile_one(torch):
    """Tile 1 on 23 rows in batches of 7: every tile's partial sum is one sample's term."""
    fam, w, ids, dense, y = TEC.small(23, seed=44)
    both(fam, w, ids, dense, y, batch_size=7, epochs=2, tile=1)


@pytest.mark.parametrize("batch", [56, 64, 72, 120, 128, 136])
def test_tile_counts_around_the_unrolled_partial_sum(torch, batch):
    """Tile 8: 7, 8, 9, 15, 16 and 17 tiles -- k_tr_dense_adam adds eight partials at a time, then the rest, here over the GRU's, the gate's
    and the AUGRU's arrays in front of the tail -- and a last batch of 5 rows."""
    fam, w, ids, dense, y = TEC.small(batch + 5, seed=batch)
    assert batch // 8 in (7, 8, 9, 15, 16, 17) and batch % 8 == 0
    want = both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=8)
    assert want.step == 2


@pytest.mark.parametrize("kw,tile", [(dict(hist_len=1, att_hidden=1, hidden=(1,)), 281), (dict(hist_len=1, att_hidden=1, hidden=(1,), emb_dim=1), 300)])
def test_a_tile_wider_than_the_workgroup(torch, kw, tile):
    """A tile of more than 256 samples: every per-sample loop of k_te_step (the head, ``da_t``, ``dl``, ...) goes round.  The tile is 300 or the
    largest that ``lds_bytes`` lets into 160 KB: 281 for T = H = 1 with a tail of (1,) at D = 3 (580 B a sample and 684 B once), 300 at
    D = 1.  N = batch = 650: three tiles, the last of 88 or 50 rows."""
    fam, w, ids, dense, y = TEC.small(650, seed=45, **kw)
    if fam.emb_dim == 3:
        assert TE.lds_bytes(fam, 0) == 684 and TE.lds_bytes(fam, 1) - TE.lds_bytes(fam, 0) == 580
    assert tile == min(300, top_tile(fam)) > 256 and TE.lds_bytes(fam, tile) <= TE.LDS_BYTES
    want = both(fam, w, ids, dense, y, batch_size=650, epochs=2, tile=tile)
    assert want.step == 2 and (650 + tile - 1) // tile == 3


MAXIMA = [(dict(emb_dim=49), 8, 135904, None, False, 28, 16),
          (dict(hist_len=12, att_hidden=256), 4, 113692, None, False, 28, 16),
          (dict(hidden=(256,) * 8), 8, 157900, 468937, False, 28, 16),
          (dict(emb_dim=64, hidden=(256,) * 8, others=False), 4, 155424, 560268, True, 28, 16),
          (dict(emb_dim=64, hist_len=12, att_hidden=256, hidden=(256,) * 8, others=False), 1, 114072, 576834, True, 12, 8)]


@pytest.mark.parametrize("kw,tile,lds,floats,round_,n,batch", MAXIMA)
def test_the_stated_maxima(torch, kw, tile, lds, floats, round_, n, batch):
    """``emb_dim`` 49, the largest that leaves room for the user and genre columns (252 of ``fc0``'s 256 input rows; 50 is refused); H = 256 at
    T = 12 (the gate's loops run over 3 072 elements a sample); eight tail layers of 256 units, whose 468 937 Dense floats stay inside one round;
    the same tail under D = 64, whose 560 268 Dense floats send k_tr_dense_adam past one round of its grid with the GRU's and the AUGRU's arrays
    in front of the tail; and every maximum at once (576 834 Dense floats, the recurrent weights read from L2 at T = 12, one sample a tile)."""
    fam, w, ids, dense, y = TEC.small(n, seed=46, **kw)
    assert TE.lds_bytes(fam, tile) == lds <= TE.LDS_BYTES and strides(TEC.dense_floats(fam)) == round_
    assert floats is None or TEC.dense_floats(fam) == floats
    if kw == dict(emb_dim=49):
        assert fam.fan0 == 252
        with pytest.raises(ValueError, match="trainer_dien takes up to"):
            TEC.family(emb_dim=50)
    if "hist_len" in kw:
        assert fam.hist_len * fam.att_hidden == 3072
    both(fam, w, ids, dense, y, batch_size=batch, epochs=2, tile=tile)


def test_a_table_beyond_one_round_of_the_grid(torch):
    """60 000 movies x 10: 600 000 floats of ``emb/movie`` at the head of the parameter vector, more than the 524 288 one round of
    k_td_table_adam's grid covers.  Step 1 hits rows 0 and 52 428 through the candidate -- a history id 0 makes no entry, so row 0 has no
    other way -- and rows 52 429 and 59 999 through a history slot: elements 524 280 .. 524 299 lie on both sides of the round's end.  Those
    rows move; rows never hit keep their bits and zero moments; a row hit in step 1 only still moves in step 3; and with no candidate 0, the
    samples whose first slot holds 0 leave row 0 as it was."""
    fam, w, ids, dense, y = TEC.small(40, seed=47, movies=60000, emb_dim=10)
    mv, T = "emb/movie", fam.hist_len
    assert TE.param_names(fam)[0] == mv and w[mv].shape == (60000, 10) and strides(TEC.table_floats(fam))
    assert 52428 * 10 < ROUND <= 52429 * 10
    first = np.array([0, 52428, 52429, 59999])
    ids[:, :T + 1] = np.random.default_rng(47).integers(100, 50000, (40, T + 1))
    ids[5::7, 1] = 0                                                                                    # masked slots in every step
    ids[:16, 0] = first[np.arange(16) % 2]
    ids[:16, 2] = first[2 + np.arange(16) % 2]
    assert (ids[16:, 0] != 0).all() and (ids[:16, 1] == 0).any() and (ids[16:32, 1] == 0).any() and (ids[32:, 1] == 0).any()
    one = both(fam, w, ids[:16], dense[:16], y[:16], batch_size=16, epochs=1, tile=8)
    two = both(fam, w, ids[:32], dense[:32], y[:32], batch_size=16, epochs=1, tile=8)
    three = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert three.step == 3
    for row in first:
        assert not same(one.weights[mv][row], w[mv][row])
        assert not same(three.weights[mv][row], two.weights[mv][row])                                   # hit in step 1 only: still moving
    never = np.ones(60000, dtype=bool)
    never[ids[:, :T + 1]] = False
    assert never.sum() > 59800 and same(three.weights[mv][never], w[mv][never]) and not three.m[mv][never].any() and not three.v[mv][never].any()
    rest = np.ones(60000, dtype=bool)
    rest[ids[:16, :T + 1]] = False
    assert same(one.weights[mv][rest], w[mv][rest]) and not one.v[mv][rest].any()
    masked = ids[:16].copy()
    masked[:, 0] = 52428
    assert (masked[:, 1:T + 1] == 0).any() and (masked[:, 0] != 0).all()
    none = both(fam, w, masked, dense[:16], y[:16], batch_size=16, epochs=1, tile=8)
    assert same(none.weights[mv][0], w[mv][0]) and not none.m[mv][0].any() and not none.v[mv][0].any() and not same(none.weights[mv][52428], w[mv][52428])


@pytest.mark.parametrize("batch,tile", [(4096, 32), (100000, 64)])
def test_the_schedule_beyond_one_round_of_the_grid(torch, batch, tile):
    """Seven id columns, N = 100 000: 700 000 elements for k_te_count and k_te_scatter to walk, of which the masked slots and the genre ids
    -1 make no entry; the entries kept are still more than 524 288, so the sort's and the table kernel's view of them passes one round too.
    In batches of 4 096 at tile 32 and as one batch at tile 64 (121 is the largest tile that fits), whose positions pass 65 535 in keys
    that hold position x 16 + column."""
    fam, w, ids, dense, y = TEC.small(100000, seed=48)
    kept = TEC.kept_entries(fam, ids)
    assert ids.size == 700000 and ROUND < kept < ids.size and strides(ids.size) and strides(kept)
    assert TE.lds_bytes(fam, tile) <= TE.LDS_BYTES and top_tile(fam) == 121 and (batch == 4096 or batch == len(y) > 65536)
    both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=tile)


def test_the_error_word_beyond_one_round_of_the_grid(torch):
    """N = 524 288 + 600: bad labels at rows 524 300 and 524 500, both in k_tr_check's second trip.  The library and both routes name row
    524 300 and no parameter moves."""
    fam, w, ids, dense, y = TEC.small(ROUND + 600, seed=49)
    assert strides(len(y))
    y[524500], y[524300] = np.nan, np.inf
    flat0 = np.concatenate([w[k].reshape(-1) for k in TE.param_names(fam)])
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 65536, 16, 1)
    assert rc == 0 and intact and word == (T.ERR_LABEL << 32 | 524300), (word >> 32, word & 0xffffffff)
    assert same(params, flat0) and not m.any() and not v.any()
    for fit in (TE.train_device, TE.train_host):
        with pytest.raises(ValueError, match="samples row 524300: the label"):
            fit(fam, w, ids, dense, y, batch_size=65536, epochs=1, tile=16)


# ---------------------------------------------------------------- trainer_dien.fit

def test_ratings_to_recommendations(torch):
    """3 900 synthetic ratings whose label the candidate carries (tests/train_dien_cases.py planted_ratings()): featureeng.build -> split(mode="time") -> trainer_dien.fit -> evaluate_device -> recommend.  The
    held-out ROC AUC after fitting is above that of the untrained weights on the same rows, the weights are ``train_host``'s, and ``predict``
    (k_dien_fused) serves them: within 2e-6 of ``forward_host``, the bound of the DIEN parity tests (tests/test_gpu_shape_sweep.py)."""
    from sparrowrecsys_amd import featureeng as FE
    from tests import featureeng_cases as cases
    ratings, movies = TEC.planted_ratings(), cases.synthetic_movies()
    built = FE.build(ratings, movies, 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    train, test = built.split(mode="time", sample=1.0)
    make = lambda: M.DIEN(seed=3, movie_buckets=cases.N_MOVIES, user_buckets=cases.N_USERS)
    model, other = make(), make()
    start = {k: v.copy() for k, v in model.weights.items()}
    before = model.evaluate_device(test.columns)
    history = TE.fit(model, train.columns, batch_size=256, epochs=3, learning_rate=0.01)
    after = model.evaluate_device(test.columns)
    print("held-out [loss, accuracy, roc_auc, pr_auc] before %r after %r; training history %r" % (before, after, history))
    assert len(history) == 3 and after[2] > before[2]
    tcols = train.to_host()
    ids, dense = other.pack(tcols)
    y = np.asarray(tcols["label"], dtype=F)
    fam = TE.family_of(other)
    want = TE.train_host(fam, start, ids, dense, y, batch_size=256, epochs=3, learning_rate=0.01)
    assert len(y) > 1000 and all(same(model.weights[k], want.weights[k]) for k in want.weights)
    assert [h[1:] for h in history] == [h[1:] for h in want.history] and not same(model.weights["augru/h0"], start["augru/h0"])
    hcols = test.to_host()
    hids, hdense = other.pack(hcols)
    served = model.predict(hcols)[:, 0]
    err = float(np.abs(served.astype(np.float64) - TE.forward_host(fam, want.weights, hids, hdense)).max())
    print("predict against forward_host on the trained weights: %.3e over %d rows" % (err, len(served)))
    assert err <= 2e-6
    store = built.store()
    users, cand = np.array([30, 12, 8, 1, 17]), np.arange(1, 116, 2)
    got = model.recommend(store, users, cand, 10)
    other.set_weights(want.weights)
    assert got == other.recommend(store, users, cand, 10) and len(got[0]) == 10
    with pytest.raises(NotImplementedError):
        model.fit(tcols)
