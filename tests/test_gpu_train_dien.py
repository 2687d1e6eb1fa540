"""``trainer_dien.train_device`` (``sprk_train_dien_fit``, csrc/k_train_dien.h) against its definition ``trainer_dien.train_host``: every
weight, every ``m``, every ``v``, every ``p`` of the last epoch, accuracy and both AUCs of every epoch byte for byte, the loss within
``max(N, 64) 2^-50`` relative (``-m gpu``).  Tiny vocabularies and tens to a few hundred rows with about a third of the history ids 0, then
one step at batch 4096 at the default tile and the chain from ratings to recommendations."""
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
