"""``trainer_din.train_device`` (``sprk_train_din_fit``, csrc/k_train_din.h) against its definition ``trainer_din.train_host``: every weight,
every ``m``, every ``v``, every ``p`` of the last epoch, accuracy and both AUCs of every epoch byte for byte, the loss within
``max(N, 64) 2^-50`` relative (``-m gpu``).  Tiny vocabularies and tens to a few hundred rows, then the step shape ``trainer_din.fit`` ships
with: batch 4096 at the default tile, the tiles below it, the stated maxima, tables, Dense parameters and schedules beyond one round of a grid
(docs/train_shapes_results.md)."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_din as TD
from sparrowrecsys_amd import trainer_fm as TF
from tests import metrics_cases as MC
from tests import train_cases as TC
from tests import train_din_cases as TDC

pytestmark = pytest.mark.gpu
F = np.float32
same = TDC.same_bits


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


def host_of(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def both(fam, w, ids, dense, y, **kw):
    """Host and device fits of one input: asserts the equalities of the module docstring, -> the host's result."""
    want = TD.train_host(fam, w, ids, dense, y, **kw)
    got = TD.train_device(fam, w, ids, dense, y, **kw)
    assert got.step == want.step and len(got.history) == len(want.history)
    for name, g, h in (("weight", got.weights, want.weights), ("m", got.m, want.m), ("v", got.v, want.v)):
        g = host_of(g)
        for k in TD.param_names(fam):
            assert same(g[k], h[k]), (name, k, np.flatnonzero(g[k].reshape(-1).view(np.uint32) != h[k].reshape(-1).view(np.uint32))[:8])
    p = got.p.cpu().numpy()
    assert same(p, want.p), np.flatnonzero(p.view(np.uint32) != want.p.view(np.uint32))[:8]
    for e, (a, b) in enumerate(zip(got.history, want.history)):
        assert a[1:] == b[1:] or (np.isnan(a[2:]).all() and np.isnan(b[2:]).all() and a[1] == b[1]), (e, a, b)
        assert abs(a[0] - b[0]) <= MC.loss_bound(len(y)) * abs(b[0]), (e, a[0], b[0])
    return want


# ---------------------------------------------------------------- rows and batches

@pytest.mark.parametrize("n,batch,tile", [(1, 4, 8), (7, 16, 8), (8, 16, 8), (9, 16, 8), (50, 12, 8), (23, 1, 8), (40, 12, 32), (30, 64, 8), (33, 32, 32)])
def test_row_counts_and_batching(torch, n, batch, tile):
    """N = 1, tile - 1, tile, tile + 1; B no multiple of the tile; a short last batch; B = 1; one batch only; three epochs."""
    fam, w, ids, dense, y = TDC.small(n, seed=n)
    want = both(fam, w, ids, dense, y, batch_size=batch, epochs=3, tile=tile)
    assert want.step == 3 * ((n + batch - 1) // batch)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_order(torch, as_tensor):
    fam, w, ids, dense, y = TDC.small(50, seed=4)
    order = np.random.default_rng(1).permutation(50)
    want = TD.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8, order=order)
    plain = TD.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8)
    assert not same(want.weights["fc0/kernel"], plain.weights["fc0/kernel"])
    dev = lambda a: torch.from_numpy(a).cuda()
    got = TD.train_device(fam, w, dev(ids), dev(dense), dev(y), batch_size=12, epochs=3, tile=8, order=dev(order) if as_tensor else order)
    assert all(same(host_of(got.weights)[k], want.weights[k]) for k in want.weights)
    assert same(got.p.cpu().numpy(), want.p) and [h[1:] for h in got.history] == [h[1:] for h in want.history]
    with pytest.raises(ValueError, match="permutation"):
        TD.train_device(fam, w, ids, dense, y, order=dev(np.zeros(50, dtype=np.int64)) if as_tensor else np.zeros(50, dtype=np.int64))


# ---------------------------------------------------------------- widths

@pytest.mark.parametrize("kw", [dict(hist_len=1), dict(hist_len=5), dict(hist_len=12), dict(emb_dim=10), dict(att_hidden=1), dict(att_hidden=31), dict(att_hidden=32),
                                dict(att_hidden=33), dict(att_hidden=64), dict(hidden=(1,)), dict(hidden=(64, 65)), dict(hidden=(128, 64)), dict(hidden=(7, 6, 5)),
                                TDC.REFERENCE_SHAPE, TDC.ODD_SHAPE])
def test_slots_widths_and_tails(torch, kw):
    """T 1, 3 (the other cases), 5 and 12; D 3 and 10; H 1, 5, 31, 32, 33 and 64; tails (1,), (64, 65), (128, 64) and (7, 6, 5); the
    reference shape and the odd one."""
    fam, w, ids, dense, y = TDC.small(40, seed=sum(map(ord, repr(sorted(kw.items())))) % 97, **kw)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


# ---------------------------------------------------------------- ids

def test_every_genre_id_none(torch):
    fam, w, ids, dense, y = TDC.small(40, seed=3)
    ids[:, 5:] = -1
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    for k in ("emb/userGenre1", "emb/movieGenre1"):
        assert same(got.weights[k], w[k]) and not got.v[k].any()
    assert not same(got.weights["emb/userId"], w["emb/userId"])


def test_one_movie_in_every_column_of_every_sample(torch):
    """All samples carry movie 3 in all T + 1 columns: one run of (T + 1) B entries per batch, and every other movie row never hit."""
    fam, w, ids, dense, y = TDC.small(48, seed=2, hist_len=5)
    ids[:, :6] = 3
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    keep = np.arange(7) != 3
    assert same(got.weights["emb/movie"][keep], w["emb/movie"][keep]) and not same(got.weights["emb/movie"][3], w["emb/movie"][3])


def test_rows_hit_three_times_by_one_sample_once_never_and_in_step_one_only(torch):
    """Sample 9 has its candidate in two slots (three entries of one row in one tile); movie 6 is hit exactly once; movie 5 never;
    movie 4 in step 1 only, and it keeps moving."""
    fam, w, ids, dense, y = TDC.small(48, seed=5)
    ids[:, :4] %= 4
    ids[9, :4] = np.array([2, 2, 1, 2])
    ids[3, 2] = 4
    ids[20, 0] = 6
    assert (ids[16:, :4] != 4).all()
    one = both(fam, w, ids[:16], dense[:16], y[:16], batch_size=16, epochs=1, tile=8)
    mv = "emb/movie"
    assert same(one.weights[mv][5:], w[mv][5:]) and not same(one.weights[mv][4], w[mv][4])
    two = both(fam, w, ids[:32], dense[:32], y[:32], batch_size=16, epochs=1, tile=8)
    three = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert not same(three.weights[mv][4], two.weights[mv][4]) and same(three.weights[mv][5], w[mv][5]) and not same(two.weights[mv][6], one.weights[mv][6])


# ---------------------------------------------------------------- arithmetic edges

def test_prelu_at_exactly_zero(torch):
    fam, w, ids, dense, y = TDC.small(40, seed=6, hidden=(4, 3))
    for k in ("att0", "fc0"):
        w[k + "/kernel"][:, 0] = 0.0
        w[k + "/bias"][0] = 0.0
    got = both(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    for k in ("att0", "fc0"):
        assert not got.m[k + "/kernel"][:, 0].any() and not got.m[k + "/bias"][0] and got.m[k + "/kernel"][:, 1:].all()
    assert not got.m["att_prelu/alpha"][:, 0].any() and not got.m["fc0_prelu/alpha"][0] and not got.m["fc1/kernel"][0].any() and not got.m["att1/kernel"][0].any()


def test_prelu_of_negative_pre_activations_with_alpha_zero_and_negative(torch):
    fam, w, ids, dense, y = TDC.small(40, seed=7, hidden=(4, 3))
    for k, al in (("att0", "att_prelu/alpha"), ("fc0", "fc0_prelu/alpha")):
        w[k + "/bias"][1:3] = -50.0
        w[al][..., 1] = 0.0
        w[al][..., 2] = -0.25
    got = both(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    assert got.m["fc0_prelu/alpha"][1] and not got.m["fc0/bias"][1] and got.m["fc0/bias"][2]
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)                   # (alpha has left zero after the first step)


@pytest.mark.parametrize("bias", [-100.0, 100.0])
def test_a_saturated_attention_sigmoid(torch, bias):
    fam, w, ids, dense, y = TDC.small(40, seed=8)
    ids[:, 0] %= 4
    ids[:, 1:4] = 4 + ids[:, 1:4] % 3
    w["att1/bias"][0] = bias
    got = both(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    for k in ("att0/kernel", "att0/bias", "att_prelu/alpha", "att1/kernel", "att1/bias"):
        assert same(got.weights[k], w[k]) and not got.m[k].any(), k
    assert got.m["emb/movie"][4:].all() if bias > 0 else not got.m["emb/movie"][4:].any()


@pytest.mark.parametrize("bias", [100.0, -100.0])
def test_a_saturated_head(torch, bias):
    fam, w, ids, dense, y = TDC.small(40, seed=7)
    w["head/bias"][0] = bias
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert set(np.unique(got.p).tolist()) <= ({1.0} if bias > 0 else {0.0}) and set(y.tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("scale", [1e-20, 1e-39])
def test_tiny_and_subnormal_weights(torch, scale):
    fam, w, ids, dense, y = TDC.small(40, seed=8, hidden=(6, 4))
    w = {k: (v.astype(np.float64) * scale).astype(F) for k, v in w.items()}
    tiny = np.finfo(F).tiny
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    sub = lambda d: any(((np.abs(a) > 0) & (np.abs(a) < tiny)).any() for a in d.values())
    assert sub(got.m) if scale == 1e-20 else sub(w)


def test_batches_beyond_the_lds_sort_capacity(torch, monkeypatch):
    """SPRK_FE_SORT_CAP=64: a batch's 40 x 7 entries take the chunked sort and the merge passes."""
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    fam, w, ids, dense, y = TDC.small(100, seed=9)
    both(fam, w, ids, dense, y, batch_size=40, epochs=2, tile=8)


@pytest.mark.parametrize("grid", ["3", "1"])
def test_grids_capped(torch, monkeypatch, grid):
    """SPRK_FE_MAX_GRID 3 and 1: every grid-stride loop of the schedule and of the two Adam kernels goes round."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", grid)
    fam, w, ids, dense, y = TDC.small(300, seed=10, **TDC.REFERENCE_SHAPE)
    assert ids.size > 3 * 256 and sum(a.size for a in w.values()) > 3 * 256
    both(fam, w, ids, dense, y, batch_size=128, epochs=1, tile=8)


# ---------------------------------------------------------------- the C ABI: errors, memory, streams

GUARD = 64


def raw_fit(torch, fam, w, ids, dense, y, batch, tile, epochs, stream=None):
    """``sprk_train_din_fit`` itself: parameters, moments, p and the workspace each inside guard bands of a fixed pattern, the workspace
    exactly as large as ``sprk_train_din_workspace_bytes`` reports.  -> (rc, params, m, v, p, error word, guards intact)."""
    lib = L.load_library()
    dev = torch.device("cuda")
    n = len(y)
    flat = TD._flatten(fam, w, dev)
    ms = TD._model_struct(fam)
    need = int(lib.sprk_train_din_workspace_bytes(C.byref(ms), n, batch, tile))
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
    rc = lib.sprk_train_din_fit(C.byref(ms), C.c_void_p(t_ids.data_ptr()), C.c_void_p(t_dense.data_ptr()), C.c_void_p(t_y.data_ptr()), None,
                                n, batch, tile, epochs, C.c_void_p(alphas.data_ptr()), float(c1), float(c2), float(eps), at(params, 4), at(m, 4), at(v, 4), at(p, 4),
                                C.c_void_p(word.data_ptr()), at(ws, 1), need, C.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream))
    (stream or torch.cuda.current_stream()).synchronize()
    intact = all(bool((b[:GUARD] == b[0]).all()) and bool((b[-GUARD:] == b[0]).all()) and (float(b[0]) in (-7.0, 90.0)) for b in (params, m, v, p, ws))
    cut = lambda b: b[GUARD:-GUARD].cpu().numpy()
    return rc, cut(params), cut(m), cut(v), cut(p), int(word.cpu()[0]), intact


def test_guard_bands_side_stream_exact_workspace(torch):
    fam, w, ids, dense, y = TDC.small(50, seed=10)
    want = TD.train_host(fam, w, ids, dense, y, batch_size=12, epochs=2, tile=8)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 12, 8, 2, stream=side)
    assert rc == 0 and word == -1 and intact
    flat = lambda d: np.concatenate([d[k].reshape(-1) for k in TD.param_names(fam)])
    assert same(params, flat(want.weights)) and same(m, flat(want.m)) and same(v, flat(want.v))
    assert same(p[50:], want.p)
    lib = L.load_library()
    ms = TD._model_struct(fam)
    need = int(lib.sprk_train_din_workspace_bytes(C.byref(ms), 50, 12, 8))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    word_t = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    f = torch.zeros(TD._flatten(fam, w, torch.device("cuda")).numel(), device="cuda")
    z = C.c_void_p(f.data_ptr())
    rc = lib.sprk_train_din_fit(C.byref(ms), z, z, z, None, 50, 12, 8, 1, z, 0.1, 0.001, 1e-7, z, z, z, z, C.c_void_p(word_t.data_ptr()), C.c_void_p(ws.data_ptr()), need - 1, None)
    assert rc == L.EINVAL and b"sprk_train_din_workspace_bytes" in lib.sprk_last_error()


def test_each_error_word_and_no_parameter_moves(torch):
    fam, w, ids, dense, y = TDC.small(40, seed=11)
    flat0 = np.concatenate([w[k].reshape(-1) for k in TD.param_names(fam)])

    def check(kind, row, message, ids=ids, dense=dense, y=y):
        rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 16, 8, 2)
        assert rc == 0 and intact and word == (kind << 32 | row), (word >> 32, word & 0xffffffff)
        assert same(params, flat0) and not m.any() and not v.any()
        for fit in (TD.train_device, TD.train_host):
            with pytest.raises(ValueError, match=message):
                fit(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    bad = ids.copy(); bad[30, 0] = 7; bad[12, 2] = -1; bad[20, 5] = -2
    check(T.ERR_ID, 12, "samples row 12: an id outside", ids=bad)
    bad = dense.copy(); bad[9, 1] = np.inf; bad[3, 0] = np.nan
    check(T.ERR_NUMERIC, 3, "samples row 3: a numeric", dense=bad)
    bad = y.copy(); bad[7] = np.nan; bad[39] = -np.inf
    check(T.ERR_LABEL, 7, "samples row 7: the label", y=bad)


def test_two_fits_give_the_same_bytes_and_a_fit_continues(torch):
    fam, w, ids, dense, y = TDC.small(200, seed=12, hidden=(65, 7))
    a = TD.train_device(fam, w, ids, dense, y, batch_size=48, epochs=2, tile=8)
    b = TD.train_device(fam, w, ids, dense, y, batch_size=48, epochs=2, tile=8)
    for x, z in ((a.weights, b.weights), (a.m, b.m), (a.v, b.v)):
        assert all(same(x[k].cpu().numpy(), z[k].cpu().numpy()) for k in x)
    assert same(a.p.cpu().numpy(), b.p.cpu().numpy()) and a.history == b.history
    one = TD.train_device(fam, w, ids, dense, y, batch_size=48, epochs=1, tile=8)
    two = TD.train_device(fam, one.weights, ids, dense, y, batch_size=48, epochs=1, tile=8, state=(one.m, one.v, one.step))
    assert two.step == a.step and all(same(two.weights[k].cpu().numpy(), a.weights[k].cpu().numpy()) and same(two.v[k].cpu().numpy(), a.v[k].cpu().numpy()) for k in w)
    none = TD.train_device(fam, w, ids, dense, y, epochs=0)
    assert none.step == 0 and none.history == [] and all(same(none.weights[k].cpu().numpy(), w[k]) for k in w)


def test_lds_refusal_in_words(torch):
    fam, w, ids, dense, y = TDC.small(20, seed=13)
    once = TD.lds_bytes(fam, 0)
    top = (TD.LDS_BYTES - once) // (TD.lds_bytes(fam, 1) - once)
    with pytest.raises(ValueError, match="tile = %d needs %d bytes of LDS" % (top + 1, TD.lds_bytes(fam, top + 1))):
        TD.train_device(fam, w, ids, dense, y, batch_size=20, epochs=1, tile=top + 1)


def test_a_step_of_more_than_48_kb_of_lds(torch):
    """The reference shape at tile 16: 73 KB of LDS, above the 48 KB a kernel gets without asking."""
    fam, w, ids, dense, y = TDC.small(40, seed=14, **TDC.REFERENCE_SHAPE)
    assert 48 * 1024 < TD.lds_bytes(fam, 16) <= TD.LDS_BYTES
    both(fam, w, ids, dense, y, batch_size=40, epochs=2, tile=16)


# ---------------------------------------------------------------- trainer_din.fit

def _ratings_model():
    from tests import featureeng_cases as cases
    return M.DIN(seed=3, movie_buckets=cases.N_MOVIES, user_buckets=cases.N_USERS)


def test_fit_on_a_dict_and_on_batches(torch):
    """``trainer_din.fit`` on a dict of host columns and on an iterable of ``(features, labels)`` batches: the history and the weights
    are ``train_host``'s, and ``predict`` serves the trained weights; ``DIN.fit`` itself still refuses."""
    from sparrowrecsys_amd import featureeng as FE
    from tests import featureeng_cases as cases
    cols = FE.samples_host(cases.synthetic_ratings(), cases.synthetic_movies(), 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    y = np.asarray(cols["label"], dtype=F)
    a, b, ref = _ratings_model(), _ratings_model(), _ratings_model()
    ids, dense = ref.pack(cols)
    want = TD.train_host(TD.family_of(ref), ref.weights, ids, dense, y, batch_size=128, epochs=1, learning_rate=0.01)
    h_a = TD.fit(a, cols, batch_size=128, epochs=1, learning_rate=0.01)
    half = len(y) // 2
    feats = {k: v for k, v in cols.items() if k != "label"}
    h_b = TD.fit(b, [({k: v[:half] for k, v in feats.items()}, y[:half]), ({k: v[half:] for k, v in feats.items()}, y[half:])], batch_size=128, epochs=1, learning_rate=0.01)
    for model, h in ((a, h_a), (b, h_b)):
        assert all(same(model.weights[k], want.weights[k]) for k in want.weights)
        assert [e[1:] for e in h] == [e[1:] for e in want.history] and abs(h[0][0] - want.history[0][0]) <= MC.loss_bound(len(y)) * want.history[0][0]
    assert not same(a.weights["att0/kernel"], ref.weights["att0/kernel"]) and a._fit_state[2] == want.step
    before, served = ref.predict(cols)[:, 0], a.predict(cols)[:, 0]
    ref.set_weights(want.weights)
    assert same(served, ref.predict(cols)[:, 0]) and not same(served, before)
    with pytest.raises(NotImplementedError):
        a.fit(cols)


def test_ratings_to_recommendations(torch):
    """A few hundred synthetic ratings: featureeng.build -> split -> trainer_din.fit(train.columns) -> evaluate_device(test.columns) ->
    recommend, against the same chain through host arrays, train_host and set_weights; a second fit continues."""
    from sparrowrecsys_amd import featureeng as FE
    from tests import featureeng_cases as cases
    ratings, movies = cases.synthetic_ratings(), cases.synthetic_movies()
    built = FE.build(ratings, movies, 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    train, test = built.split(mode="time", sample=0.5)
    model, other = _ratings_model(), _ratings_model()
    start = {k: v.copy() for k, v in model.weights.items()}
    history = TD.fit(model, train.columns, batch_size=64, epochs=2, learning_rate=0.01)
    tcols = train.to_host()
    ids, dense = other.pack(tcols)
    y = np.asarray(tcols["label"], dtype=F)
    fam = TD.family_of(other)
    want = TD.train_host(fam, start, ids, dense, y, batch_size=64, epochs=2, learning_rate=0.01)
    assert len(y) > 100 and all(same(model.weights[k], want.weights[k]) for k in want.weights)
    assert not same(model.weights["emb/movie"], start["emb/movie"]) and not same(model.weights["att_prelu/alpha"], start["att_prelu/alpha"])
    assert [h[1:] for h in history] == [h[1:] for h in want.history] and len(history) == 2
    other.set_weights(want.weights)
    assert model.evaluate_device(test.columns) == other.evaluate_device(test.columns)
    assert same(model.predict(test.to_host()), other.predict(test.to_host()))
    store = built.store()
    users, cand = np.array([30, 12, 8, 1, 17]), np.arange(1, 116, 2)
    got = model.recommend(store, users, cand, 10)
    assert got == other.recommend(store, users, cand, 10) and len(got[0]) == 10
    again = TD.fit(model, train.columns, batch_size=64, epochs=1, learning_rate=0.01)
    cont = TD.train_host(fam, want.weights, ids, dense, y, batch_size=64, epochs=1, learning_rate=0.01, state=(want.m, want.v, want.step))
    assert all(same(model.weights[k], cont.weights[k]) for k in cont.weights) and again[0][1:] == cont.history[0][1:]


def test_the_other_fits_are_what_they_were(torch):
    """``CTRModel.fit`` now runs through ``_fit_with``: ``NeuralCF.fit`` against ``trainer.train_host`` and ``DeepFMv2.fit`` against
    ``trainer_fm.train_host``."""
    model = M.NeuralCF(seed=3, movie_buckets=50, user_buckets=70)
    fam = T.family_of(model)
    ids, dense, y = TC.data(fam, 100, 3)
    start = {k: v.copy() for k, v in model.weights.items()}
    history = model.fit({"movieId": ids[:, 0], "userId": ids[:, 1], "label": y}, batch_size=32, epochs=2)
    want = T.train_host(fam, start, ids, dense, y, batch_size=32, epochs=2)
    assert all(same(model.weights[k], want.weights[k]) for k in want.weights) and [h[1:] for h in history] == [h[1:] for h in want.history]
    from sparrowrecsys_amd import featureeng as FE
    from tests import featureeng_cases as cases
    cols = FE.samples_host(cases.synthetic_ratings(), cases.synthetic_movies(), 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    fields = [("movieId", "id", cases.N_MOVIES), ("userId", "id", cases.N_USERS), ("userGenre1", "genre", 19), ("movieGenre1", "genre", 19)]
    model = M.DeepFMv2(seed=3, fields=fields, order=M.DeepFMv2.DEFAULT_ORDER)
    fam = TF.family_of(model)
    ids, dense = model.pack(cols)
    y = np.asarray(cols["label"], dtype=F)
    start = {k: v.copy() for k, v in model.weights.items()}
    history = model.fit(cols, batch_size=128, epochs=1, learning_rate=0.01)
    want = TF.train_host(fam, start, ids, dense, y, batch_size=128, epochs=1, learning_rate=0.01)
    assert all(same(model.weights[k], want.weights[k]) for k in want.weights) and [h[1:] for h in history] == [h[1:] for h in want.history]


# ---------------------------------------------------------------- the step shape trainer_din.fit ships with (docs/train_shapes_results.md)

ROUND = 2048 * 256                                                     # FE_MAX_GRID workgroups of 256 threads: what one trip of a strided loop covers


def strides(items):
    """A loop over ``items`` elements, launched with fe_grid_capped(items) workgroups, makes a second trip (tests/test_gpu_grid_rounds.py)."""
    return items > L.load_library().sprk_segments_grid(items) * 256


@pytest.mark.parametrize("kw", [TDC.REFERENCE_SHAPE, dict(TDC.REFERENCE_SHAPE, hist_len=12)])
def test_batch_4096_at_the_default_tile(torch, kw):
    """The reference shape, and the same with T = 12, N = 4096 + 77, one epoch: one full batch of ``DEFAULT_BATCH`` rows (1 024 tiles of 4: 128
    trips of k_tr_dense_adam's unrolled partial sum) and a short one of 20 tiles."""
    fam, w, ids, dense, y = TDC.small(TD.DEFAULT_BATCH + 77, seed=21, **kw)
    assert TD.default_tile(fam) == TD.DEFAULT_TILE == 4
    want = both(fam, w, ids, dense, y, epochs=1)
    assert want.step == 2


@pytest.mark.parametrize("tile", [None, 3])
def test_the_default_tile_falls_to_what_the_lds_holds(torch, tile):
    """T = 12, H = 256: tiles 1, 2 and 3 fit the LDS and ``DEFAULT_TILE`` = 4 does not, so ``default_tile`` halves to 2.  A fit that names no
    tile, and tile 3, the largest that fits."""
    fam, w, ids, dense, y = TDC.small(40, seed=22, hist_len=12, att_hidden=256)
    assert [TD.lds_bytes(fam, t) <= TD.LDS_BYTES for t in (1, 2, 3, 4)] == [True, True, True, False] and TD.default_tile(fam) == 2 < TD.DEFAULT_TILE
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=tile)


def test_tile_one(torch):
    """Tile 1 on 23 rows in batches of 7: every tile's partial sum is one sample's term."""
    fam, w, ids, dense, y = TDC.small(23, seed=23)
    both(fam, w, ids, dense, y, batch_size=7, epochs=2, tile=1)


@pytest.mark.parametrize("batch", [56, 64, 72, 120, 128, 136])
def test_tile_counts_around_the_unrolled_partial_sum(torch, batch):
    """Tile 8: 7, 8, 9, 15, 16 and 17 tiles -- k_tr_dense_adam adds eight partials at a time, then the rest -- and a last batch of 5 rows."""
    fam, w, ids, dense, y = TDC.small(batch + 5, seed=batch)
    assert batch // 8 in (7, 8, 9, 15, 16, 17)
    both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=8)


@pytest.mark.parametrize("kw", [dict(), dict(hist_len=1, att_hidden=1, hidden=(1,))])
def test_a_tile_wider_than_the_workgroup(torch, kw):
    """A tile of more than 256 samples: every per-sample loop of k_td_step goes round.  The tile is 300 or the largest that ``lds_bytes`` lets
    into 160 KB: 257 for the default small shape (163 792 B), 300 for T = H = 1 with a tail of (1,).  N = batch = 650: three tiles."""
    fam, w, ids, dense, y = TDC.small(650, seed=24, **kw)
    once = TD.lds_bytes(fam, 0)
    tile = min(300, (TD.LDS_BYTES - once) // (TD.lds_bytes(fam, 1) - once))
    assert tile > 256 and TD.lds_bytes(fam, tile) <= TD.LDS_BYTES
    both(fam, w, ids, dense, y, batch_size=650, epochs=2, tile=tile)


@pytest.mark.parametrize("kw,tile,round_", [(dict(emb_dim=49), 8, False), (dict(hist_len=12, att_hidden=256), 3, False), (dict(hidden=(256,) * 8), 8, False),
                                            (dict(emb_dim=49, hidden=(256,) * 8), 4, True)])
def test_the_stated_maxima(torch, kw, tile, round_):
    """``emb_dim`` 49, the largest the DIN class lays out (252 of ``fc0``'s 256 input rows); H = 256 at T = 12; eight tail layers of 256 units;
    and the widest ``fc0`` under the deepest tail, whose 528 623 Dense floats send k_tr_dense_adam past one round of its grid.  28 rows."""
    fam, w, ids, dense, y = TDC.small(28, seed=25, **kw)
    assert TD.lds_bytes(fam, tile) <= TD.LDS_BYTES and strides(TDC.dense_floats(fam)) == round_
    if "emb_dim" in kw:
        assert fam.fan0 == 252
        with pytest.raises(ValueError):
            TDC.family(**dict(kw, emb_dim=50))
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=tile)


def test_a_table_beyond_one_round_of_the_grid(torch):
    """60 000 movies x 10: 600 000 floats of ``emb/movie`` at the head of the parameter vector, more than the 524 288 one round of
    k_td_table_adam's grid covers.  Step 1 hits rows 0 and 52 428 through the candidate and rows 52 429 and 59 999 through a history slot:
    elements 524 280 .. 524 299 lie on both sides of the round's end.  Those rows move; rows never hit keep their bits and zero moments; a row
    hit in step 1 only still moves in step 3."""
    fam, w, ids, dense, y = TDC.small(40, seed=26, movies=60000, emb_dim=10)
    mv, T = "emb/movie", fam.hist_len
    assert TD.param_names(fam)[0] == mv and w[mv].shape == (60000, 10) and strides(TDC.table_floats(fam))
    assert 52428 * 10 < ROUND <= 52429 * 10
    first = np.array([0, 52428, 52429, 59999])
    ids[:, :T + 1] = np.random.default_rng(26).integers(100, 50000, (40, T + 1))
    ids[:16, 0] = first[np.arange(16) % 2]
    ids[:16, 2] = first[2 + np.arange(16) % 2]
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


@pytest.mark.parametrize("batch,tile", [(4096, 32), (76000, 128)])
def test_the_schedule_beyond_one_round_of_the_grid(torch, batch, tile):
    """Seven id columns, N = 76 000: 532 000 entries, so k_tr_count and k_td_scatter make a second trip; in batches of 4 096 and as one batch,
    whose positions pass 65 535 (a key holds position x 16 + column)."""
    fam, w, ids, dense, y = TDC.small(76000, seed=27)
    assert strides(ids.size) and TD.lds_bytes(fam, tile) <= TD.LDS_BYTES and (batch == 4096 or batch == len(y) > 65536)
    both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=tile)


def test_the_error_word_beyond_one_round_of_the_grid(torch):
    """N = 524 288 + 600: bad labels at rows 524 300 and 524 500, both in k_tr_check's second trip.  The library and both routes name row
    524 300 and no parameter moves."""
    fam, w, ids, dense, y = TDC.small(ROUND + 600, seed=28)
    assert strides(len(y))
    y[524500], y[524300] = np.nan, np.inf
    flat0 = np.concatenate([w[k].reshape(-1) for k in TD.param_names(fam)])
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 65536, 16, 1)
    assert rc == 0 and intact and word == (T.ERR_LABEL << 32 | 524300), (word >> 32, word & 0xffffffff)
    assert same(params, flat0) and not m.any() and not v.any()
    for fit in (TD.train_device, TD.train_host):
        with pytest.raises(ValueError, match="samples row 524300: the label"):
            fit(fam, w, ids, dense, y, batch_size=65536, epochs=1, tile=16)
