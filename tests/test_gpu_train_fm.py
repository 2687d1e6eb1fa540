"""``trainer_fm.train_device`` (``sprk_train_fm_fit``, csrc/k_train_fm.h) against its definition ``trainer_fm.train_host``: every weight,
every ``m``, every ``v``, every ``p`` of the last epoch, accuracy and both AUCs of every epoch byte for byte, the loss within
``max(N, 64) 2^-50`` relative (``-m gpu``).  Tiny vocabularies and tens to a few hundred rows, then the step shape ``model.fit`` ships
with: batch 4096 at the default tile, the stated maxima, tables and schedules beyond one round of a grid."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_fm as TF
from tests import metrics_cases as MC
from tests import train_cases as TC
from tests import train_fm_cases as TFC

pytestmark = pytest.mark.gpu
F = np.float32
same = TFC.same_bits


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


def host_of(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def both(fam, w, ids, dense, y, **kw):
    """Host and device fits of one input: asserts the equalities of the module docstring, -> the host's result."""
    want = TF.train_host(fam, w, ids, dense, y, **kw)
    got = TF.train_device(fam, w, ids, dense, y, **kw)
    assert got.step == want.step and len(got.history) == len(want.history)
    for name, g, h in (("weight", got.weights, want.weights), ("m", got.m, want.m), ("v", got.v, want.v)):
        g = host_of(g)
        for k in TF.param_names(fam):
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
    fam, w, ids, dense, y = TFC.small(n, seed=n)
    want = both(fam, w, ids, dense, y, batch_size=batch, epochs=3, tile=tile)
    assert want.step == 3 * ((n + batch - 1) // batch)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_order(torch, as_tensor):
    fam, w, ids, dense, y = TFC.small(50, seed=4)
    order = np.random.default_rng(1).permutation(50)
    want = TF.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8, order=order)
    plain = TF.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8)
    assert not same(want.weights["deep0/kernel"], plain.weights["deep0/kernel"])
    dev = lambda a: torch.from_numpy(a).cuda()
    got = TF.train_device(fam, w, dev(ids), dev(dense), dev(y), batch_size=12, epochs=3, tile=8, order=dev(order) if as_tensor else order)
    assert all(same(host_of(got.weights)[k], want.weights[k]) for k in want.weights)
    assert same(got.p.cpu().numpy(), want.p) and [h[1:] for h in got.history] == [h[1:] for h in want.history]
    with pytest.raises(ValueError, match="permutation"):
        TF.train_device(fam, w, ids, dense, y, order=dev(np.zeros(50, dtype=np.int64)) if as_tensor else np.zeros(50, dtype=np.int64))


# ---------------------------------------------------------------- widths

SEVEN, EIGHT = dict(vocabs=(6, 5, 9, 4, 7, 3, 8), kinds=("id", "genre", "id", "genre", "id", "id", "genre")), dict(vocabs=(6, 5, 9, 4, 7, 3, 8, 5), kinds=("id", "genre") * 4)


@pytest.mark.parametrize("kw", [dict(proj_dim=1), dict(proj_dim=63), dict(proj_dim=64), dict(proj_dim=65), dict(proj_dim=TF.MAX_PROJ),
                                dict(emb_dim=10), dict(vocabs=(6, 5), kinds=("id", "genre"), order=(1,)), dict(vocabs=(6, 5, 9, 4), kinds=("id", "genre", "id", "genre")),
                                dict(proj_dim=4, **EIGHT), dict(proj_dim=TF.MAX_PROJ, **SEVEN),
                                dict(hidden=(1,)), dict(hidden=(63,)), dict(hidden=(64, 65)), dict(hidden=(32, 16)), dict(hidden=(7, 6, 5)),
                                dict(vocabs=(6, 5, 9, 4), kinds=("id", "genre", "id", "genre"), order=(2, 0, 3)), TFC.REFERENCE_SHAPE])
def test_widths_groups_and_field_orders(torch, kw):
    """proj_dim 1, 5 (the other cases), 63, 64, 65 and the maximum; emb_dim 3 and 10; G = 2, 5, the maximum 9 and 8 at the widest
    proj_dim (groups x proj_dim at its maximum); hidden (1,), (63,), (64, 65), (32, 16) and depth 3; ``order`` a permuted subset; the
    reference shape."""
    fam, w, ids, dense, y = TFC.small(40, seed=sum(map(ord, repr(sorted(kw.items())))) % 97, **kw)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


# ---------------------------------------------------------------- ids

def test_runs_of_ids(torch):
    """A batch in which every sample carries one id per field (run length B), a row hit exactly once, rows never hit -- bit-equal to
    their initial value after step 1, in emb/ and in fo_cat/kernel --, a row hit in step 1 and never again, which keeps moving."""
    fam, w, ids, dense, y = TFC.small(48, seed=2, vocabs=(9, 9, 9), kinds=("id", "genre", "id"))
    ids[:16] = 3
    ids[16:, 0] = np.where(ids[16:, 0] == 3, 4, ids[16:, 0])            # row 3 of field 0: step 1 and never again
    ids[16:, 2] = 5
    ids[20, 2] = 7                                                      # hit exactly once
    ids[:, 1] = np.where(ids[:, 1] == 8, 0, ids[:, 1])                  # row 8 of field 1: never
    one = both(fam, w, ids[:16], dense[:16], y[:16], batch_size=16, epochs=1, tile=8)
    keep = np.arange(9) != 3
    for c, (k, _, _) in enumerate(fam.fields):
        fo = one.weights["fo_cat/kernel"][fam.fo_off[c]:fam.fo_off[c] + 9], w["fo_cat/kernel"][fam.fo_off[c]:fam.fo_off[c] + 9]
        for a, b in ((one.weights["emb/" + k], w["emb/" + k]), fo):
            assert same(a[keep], b[keep]) and not same(a[3], b[3])
    two = both(fam, w, ids[:32], dense[:32], y[:32], batch_size=16, epochs=1, tile=8)
    three = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    k0, k1 = fam.fields[0][0], fam.fields[1][0]
    assert not same(three.weights["emb/" + k0][3], two.weights["emb/" + k0][3])
    assert same(three.weights["emb/" + k1][8], w["emb/" + k1][8])
    assert same(three.weights["fo_cat/kernel"][fam.fo_off[1] + 8], w["fo_cat/kernel"][fam.fo_off[1] + 8])


def test_every_genre_id_none(torch):
    fam, w, ids, dense, y = TFC.small(40, seed=3, vocabs=(6, 5, 4), kinds=("id", "genre", "genre"))
    ids[:, 1:] = -1
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    for c in (1, 2):
        k, rows = fam.fields[c][0], slice(fam.fo_off[c], fam.fo_off[c] + fam.fields[c][2])
        assert same(got.weights["emb/" + k], w["emb/" + k]) and same(got.weights["fo_cat/kernel"][rows], w["fo_cat/kernel"][rows])
        assert not same(got.weights["proj/%s/bias" % k], w["proj/%s/bias" % k])


def test_a_field_outside_order_keeps_its_table(torch):
    fam, w, ids, dense, y = TFC.small(60, seed=3, vocabs=(6, 5, 9), kinds=("id", "genre", "id"), order=(2, 0))
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    out = fam.fields[1][0]
    assert same(got.weights["emb/" + out], w["emb/" + out]) and not same(got.weights["fo_cat/kernel"], w["fo_cat/kernel"])


# ---------------------------------------------------------------- arithmetic edges

def test_relu_at_exactly_zero(torch):
    fam, w, ids, dense, y = TFC.small(40, seed=6, hidden=(4, 3))
    w["deep0/kernel"][:, 0] = 0.0
    w["deep0/bias"][0] = 0.0
    got = both(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    assert not got.m["deep0/kernel"][:, 0].any() and not got.m["deep0/bias"][0]
    assert got.m["deep1/kernel"][1:].any() and not got.m["deep1/kernel"][0].any()


@pytest.mark.parametrize("bias", [100.0, -100.0, 30.0])
def test_saturated_sigmoid(torch, bias):
    fam, w, ids, dense, y = TFC.small(40, seed=7)
    w["head/bias"][0] = bias
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert set(np.unique(got.p).tolist()) <= ({1.0} if bias > 0 else {0.0})
    assert set(y.tolist()) == {0.0, 1.0}


def test_fm_that_cancels_to_exactly_zero(torch):
    """Two groups, the field's projection all zero: ``s = v``, ``q = v v`` and ``fm = 0`` exactly, while ``d_fm`` is not."""
    fam, w, ids, dense, y = TFC.small(40, seed=8, vocabs=(6, 5), kinds=("id", "genre"), order=(0,))
    k = fam.order[0]
    w["proj/%s/kernel" % k][:] = 0.0
    w["proj/%s/bias" % k][:] = 0.0
    keep = {}
    TF.forward_host(fam, w, ids, dense, keep)
    assert not keep["fm"].any() and keep["s"].any()
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert got.m["proj/%s/bias" % k].any()


def test_s_squared_overflows(torch):
    """Finite inputs, ``s s`` = infinity: the sigmoid saturates to exactly 1, and where the label is 1 the head's gradient holds
    ``inf x 0``.  One step; the definition's weights, ``m`` and ``v`` then hold NaN and infinity, and the device's are the same bits."""
    fam, w, ids, dense, y = TFC.small(16, seed=6, vocabs=(6, 5), kinds=("id", "id"))
    w["proj/num/bias"][:] = F(1e19)
    w["proj/%s/bias" % fam.order[0]][:] = F(1e19)
    w["head/kernel"][1:1 + fam.proj_dim] = np.abs(w["head/kernel"][1:1 + fam.proj_dim]) + F(0.1)
    assert all(np.isfinite(a).all() for a in w.values()) and set(y.tolist()) == {0.0, 1.0}
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert np.isnan(got.weights["head/kernel"]).any() and np.isnan(got.m["head/kernel"]).any() and np.isfinite(got.weights["deep0/kernel"]).all()
    assert (got.p == 1.0).all()


@pytest.mark.parametrize("scale", [1e-20, 1e-39])
def test_tiny_and_subnormal_weights(torch, scale):
    fam, w, ids, dense, y = TFC.small(40, seed=8, hidden=(6, 4))
    w = {k: (v.astype(np.float64) * scale).astype(F) for k, v in w.items()}
    tiny = np.finfo(F).tiny
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    sub = lambda d: any(((np.abs(a) > 0) & (np.abs(a) < tiny)).any() for a in d.values())
    assert sub(got.m) if scale == 1e-20 else sub(w)


def test_batches_beyond_the_lds_sort_capacity(torch, monkeypatch):
    """SPRK_FE_SORT_CAP=64: a batch's 40 x 3 entries take the chunked sort and the merge passes."""
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    fam, w, ids, dense, y = TFC.small(100, seed=9, vocabs=(6, 5, 9), kinds=("id", "id", "id"))
    both(fam, w, ids, dense, y, batch_size=40, epochs=2, tile=8)


# ---------------------------------------------------------------- the C ABI: errors, memory, streams

GUARD = 64


def raw_fit(torch, fam, w, ids, dense, y, batch, tile, epochs, stream=None):
    """``sprk_train_fm_fit`` itself: parameters, moments, p and the workspace each inside guard bands of a fixed pattern, the workspace
    exactly as large as ``sprk_train_fm_workspace_bytes`` reports.  -> (rc, params, m, v, p, error word, guards intact)."""
    lib = L.load_library()
    dev = torch.device("cuda")
    n = len(y)
    flat = TF._flatten(fam, w, dev)
    ms = TF._model_struct(fam)
    need = int(lib.sprk_train_fm_workspace_bytes(C.byref(ms), n, batch, tile))
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
    rc = lib.sprk_train_fm_fit(C.byref(ms), C.c_void_p(t_ids.data_ptr()), C.c_void_p(t_dense.data_ptr()), C.c_void_p(t_y.data_ptr()), None,
                               n, batch, tile, epochs, C.c_void_p(alphas.data_ptr()), float(c1), float(c2), float(eps), at(params, 4), at(m, 4), at(v, 4), at(p, 4),
                               C.c_void_p(word.data_ptr()), at(ws, 1), need, C.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream))
    (stream or torch.cuda.current_stream()).synchronize()
    intact = all(bool((b[:GUARD] == b[0]).all()) and bool((b[-GUARD:] == b[0]).all()) and (float(b[0]) in (-7.0, 90.0)) for b in (params, m, v, p, ws))
    cut = lambda b: b[GUARD:-GUARD].cpu().numpy()
    return rc, cut(params), cut(m), cut(v), cut(p), int(word.cpu()[0]), intact


def test_guard_bands_side_stream_exact_workspace(torch):
    fam, w, ids, dense, y = TFC.small(50, seed=10)
    want = TF.train_host(fam, w, ids, dense, y, batch_size=12, epochs=2, tile=8)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 12, 8, 2, stream=side)
    assert rc == 0 and word == -1 and intact
    flat = lambda d: np.concatenate([d[k].reshape(-1) for k in TF.param_names(fam)])
    assert same(params, flat(want.weights)) and same(m, flat(want.m)) and same(v, flat(want.v))
    assert same(p[50:], want.p)
    lib = L.load_library()
    ms = TF._model_struct(fam)
    need = int(lib.sprk_train_fm_workspace_bytes(C.byref(ms), 50, 12, 8))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    word_t = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    f = torch.zeros(TF._flatten(fam, w, torch.device("cuda")).numel(), device="cuda")
    z = C.c_void_p(f.data_ptr())
    rc = lib.sprk_train_fm_fit(C.byref(ms), z, z, z, None, 50, 12, 8, 1, z, 0.1, 0.001, 1e-7, z, z, z, z, C.c_void_p(word_t.data_ptr()), C.c_void_p(ws.data_ptr()), need - 1, None)
    assert rc == L.EINVAL and b"sprk_train_fm_workspace_bytes" in lib.sprk_last_error()


def test_each_error_word_and_no_parameter_moves(torch):
    fam, w, ids, dense, y = TFC.small(40, seed=11)
    flat0 = np.concatenate([w[k].reshape(-1) for k in TF.param_names(fam)])

    def check(kind, row, message, ids=ids, dense=dense, y=y):
        rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 16, 8, 2)
        assert rc == 0 and intact and word == (kind << 32 | row), (word >> 32, word & 0xffffffff)
        assert same(params, flat0) and not m.any() and not v.any()
        for fit in (TF.train_device, TF.train_host):
            with pytest.raises(ValueError, match=message):
                fit(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    bad = ids.copy(); bad[30, 0] = 6; bad[12, 0] = -1; bad[20, 1] = -2
    check(T.ERR_ID, 12, "samples row 12: an id outside", ids=bad)
    bad = dense.copy(); bad[9, 1] = np.inf; bad[3, 0] = np.nan
    check(T.ERR_NUMERIC, 3, "samples row 3: a numeric", dense=bad)
    bad = y.copy(); bad[7] = np.nan; bad[39] = -np.inf
    check(T.ERR_LABEL, 7, "samples row 7: the label", y=bad)


def test_two_fits_give_the_same_bytes_and_a_fit_continues(torch):
    fam, w, ids, dense, y = TFC.small(200, seed=12, hidden=(65, 7))
    a = TF.train_device(fam, w, ids, dense, y, batch_size=48, epochs=2, tile=8)
    b = TF.train_device(fam, w, ids, dense, y, batch_size=48, epochs=2, tile=8)
    for x, z in ((a.weights, b.weights), (a.m, b.m), (a.v, b.v)):
        assert all(same(x[k].cpu().numpy(), z[k].cpu().numpy()) for k in x)
    assert same(a.p.cpu().numpy(), b.p.cpu().numpy()) and a.history == b.history
    one = TF.train_device(fam, w, ids, dense, y, batch_size=48, epochs=1, tile=8)
    two = TF.train_device(fam, one.weights, ids, dense, y, batch_size=48, epochs=1, tile=8, state=(one.m, one.v, one.step))
    assert two.step == a.step and all(same(two.weights[k].cpu().numpy(), a.weights[k].cpu().numpy()) and same(two.v[k].cpu().numpy(), a.v[k].cpu().numpy()) for k in w)
    none = TF.train_device(fam, w, ids, dense, y, epochs=0)
    assert none.step == 0 and none.history == [] and all(same(none.weights[k].cpu().numpy(), w[k]) for k in w)


# ---------------------------------------------------------------- model.fit

def _ratings_model():
    from tests import featureeng_cases as cases
    fields = [("movieId", "id", cases.N_MOVIES), ("userId", "id", cases.N_USERS), ("userGenre1", "genre", 19), ("movieGenre1", "genre", 19)]
    model = M.DeepFMv2(seed=3, fields=fields, order=M.DeepFMv2.DEFAULT_ORDER)
    return model


def test_fit_on_a_dict_and_on_batches(torch):
    """``DeepFMv2.fit`` on a dict of host columns and on an iterable of ``(features, labels)`` batches: the history and the weights
    are ``train_host``'s, and ``predict`` serves the trained weights."""
    from sparrowrecsys_amd import featureeng as FE
    from tests import featureeng_cases as cases
    cols = FE.samples_host(cases.synthetic_ratings(), cases.synthetic_movies(), 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    y = np.asarray(cols["label"], dtype=F)
    a, b, ref = _ratings_model(), _ratings_model(), _ratings_model()
    ids, dense = ref.pack(cols)
    want = TF.train_host(TF.family_of(ref), ref.weights, ids, dense, y, batch_size=128, epochs=1, learning_rate=0.01)
    h_a = a.fit(cols, batch_size=128, epochs=1, learning_rate=0.01)
    half = len(y) // 2
    feats = {k: v for k, v in cols.items() if k != "label"}
    h_b = b.fit([({k: v[:half] for k, v in feats.items()}, y[:half]), ({k: v[half:] for k, v in feats.items()}, y[half:])], batch_size=128, epochs=1, learning_rate=0.01)
    for model, h in ((a, h_a), (b, h_b)):
        assert all(same(model.weights[k], want.weights[k]) for k in want.weights)
        assert [e[1:] for e in h] == [e[1:] for e in want.history] and abs(h[0][0] - want.history[0][0]) <= MC.loss_bound(len(y)) * want.history[0][0]
    assert not same(a.weights["proj/num/kernel"], ref.weights["proj/num/kernel"])
    before, served = ref.predict(cols)[:, 0], a.predict(cols)[:, 0]
    ref.set_weights(want.weights)
    assert same(served, ref.predict(cols)[:, 0]) and not same(served, before)


def test_ratings_to_recommendations(torch):
    """A few hundred synthetic ratings: featureeng.build -> DeepFMv2.fit(samples.columns) -> evaluate_device -> recommend, against the
    same chain through samples_host, train_host and set_weights; a second fit continues."""
    from sparrowrecsys_amd import featureeng as FE
    from tests import featureeng_cases as cases
    ratings, movies = cases.synthetic_ratings(), cases.synthetic_movies()
    built = FE.build(ratings, movies, 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    model, other = _ratings_model(), _ratings_model()
    start = {k: v.copy() for k, v in model.weights.items()}
    history = model.fit(built.columns, batch_size=128, epochs=2, learning_rate=0.01)
    cols = FE.samples_host(ratings, movies, 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    ids, dense = other.pack(cols)
    y = np.asarray(cols["label"], dtype=F)
    fam = TF.family_of(other)
    want = TF.train_host(fam, start, ids, dense, y, batch_size=128, epochs=2, learning_rate=0.01)
    assert all(same(model.weights[k], want.weights[k]) for k in want.weights)
    assert not same(model.weights["emb/userId"], start["emb/userId"]) and not same(model.weights["fo_cat/kernel"], start["fo_cat/kernel"])
    assert [h[1:] for h in history] == [h[1:] for h in want.history] and len(history) == 2
    other.set_weights(want.weights)
    assert model.evaluate_device(built.columns) == other.evaluate_device(built.columns)
    assert same(model.predict(cols), other.predict(cols))
    store = built.store()
    users, cand = np.array([30, 12, 8, 1, 17]), np.arange(1, 116, 2)
    got = model.recommend(store, users, cand, 10)
    assert got == other.recommend(store, users, cand, 10) and len(got[0]) == 10
    again = model.fit(built.columns, batch_size=128, epochs=1, learning_rate=0.01)
    cont = TF.train_host(fam, want.weights, ids, dense, y, batch_size=128, epochs=1, learning_rate=0.01, state=(want.m, want.v, want.step))
    assert all(same(model.weights[k], cont.weights[k]) for k in cont.weights) and again[0][1:] == cont.history[0][1:]


def test_neural_cf_fit_is_what_it_was(torch):
    """The dispatch in ``CTRModel.fit`` left the other trainer's route alone: ``NeuralCF.fit`` against ``trainer.train_host``."""
    model = M.NeuralCF(seed=3, movie_buckets=50, user_buckets=70)
    fam = T.family_of(model)
    ids, dense, y = TC.data(fam, 100, 3)
    start = {k: v.copy() for k, v in model.weights.items()}
    history = model.fit({"movieId": ids[:, 0], "userId": ids[:, 1], "label": y}, batch_size=32, epochs=2)
    want = T.train_host(fam, start, ids, dense, y, batch_size=32, epochs=2)
    assert all(same(model.weights[k], want.weights[k]) for k in want.weights) and [h[1:] for h in history] == [h[1:] for h in want.history]


# ---------------------------------------------------------------- the step shape model.fit ships with

def test_batch_4096_at_the_default_tile(torch):
    """The reference shape, N = 4096 + 77, one epoch: one full batch of ``DEFAULT_BATCH`` rows (512 tiles of 8: 64 rounds of the unrolled
    partial sum) and a short one of 10 tiles."""
    fam, w, ids, dense, y = TFC.small(TF.DEFAULT_BATCH + 77, seed=21, **TFC.REFERENCE_SHAPE)
    assert TF.default_tile(fam) == 8
    want = both(fam, w, ids, dense, y, epochs=1)
    assert want.step == 2


@pytest.mark.parametrize("batch", [56, 64, 72, 120, 128, 136])
def test_tile_counts_around_the_unrolled_partial_sum(torch, batch):
    """Tile 8: 7, 8, 9, 15, 16 and 17 tiles -- k_tf_dense_adam adds eight partials at a time, then the rest -- and a last batch of 5 rows."""
    fam, w, ids, dense, y = TFC.small(batch + 5, seed=batch)
    assert batch // 8 in (7, 8, 9, 15, 16, 17)
    both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=8)


def test_steps_of_more_than_48_kb_of_lds(torch):
    """The reference shape: 1 249 floats of LDS per sample.  The tiles come from ``lds_bytes``: ``mid`` = half the largest, above 48 KB (the
    step kernel needs its attribute raised), run before and after a step of 39 KB in this one process; ``top`` = the largest that fits 160 KB;
    ``top + 1`` is refused in words by the library and by ``train_device``."""
    fam, w, ids, dense, y = TFC.small(60, seed=23, **TFC.REFERENCE_SHAPE)
    per = TF.lds_bytes(fam, 1)
    top = TF.LDS_BYTES // per
    mid = top // 2
    assert 48 * 1024 < TF.lds_bytes(fam, mid) < TF.lds_bytes(fam, top) <= TF.LDS_BYTES < TF.lds_bytes(fam, top + 1) and TF.lds_bytes(fam, 8) < 48 * 1024
    for tile, n in ((mid, 50), (8, 40), (mid, 60), (top, 60)):
        both(fam, w, ids[:n], dense[:n], y[:n], batch_size=n, epochs=2, tile=tile)
    lib = L.load_library()
    ms = TF._model_struct(fam)
    assert lib.sprk_train_fm_workspace_bytes(C.byref(ms), 60, 60, top) > 0 and lib.sprk_train_fm_workspace_bytes(C.byref(ms), 60, 60, top + 1) == 0
    rc = lib.sprk_train_fm_fit(C.byref(ms), None, None, None, None, 60, 60, top + 1, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None, None, 0, None)
    assert rc == L.EINVAL and b"tile = %d needs %d bytes of LDS" % (top + 1, TF.lds_bytes(fam, top + 1)) in lib.sprk_last_error()
    with pytest.raises(ValueError, match="tile = %d needs %d bytes of LDS" % (top + 1, TF.lds_bytes(fam, top + 1))):
        TF.train_device(fam, w, ids, dense, y, batch_size=60, epochs=1, tile=top + 1)


def test_a_tile_wider_than_the_workgroup(torch):
    """Tile 300 > 256 threads: every per-sample loop of k_tf_step goes round; N = batch = 650 gives tiles of 300, 300 and 50."""
    fam, w, ids, dense, y = TFC.small(650, seed=24)
    assert TF.lds_bytes(fam, 300) <= TF.LDS_BYTES
    both(fam, w, ids, dense, y, batch_size=650, epochs=2, tile=300)


@pytest.mark.parametrize("kw", [dict(hidden=(TF.MAX_WIDTH,)), dict(hidden=(TF.MAX_WIDTH,) * TF.MAX_LAYERS),
                                dict(vocabs=(6, 5), kinds=("id", "genre"), order=(0,), emb_dim=TF.MAX_IN)])
def test_the_stated_maxima(torch, kw):
    """Hidden layers of ``MAX_WIDTH`` units, one and ``MAX_LAYERS`` of them; table rows of ``MAX_IN`` floats; 40 rows, tile 8."""
    fam, w, ids, dense, y = TFC.small(40, seed=25, **kw)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


def test_a_table_beyond_one_round_of_the_grid(torch):
    """Vocabularies (60 000, 5) x 10: 600 050 ``emb/`` floats and the 60 005 rows of ``fo_cat/kernel`` behind them, more than the 524 288 one
    round of k_tf_table_adam's grid covers.  Step 1 hits rows 0, 52 428, 52 429 and 59 999 of field 0: elements 524 280 .. 524 299 lie on both
    sides of the round's end, and every first-order row lies beyond it.  Those rows move, in ``emb/`` and in ``fo_cat/kernel``; rows never
    hit keep their bits; a row hit in step 1 only still moves in step 3."""
    fam, w, ids, dense, y = TFC.small(40, seed=26, vocabs=(60000, 5), kinds=("id", "id"), emb_dim=10)
    key, fo0 = "emb/" + fam.fields[0][0], fam.fo_off[0]
    assert fam.fields[0][2] == 60000 and TF.param_names(fam)[0] == key
    first = np.array([0, 52428, 52429, 59999])
    ids[:16, 0] = first[np.arange(16) % 4]
    ids[16:, 0] = np.random.default_rng(26).integers(100, 50000, 24)
    assert 52428 * 10 < 2048 * 256 <= 52429 * 10
    one = both(fam, w, ids[:16], dense[:16], y[:16], batch_size=16, epochs=1, tile=8)
    two = both(fam, w, ids[:32], dense[:32], y[:32], batch_size=16, epochs=1, tile=8)
    three = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert three.step == 3
    for row in first:
        for name, r in ((key, row), ("fo_cat/kernel", fo0 + row)):
            assert not same(one.weights[name][r], w[name][r])
            assert not same(three.weights[name][r], two.weights[name][r])                             # hit in step 1 only: still moving
    never = np.ones(60000, dtype=bool)
    never[ids[:, 0]] = False
    assert never.sum() > 59900 and same(three.weights[key][never], w[key][never])
    assert same(three.weights["fo_cat/kernel"][fo0:fo0 + 60000][never], w["fo_cat/kernel"][fo0:fo0 + 60000][never])
    rest = np.setdiff1d(np.arange(60000), first)
    assert same(one.weights[key][rest], w[key][rest]) and same(one.weights["fo_cat/kernel"][fo0 + rest], w["fo_cat/kernel"][fo0 + rest])


@pytest.mark.parametrize("batch,tile", [(4096, 32), (66000, 128)])
def test_the_schedule_beyond_one_round_of_the_grid(torch, batch, tile):
    """Eight fields, N = 66 000: 528 000 entries, so k_tr_count and k_tr_scatter make a second trip; in batches of 4 096 and as one batch."""
    fam, w, ids, dense, y = TFC.small(66000, seed=27, **EIGHT)
    assert ids.size > 2048 * 256
    both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=tile)


def test_the_error_word_beyond_one_round_of_the_grid(torch):
    """N = 524 288 + 600: bad labels at rows 524 300 and 524 500, both in k_tr_check's second trip.  Both routes name row 524 300 and no
    parameter moves; the check precedes any training."""
    fam, w, ids, dense, y = TFC.small(2048 * 256 + 600, seed=28)
    y[524500], y[524300] = np.nan, np.inf
    flat0 = np.concatenate([w[k].reshape(-1) for k in TF.param_names(fam)])
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 65536, 16, 1)
    assert rc == 0 and intact and word == (T.ERR_LABEL << 32 | 524300), (word >> 32, word & 0xffffffff)
    assert same(params, flat0) and not m.any() and not v.any()
    for fit in (TF.train_device, TF.train_host):
        with pytest.raises(ValueError, match="samples row 524300: the label"):
            fit(fam, w, ids, dense, y, batch_size=65536, epochs=1, tile=16)
