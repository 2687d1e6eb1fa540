"""``trainer.train_device`` (``sprk_train_fit``, csrc/k_train.h) against its definition ``trainer.train_host``: every weight, every
``m``, every ``v``, every ``p`` of the last epoch, accuracy and both AUCs of every epoch byte for byte, the loss within
``DeviceMetrics``' bound (tests/metrics_cases.py loss_bound) (``-m gpu``).  Tiny vocabularies and tens to a few hundred rows, then the
step shape ``model.fit`` ships with: batch 4096 at the default tile, the stated maxima, tables and schedules beyond one round of a grid."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from tests import metrics_cases as MC
from tests import train_cases as TC

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


def host_of(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def both(fam, w, ids, dense, y, **kw):
    """Host and device fits of one input: asserts the equalities of the module docstring, -> the host's result."""
    want = T.train_host(fam, w, ids, dense, y, **kw)
    got = T.train_device(fam, w, ids, dense, y, **kw)
    assert got.step == want.step and len(got.history) == len(want.history)
    for name, g, h in (("weight", got.weights, want.weights), ("m", got.m, want.m), ("v", got.v, want.v)):
        g = host_of(g)
        for k in T.param_names(fam):
            assert TC.same_bits(g[k], h[k]), (name, k, np.flatnonzero(g[k].reshape(-1) != h[k].reshape(-1))[:8])
    assert TC.same_bits(got.p.cpu().numpy(), want.p), np.flatnonzero(got.p.cpu().numpy() != want.p)[:8]
    for e, (a, b) in enumerate(zip(got.history, want.history)):
        assert a[1:] == b[1:] or (np.isnan(a[2:]).all() and np.isnan(b[2:]).all() and a[1] == b[1]), (e, a, b)
        assert abs(a[0] - b[0]) <= MC.loss_bound(len(y)) * abs(b[0]), (e, a[0], b[0])
    return want


def small(n, seed=0, vocabs=(6, 5, 9), kinds=("id", "genre", "id"), emb_dim=3, n_dense=2, widths=(5,)):
    fam = TC.family(list(vocabs), list(kinds), emb_dim, n_dense, list(widths))
    return (fam, TC.weights(fam, seed)) + TC.data(fam, n, seed)


# ---------------------------------------------------------------- rows and batches

@pytest.mark.parametrize("n,batch,tile", [(1, 4, 8), (7, 16, 8), (8, 16, 8), (9, 16, 8), (50, 12, 8), (23, 1, 8), (40, 12, 32), (30, 64, 8), (33, 32, 32)])
def test_row_counts_and_batching(torch, n, batch, tile):
    """N = 1, tile - 1, tile, tile + 1; B no multiple of the tile; N no multiple of B (a short last batch with its own n); B = 1 and
    B = 12; one batch only; three epochs, so Adam's t crosses epochs."""
    fam, w, ids, dense, y = small(n, seed=n)
    want = both(fam, w, ids, dense, y, batch_size=batch, epochs=3, tile=tile)
    assert want.step == 3 * ((n + batch - 1) // batch)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_order(torch, as_tensor):
    fam, w, ids, dense, y = small(50, seed=4)
    order = np.random.default_rng(1).permutation(50)
    want = T.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8, order=order)
    plain = T.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8)
    assert not TC.same_bits(want.weights["dense0/kernel"], plain.weights["dense0/kernel"])
    dev = lambda a: torch.from_numpy(a).cuda()
    got = T.train_device(fam, w, dev(ids), dev(dense), dev(y), batch_size=12, epochs=3, tile=8, order=dev(order) if as_tensor else order)
    assert all(TC.same_bits(host_of(got.weights)[k], want.weights[k]) for k in want.weights)
    assert TC.same_bits(got.p.cpu().numpy(), want.p) and [h[1:] for h in got.history] == [h[1:] for h in want.history]
    with pytest.raises(ValueError, match="permutation"):
        T.train_device(fam, w, ids, dense, y, order=dev(np.zeros(50, dtype=np.int64)) if as_tensor else np.zeros(50, dtype=np.int64))


# ---------------------------------------------------------------- widths

@pytest.mark.parametrize("widths", [(1,), (63,), (64,), (65,), (128,), (7, 6, 5), (9, 1, 17), (128, 64, 3)])
def test_hidden_stacks(torch, widths):
    """Width 1, widths around 64, width 128; depths 1 and 3."""
    fam, w, ids, dense, y = small(40, seed=len(widths) + widths[0], widths=widths)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


@pytest.mark.parametrize("emb_dim", [3, 10])
def test_embedding_widths(torch, emb_dim):
    fam, w, ids, dense, y = small(100, seed=emb_dim, vocabs=(50, 70), kinds=("id", "id"), emb_dim=emb_dim, n_dense=0, widths=(10, 10))
    both(fam, w, ids, dense, y, batch_size=32, epochs=2, tile=8)


@pytest.mark.parametrize("hidden", [(16, 8), (128, 128)])
def test_embedding_mlp_with_raw_numerics(torch, hidden):
    """EmbeddingMLP itself, at (16, 8) and at the reference's (128, 128), tens of rows, the numerics at their real magnitudes
    (releaseYear, rating counts) under trained-like weights; the default tile."""
    model = M.EmbeddingMLP(seed=5, movie_buckets=30, user_buckets=40, hidden=hidden)
    fam = T.family_of(model)
    ids, _, y = TC.data(fam, 40, 9)
    rng = np.random.default_rng(9)
    dense = np.stack([{"releaseYear": rng.integers(1930, 2016, 40), "movieRatingCount": rng.integers(1, 60000, 40), "userRatingCount": rng.integers(1, 3000, 40)}
                      .get(k, rng.uniform(0, 5, 40)) for k in model.numeric_keys], axis=1).astype(F)
    both(fam, model.weights, ids, dense, y, batch_size=16, epochs=2)


# ---------------------------------------------------------------- ids

def test_runs_of_ids(torch):
    """A batch in which every sample hits one row (run length B), a row hit exactly once, rows never hit -- bit-equal to their initial
    value after step 1 --, a row hit in step 1 and never again, which keeps moving; the same id value in every column."""
    fam, w, ids, dense, y = small(48, seed=2, vocabs=(9, 9, 9), kinds=("id", "genre", "id"))
    ids[:16] = 3                                                        # batch 0: one row of every table, the same id value in every column
    ids[16:, 0] = np.where(ids[16:, 0] == 3, 4, ids[16:, 0])            # row 3 of table 0: step 1 and never again
    ids[16:, 2] = 5
    ids[20, 2] = 7                                                      # hit exactly once
    ids[:, 1] = np.where(ids[:, 1] == 8, 0, ids[:, 1])                  # row 8 of table 1: never
    one = both(fam, w, ids[:16], dense[:16], y[:16], batch_size=16, epochs=1, tile=8)
    for c in range(3):
        keep = np.arange(9) != 3
        assert TC.same_bits(one.weights["emb/c%d" % c][keep], w["emb/c%d" % c][keep])
        assert not TC.same_bits(one.weights["emb/c%d" % c][3], w["emb/c%d" % c][3])
    two = both(fam, w, ids[:32], dense[:32], y[:32], batch_size=16, epochs=1, tile=8)
    three = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert not TC.same_bits(three.weights["emb/c0"][3], two.weights["emb/c0"][3])
    assert TC.same_bits(three.weights["emb/c1"][8], w["emb/c1"][8])


def test_every_genre_id_none(torch):
    fam, w, ids, dense, y = small(40, seed=3, vocabs=(6, 5, 4), kinds=("id", "genre", "genre"))
    ids[:, 1:] = -1
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert TC.same_bits(got.weights["emb/c1"], w["emb/c1"]) and TC.same_bits(got.weights["emb/c2"], w["emb/c2"])


# ---------------------------------------------------------------- arithmetic edges

def test_relu_at_exactly_zero(torch):
    """Unit 0 of the first layer has a zero column and a zero bias: its pre-activation is exactly 0 and passes nothing."""
    fam, w, ids, dense, y = small(40, seed=6, widths=(4, 3))
    w["dense0/kernel"][:, 0] = 0.0
    w["dense0/bias"][0] = 0.0
    got = both(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    assert not got.m["dense0/kernel"][:, 0].any() and not got.m["dense0/bias"][0]
    assert got.m["dense1/kernel"][1:].any() and not got.m["dense1/kernel"][0].any()


@pytest.mark.parametrize("bias", [100.0, -100.0, 30.0])
def test_saturated_sigmoid(torch, bias):
    """Logits that saturate sigmoid_def to exactly 1 (and, below -87, to exactly 0), against labels 0 and 1."""
    fam, w, ids, dense, y = small(40, seed=7)
    w["head/bias"][0] = bias
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert set(np.unique(got.p).tolist()) <= ({1.0} if bias > 0 else {0.0})
    assert set(y.tolist()) == {0.0, 1.0}


def test_sigmoid_def_on_its_whole_grid(torch):
    """The device's sigmoid against ``sigmoid_def`` on the CPU test's grid (cut to |z| <= 1e30): one numeric carries z, two units hold
    relu(z) and relu(-z), the head subtracts them, so the logit is z exactly; one batch, so every p comes from these weights."""
    z = TC.sigmoid_grid()
    z = z[np.abs(z) <= 1e30]
    fam = TC.family([2], ["id"], 1, 1, [2])
    w = {k: np.zeros(s, dtype=F) for k, s in T.param_shapes(fam).items()}
    w["dense0/kernel"][fam.xcol.index(-1)] = [1.0, -1.0]
    w["head/kernel"][:, 0] = [1.0, -1.0]
    ids, y = np.zeros((len(z), 1), dtype=np.int32), (np.arange(len(z)) % 2).astype(F)
    got = T.train_device(fam, w, ids, z[:, None].copy(), y, batch_size=len(z), epochs=1, tile=8)
    want = T.sigmoid_def(z)
    p = got.p.cpu().numpy()
    assert TC.same_bits(p, want), (z[p != want][:8], p[p != want][:8], want[p != want][:8])
    assert TC.same_bits(T.train_host(fam, w, ids, z[:, None].copy(), y, batch_size=len(z), epochs=1, tile=8).p, want)


@pytest.mark.parametrize("scale", [1e-20, 1e-30, 1e-39])
def test_subnormal_weights_and_moments(torch, scale):
    fam, w, ids, dense, y = small(40, seed=8, widths=(6, 4))
    w = {k: (v.astype(np.float64) * scale).astype(F) for k, v in w.items()}
    tiny = np.finfo(F).tiny
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    sub = lambda d: any(((np.abs(a) > 0) & (np.abs(a) < tiny)).any() for a in d.values())
    assert sub(got.m) if scale == 1e-20 else sub(w) if scale == 1e-39 else True


# ---------------------------------------------------------------- the long sort path

def test_batches_beyond_the_lds_sort_capacity(torch, monkeypatch):
    """SPRK_FE_SORT_CAP=64: a batch's 40 x 3 entries take the chunked sort and the merge passes."""
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    fam, w, ids, dense, y = small(100, seed=9, vocabs=(6, 5, 9), kinds=("id", "id", "id"))
    both(fam, w, ids, dense, y, batch_size=40, epochs=2, tile=8)


# ---------------------------------------------------------------- the C ABI: errors, memory, streams

GUARD = 64


def raw_fit(torch, fam, w, ids, dense, y, batch, tile, epochs, stream=None, slack=0):
    """``sprk_train_fit`` itself: parameters, moments, p and the workspace each inside guard bands of a fixed pattern, the workspace
    exactly as large as ``sprk_train_workspace_bytes`` reports (+ ``slack``).  -> (rc, params, m, v, p, error word, guards intact)."""
    lib = L.load_library()
    dev = torch.device("cuda")
    n = len(y)
    flat = T._flatten(fam, w, dev)
    ms = T._model_struct(fam)
    need = int(lib.sprk_train_workspace_bytes(C.byref(ms), n, batch, tile))
    assert need > 0 and need % 16 == 0

    def banded(count, dtype, fill=None):
        buf = torch.full((count + 2 * GUARD,), 0x5A if dtype == torch.uint8 else -7, dtype=dtype, device=dev)
        if fill is not None:
            buf[GUARD:GUARD + count] = fill
        return buf
    params, m, v = banded(flat.numel(), torch.float32, flat), banded(flat.numel(), torch.float32, 0.0), banded(flat.numel(), torch.float32, 0.0)
    p = banded(max(epochs, 1) * n, torch.float32, 0.0)
    ws = banded(need + slack, torch.uint8)
    steps = (n + batch - 1) // batch
    alphas = torch.from_numpy(np.array([T.adam_alpha(0.001, t + 1) for t in range(epochs * steps)] + [0.0], dtype=F)).to(dev)
    word = torch.full((1,), -1, dtype=torch.int64, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_ids, t_dense, t_y = up(ids), up(dense), up(y)
    c1, c2, eps = T.adam_constants()
    at = lambda b, size: C.c_void_p(b.data_ptr() + GUARD * size)
    rc = lib.sprk_train_fit(C.byref(ms), C.c_void_p(t_ids.data_ptr()), C.c_void_p(t_dense.data_ptr()) if fam.n_dense else None, C.c_void_p(t_y.data_ptr()), None,
                            n, batch, tile, epochs, C.c_void_p(alphas.data_ptr()), float(c1), float(c2), float(eps), at(params, 4), at(m, 4), at(v, 4), at(p, 4),
                            C.c_void_p(word.data_ptr()), at(ws, 1), need + slack, C.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream))
    (stream or torch.cuda.current_stream()).synchronize()
    intact = all(bool((b[:GUARD] == b[0]).all()) and bool((b[-GUARD:] == b[0]).all()) and (float(b[0]) in (-7.0, 90.0)) for b in (params, m, v, p, ws))
    cut = lambda b: b[GUARD:-GUARD].cpu().numpy()
    return rc, cut(params), cut(m), cut(v), cut(p), int(word.cpu()[0]), intact


def test_guard_bands_side_stream_exact_workspace(torch):
    fam, w, ids, dense, y = small(50, seed=10)
    want = T.train_host(fam, w, ids, dense, y, batch_size=12, epochs=2, tile=8)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 12, 8, 2, stream=side)
    assert rc == 0 and word == -1 and intact
    flat = lambda d: np.concatenate([d[k].reshape(-1) for k in T.param_names(fam)])
    assert TC.same_bits(params, flat(want.weights)) and TC.same_bits(m, flat(want.m)) and TC.same_bits(v, flat(want.v))
    assert TC.same_bits(p[50:], want.p)
    lib = L.load_library()
    ms = T._model_struct(fam)
    need = int(lib.sprk_train_workspace_bytes(C.byref(ms), 50, 12, 8))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    word_t = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    f = torch.zeros(T._flatten(fam, w, torch.device("cuda")).numel(), device="cuda")
    z = C.c_void_p(f.data_ptr())
    rc = lib.sprk_train_fit(C.byref(ms), z, z, z, None, 50, 12, 8, 1, z, 0.1, 0.001, 1e-7, z, z, z, z, C.c_void_p(word_t.data_ptr()), C.c_void_p(ws.data_ptr()), need - 1, None)
    assert rc == L.EINVAL and b"sprk_train_workspace_bytes" in lib.sprk_last_error()
    assert lib.sprk_train_workspace_bytes(C.byref(ms), (1 << 31) // 3 + 1, 12, 8) == 0           # N x columns beyond the offsets' range
    assert lib.sprk_train_workspace_bytes(C.byref(ms), 50, 12, 1 << 20) == 0                      # a tile beyond the LDS


def test_each_error_word_and_no_parameter_moves(torch):
    fam, w, ids, dense, y = small(40, seed=11)
    flat0 = np.concatenate([w[k].reshape(-1) for k in T.param_names(fam)])

    def check(kind, row, message, ids=ids, dense=dense, y=y):
        rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 16, 8, 2)
        assert rc == 0 and intact and word == (kind << 32 | row), (word >> 32, word & 0xffffffff)
        assert TC.same_bits(params, flat0) and not m.any() and not v.any()
        for fit in (T.train_device, T.train_host):
            with pytest.raises(ValueError, match=message):
                fit(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    bad = ids.copy(); bad[30, 0] = 6; bad[12, 0] = -1; bad[20, 1] = -2
    check(T.ERR_ID, 12, "samples row 12: an id outside", ids=bad)
    bad = ids.copy(); bad[5, 1] = 5
    check(T.ERR_ID, 5, "samples row 5: an id outside", ids=bad)
    bad = dense.copy(); bad[9, 1] = np.inf; bad[3, 0] = np.nan
    check(T.ERR_NUMERIC, 3, "samples row 3: a numeric", dense=bad)
    bad = y.copy(); bad[7] = np.nan; bad[39] = -np.inf
    check(T.ERR_LABEL, 7, "samples row 7: the label", y=bad)
    bd, by = dense.copy(), y.copy()
    bd[1, 0], by[0] = np.nan, np.inf
    check(T.ERR_NUMERIC, 1, "samples row 1: a numeric", dense=bd, y=by)


def test_two_device_fits_give_the_same_bytes(torch):
    fam, w, ids, dense, y = small(200, seed=12, widths=(65, 7))
    a = T.train_device(fam, w, ids, dense, y, batch_size=48, epochs=2, tile=8)
    b = T.train_device(fam, w, ids, dense, y, batch_size=48, epochs=2, tile=8)
    for x, z in ((a.weights, b.weights), (a.m, b.m), (a.v, b.v)):
        assert all(TC.same_bits(x[k].cpu().numpy(), z[k].cpu().numpy()) for k in x)
    assert TC.same_bits(a.p.cpu().numpy(), b.p.cpu().numpy()) and a.history == b.history


def test_zero_epochs_and_continuation(torch):
    fam, w, ids, dense, y = small(40, seed=13)
    got = T.train_device(fam, w, ids, dense, y, epochs=0)
    assert got.step == 0 and got.history == [] and all(TC.same_bits(got.weights[k].cpu().numpy(), w[k]) for k in w)
    one = T.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    a = T.train_device(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    b = T.train_device(fam, a.weights, ids, dense, y, batch_size=16, epochs=1, tile=8, state=(a.m, a.v, a.step))
    assert b.step == one.step and all(TC.same_bits(b.weights[k].cpu().numpy(), one.weights[k]) and TC.same_bits(b.v[k].cpu().numpy(), one.v[k]) for k in w)


# ---------------------------------------------------------------- end to end

def test_ratings_to_recommendations(torch):
    """A few hundred synthetic ratings: featureeng.build -> NeuralCF.fit(samples.columns) -> evaluate_device -> recommend, against the
    same chain through samples_host, train_host and set_weights: the weights byte for byte, the recommendations identical."""
    from sparrowrecsys_amd import featureeng as FE
    from tests import featureeng_cases as cases
    ratings, movies = cases.synthetic_ratings(), cases.synthetic_movies()
    built = FE.build(ratings, movies, 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    make = lambda: M.NeuralCF(seed=3, movie_buckets=cases.N_MOVIES, user_buckets=cases.N_USERS)
    model = make()
    model.set_weights(model.init_weights(3, trained_like=False))
    start = {k: v.copy() for k, v in model.weights.items()}
    history = model.fit(built.columns, batch_size=64, epochs=2, learning_rate=0.01)
    cols = FE.samples_host(ratings, movies, 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    other = make()
    ids, dense = other.pack(cols)
    want = T.train_host(T.family_of(other), start, ids, dense, np.asarray(cols["label"], dtype=F), batch_size=64, epochs=2, learning_rate=0.01)
    assert all(TC.same_bits(model.weights[k], want.weights[k]) for k in want.weights)
    assert not TC.same_bits(model.weights["emb/userId"], start["emb/userId"])
    assert [h[1:] for h in history] == [h[1:] for h in want.history] and len(history) == 2
    other.set_weights(want.weights)
    assert model.evaluate_device(built.columns) == other.evaluate_device(built.columns)
    assert TC.same_bits(model.predict(cols), other.predict(cols))
    store = built.store()
    users, cand = np.array([30, 12, 8, 1, 17]), np.arange(1, 116, 2)
    got = model.recommend(store, users, cand, 10)
    assert got == other.recommend(store, users, cand, 10) and len(got[0]) == 10 and got[3] == []
    again = model.fit(built.columns, batch_size=64, epochs=1, learning_rate=0.01)             # the moments were kept: the fit goes on
    cont = T.train_host(T.family_of(other), want.weights, ids, dense, np.asarray(cols["label"], dtype=F), batch_size=64, epochs=1, learning_rate=0.01,
                        state=(want.m, want.v, want.step))
    assert all(TC.same_bits(model.weights[k], cont.weights[k]) for k in cont.weights) and again[0][1:] == cont.history[0][1:]


# ---------------------------------------------------------------- the step shape model.fit ships with

def _mlp_128(n, seed):
    """``EmbeddingMLP(hidden=(128, 128))`` over small buckets: n_x = 107, the default tile 8."""
    model = M.EmbeddingMLP(seed=5, movie_buckets=30, user_buckets=40, hidden=(128, 128))
    fam = T.family_of(model)
    return (fam, model.weights) + TC.data(fam, n, seed)


@pytest.mark.parametrize("which", ["neuralcf", "embedding_mlp"])
def test_batch_4096_at_the_default_tile(torch, which):
    """N = 4096 + 77, one epoch: one full batch of ``DEFAULT_BATCH`` rows and a short one.  NeuralCF over tables of 1 001 and 30 001 rows
    (tile 16: 256 tiles, then 5); EmbeddingMLP (128, 128) (tile 8: 512 tiles, then 10 -- 64 rounds of the unrolled partial sum)."""
    n = T.DEFAULT_BATCH + 77
    if which == "neuralcf":
        model = M.NeuralCF(seed=3, movie_buckets=1001, user_buckets=30001)
        fam = T.family_of(model)
        fam, w, ids, dense, y = (fam, model.weights) + TC.data(fam, n, 21)
        assert fam.widths == [10, 10] and len(fam.xcol) == 20 and T.default_tile(fam) == 16
    else:
        fam, w, ids, dense, y = _mlp_128(n, 22)
        assert T.default_tile(fam) == 8
    want = both(fam, w, ids, dense, y, epochs=1)
    assert want.step == 2


@pytest.mark.parametrize("batch", [56, 64, 72, 120, 128, 136])
def test_tile_counts_around_the_unrolled_partial_sum(torch, batch):
    """Tile 8: 7, 8, 9, 15, 16 and 17 tiles -- k_tr_dense_adam adds eight partials at a time, then the rest -- and a last batch of 5 rows."""
    fam, w, ids, dense, y = small(batch + 5, seed=batch)
    assert batch // 8 in (7, 8, 9, 15, 16, 17)
    both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=8)


def test_steps_of_more_than_48_kb_of_lds(torch):
    """EmbeddingMLP (128, 128): 619 floats of LDS per sample.  The tiles come from ``lds_bytes``: ``mid`` = half the largest, above 48 KB (the
    step kernel needs its attribute raised), run before and after a step of 20 KB in this one process; ``top`` = the largest that fits 160 KB;
    ``top + 1`` is refused in words by the library and by ``train_device``."""
    fam, w, ids, dense, y = _mlp_128(60, 23)
    per = T.lds_bytes(fam, 1)
    assert per == 619 * 4
    top = T.LDS_BYTES // per
    mid = top // 2
    assert 48 * 1024 < T.lds_bytes(fam, mid) < T.lds_bytes(fam, top) <= T.LDS_BYTES < T.lds_bytes(fam, top + 1) and T.lds_bytes(fam, 8) < 48 * 1024
    for tile, n in ((mid, 50), (8, 40), (mid, 60), (top, 60)):
        both(fam, w, ids[:n], dense[:n], y[:n], batch_size=n, epochs=2, tile=tile)
    lib = L.load_library()
    ms = T._model_struct(fam)
    assert lib.sprk_train_workspace_bytes(C.byref(ms), 60, 60, top) > 0 and lib.sprk_train_workspace_bytes(C.byref(ms), 60, 60, top + 1) == 0
    rc = lib.sprk_train_fit(C.byref(ms), None, None, None, None, 60, 60, top + 1, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None, None, 0, None)
    assert rc == L.EINVAL and b"tile = %d needs %d bytes of LDS" % (top + 1, T.lds_bytes(fam, top + 1)) in lib.sprk_last_error()
    with pytest.raises(ValueError, match="tile = %d needs %d bytes of LDS" % (top + 1, T.lds_bytes(fam, top + 1))):
        T.train_device(fam, w, ids, dense, y, batch_size=60, epochs=1, tile=top + 1)


def test_a_tile_wider_than_the_workgroup(torch):
    """Tile 300 > 256 threads: every per-sample loop of k_tr_step goes round; N = batch = 650 gives tiles of 300, 300 and 50."""
    fam, w, ids, dense, y = small(650, seed=24)
    assert T.lds_bytes(fam, 300) <= 48 * 1024
    both(fam, w, ids, dense, y, batch_size=650, epochs=2, tile=300)


@pytest.mark.parametrize("layers", [1, T.MAX_LAYERS])
def test_the_stated_maxima(torch, layers):
    """16 id columns x emb_dim 16 = 256 input rows, layers of 256 units, one and eight of them; 40 rows, tile 8."""
    fam = TC.family([5] * T.MAX_COLS, ["id", "genre"] * (T.MAX_COLS // 2), 16, 0, [T.MAX_WIDTH] * layers)
    assert len(fam.xcol) == T.MAX_X and len(fam.columns) == T.MAX_COLS
    w = TC.weights(fam, 25)
    ids, dense, y = TC.data(fam, 40, 25)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


def test_a_table_beyond_one_round_of_the_grid(torch):
    """Vocabularies (60 000, 5) x 10: 600 050 table floats, more than the 524 288 one round of k_tr_table_adam's grid covers.  Step 1 hits
    rows 0, 52 428, 52 429 and 59 999: elements 524 280 .. 524 299 lie on both sides of the round's end.  Those rows move, rows never hit
    keep their bits, and a row hit in step 1 only still moves in step 3."""
    fam = TC.family([60000, 5], ["id", "id"], 10, 2, [6])
    w = TC.weights(fam, 26)
    ids, dense, y = TC.data(fam, 40, 26)
    first = np.array([0, 52428, 52429, 59999])
    ids[:16, 0] = first[np.arange(16) % 4]
    later = np.random.default_rng(26).integers(100, 50000, 24)
    ids[16:, 0] = later
    assert (ids[16:, 0] != 52428).all() and 52428 * 10 < 2048 * 256 <= 52429 * 10
    one = both(fam, w, ids[:16], dense[:16], y[:16], batch_size=16, epochs=1, tile=8)
    two = both(fam, w, ids[:32], dense[:32], y[:32], batch_size=16, epochs=1, tile=8)
    three = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert three.step == 3
    for row in first:
        assert not TC.same_bits(one.weights["emb/c0"][row], w["emb/c0"][row])
        assert not TC.same_bits(three.weights["emb/c0"][row], two.weights["emb/c0"][row])             # hit in step 1 only: still moving
    never = np.ones(60000, dtype=bool)
    never[ids[:, 0]] = False
    assert never.sum() > 59900 and TC.same_bits(three.weights["emb/c0"][never], w["emb/c0"][never])
    assert TC.same_bits(one.weights["emb/c0"][np.setdiff1d(np.arange(60000), first)], w["emb/c0"][np.setdiff1d(np.arange(60000), first)])


@pytest.mark.parametrize("batch,tile", [(4096, 32), (33000, 128)])
def test_the_schedule_beyond_one_round_of_the_grid(torch, batch, tile):
    """16 columns of vocabulary 7, emb_dim 2, N = 33 000: 528 000 entries, so k_tr_count and k_tr_scatter make a second trip; in batches
    of 4 096 and as one batch of 33 000."""
    fam = TC.family([7] * 16, ["id", "genre"] * 8, 2, 1, [4])
    w = TC.weights(fam, 27)
    ids, dense, y = TC.data(fam, 33000, 27)
    assert ids.size > 2048 * 256
    both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=tile)


def test_the_error_word_beyond_one_round_of_the_grid(torch):
    """N = 524 288 + 600: bad labels at rows 524 300 and 524 500, both in k_tr_check's second trip.  Both routes name row 524 300 and no
    parameter moves; the check precedes any training."""
    fam, w, ids, dense, y = small(2048 * 256 + 600, seed=28)
    y[524500], y[524300] = np.nan, np.inf
    flat0 = np.concatenate([w[k].reshape(-1) for k in T.param_names(fam)])
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, y, 65536, 16, 1)
    assert rc == 0 and intact and word == (T.ERR_LABEL << 32 | 524300), (word >> 32, word & 0xffffffff)
    assert TC.same_bits(params, flat0) and not m.any() and not v.any()
    for fit in (T.train_device, T.train_host):
        with pytest.raises(ValueError, match="samples row 524300: the label"):
            fit(fam, w, ids, dense, y, batch_size=65536, epochs=1, tile=16)
