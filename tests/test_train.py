"""The trainer's definition (sparrowrecsys_amd/trainer.py, ``train_host``) against independent implementations; no GPU.  The measured
figures are in docs/train_results.md."""
import math

import numpy as np
import pytest

from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd.metrics import exact_roc_auc
from tests import train_cases as TC

F = np.float32


# ---------------------------------------------------------------- forward

@pytest.mark.parametrize("name", ["neural_cf", "embedding_mlp"])
def test_forward_matches_the_float64_oracle(samples, name):
    """The definition's float32 forward against oracle.ctr_oracle in float64, random trained-like weights, the reference widths:
    within 1e-4 absolute, smoke()'s bound for a float32 forward against this oracle."""
    from oracle import ctr_oracle as O
    model = {"neural_cf": M.NeuralCF, "embedding_mlp": M.EmbeddingMLP}[name](seed=11)
    fam = T.family_of(model)
    ids, dense = model._pack_python(samples)
    got = T.forward_host(fam, model.weights, ids, dense)
    want = O.FORWARDS[name](samples, model.weights, dtype=np.float64).reshape(-1)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: max |p - oracle| = %.3e over %d rows" % (name, err, len(got)))
    assert got.dtype == F and err <= 1e-4


# ---------------------------------------------------------------- sigmoid_def

def test_sigmoid_def_sweep():
    """Monotone, within [0, 1], exactly 0.5 at 0, exactly 0 and 1 at the ends, never a NaN or an infinity; and its largest error
    against 1 / (1 + exp(-z)) in float64 over the grid: 1.232081 float32 ulps of the true value (at z = -86.825, beyond the corrected
    range; 1.01 ulp at most inside it), 1 as a distance between float32 neighbours.  The grid is fixed, so both figures are asserted as they are."""
    z = TC.sigmoid_grid()
    p = T.sigmoid_def(z)
    assert p.dtype == F and np.isfinite(p).all() and p.min() == 0.0 and p.max() == 1.0
    assert (np.diff(p) >= 0).all()
    assert T.sigmoid_def(F(0.0)).tobytes() == F(0.5).tobytes() and T.sigmoid_def(F(-0.0)).tobytes() == F(0.5).tobytes()
    assert (p[z < -87] == 0).all() and (p[z >= -87] > 0).all() and (p[z >= 20] == 1).all()
    inside = z >= -87                                                   # (below: the definition's cut to exactly 0)
    with np.errstate(over="ignore"):
        ref = 1.0 / (1.0 + np.exp(-z[inside].astype(np.float64)))
    ulp = np.spacing(ref.astype(F)).astype(np.float64)
    err = np.abs(p[inside].astype(np.float64) - ref) / ulp
    steps = np.abs(p[inside].view(np.int32).astype(np.int64) - ref.astype(F).view(np.int32).astype(np.int64))
    print("sigmoid_def over %d points: max error %.6f ulp at z = %r, %d float32 steps" % (len(z), err.max(), float(z[inside][err.argmax()]), steps.max()))
    assert round(float(err.max()), 6) == 1.232081 and float(z[inside][err.argmax()]) == float(F(-86.825))
    assert int(steps.max()) == 1


# ---------------------------------------------------------------- gradients

GRAD_FAMILIES = {"neural_cf": ([50, 70], ["id", "id"], 10, 0, [10, 10]),
                 "embedding_mlp": ([20, 20, 40, 90], ["genre", "genre", "id", "id"], 10, 7, [128, 128]),
                 "odd": ([7, 5, 9], ["id", "genre", "id"], 3, 2, [65, 1, 17])}


GRAD_SEEDS = 5


@pytest.mark.parametrize("name", sorted(GRAD_FAMILIES))
@pytest.mark.parametrize("tile", [7, 32])
def test_step_gradients_match_torch_autograd(name, tile):
    """One step's gradients against torch CPU autograd in float64 on the same graph.  Per tensor: the definition's largest error
    relative to the tensor's largest magnitude is at most 4 x the same error of torch's own float32 autograd (both are float32 sums
    of the same lengths in different orders; measured ratios in docs/train_results.md).  Each error is the largest over five fixed
    draws of weights and data: a bias of the head is ONE number, torch's float32 value of it is often the correctly rounded one, whose
    error is anywhere between 0 and half a step, and a single draw of such a ratio says nothing about either implementation."""
    import torch
    fam = TC.family(*GRAD_FAMILIES[name])
    mine, theirs = {}, {}
    for seed in range(GRAD_SEEDS):
        w = TC.weights(fam, 3 + seed)
        ids, dense, y = TC.data(fam, 200, 5 + seed)
        g, p = T.step_gradients(fam, w, ids, dense, y, tile)
        g64, p64 = TC.torch_gradients(fam, w, ids, dense, y, torch.float64)
        g32, _ = TC.torch_gradients(fam, w, ids, dense, y, torch.float32)
        assert float(np.abs(p - p64).max()) <= 1e-6
        assert set(g) == set(T.param_names(fam))
        for k in T.param_names(fam):
            assert g[k].dtype == F and g[k].shape == w[k].shape
            big = float(np.abs(g64[k]).max())
            if big == 0.0:                                              # (a dead unit in front of it: exactly zero on both sides)
                assert not g[k].any() and not g32[k].any()
                continue
            mine[k] = max(mine.get(k, 0.0), float(np.abs(g[k] - g64[k]).max()) / big)
            theirs[k] = max(theirs.get(k, 0.0), float(np.abs(g32[k] - g64[k]).max()) / big)
    for k in sorted(mine):
        print("%s tile %d %-14s definition %.3e torch float32 %.3e ratio %.2f" % (name, tile, k, mine[k], theirs[k], mine[k] / theirs[k]))
        assert mine[k] <= 4.0 * theirs[k], k


def test_gradient_tiles_change_the_order_only():
    """``tile`` regroups the sums: gradients of different tiles agree to float32 rounding, and a tile of at least the batch is the
    plain sample-order sum."""
    fam = TC.family([9, 6], ["id", "genre"], 4, 1, [8])
    w = TC.weights(fam, 1)
    ids, dense, y = TC.data(fam, 50, 2)
    a, _ = T.step_gradients(fam, w, ids, dense, y, 50)
    b, _ = T.step_gradients(fam, w, ids, dense, y, 64)
    c, _ = T.step_gradients(fam, w, ids, dense, y, 3)
    for k in a:
        assert TC.same_bits(a[k], b[k])
        assert np.abs(a[k] - c[k]).max() <= 1e-6 * max(np.abs(a[k]).max(), 1e-30)


# ---------------------------------------------------------------- Adam

def _adam64(w, m, v, g, lr, t, b1=0.9, b2=0.999, eps=1e-7):
    """TensorFlow's documented ApplyAdam in float64: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); m += (g - m)(1 - b1);
    v += (g g - v)(1 - b2); var -= lr_t m / (sqrt(v) + eps)."""
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    m = m + (g - m) * (1.0 - b1)
    v = v + (g * g - v) * (1.0 - b2)
    return w - lr_t * m / (np.sqrt(v) + eps), m, v


def _adam32_fused(w, m, v, g, lr, t):
    """The same in float32 with fused multiply-adds where the formula has a product next to a sum (each emulated in float64 and
    rounded once)."""
    lr_t = F(lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
    c1, c2, eps = F(1.0) - F(0.9), F(1.0) - F(0.999), F(1e-7)
    m = ((g - m).astype(np.float64) * np.float64(c1) + m.astype(np.float64)).astype(F)
    v = ((g.astype(np.float64) * g.astype(np.float64) - v.astype(np.float64)).astype(F).astype(np.float64) * np.float64(c2) + v.astype(np.float64)).astype(F)
    q = ((lr_t * m) / (np.sqrt(v) + eps)).astype(F)
    return (w - q).astype(F), m, v


@pytest.mark.parametrize("steps", [1, 50])
def test_adam_matches_the_documented_formula(steps):
    """One step and a run of 50 on a fixed gradient sequence against the float64 restatement; the margin is measured: at most 4 x the
    error of the fused float32 restatement (with a floor of one float32 half-ulp of the largest weight)."""
    rng = np.random.default_rng(7)
    w0 = rng.standard_normal(4096).astype(F)
    gs = [(rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 1, size=4096)).astype(F) for _ in range(steps)]
    gs[0][:64] = 0.0                                                    # untouched rows: g = 0 still moves m, v and w on later steps
    w, m, v = w0.copy(), np.zeros_like(w0), np.zeros_like(w0)
    w64, m64, v64 = w0.astype(np.float64), np.zeros(4096), np.zeros(4096)
    wf, mf, vf = w0.copy(), np.zeros_like(w0), np.zeros_like(w0)
    for t, g in enumerate(gs, 1):
        T.adam_step(w, m, v, g, T.adam_alpha(0.001, t))
        w64, m64, v64 = _adam64(w64, m64, v64, g.astype(np.float64), 0.001, t)
        wf, mf, vf = _adam32_fused(wf, mf, vf, g, 0.001, t)
    for what, mine, fused, ref in (("w", w, wf, w64), ("m", m, mf, m64), ("v", v, vf, v64)):
        big = float(np.abs(ref).max())
        e_mine, e_fused = float(np.abs(mine - ref).max()) / big, float(np.abs(fused - ref).max()) / big
        print("%d steps %s: definition %.3e fused float32 %.3e" % (steps, what, e_mine, e_fused))
        assert e_mine <= 4.0 * max(e_fused, 2.0 ** -24), what
    if steps > 1:
        assert (w[:64] != w0[:64]).any()


def test_adam_constants_and_alpha():
    c1, c2, eps = T.adam_constants()
    assert c1 == F(1.0) - F(0.9) and c2 == F(1.0) - F(0.999) and eps == F(1e-7)
    assert T.adam_alpha(0.001, 1) == F(0.001 * math.sqrt(1.0 - 0.999) / (1.0 - 0.9))


# ---------------------------------------------------------------- it learns

def test_it_learns():
    """Planted structure (tests/train_cases.py planted()): NeuralCF at the reference widths, batch 256, 5 epochs, lr 0.01.  Every
    epoch's loss is below the one before, and the held-out rank AUC clears 0.729: torch.optim.Adam(eps=1e-7) on the same graph and
    arrays over five seeds (scripts/train_torch_baseline.py) gave falling losses for all five and held-out AUCs 0.7636 .. 0.7977 from
    0.49 .. 0.50, the teacher at 0.9065; the threshold is torch's lowest minus torch's own spread, 0.7636 - 0.0342.  Measured here:
    0.7956."""
    (ids, y), (tids, ty), _ = TC.planted()
    model = TC.planted_model(0)
    fam = T.family_of(model)
    none = lambda n: np.zeros((n, 0), dtype=F)
    before = exact_roc_auc(ty, T.forward_host(fam, model.weights, tids, none(len(ty))))
    got = T.train_host(fam, model.weights, ids, none(len(y)), y, batch_size=256, epochs=5, learning_rate=0.01)
    losses = [h[0] for h in got.history]
    after = exact_roc_auc(ty, T.forward_host(fam, got.weights, tids, none(len(ty))))
    print("losses %s; held-out AUC %.4f -> %.4f" % (" ".join("%.4f" % l for l in losses), before, after))
    assert got.step == 5 * 64 and len(losses) == 5
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert after >= 0.729


# ---------------------------------------------------------------- errors and edges

def _small():
    fam = TC.family([6, 5], ["id", "genre"], 3, 2, [4])
    return (fam, TC.weights(fam, 0)) + TC.data(fam, 40, 0)


def test_errors_name_the_smallest_failing_row_and_change_nothing():
    fam, w, ids, dense, y = _small()
    keep = {k: v.copy() for k, v in w.items()}

    def raises(match, ids=ids, dense=dense, y=y):
        with pytest.raises(ValueError, match=match):
            T.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1)
        assert all(TC.same_bits(w[k], keep[k]) for k in w)
    bad = ids.copy(); bad[30, 0] = 6; bad[12, 0] = -1; bad[20, 1] = -2
    raises("samples row 12: an id outside", ids=bad)
    bad = ids.copy(); bad[5, 1] = 5
    raises("samples row 5: an id outside", ids=bad)
    bad = dense.copy(); bad[9, 1] = np.inf; bad[3, 0] = np.nan
    raises("samples row 3: a numeric feature is not finite", dense=bad)
    bad = y.copy(); bad[7] = np.nan
    raises("samples row 7: the label is not finite", y=bad)
    # the kinds rank id < numeric < label, whatever the rows
    bd, by, bi = dense.copy(), y.copy(), ids.copy()
    bd[1, 0], by[0], bi[39, 0] = np.nan, np.inf, 99
    raises("samples row 39: an id outside", ids=bi, dense=bd, y=by)
    raises("samples row 1: a numeric", dense=bd, y=by)
    ok_none = ids.copy(); ok_none[:, 1] = -1                              # -1 is a value of a genre column
    T.train_host(fam, w, ok_none, dense, y, batch_size=16, epochs=1)
    with pytest.raises(ValueError, match="permutation"):
        T.train_host(fam, w, ids, dense, y, order=np.zeros(40, dtype=np.int64))
    for kw in ({"batch_size": 0}, {"epochs": -1}, {"learning_rate": 0.0}, {"learning_rate": float("nan")}, {"tile": 0}):
        with pytest.raises(ValueError):
            T.train_host(fam, w, ids, dense, y, **kw)


def test_zero_epochs_return_the_input_bits():
    fam, w, ids, dense, y = _small()
    got = T.train_host(fam, w, ids, dense, y, epochs=0)
    assert got.step == 0 and got.history == []
    assert all(TC.same_bits(got.weights[k], w[k]) and not got.m[k].any() and not got.v[k].any() for k in w)
    assert all(got.weights[k] is not w[k] for k in w)


def test_batches_order_and_continuation():
    """A short last batch is a step of its own; ``order`` permutes once; two fits of one epoch equal one fit of two."""
    fam, w, ids, dense, y = _small()
    one = T.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5)
    assert one.step == 6 and len(one.history) == 2 and one.p.shape == (40,)
    a = T.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=5)
    b = T.train_host(fam, a.weights, ids, dense, y, batch_size=16, epochs=1, tile=5, state=(a.m, a.v, a.step))
    assert b.step == 6 and all(TC.same_bits(b.weights[k], one.weights[k]) and TC.same_bits(b.m[k], one.m[k]) and TC.same_bits(b.v[k], one.v[k]) for k in w)
    order = np.random.default_rng(3).permutation(40)
    c = T.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5, order=order)
    d = T.train_host(fam, w, ids[order], dense[order], y[order], batch_size=16, epochs=2, tile=5)
    assert all(TC.same_bits(c.weights[k], d.weights[k]) for k in w) and TC.same_bits(c.p, d.p) and c.history == d.history
    assert not all(TC.same_bits(c.weights[k], one.weights[k]) for k in w)


def test_rows_a_batch_did_not_touch():
    """After step 1 a row never hit holds its initial bits (m = v = 0 gives a zero update); a row hit in step 1 and never again keeps
    moving, as under Keras' Adam."""
    fam = TC.family([8], ["id"], 3, 0, [4])
    w = TC.weights(fam, 2)
    ids = np.array([[0]] * 4 + [[1]] * 8, dtype=np.int32)
    y = np.array([1, 0, 1, 1] + [0, 1] * 4, dtype=F)
    none = np.zeros((12, 0), dtype=F)
    s1 = T.train_host(fam, w, ids[:4], none[:4], y[:4], batch_size=4, epochs=1)
    assert TC.same_bits(s1.weights["emb/c0"][1:], w["emb/c0"][1:]) and not TC.same_bits(s1.weights["emb/c0"][0], w["emb/c0"][0])
    s3 = T.train_host(fam, w, ids, none, y, batch_size=4, epochs=1)
    s2 = T.train_host(fam, w, ids[:8], none[:8], y[:8], batch_size=4, epochs=1)
    assert not TC.same_bits(s3.weights["emb/c0"][0], s2.weights["emb/c0"][0])            # row 0 moved in step 3 without being hit
    assert TC.same_bits(s3.weights["emb/c0"][2:], w["emb/c0"][2:])


@pytest.mark.parametrize("make", [lambda: M.WideNDeep(seed=1), lambda: M.NeuralCF(seed=1, arch=2), lambda: M.DeepFM(seed=1), lambda: M.DIN(seed=1)])
def test_fit_outside_the_family_raises(make):
    model = make()
    with pytest.raises(NotImplementedError, match=r"NeuralCF\(arch=1\) and EmbeddingMLP"):
        model.fit({"label": np.zeros(1)})


def test_fit_without_a_device_points_to_the_host_definition(samples):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no HIP device.*train_host"):
        M.NeuralCF(seed=1).fit(samples)
    fam = T.family_of(M.NeuralCF(seed=1))
    with pytest.raises(RuntimeError, match="no HIP device.*train_host"):
        T.train_device(fam, M.NeuralCF(seed=1).weights, np.zeros((1, 2), np.int32), np.zeros((1, 0), F), np.zeros(1, F))


LIMIT_STRUCT = {"columns": ("n_cols", T.MAX_COLS + 1), "layers": ("n_layers", T.MAX_LAYERS + 1), "rows": ("n_x", T.MAX_X + 1), "width": ("width", T.MAX_WIDTH + 1)}


@pytest.mark.parametrize("what,kw", [("columns", dict(vocabs=[5] * (T.MAX_COLS + 1), kinds=["id"] * (T.MAX_COLS + 1), emb_dim=2, n_dense=0, widths=[4])),
                                     ("layers", dict(vocabs=[5], kinds=["id"], emb_dim=2, n_dense=0, widths=[2] * (T.MAX_LAYERS + 1))),
                                     ("rows", dict(vocabs=[5] * T.MAX_COLS, kinds=["id"] * T.MAX_COLS, emb_dim=16, n_dense=1, widths=[4])),
                                     ("width", dict(vocabs=[5], kinds=["id"], emb_dim=2, n_dense=0, widths=[T.MAX_WIDTH + 1]))])
def test_one_more_than_each_maximum_is_refused_in_words(lib, what, kw):
    """17 id columns, 9 hidden layers, 257 input rows, a layer of 257 units: ``_check_family`` names the limits, and the library, given the
    largest family with that one field raised, reports no workspace and refuses the fit before any device call, naming them too."""
    import ctypes as C
    from sparrowrecsys_amd import _lib as L
    with pytest.raises(ValueError, match="up to %d id columns, %d hidden layers of up to %d units and %d input rows" % (T.MAX_COLS, T.MAX_LAYERS, T.MAX_WIDTH, T.MAX_X)):
        TC.family(**kw)
    fam = TC.family([5] * T.MAX_COLS, ["id"] * T.MAX_COLS, 16, 0, [T.MAX_WIDTH] * T.MAX_LAYERS)
    assert len(fam.xcol) == T.MAX_X
    ms = T._model_struct(fam)
    assert lib.sprk_train_workspace_bytes(C.byref(ms), 40, 16, 8) > 0
    field, value = LIMIT_STRUCT[what]
    if field == "width":
        ms.width[3] = value
    else:
        setattr(ms, field, value)
    assert lib.sprk_train_workspace_bytes(C.byref(ms), 40, 16, 8) == 0
    rc = lib.sprk_train_fit(C.byref(ms), None, None, None, None, 40, 16, 8, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None, None, 0, None)
    assert rc == L.EINVAL
    assert b"bad model (need 1..%d id columns, 1..%d hidden layers of 1..%d units, 1..%d input rows" % (T.MAX_COLS, T.MAX_LAYERS, T.MAX_WIDTH, T.MAX_X) in lib.sprk_last_error()


def test_families_of_the_two_models():
    ncf = T.family_of(M.NeuralCF(seed=1))
    assert ncf.xcol == [0] * 10 + [1] * 10 and ncf.xsub == list(range(10)) * 2 and ncf.n_dense == 0 and ncf.widths == [10, 10]
    model = M.EmbeddingMLP(seed=1)
    mlp = T.family_of(model)
    rows = model._deep_blocks_order()
    assert len(mlp.xcol) == 107 == model._deep_in() and sorted(T.param_names(mlp)) == sorted(model.weight_shapes())
    assert all(T.param_shapes(mlp)[k] == tuple(s) for k, s in model.weight_shapes().items())
    for j, k in enumerate(model.numeric_keys):
        assert mlp.xcol[rows[k]] == -1 and mlp.xsub[rows[k]] == j
    c = model.EMB_KEYS.index("movieId")
    assert [mlp.xcol[rows["movieId_embedding"] + d] for d in range(10)] == [c] * 10
    assert T.default_tile(ncf) == 16 and T.default_tile(mlp) == 8 and T.lds_bytes(mlp, 32) <= T.LDS_BYTES
