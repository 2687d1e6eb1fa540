"""The DIN trainer's definition (sparrowrecsys_amd/trainer_din.py, ``train_host``) against independent implementations; no GPU.
The measured figures are in docs/train_din_results.md."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_din as TD
from sparrowrecsys_amd.metrics import exact_roc_auc
from tests import train_din_cases as TDC
from tests.conftest import ROOT

F = np.float32
same = TDC.same_bits


# ---------------------------------------------------------------- forward

def test_forward_matches_the_float64_oracle(samples):
    """The definition's float32 forward against oracle.ctr_oracle.din_forward in float64 on the golden rows, random trained-like
    weights, the reference shape: within 1e-4 absolute, the existing trainers' bound."""
    from oracle import ctr_oracle as O
    model = M.DIN(seed=11)
    fam = TD.family_of(model)
    assert (len(fam.columns), fam.hist_len, fam.emb_dim, fam.att_hidden, fam.hidden, fam.n_dense, fam.fan0) == (9, 5, 10, 32, [128, 64], 7, 57)
    ids, dense = model._pack_python(samples)
    got = TD.forward_host(fam, model.weights, ids, dense)
    want = O.din_forward(samples, model.weights, dtype=np.float64).reshape(-1)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("din: max |p - oracle| = %.3e over %d rows" % (err, len(got)))
    assert got.dtype == F and len(got) == 256 and err <= 1e-4


# ---------------------------------------------------------------- gradients

GRAD_SHAPES = {"reference": TDC.REFERENCE_SHAPE, "odd": TDC.ODD_SHAPE}
GRAD_SEEDS = 5


@pytest.mark.parametrize("name", sorted(GRAD_SHAPES))
@pytest.mark.parametrize("tile", [7, 32])
def test_step_gradients_match_torch_autograd(name, tile):
    """One step's gradients against torch CPU autograd in float64 on the same graph, 200 rows, five fixed draws.  Per tensor: the
    definition's largest error relative to the tensor's largest magnitude is at most 4 x the same error of torch's own float32
    autograd (docs/train_results.md section 1 explains the bound).  A tensor of at most T H elements whose gradient is a cancelling sum
    over the samples may exceed the ratio and is then held to the sequential-sum bound (terms - 1) 2^-24 sum |term| instead, the terms
    from the float64 run; docs/train_din_results.md has the measured ratios and lists such tensors: ``head/bias`` at the odd shape (ratio
    18.14 at tile 7, 7.20 at tile 32; at most 0.005 of the bound).  The odd shape: T 3, D 3, H 5, tail (17, 1), a quarter of the genre ids -1, movie ids from a
    vocabulary of 7, so that candidates and slots collide."""
    import torch
    fam = TDC.family(**GRAD_SHAPES[name])
    mine, theirs, runs = {}, {}, []
    for seed in range(GRAD_SEEDS):
        w = TDC.weights(fam, 3 + seed)
        ids, dense, y = TDC.data(fam, 200, 5 + seed)
        if name == "odd":
            assert (ids[:, 1:4] == ids[:, :1]).any() and (ids[:, 4:] == -1).any() and (ids[:, 1:4] == 0).any()
        g, p = TD.step_gradients(fam, w, ids, dense, y, tile)
        g64, p64 = TDC.torch_gradients(fam, w, ids, dense, y, torch.float64)
        g32, _ = TDC.torch_gradients(fam, w, ids, dense, y, torch.float32)
        runs.append((w, ids, dense, y, g, g64))
        assert float(np.abs(p - p64).max()) <= 1e-6
        assert set(g) == set(TD.param_names(fam)) == set(w)
        for k in TD.param_names(fam):
            assert g[k].dtype == F and g[k].shape == w[k].shape
            big = float(np.abs(g64[k]).max())
            assert big > 0.0, k
            mine[k] = max(mine.get(k, 0.0), float(np.abs(g[k] - g64[k]).max()) / big)
            theirs[k] = max(theirs.get(k, 0.0), float(np.abs(g32[k] - g64[k]).max()) / big)
    for k in sorted(mine):
        print("%s tile %d %-18s definition %.3e torch float32 %.3e ratio %.2f" % (name, tile, k, mine[k], theirs[k], mine[k] / theirs[k]))
    for k in sorted(mine):
        if mine[k] <= 4.0 * theirs[k]:
            continue
        assert w[k].size <= fam.hist_len * fam.att_hidden, k                 # a small tensor whose gradient is a cancelling sum over the samples
        for w_, ids, dense, y, g, g64 in runs:
            terms = TDC.torch_sample_terms(fam, w_, ids, dense, y, k)
            bound = (len(y) - 1) * 2.0 ** -24 * np.abs(terms).sum(axis=0)
            worst = float((np.abs(g[k] - g64[k]) / bound).max())
            print("%s tile %d %-18s cancelling sum: |g| / sum |term| = %.2e, error / sequential-sum bound = %.3f" % (
                name, tile, k, float((np.abs(g64[k]) / np.abs(terms).sum(axis=0)).min()), worst))
            assert worst <= 1.0, k


# ---------------------------------------------------------------- Adam

def test_one_step_is_step_gradients_and_adam_step():
    fam, w, ids, dense, y = TDC.small(40, seed=1)
    got = TD.train_host(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    g, p = TD.step_gradients(fam, w, ids, dense, y, 8)
    assert got.step == 1 and same(got.p, p)
    for k in TD.param_names(fam):
        wk, m, v = w[k].copy(), np.zeros_like(w[k]), np.zeros_like(w[k])
        T.adam_step(wk, m, v, g[k], T.adam_alpha(0.001, 1))
        assert same(got.weights[k], wk) and same(got.m[k], m) and same(got.v[k], v), k
        assert not same(wk, w[k]), k


# ---------------------------------------------------------------- PReLU and the attention sigmoid

def test_prelu_at_exactly_zero_in_the_attention_and_in_the_tail():
    """A pre-activation of exactly 0 gives ``+0`` and sends nothing to ``z`` or ``alpha``: unit 0 of ``att0`` and of ``fc0`` with a
    zero kernel column and a zero bias."""
    fam, w, ids, dense, y = TDC.small(40, seed=6, hidden=(4, 3))
    for k in ("att0", "fc0"):
        w[k + "/kernel"][:, 0] = 0.0
        w[k + "/bias"][0] = 0.0
    keep = {}
    g, _ = TD.step_gradients(fam, w, ids, dense, y, 8, keep)
    plus0 = lambda a: not a.any() and not np.signbit(a).any()
    assert plus0(keep["u"][:, :, 0]) and plus0(keep["ya"][:, :, 0]) and plus0(keep["zs"][0][:, 0]) and plus0(keep["acts"][1][:, 0])
    for k in ("att0/kernel", "fc0/kernel"):
        assert plus0(g[k][:, 0]) and g[k][:, 1:].all()
    assert plus0(g["att0/bias"][:1]) and plus0(g["fc0/bias"][:1]) and plus0(g["att_prelu/alpha"][:, 0]) and plus0(g["fc0_prelu/alpha"][:1])
    assert plus0(g["att1/kernel"][0]) and g["att1/kernel"][1:].all() and plus0(g["fc1/kernel"][0]) and g["fc1/kernel"][1:].all()
    assert g["att_prelu/alpha"][:, 1:].all() and g["fc0_prelu/alpha"][1:].all()


def test_prelu_of_a_negative_pre_activation_with_alpha_zero_and_negative():
    """Units 1 and 2 of ``fc0`` and of ``att0`` pushed negative by their bias.  ``alpha = 0``: the output and the gradient to ``z`` are
    zero while ``alpha`` itself gets ``sum dy z``; ``alpha < 0``: the output is ``alpha z > 0`` and the unit's gradients are torch's
    float64 ones within 1e-3 of their largest: 40 rows in float32 leave four orders of room, and another rule for the sign would differ
    by the gradient's own size."""
    import torch
    fam, w, ids, dense, y = TDC.small(40, seed=7, hidden=(4, 3))
    for k, al in (("att0", "att_prelu/alpha"), ("fc0", "fc0_prelu/alpha")):
        w[k + "/bias"][1:3] = -50.0
        w[al][..., 1] = 0.0
        w[al][..., 2] = -0.25
    keep = {}
    g, _ = TD.step_gradients(fam, w, ids, dense, y, 8, keep)
    g64, _ = TDC.torch_gradients(fam, w, ids, dense, y, torch.float64)
    for z, a, name, al in ((keep["u"], keep["ya"], "att0", "att_prelu/alpha"), (keep["zs"][0], keep["acts"][1], "fc0", "fc0_prelu/alpha")):
        assert (z[..., 1:3] < 0).all() and not a[..., 1].any() and same(a[..., 2], (F(-0.25) * z[..., 2]).astype(F)) and (a[..., 2] > 0).all()
        assert not g[name + "/kernel"][:, 1].any() and not g[name + "/bias"][1] and g[al][..., 1].all()
        for k in (name + "/kernel", name + "/bias", al):                       # (a wrong rule is wrong by the size of the gradient itself)
            assert g[k][..., 2].all() and np.abs(g[k][..., 2] - g64[k][..., 2]).max() <= 1e-3 * np.abs(g64[k][..., 2]).max(), k


@pytest.mark.parametrize("bias,s", [(-100.0, 0.0), (100.0, 1.0)])
def test_a_saturated_attention_sigmoid(bias, s):
    """``s_t`` exactly 0 or exactly 1: ``(ds s)(1 - s)`` is zero and nothing reaches ``att*``.  Candidates are movies 0 .. 3 and the
    history movies 4 .. 6: with ``s_t = 1`` the pooled path alone trains the history's rows, with ``s_t = 0`` nothing does."""
    fam, w, ids, dense, y = TDC.small(40, seed=8)
    ids[:, 0] %= 4
    ids[:, 1:4] = 4 + ids[:, 1:4] % 3
    w["att1/bias"][0] = bias
    keep = {}
    g, _ = TD.step_gradients(fam, w, ids, dense, y, 8, keep)
    assert (keep["s"] == F(s)).all() and keep["ds"].all()
    for k in ("att0/kernel", "att0/bias", "att_prelu/alpha", "att1/kernel", "att1/bias"):
        assert not g[k].any(), k
    assert g["emb/movie"][:4].all() and (g["emb/movie"][4:].all() if s else not g["emb/movie"][4:].any())
    if s:
        assert same(keep["drow"][:, 1], keep["dpooled"]) and same(keep["pooled"], ((F(0) + keep["h"][:, 0]) + keep["h"][:, 1]) + keep["h"][:, 2])


# ---------------------------------------------------------------- table rows

def test_rows_a_batch_did_not_touch_and_history_id_zero():
    """After step 1 a movie row never hit holds its initial bits with zero moments; a row hit in step 1 only keeps moving, as under
    Keras' Adam; history id 0 gathers row 0 and trains it: no masking."""
    fam, w, ids, dense, y = TDC.small(24, seed=2)
    ids[:8, :4] = np.array([1, 0, 2, 0])                                # step 1: the candidate is movie 1, the history 0, 2, 0
    ids[8:, :4] = 3 + ids[8:, :4] % 3                                   # later steps: movies 3 .. 5; movie 6 never
    s1 = TD.train_host(fam, w, ids[:8], dense[:8], y[:8], batch_size=8, epochs=1)
    mv = "emb/movie"
    assert same(s1.weights[mv][3:], w[mv][3:]) and not s1.m[mv][3:].any() and not s1.v[mv][3:].any()
    assert all(not same(s1.weights[mv][r], w[mv][r]) for r in (0, 1, 2)) and s1.m[mv][0].all()
    s2 = TD.train_host(fam, w, ids[:16], dense[:16], y[:16], batch_size=8, epochs=1)
    s3 = TD.train_host(fam, w, ids, dense, y, batch_size=8, epochs=1)
    assert all(not same(s3.weights[mv][r], s2.weights[mv][r]) for r in (0, 1, 2))        # moved in step 3 without being hit
    assert same(s3.weights[mv][6], w[mv][6]) and not s3.v[mv][6].any()


def test_a_row_read_through_three_columns_of_one_sample():
    """``movieId == userRatedMovie1 == userRatedMovie3 == 5`` in sample 9 only: row 5's gradient is the stated three-entry sum of
    sample 9's tile, in column order from ``+0``, then the tiles from ``+0``."""
    fam, w, ids, dense, y = TDC.small(20, seed=3)
    ids[:, :4] %= 5
    ids[9, :4] = np.array([5, 5, 2, 5])
    keep = {}
    g, _ = TD.step_gradients(fam, w, ids, dense, y, 8, keep)
    d = keep["drow"][9]
    tile_sum = ((F(0) + d[0]) + d[1]) + d[3]
    assert same(g["emb/movie"][5], (F(0) + tile_sum).astype(F)) and g["emb/movie"][5].all()
    c, h, dA, s, dp = keep["c"][9], keep["h"][9], keep["dA"][9], keep["s"][9], keep["dpooled"][9]
    assert same(d[1], ((dp * s[0] + dA[0, 0]) + dA[0, 1]) + dA[0, 3] * c)
    x = keep["dx"][9][[k for k in range(fam.fan0) if fam.xsrc[k] == 0]]
    for t in range(3):
        x = ((x - dA[t, 0]) + dA[t, 2]) + dA[t, 3] * h[t]
    assert same(d[0], x)
    ids[10, :4] = np.array([5, 1, 5, 2])                               # the same tile: five entries, (sample, column) order
    g, _ = TD.step_gradients(fam, w, ids, dense, y, 8, keep)
    d9, d10 = keep["drow"][9], keep["drow"][10]
    assert same(g["emb/movie"][5], (F(0) + (((((F(0) + d9[0]) + d9[1]) + d9[3]) + d10[0]) + d10[2])).astype(F))


# ---------------------------------------------------------------- it learns

def test_it_learns():
    """Planted structure that needs the attention (tests/train_din_cases.py planted()): the label says whether the candidate's cluster
    is among the history's.  DIN at the reference widths, batch 256, 5 epochs, lr 0.01.  Every epoch's loss is below the one before,
    and the held-out rank AUC clears 0.6048: torch.optim.Adam(eps=1e-7) on the same graph and arrays over five seeds
    (scripts/train_din_torch_baseline.py) gave falling losses for all five and held-out AUCs 0.7741, 0.7019, 0.7440, 0.7990, 0.7870
    from 0.50 .. 0.52; the threshold is torch's lowest minus torch's own spread, 0.7019 - 0.0971."""
    (ids, dense, y), (tids, tdense, ty) = TDC.planted()
    model = TDC.planted_model(0)
    fam = TD.family_of(model)
    before = exact_roc_auc(ty, TD.forward_host(fam, model.weights, tids, tdense))
    got = TD.train_host(fam, model.weights, ids, dense, y, batch_size=256, epochs=5, learning_rate=0.01)
    losses = [h[0] for h in got.history]
    after = exact_roc_auc(ty, TD.forward_host(fam, got.weights, tids, tdense))
    print("losses %s; held-out AUC %.4f -> %.4f" % (" ".join("%.4f" % l for l in losses), before, after))
    assert got.step == 5 * 32 and len(losses) == 5
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert after >= 0.6048


# ---------------------------------------------------------------- rejections, limits, errors

def test_family_of_takes_din_itself_only():
    class Sub(M.DIN):
        pass
    for make in (lambda: Sub(seed=1), lambda: M.DIEN(seed=1), lambda: M.NeuralCF(seed=1), lambda: M.DeepFMv2(seed=1)):
        with pytest.raises(NotImplementedError, match="trainer_din trains DIN, not"):
            TD.family_of(make())
    with pytest.raises(NotImplementedError, match=r"NeuralCF\(arch=1\) and EmbeddingMLP, and DeepFMv2 through trainer_fm"):
        M.DIN(seed=1).fit({"label": np.zeros(1)})
    model = M.DIN(seed=1)
    fam = TD.family_of(model)
    assert [k for k, _, _ in fam.columns] == ["movieId"] + ["userRatedMovie%d" % t for t in range(1, 6)] + ["userId", "userGenre1", "movieGenre1"]
    assert fam.table_of == [0] * 6 + [1, 2, 3]
    assert TD.param_names(fam) == list(model.weight_shapes()) and all(TD.param_shapes(fam)[k] == tuple(s) for k, s in model.weight_shapes().items())
    assert TD.default_tile(fam) == TD.DEFAULT_TILE and TD.lds_bytes(fam, TD.default_tile(fam)) <= TD.LDS_BYTES
    rows, fan = model._fc_rows()
    assert fan == fam.fan0 and [fam.xsrc[rows["__pooled__"][0] + d] for d in range(10)] == [TD.SRC_POOLED] * 10
    assert [fam.xsrc[rows[k][0]] for k in model.numeric_keys] == [TD.SRC_NUMERIC] * 7 and [fam.xsub[rows[k][0]] for k in model.numeric_keys] == list(range(7))


@pytest.mark.parametrize("kw", [dict(hist_len=TD.MAX_HIST + 1), dict(emb_dim=TD.MAX_EMB + 1), dict(att_hidden=TD.MAX_WIDTH + 1), dict(hidden=(TD.MAX_WIDTH + 1,)),
                                dict(hidden=(2,) * (TD.MAX_LAYERS + 1))])
def test_limits_raise(kw):
    with pytest.raises(ValueError, match="trainer_din takes up to 16 id columns"):
        TDC.family(**kw)


def test_the_stated_maxima_are_inside_the_limits():
    for kw in (dict(hist_len=TD.MAX_HIST), dict(emb_dim=49), dict(att_hidden=TD.MAX_WIDTH), dict(hidden=(TD.MAX_WIDTH,) * TD.MAX_LAYERS)):
        assert TD.lds_bytes(TDC.family(**kw), 1) <= TD.LDS_BYTES
    with pytest.raises(ValueError, match="fc0 input rows"):
        TDC.family(emb_dim=50)                                          # DIN's fc0 has 5 x emb_dim + 7 input rows: 257


def test_family_checks_refuse_what_the_kernel_does_not_take():
    fam = TDC.family()
    with pytest.raises(ValueError, match="read table 0"):
        TD._check_family(fam._replace(table_of=[0, 0, 1, 0, 1, 2, 3]))
    with pytest.raises(ValueError, match="share its vocabulary"):
        TD._check_family(fam._replace(columns=fam.columns[:2] + [("x", "id", 8)] + fam.columns[3:]))
    with pytest.raises(ValueError, match="once each"):
        TD._check_family(fam._replace(xsrc=[TD.SRC_NUMERIC if s == TD.SRC_POOLED else s for s in fam.xsrc]))
    with pytest.raises(ValueError, match="history column"):
        TD._check_family(fam._replace(xsrc=fam.xsrc + [2], xsub=fam.xsub + [0]))


def test_errors_name_the_smallest_failing_row_and_change_nothing():
    fam, w, ids, dense, y = TDC.small(40, seed=0)
    keep = {k: v.copy() for k, v in w.items()}

    def raises(match, ids=ids, dense=dense, y=y):
        with pytest.raises(ValueError, match=match):
            TD.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1)
        assert all(same(w[k], keep[k]) for k in w)
    bad = ids.copy(); bad[30, 0] = 7; bad[12, 2] = -1; bad[20, 5] = -2
    raises("samples row 12: an id outside", ids=bad)
    bad = ids.copy(); bad[33, 3] = 7
    raises("samples row 33: an id outside", ids=bad)
    bad = dense.copy(); bad[9, 1] = np.inf; bad[3, 0] = np.nan
    raises("samples row 3: a numeric feature is not finite", dense=bad)
    bad = y.copy(); bad[7] = np.nan
    raises("samples row 7: the label is not finite", y=bad)
    with pytest.raises(ValueError, match="permutation"):
        TD.train_host(fam, w, ids, dense, y, order=np.zeros(40, dtype=np.int64))
    for kw in ({"batch_size": 0}, {"epochs": -1}, {"learning_rate": 0.0}, {"learning_rate": np.nan}, {"tile": 0}, {"batch_size": TD.MAX_BATCH + 1}):
        with pytest.raises(ValueError):
            TD.train_host(fam, w, ids, dense, y, **kw)
    with pytest.raises(ValueError, match=r"ids must be \[N, 7\]"):
        TD.train_host(fam, w, ids[:, :6], dense, y)
    with pytest.raises(ValueError, match="weight 'att_prelu/alpha' has shape"):
        TD.train_host(fam, dict(w, **{"att_prelu/alpha": w["att_prelu/alpha"][:2]}), ids, dense, y)


def test_batches_order_and_continuation():
    fam, w, ids, dense, y = TDC.small(40, seed=5)
    one = TD.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5)
    assert one.step == 6 and len(one.history) == 2 and one.p.shape == (40,)
    a = TD.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=5)
    b = TD.train_host(fam, a.weights, ids, dense, y, batch_size=16, epochs=1, tile=5, state=(a.m, a.v, a.step))
    assert b.step == 6 and all(same(b.weights[k], one.weights[k]) and same(b.m[k], one.m[k]) and same(b.v[k], one.v[k]) for k in w)
    order = np.random.default_rng(3).permutation(40)
    c = TD.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5, order=order)
    d = TD.train_host(fam, w, ids[order], dense[order], y[order], batch_size=16, epochs=2, tile=5)
    assert all(same(c.weights[k], d.weights[k]) for k in w) and same(c.p, d.p) and c.history == d.history
    other = TD.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert not same(other.weights["fc0/kernel"], one.weights["fc0/kernel"])        # the tile is part of the definition


def test_fit_without_a_device_points_to_the_host_definition(samples):
    import torch
    model = M.DIN(seed=1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device.*trainer_din.train_host"):
            TD.fit(model, samples)
        with pytest.raises(RuntimeError, match="no HIP device.*train_host"):
            TD.train_device(TD.family_of(model), model.weights, np.zeros((1, 9), np.int32), np.zeros((1, 7), F), np.zeros(1, F))
    with pytest.raises(NotImplementedError, match="trainer_din trains DIN"):
        TD.fit(M.DIEN(seed=1), samples)


# ---------------------------------------------------------------- the C side, without a device

def test_lds_bytes_is_what_the_library_reports(lib):
    """``sprk_train_din_fit`` checks its arguments before any device call: a tile beyond the LDS is refused with the bytes it would take,
    and ``sprk_train_din_workspace_bytes`` is 0 from the first tile that does not fit."""
    for kw in (TDC.REFERENCE_SHAPE, TDC.ODD_SHAPE, dict(hidden=(64, 65)), dict(hidden=(7, 200, 3), att_hidden=2), dict(hist_len=12, emb_dim=10, att_hidden=64),
               dict(hist_len=1, att_hidden=1, hidden=(1,))):
        fam = TDC.family(**kw)
        ms = TD._model_struct(fam)
        once = TD.lds_bytes(fam, 0)
        fits = (TD.LDS_BYTES - once) // (TD.lds_bytes(fam, 1) - once)
        assert TD.lds_bytes(fam, fits) <= TD.LDS_BYTES < TD.lds_bytes(fam, fits + 1)
        assert lib.sprk_train_din_workspace_bytes(C.byref(ms), 100, 50, fits) > 0 and lib.sprk_train_din_workspace_bytes(C.byref(ms), 100, 50, fits + 1) == 0
        rc = lib.sprk_train_din_fit(C.byref(ms), None, None, None, None, 100, 50, fits + 3, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None, None, 0, None)
        assert rc == L.EINVAL
        told = re.search(rb"tile = (\d+) needs (\d+) bytes of LDS", lib.sprk_last_error())
        assert told and int(told.group(1)) == fits + 3 and int(told.group(2)) == TD.lds_bytes(fam, fits + 3)


def test_the_library_refuses_what_the_family_check_refuses(lib):
    fam = TDC.family()
    fit = lambda ms, batch=16: lib.sprk_train_din_fit(C.byref(ms), None, None, None, None, 40, batch, 8, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None, None, 0, None)

    def bad(change):
        ms = TD._model_struct(fam)
        assert lib.sprk_train_din_workspace_bytes(C.byref(ms), 40, 16, 8) > 0
        change(ms)
        assert lib.sprk_train_din_workspace_bytes(C.byref(ms), 40, 16, 8) == 0 and fit(ms) == L.EINVAL
        assert b"train_din_fit: bad model (need hist_len 1..%d, hist_len + 1 .. %d id columns" % (TD.MAX_HIST, TD.MAX_COLS) in lib.sprk_last_error()
    bad(lambda ms: setattr(ms, "hist_len", TD.MAX_HIST + 1))
    bad(lambda ms: setattr(ms, "n_cols", TD.MAX_COLS + 1))
    bad(lambda ms: setattr(ms, "emb_dim", TD.MAX_EMB + 1))
    bad(lambda ms: setattr(ms, "att_hidden", TD.MAX_WIDTH + 1))
    bad(lambda ms: setattr(ms, "n_layers", TD.MAX_LAYERS + 1))
    bad(lambda ms: setattr(ms, "n_x", TD.MAX_X + 1))
    bad(lambda ms: ms.width.__setitem__(0, TD.MAX_WIDTH + 1))
    bad(lambda ms: ms.table.__setitem__(2, 1))                           # a history slot that reads another table
    bad(lambda ms: ms.table.__setitem__(6, 4))                           # a gap in the tables
    bad(lambda ms: ms.vocab.__setitem__(1, 8))                           # two columns of one table that disagree
    bad(lambda ms: ms.xsrc.__setitem__(0, 2))                            # an input row from a history column
    bad(lambda ms: ms.xsub.__setitem__(list(ms.xsrc).index(TD.SRC_POOLED), 1))       # a pooled element twice, another missing
    ms = TD._model_struct(fam)
    assert lib.sprk_train_din_workspace_bytes(C.byref(ms), 40, TD.MAX_BATCH, 8) > 0 and lib.sprk_train_din_workspace_bytes(C.byref(ms), 40, TD.MAX_BATCH + 1, 8) == 0
    assert fit(ms, TD.MAX_BATCH + 1) == L.EINVAL and b"a batch has up to 2^28 rows" in lib.sprk_last_error()


def test_header_exports_and_prototypes_agree(lib):
    import subprocess
    header = open(os.path.join(ROOT, "include", "sparrow_hip.h")).read()
    names = ["sprk_train_din_workspace_bytes", "sprk_train_din_fit"]
    declared = set(re.findall(r"\b(sprk_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in names:
        assert name in declared and name in L.EXPORTED_SYMBOLS and name in exported and hasattr(lib, name)
    assert re.search(r"\}\s*sprk_train_din_model;", header)
    consts = dict(re.findall(r"#define\s+(SPRK_TRAIN_DIN_[A-Z_]+)\s+(\d+)", header))
    assert {k: int(v) for k, v in consts.items()} == {"SPRK_TRAIN_DIN_MAX_COLS": L.TRAIN_DIN_MAX_COLS, "SPRK_TRAIN_DIN_MAX_LAYERS": L.TRAIN_DIN_MAX_LAYERS,
                                                      "SPRK_TRAIN_DIN_MAX_X": L.TRAIN_DIN_MAX_X, "SPRK_TRAIN_DIN_MAX_WIDTH": L.TRAIN_DIN_MAX_WIDTH,
                                                      "SPRK_TRAIN_DIN_MAX_EMB": L.TRAIN_DIN_MAX_EMB}
    assert (TD.MAX_COLS, TD.MAX_LAYERS, TD.MAX_X, TD.MAX_WIDTH, TD.MAX_EMB) == (L.TRAIN_DIN_MAX_COLS, L.TRAIN_DIN_MAX_LAYERS, L.TRAIN_DIN_MAX_X, L.TRAIN_DIN_MAX_WIDTH,
                                                                                L.TRAIN_DIN_MAX_EMB)
    assert C.sizeof(L.TrainDinModel) == 4 * (7 + 3 * L.TRAIN_DIN_MAX_COLS + L.TRAIN_DIN_MAX_LAYERS + 2 * L.TRAIN_DIN_MAX_X)        # all int32: no padding
    assert lib.sprk_train_din_fit.argtypes[1:] == lib.sprk_train_fit.argtypes[1:] and lib.sprk_train_din_fit.restype == C.c_int
    assert lib.sprk_train_din_workspace_bytes.restype == C.c_size_t
    proto = lambda name: re.sub(r"\s+", " ", re.search(name + r"\(const sprk_train\w*_model\* model,(.*?)\);", header, re.S).group(1))
    assert proto("sprk_train_din_fit") == proto("sprk_train_fit") and proto("sprk_train_din_workspace_bytes") == proto("sprk_train_workspace_bytes")
