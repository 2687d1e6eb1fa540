"""``trainer_tower``: the two-tower NeuralCF trainer's definition (``train_host``), its tower vectors (``tower_rows_host``, ``towers_host``) and the C
side's argument checks, without a GPU: the family, the forward against the float64 oracle, one step's gradients against a float64 restatement
and torch autograd, the arithmetic's order and edge values, that it learns what only the dot can carry, and the contract of errors, batches,
``order`` and ``state``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import als as A
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_tower as TT
from tests import train_tower_cases as TWC

F = np.float32
same = TWC.same_bits
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the family

def test_family_of_the_reference_model():
    model = M.NeuralCF(seed=1, arch=2)
    fam = TT.family_of(model)
    assert fam.columns == [("movieId", "id", model.movie_buckets), ("userId", "id", model.user_buckets)] and (fam.emb_dim, fam.hidden) == (10, [10, 10])
    names, shapes = TT.param_names(fam), TT.param_shapes(fam)
    assert names == ["emb/movieId", "emb/userId", "item0/kernel", "item0/bias", "item1/kernel", "item1/bias", "user0/kernel", "user0/bias", "user1/kernel",
                     "user1/bias", "head/kernel", "head/bias"] == list(model.weight_shapes())
    assert shapes == {k: tuple(s) for k, s in model.weight_shapes().items()}
    assert TT.default_tile(fam) == TT.DEFAULT_TILE and TT.lds_bytes(fam, 8) == 4 * (160 + 4 * 80 + 2 * 8 + 2 * 160)
    assert TT.lds_bytes(TWC.family(emb_dim=1, hidden=(1,)), 1) == 4 * (4 + 2 * 4 + 2 * 4 + 2 * 4)      # every part a multiple of 16 bytes
    assert TT.family_from_weights(model.weights) == fam


@pytest.mark.parametrize("kw", [dict(), dict(emb_dim=16, hidden=(7,)), dict(emb_dim=3, hidden=(4, 5, 6), movie_buckets=9, user_buckets=11)])
def test_param_shapes_are_weight_shapes(kw):
    model = M.NeuralCF(seed=1, arch=2, **kw)
    fam = TT.family_of(model)
    assert TT.param_shapes(fam) == {k: tuple(s) for k, s in model.weight_shapes().items()} and sorted(TT.param_names(fam)) == sorted(model.weight_shapes())
    assert TT.n_params(fam) == sum(int(np.prod(s)) for s in model.weight_shapes().values())


def test_family_of_takes_the_two_tower_neuralcf_only(samples):
    class Sub(M.NeuralCF):
        pass
    with pytest.raises(NotImplementedError, match=r"trainer_tower trains NeuralCF\(arch=2\), not NeuralCF\(arch=1\)"):
        TT.family_of(M.NeuralCF(seed=1))
    with pytest.raises(NotImplementedError, match="not Sub"):
        TT.family_of(Sub(seed=1, arch=2))
    with pytest.raises(NotImplementedError, match="not DeepFM"):
        TT.fit(M.DeepFM(seed=1), samples)
    with pytest.raises(NotImplementedError, match=r"NeuralCF\(arch=1\) and EmbeddingMLP, and DeepFMv2 through trainer_fm, not for NeuralCF\(arch=2\)"):
        M.NeuralCF(seed=1, arch=2).fit({"label": np.zeros(1)})


def test_one_over_each_limit_raises_in_words():
    words = "trainer_tower takes 1 to 8 hidden layers of up to 256 units per tower, 2 x emb_dim up to 256"
    assert (TT.MAX_LAYERS, TT.MAX_WIDTH, TT.MAX_DIM) == (T.MAX_LAYERS, T.MAX_WIDTH, T.MAX_X // 2) == (8, 256, 128)
    for kw in (dict(emb_dim=TT.MAX_DIM + 1), dict(emb_dim=0), dict(hidden=(TT.MAX_WIDTH + 1,)), dict(hidden=(2,) * (TT.MAX_LAYERS + 1)), dict(hidden=()),
               dict(hidden=(3, 0)), dict(movies=0), dict(users=0)):
        with pytest.raises(ValueError, match=words):
            TWC.family(**kw)
    fam = TWC.family(emb_dim=TT.MAX_DIM, hidden=(TT.MAX_WIDTH,) * TT.MAX_LAYERS)
    assert fam.emb_dim == 128 and len(fam.hidden) == 8
    with pytest.raises(ValueError, match="the schedule's key holds fewer than 2\\^31 - 1 rows"):
        TWC.family(movies=TT.MAX_ROWS - 5, users=5)
    with pytest.raises(ValueError, match="movieId and userId, in this order"):
        TT._check_family(fam._replace(columns=fam.columns[::-1]))


# ---------------------------------------------------------------- forward

def test_forward_matches_the_float64_oracle(samples):
    """The definition's float32 forward against oracle.ctr_oracle.neural_cf2_forward in float64 on the golden rows, random trained-like weights,
    within 1e-4 absolute: the bound tests/test_train_pair.py holds the same comparison to."""
    from oracle import ctr_oracle as O
    model = M.NeuralCF(seed=11, arch=2)
    fam = TT.family_of(model)
    ids, dense = model._pack_python(samples)
    got = TT.forward_host(fam, model.weights, ids, dense)
    want = O.neural_cf2_forward(samples, model.weights, dtype=np.float64).reshape(-1)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("two-tower NeuralCF: max |p - oracle| = %.3e over %d rows" % (err, len(got)))
    assert got.dtype == F and len(got) == 256 and err <= 1e-4 and float(want.max() - want.min()) > 1e-3


# ---------------------------------------------------------------- gradients

@pytest.mark.parametrize("tile", [1, 8, 200])
def test_step_gradients_match_float64_and_torch_autograd(tile):
    """One step's gradients against a float64 restatement in plain numpy (which must agree with torch CPU autograd in float64 to 1e-12) on 200
    rows (tile 200 = n), five fixed draws, every parameter.  tests/test_train_pair.py's bounds for the same comparisons, unchanged: ``p`` within
    1e-6 of the float64 run; per tensor, the definition's largest error relative to the tensor's largest magnitude is at most 4 x the same error
    of torch's own float32 autograd; a small tensor whose gradient is a cancelling sum over the samples may exceed the ratio and is then held to
    the sequential-sum bound (terms - 1) 2^-24 sum |term|, the terms from the float64 run."""
    import torch
    fam = TWC.family()
    mine, theirs, runs = {}, {}, []
    for seed in range(5):
        w = TWC.weights(fam, 3 + seed)
        ids, dense, y = TWC.data(fam, 200, 5 + seed)
        g, p = TT.step_gradients(fam, w, ids, dense, y, tile)
        g64, p64 = TWC.torch_gradients(fam, w, ids, y, torch.float64)
        gnp, pnp = TWC.float64_gradients(fam, w, ids, y)
        g32, _ = TWC.torch_gradients(fam, w, ids, y, torch.float32)
        runs.append((w, ids, y, g, g64))
        assert float(np.abs(p - p64).max()) <= 1e-6 and float(np.abs(pnp - p64).max()) <= 1e-12
        assert set(g) == set(TT.param_names(fam)) == set(w) == set(gnp)
        for k in TT.param_names(fam):
            assert g[k].dtype == F and g[k].shape == w[k].shape
            big = float(np.abs(g64[k]).max())
            assert big > 0.0, k
            assert float(np.abs(gnp[k].reshape(g64[k].shape) - g64[k]).max()) <= 1e-12 * max(big, 1.0), k
            mine[k] = max(mine.get(k, 0.0), float(np.abs(g[k] - g64[k]).max()) / big)
            theirs[k] = max(theirs.get(k, 0.0), float(np.abs(g32[k] - g64[k]).max()) / big)
    for k in sorted(mine):
        print("tile %d %-14s definition %.3e torch float32 %.3e ratio %.2f" % (tile, k, mine[k], theirs[k], mine[k] / max(theirs[k], 1e-300)))
    for k in sorted(mine):
        if mine[k] <= 4.0 * theirs[k]:
            continue
        assert w[k].size <= 64, k                                          # a small tensor whose gradient is a cancelling sum over the samples
        for w_, ids, y, g, g64 in runs:
            terms = TWC.torch_sample_terms(fam, w_, ids, y, k)
            bound = (len(y) - 1) * 2.0 ** -24 * np.abs(terms).sum(axis=0)
            worst = float((np.abs(g[k] - g64[k]) / np.maximum(bound, 1e-300)).max())
            print("tile %d %-14s cancelling sum: error / sequential-sum bound = %.3f" % (tile, k, worst))
            assert worst <= 1.0, k


# ---------------------------------------------------------------- arithmetic

def test_the_kept_dot_is_the_als_dot_of_the_tower_rows():
    """The forward's dot of a pair = ``als.predict_host`` on ``tower_rows_host``'s vectors, bit for bit: the score the top-K sorts by."""
    fam, w, ids, dense, y = TWC.small(60, seed=3, emb_dim=5, hidden=(9, 7))
    keep = {}
    p = TT.forward_host(fam, w, ids, dense, keep)
    itf, uf = TT.tower_rows_host(fam, w, "item"), TT.tower_rows_host(fam, w, "user")
    assert itf.shape == (7, 7) and uf.shape == (5, 7) and itf.dtype == F and (itf > 0).any() and (itf == 0).any()
    assert same(keep["item"][-1], itf[ids[:, 0]]) and same(keep["user"][-1], uf[ids[:, 1]])
    ones = lambda n: np.ones(n, dtype=np.uint8)
    got = A.predict_host(ids[:, 1], ids[:, 0], uf, ones(5), itf, ones(7))
    assert same(got, keep["dot"]) and keep["dot"].any()
    assert same(p, T.sigmoid_def(T._dense(keep["dot"][:, None], w["head/kernel"], w["head/bias"])[:, 0]))
    wide = float(np.abs(keep["dot"].astype(np.float64) - (itf[ids[:, 0]].astype(np.float64) * uf[ids[:, 1]]).sum(axis=1)).max())
    assert wide < 1e-5


def test_each_tower_receives_the_other_towers_output():
    """One sample, one layer per tower: the item tower's kernel gradient is ``x_movie^T (mask_item (ddot user_out))`` in the definition's order."""
    for seed in range(10):                                                  # the first seed whose sample has live units in both towers
        fam, w, ids, dense, y = TWC.small(1, seed=seed, hidden=(4,))
        live = {}
        TT.forward_host(fam, w, ids, dense, live)
        if (live["item"][-1] > 0).any() and (live["user"][-1] > 0).any():
            break
    keep = {}
    g, p = TT.step_gradients(fam, w, ids, dense, y, 8)
    TT.forward_host(fam, w, ids, dense, keep)
    dl = ((p - y) / F(1)).astype(F)[0]
    ddot = (F(0) + w["head/kernel"][0, 0] * dl).astype(F)
    it, us = keep["item"][-1][0], keep["user"][-1][0]
    assert (it > 0).any() and (us > 0).any()
    for side, own, other, col in (("item", it, us, 0), ("user", us, it, 1)):
        dz = np.where(own > 0, ddot * other, F(0)).astype(F)
        x = w["emb/" + fam.columns[col][0]][ids[0, col]]
        assert same(g[side + "0/kernel"], ((np.zeros((3, 4), dtype=F) + x[:, None] * dz[None, :]) + np.zeros((3, 4), dtype=F)).astype(F))
        assert same(g[side + "0/bias"], (np.zeros(4, dtype=F) + dz).astype(F))
    assert same(g["head/kernel"][0, 0], (F(0) + keep["dot"][0] * dl).astype(F))


def test_gradients_are_summed_tile_by_tile():
    """Every sample carries the same pair: the head's kernel gradient is the explicit two-level float32 sum -- a tile's samples from +0, then the
    tiles from +0 -- and differs in bits from the flat sum (checked here, not assumed); a table row's likewise."""
    fam, w, ids, dense, y = TWC.small(50, seed=0)
    ids[:] = 1
    tile = 8
    g, p = TT.step_gradients(fam, w, ids, dense, y, tile)
    dl = ((p - y) / F(50)).astype(F)

    def sums(terms):
        two = np.zeros(terms.shape[1:], dtype=F)
        for t0 in range(0, 50, tile):
            s = np.zeros(terms.shape[1:], dtype=F)
            for i in range(t0, min(50, t0 + tile)):
                s = s + terms[i]
            two = two + s
        flat = np.zeros(terms.shape[1:], dtype=F)
        for i in range(50):
            flat = flat + terms[i]
        return two, flat
    two, flat = sums(dl)
    assert same(g["head/bias"][0], two) and not same(two, flat)
    whole, _ = TT.step_gradients(fam, w, ids, dense, y, 50)
    assert same(whole["head/bias"][0], flat)
    assert not g["emb/movieId"][[0, 2, 3, 4, 5, 6]].any() and g["emb/movieId"][1].any() and g["emb/userId"][1].any()
    other = TT.train_host(fam, w, ids, dense, y, batch_size=50, epochs=1, tile=5)
    one = TT.train_host(fam, w, ids, dense, y, batch_size=50, epochs=1, tile=8)
    again = TT.train_host(fam, w, ids, dense, y, batch_size=50, epochs=1, tile=8)
    assert not same(other.m["head/bias"], one.m["head/bias"])               # the tile is part of the definition
    assert all(same(one.weights[k], again.weights[k]) and same(one.m[k], again.m[k]) for k in w) and same(one.p, again.p)


def test_one_step_is_step_gradients_and_adam_step():
    fam, w, ids, dense, y = TWC.small(40, seed=1)
    got = TT.train_host(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    g, p = TT.step_gradients(fam, w, ids, dense, y, 8)
    assert got.step == 1 and same(got.p, p)
    for k in TT.param_names(fam):
        wk, m, v = w[k].copy(), np.zeros_like(w[k]), np.zeros_like(w[k])
        T.adam_step(wk, m, v, g[k], T.adam_alpha(0.001, 1))
        assert same(got.weights[k], wk) and same(got.m[k], m) and same(got.v[k], v), k
        assert not same(wk, w[k]), k


# ---------------------------------------------------------------- edge values

def dead(w, side, L):
    """The side's last layer with every pre-activation <= 0: a zero kernel under a bias of -1 and 0."""
    w = {k: v.copy() for k, v in w.items()}
    w["%s%d/kernel" % (side, L - 1)][:] = 0
    w["%s%d/bias" % (side, L - 1)][:] = np.where(np.arange(len(w["%s%d/bias" % (side, L - 1)])) % 2, F(-1), F(0))
    return w


@pytest.mark.parametrize("side", ["item", "user"])
def test_a_dead_tower(side):
    """Every last-layer pre-activation of one tower <= 0 (half of them exactly 0): its output is +0, the dot is +0, and every gradient of BOTH
    towers and both tables is exactly zero -- the dead tower's by its mask, the other's because it receives ``ddot * 0`` -- while ``head/bias``
    moves."""
    fam, w, ids, dense, y = TWC.small(40, seed=4)
    w = dead(w, side, 2)
    g, p = TT.step_gradients(fam, w, ids, dense, y, 8)
    assert same(p, np.full(40, T.sigmoid_def(w["head/bias"])[0], dtype=F))
    for k in TT.param_names(fam):
        if k != "head/bias":
            assert not g[k].any(), k
    assert g["head/bias"].any()
    got = TT.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert all(same(got.weights[k], w[k]) for k in w if k != "head/bias") and not same(got.weights["head/bias"], w["head/bias"])


def test_a_relu_at_exactly_zero():
    """A unit whose pre-activation is exactly 0 is off: ``z > 0`` is false, its output is +0 and nothing flows back through it."""
    fam, w, ids, dense, y = TWC.small(20, seed=5, hidden=(4,))
    w["item0/kernel"][:, 1] = 0
    w["item0/bias"][1] = 0
    w["user0/bias"][:] = F(0.5)
    w["user0/kernel"][:] = np.abs(w["user0/kernel"])
    w["emb/userId"][:] = np.abs(w["emb/userId"])
    g, p = TT.step_gradients(fam, w, ids, dense, y, 8)
    assert not g["item0/kernel"][:, 1].any() and g["item0/bias"][1] == 0 and g["item0/kernel"][:, [0, 2, 3]].any()
    assert not g["user0/kernel"][:, 1].any() and g["user0/bias"][1] == 0     # the user tower's unit 1 receives ddot * (+0)


@pytest.mark.parametrize("bias", [100.0, -100.0])
def test_a_saturated_head(bias):
    fam, w, ids, dense, y = TWC.small(40, seed=7)
    w["head/bias"][0] = bias
    got = TT.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert set(np.unique(got.p).tolist()) == ({1.0} if bias > 0 else {0.0}) and set(y.tolist()) == {0.0, 1.0}
    assert all(np.isfinite(a).all() for a in got.weights.values())


def overflowing(n=16):
    """Towers that pass rows of 1e20 on (identity kernels, zero biases): every dot is +inf, p is exactly 1, and a sample of label 1 has
    ``dlogit = 0``, so the head's kernel gradient adds ``inf * 0``."""
    fam, w, ids, dense, y = TWC.small(n, seed=6, emb_dim=4, hidden=(4,))
    for side in ("item", "user"):
        w[side + "0/kernel"][:] = np.eye(4, dtype=F)
        w[side + "0/bias"][:] = 0
    w["emb/movieId"][:] = F(1e20)
    w["emb/userId"][:] = F(1e20)
    w["head/kernel"][:] = F(1.0)
    return fam, w, ids, dense, y


def test_an_overflowing_dot_is_stored_as_the_quiet_nan():
    fam, w, ids, dense, y = overflowing()
    assert all(np.isfinite(a).all() for a in w.values()) and set(y.tolist()) == {0.0, 1.0} and TT.QNAN.view(np.uint32) == 0x7fc00000
    keep = {}
    p = TT.forward_host(fam, w, ids, dense, keep)
    assert np.isposinf(keep["dot"]).all() and (p == 1).all()
    g, _ = TT.step_gradients(fam, w, ids, dense, y, 8)
    assert np.isnan(g["head/kernel"]).all()                                 # inf * 0
    got = TT.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert (got.p.view(np.uint32) == 0x7fc00000).all()
    seen = 0
    for d in (got.weights, got.m, got.v):
        for a in d.values():
            seen += int(np.isnan(a).sum())
            assert (a.view(np.uint32)[np.isnan(a)] == 0x7fc00000).all()
    assert seen > 0 and np.isnan(got.weights["head/kernel"]).all() and np.isnan(got.weights["emb/movieId"]).any()


# ---------------------------------------------------------------- it learns

def test_it_learns_what_only_the_dot_carries():
    """``label = (movie's group == user's group)`` over 12 x 12 ids in 3 groups (tests/train_tower_cases.py learning()): neither tower sees the
    other side's id, so only the dot of the two outputs can carry the label.  384 rows, ``emb_dim`` 8, one layer of 16 per tower, batch 64, 80 epochs, lr 0.02.  The last epoch's AUC is
    above the first's, and the training AUC (exact, of all rows under the final weights) is at least what ``torch.optim.Adam(eps=1e-7)`` on the
    same graph, arrays and batches reaches in this test over five initialisation seeds: their worst minus their spread, the margin
    tests/test_train_pair.py's twin uses.  The definition runs at the five seeds too and is held to the threshold at each."""
    twins, mine = [], []
    for seed in range(5):
        fam, w, ids, dense, y = TWC.learning(seed=seed)
        assert 0.25 < y.mean() < 0.45
        got = TT.train_host(fam, w, ids, dense, y, batch_size=64, epochs=80, learning_rate=0.02)
        assert got.history[-1][2] > got.history[0][2], (seed, got.history[0], got.history[-1])
        mine.append(TWC.auc(y, TT.forward_host(fam, got.weights, ids, dense)))
        twins.append(TWC.torch_adam_fit(fam, w, ids, y, 64, 80, 0.02))
    threshold = min(twins) - (max(twins) - min(twins))
    print("training AUC: definition %s, torch twin %s -> threshold %.4f" % (["%.4f" % a for a in mine], ["%.4f" % a for a in twins], threshold))
    assert threshold > 0.6 and min(mine) >= threshold                      # (a coin gives 0.5)


# ---------------------------------------------------------------- errors, order, continuation

def test_errors_name_the_smallest_failing_row_and_change_nothing():
    fam, w, ids, dense, y = TWC.small(40, seed=0)
    keep = {k: v.copy() for k, v in w.items()}

    def raises(match, ids=ids, y=y):
        with pytest.raises(ValueError, match=match):
            TT.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1)
        assert all(same(w[k], keep[k]) for k in w)
    bad = ids.copy(); bad[30, 0] = 7; bad[12, 1] = -1
    raises("samples row 12: an id outside", ids=bad)
    bad = ids.copy(); bad[35, 1] = 5                                        # == the user vocabulary
    raises("samples row 35: an id outside", ids=bad)
    bad = y.copy(); bad[7] = np.nan; bad[30] = np.inf
    raises("samples row 7: the label is not finite", y=bad)
    with pytest.raises(ValueError, match="permutation"):
        TT.train_host(fam, w, ids, dense, y, order=np.zeros(40, dtype=np.int64))
    for kw in ({"batch_size": 0}, {"epochs": -1}, {"learning_rate": 0.0}, {"learning_rate": np.nan}, {"tile": 0}):
        with pytest.raises(ValueError):
            TT.train_host(fam, w, ids, dense, y, **kw)
    with pytest.raises(ValueError, match=r"ids must be \[N, 2\]"):
        TT.train_host(fam, w, ids[:, :1], dense, y)
    with pytest.raises(ValueError, match="weight 'item1/kernel' has shape"):
        TT.train_host(fam, dict(w, **{"item1/kernel": w["item1/kernel"][:3]}), ids, dense, y)


def test_batches_order_and_continuation():
    fam, w, ids, dense, y = TWC.small(40, seed=5)
    one = TT.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5)
    assert one.step == 6 and len(one.history) == 2 and one.p.shape == (40,)
    a = TT.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=5)
    b = TT.train_host(fam, a.weights, ids, None, y, batch_size=16, epochs=1, tile=5, state=(a.m, a.v, a.step))
    assert b.step == 6 and all(same(b.weights[k], one.weights[k]) and same(b.m[k], one.m[k]) and same(b.v[k], one.v[k]) for k in w)
    order = np.random.default_rng(3).permutation(40)
    c = TT.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5, order=order)
    d = TT.train_host(fam, w, ids[order], dense, y[order], batch_size=16, epochs=2, tile=5)
    assert all(same(c.weights[k], d.weights[k]) for k in w) and same(c.p, d.p) and c.history == d.history
    assert not same(c.weights["head/kernel"], one.weights["head/kernel"])
    other = TT.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert not same(other.weights["item0/kernel"], one.weights["item0/kernel"])     # the tile is part of the definition
    none = TT.train_host(fam, w, ids, dense, y, epochs=0)
    assert none.step == 0 and none.history == [] and all(same(none.weights[k], w[k]) for k in w)


def test_fit_without_a_device_points_to_the_host_definition(samples):
    import torch
    model = M.NeuralCF(seed=1, arch=2)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device.*trainer_tower.train_host"):
            TT.fit(model, samples)
        with pytest.raises(RuntimeError, match="no HIP device.*train_host"):
            TT.train_device(TT.family_of(model), model.weights, np.zeros((1, 2), np.int32), None, np.zeros(1, F))
        with pytest.raises(RuntimeError, match="no HIP device.*tower_rows_host"):
            TT.tower_rows_device(TT.family_of(model), model.weights, "item")
        with pytest.raises(RuntimeError, match="no HIP device.*towers_host"):
            TT.towers(model)


# ---------------------------------------------------------------- towers

def test_towers_has_and_count_come_from_seen():
    fam, w, ids, dense, y = TWC.small(30, seed=8)                           # seed 8: a positive head
    ids[:, 0] = np.where(ids[:, 0] == 3, 2, ids[:, 0])                      # movie 3: never seen
    uf, itf, uh, ih, uc, ic, sign = TT.towers_host(fam, w, {"movieId": ids[:, 0], "userId": ids[:, 1]})
    assert sign == 1 and same(itf, TT.tower_rows_host(fam, w, "item")) and same(uf, TT.tower_rows_host(fam, w, "user"))
    assert ic.dtype == uc.dtype == np.int32 and ih.dtype == uh.dtype == np.uint8
    assert np.array_equal(ic, np.bincount(ids[:, 0], minlength=7)) and np.array_equal(uc, np.bincount(ids[:, 1], minlength=5))
    assert np.array_equal(ih, ic > 0) and ih[3] == 0 and ih.sum() == 6 and np.array_equal(uh, uc > 0)
    uf, itf, uh, ih, uc, ic, sign = TT.towers_host(fam, w)
    assert uh.all() and ih.all() and not uc.any() and not ic.any() and len(uh) == 5 and len(ih) == 7
    rows, scores = A.topk_host(uf, uh, itf, ih, 3)
    assert rows.shape == (5, 3) and same(scores[:, 0], A.predict_host(np.arange(5), rows[:, 0], uf, uh, itf, ih))
    with pytest.raises(ValueError, match="inside the vocabularies"):
        TT.towers_host(fam, w, {"movieId": np.array([7]), "userId": np.array([0])})
    with pytest.raises(KeyError, match="movieId"):
        TT.towers_host(fam, w, {"userId": np.array([0])})


def test_towers_sign_rule():
    """A negative head stores the user vectors negated -- exact, so every dot is the exact negation (a dot of +0 stays +0) and the largest dot is the best score --; a
    zero head raises; a last width of 17 is beyond ``sprk_als_topk`` and is refused in words."""
    fam, w, ids, dense, y = TWC.small(30, seed=9)                           # seed 9: a negative head
    assert w["head/kernel"][0, 0] < 0
    uf, itf, uh, ih, uc, ic, sign = TT.towers_host(fam, w)
    assert sign == -1 and same(uf, -TT.tower_rows_host(fam, w, "user")) and same(itf, TT.tower_rows_host(fam, w, "item"))
    keep = {}
    p = TT.forward_host(fam, w, ids, dense, keep)
    score = A.predict_host(ids[:, 1], ids[:, 0], uf, uh, itf, ih)
    nz = keep["dot"] != 0                                                   # (a dot of +0 stays +0: the sum starts at +0)
    assert np.array_equal(score, -keep["dot"]) and same(score[nz], -keep["dot"][nz]) and nz.any()
    order = np.argsort(score, kind="stable")
    assert (np.diff(p[order].astype(np.float64)) >= 0).all() and p.max() > p.min()      # p is a monotone function of the stored dot
    for zero in (0.0, -0.0):
        with pytest.raises(ValueError, match="every pair scores the same"):
            TT.towers_host(fam, dict(w, **{"head/kernel": np.array([[zero]], dtype=F)}))
    assert TT.head_sign(np.array([[1e-45]], dtype=F)) == 1 and TT.head_sign(np.array([[-1e-45]], dtype=F)) == -1
    wide = TWC.family(hidden=(5, 17))
    with pytest.raises(ValueError, match="hidden\\[-1\\] = 17: sprk_als_topk takes vectors of up to 16"):
        TT.towers_host(wide, TWC.weights(wide, 0))
    assert TT.tower_rows_host(wide, TWC.weights(wide, 0), "user").shape == (5, 17)
    ok = TWC.family(hidden=(17, 16))
    assert TT.towers_host(ok, TWC.weights(ok, 0))[0].shape == (5, 16)


# ---------------------------------------------------------------- the C side, without a device

def _fit_null(lib, ms, n=100, batch=50, tile=8):
    return lib.sprk_train_tower_fit(C.byref(ms) if ms is not None else None, None, None, None, n, batch, tile, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None,
                                    None, 0, None)


def test_lds_bytes_is_what_the_library_reports(lib):
    """``sprk_train_tower_fit`` checks its arguments before any device call: a tile beyond the LDS is refused with the bytes it would take, and
    ``sprk_train_tower_workspace_bytes`` is 0 from the first tile that does not fit."""
    for kw in (dict(), dict(emb_dim=10, hidden=(10, 10)), dict(emb_dim=1, hidden=(1,)), dict(emb_dim=17, hidden=(3, 256)), dict(emb_dim=128, hidden=(256,) * 8),
               dict(emb_dim=5, hidden=(7, 200, 3))):
        fam = TWC.family(**kw)
        ms = TT._model_struct(fam)
        fits = max(t for t in range(1, 5000) if TT.lds_bytes(fam, t) <= TT.LDS_BYTES)
        assert fits < 4999 and TT.lds_bytes(fam, fits + 1) > TT.LDS_BYTES and TT.lds_bytes(fam, fits) % 16 == 0
        assert lib.sprk_train_tower_workspace_bytes(C.byref(ms), 100, 50, fits) > 0 and lib.sprk_train_tower_workspace_bytes(C.byref(ms), 100, 50, fits + 1) == 0
        for tile in (fits + 1, fits + 3):
            assert _fit_null(lib, ms, tile=tile) == L.EINVAL
            told = re.search(rb"tile = (\d+) needs (\d+) bytes of LDS", lib.sprk_last_error())
            assert told and int(told.group(1)) == tile and int(told.group(2)) == TT.lds_bytes(fam, tile)
    assert TT.lds_bytes(TWC.family(emb_dim=128, hidden=(256,) * 8), 4) <= TT.LDS_BYTES      # every maximum at once fits a tile of 4


def test_the_library_refuses_what_the_family_check_refuses(lib):
    fam = TWC.family()

    def bad(change):
        ms = TT._model_struct(fam)
        assert lib.sprk_train_tower_workspace_bytes(C.byref(ms), 40, 16, 8) > 0
        change(ms)
        assert lib.sprk_train_tower_workspace_bytes(C.byref(ms), 40, 16, 8) == 0 and _fit_null(lib, ms, 40, 16) == L.EINVAL
        assert b"train_tower_fit: bad model (need emb_dim 1..128, 1..8 hidden layers of 1..256 units" in lib.sprk_last_error()
        z = (C.c_float * 4)()
        assert lib.sprk_tower_rows(C.byref(ms), z, 0, 8, z, 4, None) == L.EINVAL and b"tower_rows: bad model" in lib.sprk_last_error()
    bad(lambda ms: setattr(ms, "n_layers", TT.MAX_LAYERS + 1))
    bad(lambda ms: setattr(ms, "n_layers", 0))
    bad(lambda ms: setattr(ms, "emb_dim", TT.MAX_DIM + 1))
    bad(lambda ms: setattr(ms, "emb_dim", 0))
    bad(lambda ms: ms.width.__setitem__(1, TT.MAX_WIDTH + 1))
    bad(lambda ms: ms.width.__setitem__(0, 0))
    bad(lambda ms: ms.vocab.__setitem__(0, 0))
    bad(lambda ms: (ms.vocab.__setitem__(0, 2 ** 30), ms.vocab.__setitem__(1, 2 ** 30)))
    assert _fit_null(lib, None) == L.EINVAL
    ms = TT._model_struct(fam)
    for kw, words in ((dict(n=-1), b"n = -1"), (dict(batch=0), b"batch = 0"), (dict(tile=0), b"tile = 0"), (dict(n=2 ** 30), b"fewer than 2^31 - 1 entries")):
        assert _fit_null(lib, ms, **kw) == L.EINVAL and words in lib.sprk_last_error()
    assert _fit_null(lib, ms) == L.EINVAL and b"NULL error word" in lib.sprk_last_error()
    z = (C.c_float * 64)()
    for args, words in (((z, 2, 8, z, 4), b"side = 2"), ((z, 0, 0, z, 4), b"tile = 0"), ((z, 0, 8, z, 3), b"out_stride = 3 below the last width 4"),
                        ((None, 0, 8, z, 4), b"NULL parameters or out"), ((z, 1, 8, None, 4), b"NULL parameters or out"),
                        ((z, 0, 1 << 20, z, 4), b"bytes of LDS")):
        assert lib.sprk_tower_rows(C.byref(ms), *args, None) == L.EINVAL and words in lib.sprk_last_error(), words


def test_header_exports_and_ctypes_agree(lib):
    header = open(os.path.join(ROOT, "include", "sparrow_hip.h")).read()
    for name in ("sprk_train_tower_workspace_bytes", "sprk_train_tower_fit", "sprk_tower_rows"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\(" % name, header)
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(SPRK_TRAIN_TOWER_[A-Z_]+)\s+(\d+)", header)}
    assert consts == {"SPRK_TRAIN_TOWER_MAX_LAYERS": L.TRAIN_TOWER_MAX_LAYERS, "SPRK_TRAIN_TOWER_MAX_WIDTH": L.TRAIN_TOWER_MAX_WIDTH, "SPRK_TRAIN_TOWER_MAX_DIM": L.TRAIN_TOWER_MAX_DIM}
    assert (TT.MAX_LAYERS, TT.MAX_WIDTH, TT.MAX_DIM) == (L.TRAIN_TOWER_MAX_LAYERS, L.TRAIN_TOWER_MAX_WIDTH, L.TRAIN_TOWER_MAX_DIM)
    body = re.sub(r"\s+", " ", re.search(r"typedef struct \{([^}]*)\}\s*sprk_train_tower_model;", header).group(1))
    fields = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.replace("int32_t", "").strip())]
    assert fields == [f[0] for f in L.TrainTowerModel._fields_] and C.sizeof(L.TrainTowerModel) == 4 * (2 + 2 + 8)
    a = lib.sprk_train_fit.argtypes
    assert lib.sprk_train_tower_fit.argtypes[1:] == [a[1]] + a[3:] and lib.sprk_train_tower_fit.restype == C.c_int and lib.sprk_tower_rows.restype == C.c_int
    assert lib.sprk_train_tower_workspace_bytes.restype == C.c_size_t
    proto = lambda name: re.sub(r"\s+", " ", re.search(name + r"\(const sprk_train\w*_model\* model,(.*?)\);", header, re.S).group(1))
    assert proto("sprk_train_tower_fit") == proto("sprk_train_fit").replace(" const float* dense,", "") != proto("sprk_train_fit")
    assert proto("sprk_train_tower_workspace_bytes") == proto("sprk_train_workspace_bytes")
