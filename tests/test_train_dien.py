"""The DIEN trainer's definition (sparrowrecsys_amd/trainer_dien.py, ``train_host``) against independent implementations; no GPU.
The bounds of the three float64 comparisons are four times the largest deviation measured over the inputs listed in each test
(docs/train_dien_results.md section 1 has the measured figures)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_dien as TE
from tests import train_dien_cases as TEC
from tests.conftest import ROOT

F = np.float32
same = TEC.same_bits
plus_zero = lambda a: not np.asarray(a).any() and not np.signbit(a).any()


# ---------------------------------------------------------------- forward

FORWARD_BOUND = {"p": 4 * 1.20e-7, "g": 4 * 1.20e-7, "a": 4 * 1.20e-7, "hs": 4 * 1.20e-7}      # measured: the docstring below


@pytest.mark.parametrize("name", ["small", "reference", "model"])
def test_forward_matches_the_float64_oracle(name, samples):
    """The definition's float32 forward against oracle.ctr_oracle.dien_forward in float64 on the same weights: ``p``, the GRU's outputs
    ``g``, the gate ``a`` and the AUGRU's last state.  The small shape (D 3, T 3, H 5, tail (6, 4)) and the reference shape on 200 rows of
    seed 3, and ``models.DIEN(seed=11)`` on the golden rows.  Largest absolute deviations measured (small / reference / model): p 1.19e-7 /
    5.96e-8 / 5.96e-8, g 8.88e-8 / 8.76e-8 / 8.71e-8, a 3.93e-8 / 6.34e-8 / 5.23e-8, hs 1.13e-7 / 7.93e-8 / 8.84e-8; the bound is four
    times the largest, 1.2e-7, for each."""
    from oracle import ctr_oracle as O
    if name == "model":
        model = M.DIEN(seed=11)
        fam, w = TE.family_of(model), model.weights
        assert (len(fam.columns), fam.hist_len, fam.emb_dim, fam.att_hidden, fam.hidden, fam.n_dense, fam.fan0) == (9, 5, 10, 32, [128, 64], 7, 57)
        ids, dense = model._pack_python(samples)
        feats, kw = samples, {}
    else:
        fam, w, ids, dense, _ = TEC.small(200, seed=3, **({} if name == "small" else TEC.REFERENCE_SHAPE))
        feats, kw = TEC.features(fam, ids, dense), dict(hist_len=fam.hist_len, movie_buckets=fam.columns[0][2], user_buckets=fam.columns[fam.hist_len + 1][2])
    keep = {}
    got = TE.forward_host(fam, w, ids, dense, keep)
    want, parts = O.dien_forward(feats, w, dtype=np.float64, return_parts=True, **kw)
    err = {"p": np.abs(got - want.reshape(-1)).max(), "g": np.abs(keep["g"] - parts["gru"]).max(), "a": np.abs(keep["a"] - parts["att"]).max(),
           "hs": np.abs(keep["hs"] - parts["augru"]).max()}
    print("dien %s: max |definition - float64 oracle| over %d rows: %s" % (name, len(got), ", ".join("%s %.3e" % (k, v) for k, v in err.items())))
    assert got.dtype == F and (ids[:, 1:fam.hist_len + 1] == 0).any()
    for k in err:
        assert err[k] <= FORWARD_BOUND[k], (k, err[k])


TANH_BOUND = 4 * 6.23e-8


def test_tanh_def_against_numpy_in_float64():
    """``tanh_def`` against ``np.tanh`` in float64 over 0, +-subnormal, +-1e-4, +-0.5, +-9, +-44 and 4 001 points of [-10, 10].  The
    largest absolute deviation measured is 6.23e-8 (about 2^-24: ``s`` is rounded at 2^-25 and doubled); the bound is four times that.  ``tanh_def(0)``
    is exactly 0, it saturates at exactly +-1, and it is odd only within that bound: below about 1e-4 the subtraction leaves few bits,
    which is why the comparison is absolute."""
    z = np.concatenate([np.array([0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1e-4, -1e-4, 0.5, -0.5, 9.0, -9.0, 44.0, -44.0]), np.linspace(-10.0, 10.0, 4001)]).astype(F)
    got = TE.tanh_def(z)
    err = float(np.abs(got.astype(np.float64) - np.tanh(z.astype(np.float64))).max())
    print("tanh_def: max |tanh_def - np.tanh| = %.3e over %d points" % (err, len(z)))
    assert got.dtype == F and err <= TANH_BOUND
    assert plus_zero(TE.tanh_def(np.zeros(3, dtype=F))) and TE.tanh_def(F(44.0)) == 1.0 and TE.tanh_def(F(-44.0)) == -1.0 and 0.999 < TE.tanh_def(F(4.0)) < 1.0


# ---------------------------------------------------------------- gradients

GRAD_BOUND = {"small": 4 * 7.61e-7, "reference": 4 * 4.10e-6}


@pytest.mark.parametrize("name", ["small", "reference"])
def test_step_gradients_match_torch_autograd(name):
    """One step's gradients against torch CPU autograd in float64 over a restatement of the graph written in tests/train_dien_cases.py
    (mask included), for every array of ``param_names``: 200 rows, seeds 3, 4 and 5, tiles 7 and 32.  Per array the error is taken relative to
    the array's largest gradient magnitude.  Largest measured over all arrays: 7.61e-7 at the small shape (``augru_r_hid/kernel``), 4.10e-6 at the reference
    shape (``att1/kernel``, a sum over 1 000 pairs of terms that nearly cancel); the bounds are four times these."""
    import torch
    fam = TEC.family(**({} if name == "small" else TEC.REFERENCE_SHAPE))
    worst = {}
    for seed in (3, 4, 5):
        w = TEC.weights(fam, seed)
        ids, dense, y = TEC.data(fam, 200, seed)
        g64, p64 = TEC.torch_gradients(fam, w, ids, dense, y, torch.float64)
        for tile in (7, 32):
            g, p = TE.step_gradients(fam, w, ids, dense, y, tile)
            assert float(np.abs(p - p64).max()) <= 1e-6 and set(g) == set(TE.param_names(fam)) == set(w)
            for k in TE.param_names(fam):
                assert g[k].dtype == F and g[k].shape == w[k].shape
                big = float(np.abs(g64[k]).max())
                assert big > 0.0, k
                worst[k] = max(worst.get(k, 0.0), float(np.abs(g[k] - g64[k]).max()) / big)
    top = max(worst, key=worst.get)
    print("dien %s: largest gradient error relative to the array's largest magnitude: %.3e (%s)" % (name, worst[top], top))
    for k, v in worst.items():
        assert v <= GRAD_BOUND[name], (k, v)


def test_one_step_is_step_gradients_and_adam_step():
    fam, w, ids, dense, y = TEC.small(40, seed=1)
    got = TE.train_host(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    g, p = TE.step_gradients(fam, w, ids, dense, y, 8)
    assert got.step == 1 and same(got.p, p)
    for k in TE.param_names(fam):
        wk, m, v = w[k].copy(), np.zeros_like(w[k]), np.zeros_like(w[k])
        T.adam_step(wk, m, v, g[k], T.adam_alpha(0.001, 1))
        assert same(got.weights[k], wk) and same(got.m[k], m) and same(got.v[k], v), k
        assert not same(wk, w[k]), k


# ---------------------------------------------------------------- the mask

def grads(fam, w, ids, dense, y, tile=8):
    keep = {}
    g, _ = TE.step_gradients(fam, w, ids, dense, y, tile, keep)
    return g, keep


def test_all_slots_masked():
    """``g`` is zeros, the GRU arrays get gradient exactly ``+0``, every history entry carries ``+0``, and row 0 of ``emb/movie`` gets what
    the one sample whose candidate is 0 sends it, bit for bit -- and ``+0`` when no candidate is 0."""
    fam, w, ids, dense, y = TEC.small(24, seed=2)
    ids[:, 1:4] = 0
    ids[:, 0] = 1 + ids[:, 0] % 6
    g, keep = grads(fam, w, ids, dense, y)
    assert plus_zero(keep["g"]) and plus_zero(keep["drow"][:, 1:4])
    for k in ("gru/kernel", "gru_rec/kernel", "gru/bias"):
        assert plus_zero(g[k]), k
    assert plus_zero(g["emb/movie"][0]) and g["emb/movie"][1:].any() and g["augru_h_hid/kernel"].any() and g["att0/bias"].any()
    ids[13, 0] = 0
    g, keep = grads(fam, w, ids, dense, y)
    assert keep["drow"][13, 0].all() and same(g["emb/movie"][0], keep["drow"][13, 0])


def test_only_the_first_slot_masked():
    """History ``[0, a, b]``: the GRU starts at slot 1 from ``+0``, so its outputs there are those of ``[a, b, 0]`` at slots 0 and 1; slot
    0 sends nothing to the table or the GRU arrays, and what the later layers send to ``g_0`` is dropped."""
    fam, w, ids, dense, y = TEC.small(24, seed=3)
    ids[:, 1:4] = 1 + ids[:, 1:4] % 6
    ids[:, 1] = 0
    g, keep = grads(fam, w, ids, dense, y)
    shifted = ids.copy()
    shifted[:, 1:4] = np.stack([ids[:, 2], ids[:, 3], 0 * ids[:, 1]], axis=1)
    other = {}
    TE.forward_host(fam, w, shifted, dense, other)
    assert plus_zero(keep["g"][:, 0]) and same(keep["g"][:, 1:], other["g"][:, :2]) and same(other["g"][:, 2], other["g"][:, 1])
    assert plus_zero(keep["drow"][:, 1]) and plus_zero(keep["dmx"][:, 0]) and plus_zero(keep["dmh"][:, 0]) and keep["dg"][:, 0].any() and keep["dmx"][:, 1:].all()


def test_a_masked_slot_between_two_movies():
    """History ``[a, 0, b]``: slot 1 repeats slot 0's output, carries ``+0`` to the table, and its gradient lands on slot 0's step: with
    every later path cut (``gru_rec/kernel = 0`` and ``z = 0`` through a large negative ``z`` bias, so the state passes nothing on),
    ``dhn`` at slot 0 is exactly ``dg_0 + dg_1`` and the row of slot 0 is ``_back(gru/kernel, dmx)`` of it."""
    fam, w, ids, dense, y = TEC.small(24, seed=4)
    ids[:, 1:4] = 1 + ids[:, 1:4] % 6
    ids[:, 2] = 0
    g, keep = grads(fam, w, ids, dense, y)
    assert same(keep["g"][:, 1], keep["g"][:, 0]) and not same(keep["g"][:, 2], keep["g"][:, 1])
    assert plus_zero(keep["drow"][:, 2]) and plus_zero(keep["dmx"][:, 1]) and keep["drow"][:, 1].all() and keep["drow"][:, 3].all()
    import torch
    g64, _ = TEC.torch_gradients(fam, w, ids, dense, y, torch.float64)
    for k in ("emb/movie", "gru/kernel", "gru_rec/kernel", "gru/bias"):
        assert float(np.abs(g[k] - g64[k]).max()) <= GRAD_BOUND["small"] * float(np.abs(g64[k]).max()), k
    w["gru_rec/kernel"][...] = 0.0
    w["gru/bias"][:, :3] = -100.0                                              # z = 0 exactly: hn = hh, and dh receives dhn z = 0
    g, keep = grads(fam, w, ids, dense, y)
    assert plus_zero(keep["gz"])
    D, one = fam.emb_dim, F(1.0)
    dhn = (np.zeros_like(keep["dg"][:, 1]) + keep["dg"][:, 1]) + keep["dg"][:, 0]
    hh = keep["ghh"][:, 0]
    dp_h = (dhn * (one - keep["gz"][:, 0])) * (one - hh * hh)
    assert same(keep["dmx"][:, 0, 2 * D:], dp_h.astype(F)) and keep["dg"][:, 1].all()
    assert same(keep["drow"][:, 1], T._back(w["gru/kernel"], keep["dmx"][:, 0]))


def test_only_the_last_slot_unmasked():
    """History ``[0, 0, a]``: ``g`` is zeros before the last slot, which equals slot 0 of ``[a, 0, 0]``; only the last slot's entry moves
    a row."""
    fam, w, ids, dense, y = TEC.small(24, seed=5)
    ids[:, 1:3] = 0
    ids[:, 3] = 1 + ids[:, 3] % 6
    g, keep = grads(fam, w, ids, dense, y)
    first = ids.copy()
    first[:, 1], first[:, 3] = ids[:, 3], 0
    other = {}
    TE.forward_host(fam, w, first, dense, other)
    assert plus_zero(keep["g"][:, :2]) and same(keep["g"][:, 2], other["g"][:, 0]) and same(other["g"][:, 2], other["g"][:, 0])
    assert plus_zero(keep["drow"][:, 1:3]) and keep["drow"][:, 3].all() and plus_zero(keep["dmx"][:, :2]) and g["gru/kernel"].any()
    assert plus_zero(g["gru_rec/kernel"])                                     # the one step starts from the state +0


def test_a_candidate_that_is_also_in_two_history_slots():
    """``movieId == userRatedMovie1 == userRatedMovie3 == 5`` in sample 9 only: row 5's gradient is the sum of that sample's three
    entries in column order from ``+0``."""
    fam, w, ids, dense, y = TEC.small(24, seed=6)
    ids[:, :4] = 1 + ids[:, :4] % 4
    ids[9, :4] = np.array([5, 5, 2, 5])
    g, keep = grads(fam, w, ids, dense, y)
    d = keep["drow"][9]
    assert same(g["emb/movie"][5], ((np.zeros(3, dtype=F) + d[0]) + d[1]) + d[3]) and d[0].all() and d[1].all() and d[3].all()
    assert plus_zero(g["emb/movie"][6]) and plus_zero(g["emb/movie"][0])


# ---------------------------------------------------------------- batches, order, continuation

def test_two_steps_are_two_one_step_fits_continued_through_state():
    fam, w, ids, dense, y = TEC.small(40, seed=5)
    one = TE.train_host(fam, w, ids, dense, y, batch_size=20, epochs=1, tile=5)
    a = TE.train_host(fam, w, ids[:20], dense[:20], y[:20], batch_size=20, epochs=1, tile=5)
    b = TE.train_host(fam, a.weights, ids[20:], dense[20:], y[20:], batch_size=20, epochs=1, tile=5, state=(a.m, a.v, a.step))
    assert one.step == b.step == 2 and all(same(b.weights[k], one.weights[k]) and same(b.m[k], one.m[k]) and same(b.v[k], one.v[k]) for k in w)
    assert same(one.p, np.concatenate([a.p, b.p]))
    order = np.random.default_rng(3).permutation(40)
    c = TE.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5, order=order)
    d = TE.train_host(fam, w, ids[order], dense[order], y[order], batch_size=16, epochs=2, tile=5)
    assert all(same(c.weights[k], d.weights[k]) for k in w) and same(c.p, d.p) and c.history == d.history
    other = TE.train_host(fam, w, ids, dense, y, batch_size=20, epochs=1, tile=8)
    assert not same(other.weights["gru/kernel"], one.weights["gru/kernel"])        # the tile is part of the definition


# ---------------------------------------------------------------- rejections, limits, errors

def test_family_of_takes_dien_itself_only():
    class Sub(M.DIEN):
        pass
    for make in (lambda: Sub(seed=1), lambda: M.DIN(seed=1), lambda: M.NeuralCF(seed=1)):
        with pytest.raises(NotImplementedError, match="trainer_dien trains DIEN, not"):
            TE.family_of(make())
    model = M.DIEN(seed=1)
    with pytest.raises(NotImplementedError):
        model.fit({"label": np.zeros(1)})
    fam = TE.family_of(model)
    assert [k for k, _, _ in fam.columns] == ["movieId"] + ["userRatedMovie%d" % t for t in range(1, 6)] + ["userId", "userGenre1", "movieGenre1"]
    assert fam.table_of == [0] * 6 + [1, 2, 3]
    assert TE.param_names(fam) == list(model.weight_shapes()) and all(TE.param_shapes(fam)[k] == tuple(s) for k, s in model.weight_shapes().items())
    assert TE.default_tile(fam) == TE.DEFAULT_TILE and TE.lds_bytes(fam, TE.default_tile(fam)) <= TE.LDS_BYTES
    assert fam == TEC.family(**dict(TEC.REFERENCE_SHAPE, movies=model.movie_buckets, users=model.user_buckets))
    assert TE.family_of(M.DIEN(seed=1, emb_dim=16, hist_len=7)).emb_dim == 16


@pytest.mark.parametrize("kw", [dict(hist_len=TE.MAX_HIST + 1), dict(emb_dim=TE.MAX_EMB + 1, others=False), dict(att_hidden=TE.MAX_WIDTH + 1),
                                dict(hidden=(TE.MAX_WIDTH + 1,)), dict(hidden=(2,) * (TE.MAX_LAYERS + 1)), dict(emb_dim=50)])
def test_limits_raise(kw):
    with pytest.raises(ValueError, match="trainer_dien takes up to 16 id columns"):
        TEC.family(**kw)


def test_the_stated_maxima_are_inside_the_limits_and_fit_the_lds_with_one_sample():
    for kw in (dict(hist_len=TE.MAX_HIST), dict(emb_dim=49), dict(emb_dim=TE.MAX_EMB, others=False), dict(att_hidden=TE.MAX_WIDTH),
               dict(hidden=(TE.MAX_WIDTH,) * TE.MAX_LAYERS), dict(hist_len=TE.MAX_HIST, att_hidden=TE.MAX_WIDTH)):
        assert TE.lds_bytes(TEC.family(**kw), 1) <= TE.LDS_BYTES
    widest = TEC.family(hist_len=TE.MAX_HIST, emb_dim=TE.MAX_EMB, att_hidden=TE.MAX_WIDTH, hidden=(TE.MAX_WIDTH,) * TE.MAX_LAYERS, others=False)
    assert 100 * 1024 < TE.lds_bytes(widest, 1) <= TE.LDS_BYTES < TE.lds_bytes(widest, 2)          # every family inside the limits fits with one sample
    fam = TEC.family(hist_len=TE.MAX_HIST, att_hidden=TE.MAX_WIDTH, emb_dim=10, hidden=(TE.MAX_WIDTH,) * TE.MAX_LAYERS)
    assert TE.lds_bytes(fam, TE.DEFAULT_TILE) > TE.LDS_BYTES >= TE.lds_bytes(fam, TE.default_tile(fam)) and TE.default_tile(fam) < TE.DEFAULT_TILE


def test_family_checks_refuse_what_the_kernel_does_not_take():
    fam = TEC.family()
    with pytest.raises(ValueError, match="read table 0"):
        TE._check_family(fam._replace(table_of=[0, 0, 1, 0, 1, 2, 3]))
    with pytest.raises(ValueError, match="share its vocabulary"):
        TE._check_family(fam._replace(columns=fam.columns[:2] + [("x", "id", 8)] + fam.columns[3:]))
    with pytest.raises(ValueError, match="once each"):
        TE._check_family(fam._replace(xsrc=[TE.SRC_NUMERIC if s == TE.SRC_POOLED else s for s in fam.xsrc]))
    with pytest.raises(ValueError, match="history column"):
        TE._check_family(fam._replace(xsrc=fam.xsrc + [2], xsub=fam.xsub + [0]))
    with pytest.raises(ValueError, match="0 masks a history slot"):
        TE._check_family(fam._replace(columns=[(k, "genre", v) if c < 4 else (k, kind, v) for c, (k, kind, v) in enumerate(fam.columns)]))


def test_errors_name_the_smallest_failing_row_and_change_nothing():
    fam, w, ids, dense, y = TEC.small(40, seed=0)
    keep = {k: v.copy() for k, v in w.items()}

    def raises(match, ids=ids, dense=dense, y=y):
        with pytest.raises(ValueError, match=match):
            TE.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1)
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
        TE.train_host(fam, w, ids, dense, y, order=np.zeros(40, dtype=np.int64))
    with pytest.raises(ValueError, match="permutation"):
        TE.train_host(fam, w, ids, dense, y, order=np.arange(39))
    for kw in ({"batch_size": 0}, {"epochs": -1}, {"learning_rate": 0.0}, {"learning_rate": np.nan}, {"tile": 0}, {"batch_size": TE.MAX_BATCH + 1}):
        with pytest.raises(ValueError):
            TE.train_host(fam, w, ids, dense, y, **kw)
    with pytest.raises(ValueError, match=r"ids must be \[N, 7\]"):
        TE.train_host(fam, w, ids[:, :6], dense, y)
    with pytest.raises(ValueError, match="weight 'augru/h0' has shape"):
        TE.train_host(fam, dict(w, **{"augru/h0": w["augru/h0"][0]}), ids, dense, y)


def test_fit_without_a_device_points_to_the_host_definition(samples):
    import torch
    model = M.DIEN(seed=1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device.*trainer_dien.train_host"):
            TE.fit(model, samples)
        with pytest.raises(RuntimeError, match="no HIP device.*train_host"):
            TE.train_device(TE.family_of(model), model.weights, np.zeros((1, 9), np.int32), np.zeros((1, 7), F), np.zeros(1, F))
    with pytest.raises(NotImplementedError, match="trainer_dien trains DIEN"):
        TE.fit(M.DIN(seed=1), samples)


# ---------------------------------------------------------------- a label only the order of the history carries

def test_the_order_of_the_history_is_learned():
    """tests/train_dien_cases.py ordered_pairs(): 48 pairs of samples that hold the same two movies in the two orders, with labels 1 and 0
    and everything else equal.  With every history id 0 the two samples of a pair are one input, and no fit can bring the loss under
    ln 2; the same fit on the ordered histories must end lower than that run does."""
    fam, ids, dense, y = TEC.ordered_pairs()
    w = TEC.weights(fam, 1)
    kw = dict(batch_size=32, epochs=60, learning_rate=0.02, tile=8)
    seen = TE.train_host(fam, w, ids, dense, y, **kw)
    blind_ids = ids.copy()
    blind_ids[:, 1:3] = 0
    blind = TE.train_host(fam, w, blind_ids, dense, y, **kw)
    print("ordered pairs: loss after %d epochs %.4f with the histories, %.4f with every history id 0 (first epoch %.4f / %.4f)" % (
        kw["epochs"], seen.history[-1][0], blind.history[-1][0], seen.history[0][0], blind.history[0][0]))
    assert seen.history[-1][0] < blind.history[-1][0]


# ---------------------------------------------------------------- the C side, without a device

def test_lds_bytes_is_what_the_library_reports(lib):
    """``sprk_train_dien_fit`` checks its arguments before any device call: a tile beyond the LDS is refused with the bytes it would take,
    and ``sprk_train_dien_workspace_bytes`` is 0 from the first tile that does not fit."""
    for kw in (TEC.REFERENCE_SHAPE, dict(), dict(hidden=(64, 65)), dict(hidden=(7, 200, 3), att_hidden=2), dict(hist_len=12, emb_dim=10, att_hidden=64),
               dict(hist_len=1, att_hidden=1, hidden=(1,)), dict(emb_dim=16), dict(emb_dim=17), dict(emb_dim=64, others=False)):
        fam = TEC.family(**kw)
        ms = TE._model_struct(fam)
        once = TE.lds_bytes(fam, 0)
        fits = (TE.LDS_BYTES - once) // (TE.lds_bytes(fam, 1) - once)
        assert TE.lds_bytes(fam, fits) <= TE.LDS_BYTES < TE.lds_bytes(fam, fits + 1) and (once > 0) == (fam.emb_dim <= TE.STAGE_EMB)
        assert lib.sprk_train_dien_workspace_bytes(C.byref(ms), 100, 50, fits) > 0 and lib.sprk_train_dien_workspace_bytes(C.byref(ms), 100, 50, fits + 1) == 0
        rc = lib.sprk_train_dien_fit(C.byref(ms), None, None, None, None, 100, 50, fits + 3, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None, None, 0, None)
        assert rc == L.EINVAL
        told = re.search(rb"tile = (\d+) needs (\d+) bytes of LDS", lib.sprk_last_error())
        assert told and int(told.group(1)) == fits + 3 and int(told.group(2)) == TE.lds_bytes(fam, fits + 3)


def test_the_library_refuses_a_null_model_a_bad_model_and_a_short_workspace(lib):
    fam = TEC.family()
    args = lambda batch=16: (None, None, None, None, 40, batch, 8, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None, None, 0, None)
    assert lib.sprk_train_dien_workspace_bytes(None, 40, 16, 8) == 0
    assert lib.sprk_train_dien_fit(None, *args()) == L.EINVAL and b"train_dien_fit: bad model" in lib.sprk_last_error()

    def bad(change):
        ms = TE._model_struct(fam)
        assert lib.sprk_train_dien_workspace_bytes(C.byref(ms), 40, 16, 8) > 0
        change(ms)
        assert lib.sprk_train_dien_workspace_bytes(C.byref(ms), 40, 16, 8) == 0 and lib.sprk_train_dien_fit(C.byref(ms), *args()) == L.EINVAL
        assert b"train_dien_fit: bad model (need hist_len 1..%d, hist_len + 1 .. %d id columns" % (TE.MAX_HIST, TE.MAX_COLS) in lib.sprk_last_error()
    bad(lambda ms: setattr(ms, "hist_len", TE.MAX_HIST + 1))
    bad(lambda ms: setattr(ms, "n_cols", TE.MAX_COLS + 1))
    bad(lambda ms: setattr(ms, "emb_dim", TE.MAX_EMB + 1))
    bad(lambda ms: setattr(ms, "att_hidden", TE.MAX_WIDTH + 1))
    bad(lambda ms: setattr(ms, "n_layers", TE.MAX_LAYERS + 1))
    bad(lambda ms: setattr(ms, "n_x", TE.MAX_X + 1))
    bad(lambda ms: ms.width.__setitem__(0, TE.MAX_WIDTH + 1))
    bad(lambda ms: ms.genre.__setitem__(0, 1))                           # movie ids that may be -1
    bad(lambda ms: ms.table.__setitem__(2, 1))                           # a history slot that reads another table
    bad(lambda ms: ms.table.__setitem__(6, 4))                           # a gap in the tables
    bad(lambda ms: ms.vocab.__setitem__(1, 8))                           # two columns of one table that disagree
    bad(lambda ms: ms.xsrc.__setitem__(0, 2))                            # an input row from a history column
    bad(lambda ms: ms.xsub.__setitem__(list(ms.xsrc).index(TE.SRC_POOLED), 1))       # an element of the state twice, another missing
    ms = TE._model_struct(fam)
    assert lib.sprk_train_dien_workspace_bytes(C.byref(ms), 40, TE.MAX_BATCH, 8) > 0 and lib.sprk_train_dien_workspace_bytes(C.byref(ms), 40, TE.MAX_BATCH + 1, 8) == 0
    assert lib.sprk_train_dien_fit(C.byref(ms), *args(TE.MAX_BATCH + 1)) == L.EINVAL and b"a batch has up to 2^28 rows" in lib.sprk_last_error()
    # a workspace one byte short: refused by name before any device call (every pointer here is a host address that is never read)
    need = int(lib.sprk_train_dien_workspace_bytes(C.byref(ms), 40, 16, 8))
    buf = (C.c_uint64 * (need // 8 + 64))()
    at = C.c_void_p((C.addressof(buf) + 15) & ~15)
    rc = lib.sprk_train_dien_fit(C.byref(ms), at, at, at, None, 40, 16, 8, 1, at, 0.1, 0.001, 1e-7, at, at, at, at, at, at, need - 1, None)
    assert need > 0 and rc == L.EINVAL and b"sprk_train_dien_workspace_bytes" in lib.sprk_last_error()
    assert lib.sprk_train_dien_fit(C.byref(ms), at, at, at, None, 40, 16, 8, 1, at, 0.1, 0.001, 1e-7, at, at, at, at, None, at, need, None) == L.EINVAL
    assert b"NULL error word" in lib.sprk_last_error()


def test_header_exports_and_prototypes_agree(lib):
    import subprocess
    header = open(os.path.join(ROOT, "include", "sparrow_hip.h")).read()
    names = ["sprk_train_dien_workspace_bytes", "sprk_train_dien_fit"]
    declared = set(re.findall(r"\b(sprk_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in names:
        assert name in declared and name in L.EXPORTED_SYMBOLS and name in exported and hasattr(lib, name)
    assert re.search(r"\}\s*sprk_train_dien_model;", header)
    assert C.sizeof(L.TrainDienModel) == C.sizeof(L.TrainDinModel) and [f[0] for f in L.TrainDienModel._fields_] == [f[0] for f in L.TrainDinModel._fields_]
    struct = lambda name: re.sub(r"\s+", " ", re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", header).group(1))
    assert struct("sprk_train_dien_model") == struct("sprk_train_din_model")
    assert lib.sprk_train_dien_fit.argtypes[1:] == lib.sprk_train_fit.argtypes[1:] and lib.sprk_train_dien_fit.restype == C.c_int
    assert lib.sprk_train_dien_workspace_bytes.restype == C.c_size_t
    proto = lambda name: re.sub(r"\s+", " ", re.search(name + r"\(const sprk_train\w*_model\* model,(.*?)\);", header, re.S).group(1))
    assert proto("sprk_train_dien_fit") == proto("sprk_train_fit") and proto("sprk_train_dien_workspace_bytes") == proto("sprk_train_workspace_bytes")
