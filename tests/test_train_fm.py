"""The DeepFM_v2 trainer's definition (sparrowrecsys_amd/trainer_fm.py, ``train_host``) against independent implementations; no GPU.
The measured figures are in docs/train_fm_results.md."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_fm as TF
from sparrowrecsys_amd.metrics import exact_roc_auc
from tests import train_fm_cases as TFC
from tests.conftest import ROOT

F = np.float32
same = TFC.same_bits


# ---------------------------------------------------------------- forward

def test_forward_matches_the_float64_oracle(samples):
    """The definition's float32 forward against oracle.ctr_oracle.deepfm_v2_forward in float64 on the golden rows, random trained-like
    weights, the reference shape: within 1e-4 absolute, the existing trainer's bound."""
    from oracle import ctr_oracle as O
    model = M.DeepFMv2(seed=11)
    fam = TF.family_of(model)
    assert (len(fam.fields), fam.emb_dim, fam.proj_dim, fam.hidden, fam.n_dense) == (4, 10, 64, [32, 16], 7)
    ids, dense = model._pack_python(samples)
    got = TF.forward_host(fam, model.weights, ids, dense)
    want = O.deepfm_v2_forward(samples, model.weights, dtype=np.float64).reshape(-1)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("deepfm_v2: max |p - oracle| = %.3e over %d rows" % (err, len(got)))
    assert got.dtype == F and err <= 1e-4


# ---------------------------------------------------------------- gradients

GRAD_SHAPES = {"reference": TFC.REFERENCE_SHAPE, "odd": TFC.ODD_SHAPE}
GRAD_SEEDS = 5


@pytest.mark.parametrize("name", sorted(GRAD_SHAPES))
@pytest.mark.parametrize("tile", [7, 32])
def test_step_gradients_match_torch_autograd(name, tile):
    """One step's gradients against torch CPU autograd in float64 on the same graph, 200 rows, five fixed draws.  Per tensor: the
    definition's largest error relative to the tensor's largest magnitude is at most 4 x the same error of torch's own float32
    autograd (docs/train_results.md section 1 explains the bound; the measured ratios are in docs/train_fm_results.md).  The odd shape:
    emb_dim 3, proj_dim 5, hidden (17, 1), three of four fields in ``order`` and not in field order, genre ids -1 at a quarter."""
    import torch
    fam = TFC.family(**GRAD_SHAPES[name])
    if name == "odd":
        assert len(fam.order) < len(fam.fields) and fam.order != [k for k, _, _ in fam.fields if k in fam.order]
    mine, theirs = {}, {}
    for seed in range(GRAD_SEEDS):
        w = TFC.weights(fam, 3 + seed)
        ids, dense, y = TFC.data(fam, 200, 5 + seed)
        g, p = TF.step_gradients(fam, w, ids, dense, y, tile)
        g64, p64 = TFC.torch_gradients(fam, w, ids, dense, y, torch.float64)
        g32, _ = TFC.torch_gradients(fam, w, ids, dense, y, torch.float32)
        assert float(np.abs(p - p64).max()) <= 1e-6
        assert set(g) == set(TF.param_names(fam)) == set(w)
        for k in TF.param_names(fam):
            assert g[k].dtype == F and g[k].shape == w[k].shape
            big = float(np.abs(g64[k]).max())
            if big == 0.0:                                              # (the table of a field outside `order`, or a dead unit in front)
                assert not g[k].any() and not g32[k].any()
                continue
            mine[k] = max(mine.get(k, 0.0), float(np.abs(g[k] - g64[k]).max()) / big)
            theirs[k] = max(theirs.get(k, 0.0), float(np.abs(g32[k] - g64[k]).max()) / big)
    for k in sorted(mine):
        print("%s tile %d %-16s definition %.3e torch float32 %.3e ratio %.2f" % (name, tile, k, mine[k], theirs[k], mine[k] / theirs[k]))
        assert mine[k] <= 4.0 * theirs[k], k


# ---------------------------------------------------------------- Adam

def test_one_step_is_step_gradients_and_adam_step():
    fam, w, ids, dense, y = TFC.small(40, seed=1)
    got = TF.train_host(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    g, p = TF.step_gradients(fam, w, ids, dense, y, 8)
    assert got.step == 1 and same(got.p, p)
    for k in TF.param_names(fam):
        wk, m, v = w[k].copy(), np.zeros_like(w[k]), np.zeros_like(w[k])
        T.adam_step(wk, m, v, g[k], T.adam_alpha(0.001, 1))
        assert same(got.weights[k], wk) and same(got.m[k], m) and same(got.v[k], v), k
        assert not same(wk, w[k]) or k.startswith("emb/") or k == "fo_cat/kernel", k


# ---------------------------------------------------------------- the structure of the definition

def test_rows_a_batch_did_not_touch():
    """After step 1 a row never hit holds its initial bits, in its ``emb/`` table and in ``fo_cat/kernel`` (m = v = 0 gives a zero
    update); a row hit in step 1 and never again keeps moving, as under Keras' Adam."""
    fam = TFC.family(vocabs=(8,), kinds=("id",), emb_dim=3, proj_dim=4, hidden=(4,))
    w = TFC.weights(fam, 2)
    ids = np.array([[0]] * 4 + [[1]] * 8, dtype=np.int32)
    y = np.array([1, 0, 1, 1] + [0, 1] * 4, dtype=F)
    dense = np.random.default_rng(0).standard_normal((12, 7)).astype(F)
    s1 = TF.train_host(fam, w, ids[:4], dense[:4], y[:4], batch_size=4, epochs=1)
    for k in ("emb/f0", "fo_cat/kernel"):
        assert same(s1.weights[k][1:], w[k][1:]) and not same(s1.weights[k][0], w[k][0])
    s3 = TF.train_host(fam, w, ids, dense, y, batch_size=4, epochs=1)
    s2 = TF.train_host(fam, w, ids[:8], dense[:8], y[:8], batch_size=4, epochs=1)
    for k in ("emb/f0", "fo_cat/kernel"):
        assert not same(s3.weights[k][0], s2.weights[k][0])                 # row 0 moved in step 3 without being hit
        assert same(s3.weights[k][2:], w[k][2:])


def test_a_field_outside_order_keeps_its_table():
    fam, w, ids, dense, y = TFC.small(60, seed=3, vocabs=(6, 5, 9), kinds=("id", "genre", "id"), order=(2, 0))
    out = fam.fields[1][0]
    assert out not in fam.order
    got = TF.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert same(got.weights["emb/" + out], w["emb/" + out]) and not got.m["emb/" + out].any() and not got.v["emb/" + out].any()
    rows = slice(fam.fo_off[1], fam.fo_off[1] + 5)
    assert not same(got.weights["fo_cat/kernel"][rows], w["fo_cat/kernel"][rows])
    assert not same(got.weights["emb/" + fam.order[0]], w["emb/" + fam.order[0]])


def test_fm_of_bias_only_groups_in_the_stated_order():
    """``order`` of one field whose ids are all -1, numerics all zero: both groups are their biases, ``fm = s s - q`` with
    ``s = (0 + b0) + b1`` and ``q = (0 + b0 b0) + b1 b1``.  With equal biases ``fm`` is exactly ``2 fl(b b)``: ``fl(2b 2b) - 2 fl(b b)``."""
    fam = TFC.family(vocabs=(6, 5), kinds=("id", "genre"), order=(1,), emb_dim=3, proj_dim=5, hidden=(4,))
    w = TFC.weights(fam, 4)
    ids, dense, _ = TFC.data(fam, 9, 4)
    ids[:, 1] = -1
    dense[:] = 0.0
    k = fam.order[0]
    keep = {}
    TF.forward_host(fam, w, ids, dense, keep)
    b0, b1 = w["proj/%s/bias" % k], w["proj/num/bias"]
    s = (F(0) + b0) + b1
    q = (F(0) + b0 * b0) + b1 * b1
    assert same(keep["fm"], np.tile((s * s - q).astype(F), (9, 1))) and keep["fm"].any()
    w["proj/num/bias"] = b0.copy()
    TF.forward_host(fam, w, ids, dense, keep)
    assert same(keep["fm"], np.tile((F(2) * (b0 * b0)).astype(F), (9, 1)))


# ---------------------------------------------------------------- it learns

def test_it_learns():
    """Planted structure (tests/train_fm_cases.py planted()): DeepFM_v2 at the reference widths, batch 256, 5 epochs, lr 0.01.  Every
    epoch's loss is below the one before, and the held-out rank AUC clears 0.7662: torch.optim.Adam(eps=1e-7) on the same graph and
    arrays over five seeds (scripts/train_fm_torch_baseline.py) gave falling losses for all five and held-out AUCs 0.8687, 0.8691,
    0.8676, 0.8478, 0.8177 from 0.49 .. 0.51; the threshold is torch's lowest minus torch's own spread, 0.8177 - 0.0515.  Measured
    here: 0.8665."""
    (ids, dense, y), (tids, tdense, ty) = TFC.planted()
    model = TFC.planted_model(0)
    fam = TF.family_of(model)
    before = exact_roc_auc(ty, TF.forward_host(fam, model.weights, tids, tdense))
    got = TF.train_host(fam, model.weights, ids, dense, y, batch_size=256, epochs=5, learning_rate=0.01)
    losses = [h[0] for h in got.history]
    after = exact_roc_auc(ty, TF.forward_host(fam, got.weights, tids, tdense))
    print("losses %s; held-out AUC %.4f -> %.4f" % (" ".join("%.4f" % l for l in losses), before, after))
    assert got.step == 5 * 64 and len(losses) == 5
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert after >= 0.7662


# ---------------------------------------------------------------- rejections, limits, errors

def test_family_of_takes_deepfm_v2_itself_only():
    class Sub(M.DeepFMv2):
        pass
    for make in (lambda: Sub(seed=1), lambda: M.DeepFM(seed=1), lambda: M.NeuralCF(seed=1), lambda: M.EmbeddingMLP(seed=1)):
        with pytest.raises(NotImplementedError, match="DeepFMv2"):
            TF.family_of(make())
    with pytest.raises(NotImplementedError, match=r"NeuralCF\(arch=1\) and EmbeddingMLP, and DeepFMv2 through trainer_fm"):
        T.family_of(M.DeepFMv2(seed=1))
    fam = TF.family_of(M.DeepFMv2(seed=1))
    assert [k for k, _, _ in fam.fields] == ["movieId", "userId", "userGenre1", "movieGenre1"] and fam.order == M.DeepFMv2.DEFAULT_ORDER
    assert fam.fo_off == [19, 1039, 1020, 0]
    assert sorted(TF.param_names(fam)) == sorted(M.DeepFMv2(seed=1).weight_shapes())
    assert all(TF.param_shapes(fam)[k] == tuple(s) for k, s in M.DeepFMv2(seed=1).weight_shapes().items())
    assert TF.param_names(fam)[:5] == ["emb/movieId", "emb/userId", "emb/userGenre1", "emb/movieGenre1", "fo_cat/kernel"]
    assert TF.lds_bytes(fam, TF.default_tile(fam)) <= TF.LDS_BYTES


@pytest.mark.parametrize("kw", [dict(vocabs=(3,) * 9, kinds=("id",) * 9), dict(proj_dim=TF.MAX_PROJ + 1), dict(vocabs=(3,) * 8, kinds=("id",) * 8, proj_dim=TF.MAX_PROJ),
                                dict(hidden=(TF.MAX_WIDTH + 1,)), dict(hidden=(2,) * (TF.MAX_LAYERS + 1)), dict(order=())])
def test_limits_raise(kw):
    with pytest.raises(ValueError):
        TFC.family(**kw)


@pytest.mark.parametrize("field,value", [("n_fields", TF.MAX_FIELDS + 1), ("n_layers", TF.MAX_LAYERS + 1), ("width", TF.MAX_WIDTH + 1), ("proj_dim", TF.MAX_PROJ + 1),
                                         ("emb_dim", TF.MAX_IN + 1), ("n_dense", TF.MAX_IN + 1)])
def test_one_more_than_each_maximum_is_refused_by_the_library_in_words(lib, field, value):
    """The other route of ``test_limits_raise``: a valid model with one field raised past its maximum has no workspace, and the fit is
    refused before any device call in a message that names the limits."""
    ms = TF._model_struct(TFC.family(hidden=(TF.MAX_WIDTH,) * TF.MAX_LAYERS))
    assert lib.sprk_train_fm_workspace_bytes(C.byref(ms), 40, 16, 8) > 0
    if field == "width":
        ms.width[3] = value
    else:
        setattr(ms, field, value)
    assert lib.sprk_train_fm_workspace_bytes(C.byref(ms), 40, 16, 8) == 0
    rc = lib.sprk_train_fm_fit(C.byref(ms), None, None, None, None, 40, 16, 8, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None, None, 0, None)
    assert rc == L.EINVAL
    assert b"1..%d fields" % TF.MAX_FIELDS in lib.sprk_last_error() and b"1..%d hidden layers of 1..%d units, emb_dim 1..%d, 0..%d numerics" % (
        TF.MAX_LAYERS, TF.MAX_WIDTH, TF.MAX_IN, TF.MAX_IN) in lib.sprk_last_error()
    base = TFC.family()
    more = {"n_fields": dict(fields=base.fields + [("x%d" % i, "id", 3) for i in range(value - len(base.fields))]), "n_layers": dict(hidden=[2] * value),
            "width": dict(hidden=[value]), "proj_dim": dict(proj_dim=value), "emb_dim": dict(emb_dim=value), "n_dense": dict(n_dense=value)}[field]
    with pytest.raises(ValueError, match="trainer_fm takes up to %d fields" % TF.MAX_FIELDS):
        TF._check_family(base._replace(**more))


def test_the_stated_maxima_are_inside_the_limits():
    for kw in (dict(proj_dim=TF.MAX_PROJ), dict(vocabs=(3,) * 8, kinds=("id",) * 8, proj_dim=TF.MAX_FLAT // 9), dict(hidden=(TF.MAX_WIDTH,) * TF.MAX_LAYERS)):
        fam = TFC.family(**kw)
        assert TF.lds_bytes(fam, 1) <= TF.LDS_BYTES


def test_errors_name_the_smallest_failing_row_and_change_nothing():
    fam, w, ids, dense, y = TFC.small(40, seed=0, vocabs=(6, 5), kinds=("id", "genre"))
    keep = {k: v.copy() for k, v in w.items()}

    def raises(match, ids=ids, dense=dense, y=y):
        with pytest.raises(ValueError, match=match):
            TF.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1)
        assert all(same(w[k], keep[k]) for k in w)
    bad = ids.copy(); bad[30, 0] = 6; bad[12, 0] = -1; bad[20, 1] = -2
    raises("samples row 12: an id outside", ids=bad)
    bad = dense.copy(); bad[9, 1] = np.inf; bad[3, 0] = np.nan
    raises("samples row 3: a numeric feature is not finite", dense=bad)
    bad = y.copy(); bad[7] = np.nan
    raises("samples row 7: the label is not finite", y=bad)
    with pytest.raises(ValueError, match="permutation"):
        TF.train_host(fam, w, ids, dense, y, order=np.zeros(40, dtype=np.int64))
    for kw in ({"batch_size": 0}, {"epochs": -1}, {"learning_rate": 0.0}, {"tile": 0}):
        with pytest.raises(ValueError):
            TF.train_host(fam, w, ids, dense, y, **kw)


def test_batches_order_and_continuation():
    fam, w, ids, dense, y = TFC.small(40, seed=5)
    one = TF.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5)
    assert one.step == 6 and len(one.history) == 2 and one.p.shape == (40,)
    a = TF.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=5)
    b = TF.train_host(fam, a.weights, ids, dense, y, batch_size=16, epochs=1, tile=5, state=(a.m, a.v, a.step))
    assert b.step == 6 and all(same(b.weights[k], one.weights[k]) and same(b.m[k], one.m[k]) and same(b.v[k], one.v[k]) for k in w)
    order = np.random.default_rng(3).permutation(40)
    c = TF.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5, order=order)
    d = TF.train_host(fam, w, ids[order], dense[order], y[order], batch_size=16, epochs=2, tile=5)
    assert all(same(c.weights[k], d.weights[k]) for k in w) and same(c.p, d.p) and c.history == d.history


def test_a_stored_nan_is_the_quiet_nan():
    """``s s`` overflows with finite inputs; where the label equals the saturated ``p``, ``inf x 0`` enters the head's gradient: the
    weights then hold NaN, every one of them ``0x7fc00000``."""
    fam, w, ids, dense, y = TFC.small(16, seed=6, vocabs=(6, 5), kinds=("id", "id"))
    w["proj/num/bias"][:] = F(1e19)
    w["proj/%s/bias" % fam.order[0]][:] = F(1e19)
    w["head/kernel"][1:1 + fam.proj_dim] = np.abs(w["head/kernel"][1:1 + fam.proj_dim]) + F(0.1)
    y[:] = 1.0
    keep = {}
    TF.forward_host(fam, w, ids, dense, keep)
    assert np.isinf(keep["fm"]).all() and np.isfinite(keep["s"]).all()
    got = TF.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    bits = got.weights["head/kernel"].view(np.uint32)
    assert np.isnan(got.weights["head/kernel"]).any() and set(bits[np.isnan(got.weights["head/kernel"])].tolist()) == {0x7fc00000}


def test_fit_without_a_device_points_to_the_host_definition(samples):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no HIP device.*train_host"):
        M.DeepFMv2(seed=1).fit(samples)
    model = M.DeepFMv2(seed=1)
    with pytest.raises(RuntimeError, match="no HIP device.*train_host"):
        TF.train_device(TF.family_of(model), model.weights, np.zeros((1, 4), np.int32), np.zeros((1, 7), F), np.zeros(1, F))


# ---------------------------------------------------------------- the C side, without a device

def test_lds_bytes_is_what_the_library_reports(lib):
    """``sprk_train_fm_fit`` checks its arguments before any device call: a tile beyond the LDS is refused with the bytes it would take,
    and ``sprk_train_fm_workspace_bytes`` is 0 from the first tile that does not fit."""
    for kw in (TFC.REFERENCE_SHAPE, TFC.ODD_SHAPE, dict(hidden=(64, 65)), dict(hidden=(7, 200, 3), proj_dim=2)):
        fam = TFC.family(**kw)
        ms = TF._model_struct(fam)
        per = TF.lds_bytes(fam, 1)
        fits = TF.LDS_BYTES // per
        assert lib.sprk_train_fm_workspace_bytes(C.byref(ms), 100, 50, fits) > 0 and lib.sprk_train_fm_workspace_bytes(C.byref(ms), 100, 50, fits + 1) == 0
        rc = lib.sprk_train_fm_fit(C.byref(ms), None, None, None, None, 100, 50, fits + 3, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None, None, 0, None)
        assert rc == L.EINVAL
        told = re.search(rb"tile = (\d+) needs (\d+) bytes of LDS", lib.sprk_last_error())
        assert told and int(told.group(1)) == fits + 3 and int(told.group(2)) == TF.lds_bytes(fam, fits + 3)
    ms = TF._model_struct(TFC.family())
    ms.fo_off[0] += 1                                                       # first-order blocks that do not tile the kernel's rows
    assert lib.sprk_train_fm_workspace_bytes(C.byref(ms), 100, 50, 8) == 0
    ms = TF._model_struct(TFC.family())
    ms.order[1] = ms.order[0]
    assert lib.sprk_train_fm_workspace_bytes(C.byref(ms), 100, 50, 8) == 0


def test_header_exports_and_prototypes_agree(lib):
    import subprocess
    header = open(os.path.join(ROOT, "include", "sparrow_hip.h")).read()
    names = ["sprk_train_fm_workspace_bytes", "sprk_train_fm_fit"]
    declared = set(re.findall(r"\b(sprk_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert "global: sprk_*;" in open(os.path.join(ROOT, "sparrowrecsys_amd", "csrc", "exports.map")).read()
    for name in names:
        assert name in declared and name in L.EXPORTED_SYMBOLS and name in exported and hasattr(lib, name)
    assert "sprk_train_fm_model" not in declared and re.search(r"\}\s*sprk_train_fm_model;", header)
    consts = dict(re.findall(r"#define\s+(SPRK_TRAIN_FM_[A-Z_]+)\s+(\d+)", header))
    assert {k: int(v) for k, v in consts.items()} == {"SPRK_TRAIN_FM_MAX_FIELDS": L.TRAIN_FM_MAX_FIELDS, "SPRK_TRAIN_FM_MAX_LAYERS": L.TRAIN_FM_MAX_LAYERS,
                                                      "SPRK_TRAIN_FM_MAX_PROJ": L.TRAIN_FM_MAX_PROJ, "SPRK_TRAIN_FM_MAX_FLAT": L.TRAIN_FM_MAX_FLAT,
                                                      "SPRK_TRAIN_FM_MAX_WIDTH": L.TRAIN_FM_MAX_WIDTH, "SPRK_TRAIN_FM_MAX_IN": L.TRAIN_FM_MAX_IN}
    assert (TF.MAX_FIELDS, TF.MAX_LAYERS, TF.MAX_PROJ, TF.MAX_FLAT, TF.MAX_WIDTH, TF.MAX_IN) == (L.TRAIN_FM_MAX_FIELDS, L.TRAIN_FM_MAX_LAYERS, L.TRAIN_FM_MAX_PROJ,
                                                                                                    L.TRAIN_FM_MAX_FLAT, L.TRAIN_FM_MAX_WIDTH, L.TRAIN_FM_MAX_IN)
    assert C.sizeof(L.TrainFmModel) == 4 * (6 + 4 * L.TRAIN_FM_MAX_FIELDS + L.TRAIN_FM_MAX_LAYERS)       # all int32: no padding
    assert lib.sprk_train_fm_fit.argtypes[1:] == lib.sprk_train_fit.argtypes[1:] and lib.sprk_train_fm_fit.restype == C.c_int
    assert lib.sprk_train_fm_workspace_bytes.restype == C.c_size_t
    proto = lambda name: re.sub(r"\s+", " ", re.search(name + r"\(const sprk_train\w*_model\* model,(.*?)\);", header, re.S).group(1))
    assert proto("sprk_train_fm_fit") == proto("sprk_train_fit") and proto("sprk_train_fm_workspace_bytes") == proto("sprk_train_workspace_bytes")
