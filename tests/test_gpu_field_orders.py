"""Field orders on every DeepFM kernel route (``-m gpu``).  The engine does not run the plan in the order Python wrote it: at finalize
its plan matchers (match_v2_chain, setup_v2_joint, setup_rows_v2; setup_deepfm_pairs) rebuild each field <-> kernel slot map from the
plan's segments.  Here the models are built with field orders that are not the identity (tests/field_orders.py), and every route
must (a) be the kernel the case is written for (engine.describe()), (b) agree with the fp64 oracle within TIGHT at B = 4099 / 17 / 1
with missing ids, and (c) agree with the same model built another way.  Where the same kernel runs the same field split, the bits
must agree too.  tests/test_field_orders_cpu.py checks the constructions themselves and the sensitivity guard on CPU."""
import contextlib
import os

import numpy as np
import pytest

from oracle import ctr_oracle as O
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import synthetic as SY
from tests import field_orders as FO

pytestmark = pytest.mark.gpu
TIGHT = FO.TIGHT
SWITCHES = ("SPRK_V2J_ONE", "SPRK_V2J1_HOIST", "SPRK_V2_HALF", "SPRK_V2_JOINT", "SPRK_V2_ROWS", "SPRK_V2_FOLD", "SPRK_ROWS_UNF",
            "SPRK_FORCE_INTERPRETER", "SPRK_V1_CHAIN", "SPRK_V1_ONE", "SPRK_DYN_F16")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


@contextlib.contextmanager
def _env(settings):
    """The engine reads its switches once, at finalize: the model is built and run inside this block."""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(settings)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _kernel(model):
    return model.engine.describe()["kernel"]


def _kernel_is(got, want):
    return got.startswith(want[:-1]) if want.endswith("*") else got == want


def _scores(torch, model, feats):
    ids, dense = model.pack(feats)
    out = model.predict_device(torch.from_numpy(ids).cuda(), torch.from_numpy(dense).cuda()).cpu().numpy()
    model.engine.check_ids()
    return out


def _batches(fields, seed, dist):
    feats = {B: SY.synth_fields(B, fields, seed=seed + B, dist=dist) for B in FO.BATCHES}
    assert any((np.asarray(feats[4099][k]) == -1).any() for k, kind, _ in fields if kind == "genre"), "no missing ids"
    return feats


# ---- DeepFM_v2 ------------------------------------------------------------------------------------------------------------------
J33 = "k_deepfm_v2_joint<G_BIG=3,NJF=3,KPC=1,split-f16>"
R133 = "k_rows_chain<KPC=1,H0C=2,H1C=1,G_BIG=3,NJF=3>"
ROUTES_3BIG = {                    # route -> (switches, expected kernel; a trailing * = prefix)
    "default": ({}, J33),
    "looped": ({"SPRK_V2J_ONE": "0"}, J33),
    "hoisted": ({"SPRK_V2J1_HOIST": "1"}, J33),
    "joint-f32": ({"SPRK_V2_HALF": "0"}, "k_deepfm_v2_joint<G_BIG=3,NJF=3,KPC=1,f32>"),
    "joint-declined": ({"SPRK_V2_JOINT": "0"}, R133),
    "rows": ({"SPRK_V2_ROWS": "1"}, R133),
    "no-fold": ({"SPRK_V2_FOLD": "0"}, "k_rows_chain<*"),
    "interpreter": ({"SPRK_FORCE_INTERPRETER": "1"}, "k_tile_forward"),
}
ROUTES = {
    "S3-reference-order": {
        "default": ({}, "k_deepfm_v2_joint<G_BIG=2,NJF=2,KPC=1,split-f16>"),
        "looped": ({"SPRK_V2J_ONE": "0"}, "k_deepfm_v2_joint<G_BIG=2,NJF=2,KPC=1,split-f16>"),
        "joint-f32": ({"SPRK_V2_HALF": "0"}, "k_deepfm_v2_joint<G_BIG=2,NJF=2,KPC=1,f32>"),
        "joint-declined": ({"SPRK_V2_JOINT": "0"}, "k_tile_forward"),     # no k_rows_chain<KPC=1, G_BIG=2> instantiation
        "rows": ({"SPRK_V2_ROWS": "1"}, "k_tile_forward"),
    },
    "S4-proj32": {
        "default": ({}, "k_rows_chain<KPC=2,H0C=2,H1C=1,G_BIG=2,NJF=2,UNF>"),
        "folded-rows": ({"SPRK_ROWS_UNF": "0"}, "k_rows_chain<KPC=2,H0C=2,H1C=1,G_BIG=2,NJF=2>"),
        "interpreter": ({"SPRK_FORCE_INTERPRETER": "1"}, "k_tile_forward"),
    },
    "S4-reference": {
        "default": ({}, "k_rows_chain<KPC=4,H0C=2,H1C=1,G_BIG=2,NJF=2,UNF>"),
        "folded-rows": ({"SPRK_ROWS_UNF": "0"}, "k_rows_chain<KPC=4,H0C=2,H1C=1,G_BIG=2,NJF=2>"),
    },
}
for _case in FO.V2_CASES:
    if _case[:2] in ("S1", "S2"):
        ROUTES[_case] = ROUTES_3BIG
SAME_BITS = [("default", "looped"), ("default", "hoisted"), ("joint-declined", "rows")]
MANY = ("default", "joint-declined")


def _v2_model(case, weights=None, fields=None, order=None):
    f0, o0, D, P, seed = FO.V2_CASES[case]
    return M.DeepFMv2(weights=weights, seed=seed, emb_dim=D, fields=fields or f0, order=order or o0, proj_dim=P)


@pytest.mark.parametrize("case", sorted(ROUTES))
def test_deepfm_v2_field_order_routes(torch, case):
    fields, order, _, P, seed = FO.V2_CASES[case]
    sig = FO.perm_of(fields, order)
    feats = _batches(fields, seed, "zipf" if case.startswith("S2") else "uniform")
    base = _v2_model(case)
    w = base.weights
    ref = {B: O.deepfm_v2_forward(f, w, dtype=np.float64, fields=fields, order=order)[:, 0] for B, f in feats.items()}
    if not FO.is_identity(sig):
        # sensitivity guard: two moved fields' first-order blocks exchanged move the oracle far beyond TIGHT
        if "cycle" in case:
            assert not FO.is_involution(sig)
        a, b = FO.guard_pair(fields, order)
        moved = O.deepfm_v2_forward(feats[4099], FO.swap_fo_blocks(fields, w, a, b), dtype=np.float64, fields=fields, order=order)[:, 0]
        assert np.abs(moved - ref[4099]).max() > 100 * TIGHT
    other = {
        "fields-shuffled": (FO.shuffled(fields, 7), order, w),
        "identity-order": (fields,) + FO.v2_identity_order(fields, order, w, P),
    }
    problems, outs = [], {}
    for route, (env, want) in ROUTES[case].items():
        with _env(env):
            model = _v2_model(case, weights=w)
            kern = _kernel(model)
            print("%s / %s: %s" % (case, route, kern))
            if not _kernel_is(kern, want):
                problems.append("%s: runs %s, not %s" % (route, kern, want))
            outs[route] = {B: _scores(torch, model, f) for B, f in feats.items()}
            for B in FO.BATCHES:
                err = float(np.abs(outs[route][B] - ref[B]).max())
                if not err <= TIGHT:
                    problems.append("%s, B=%d: max|p - oracle| %.3e" % (route, B, err))
            for name, (f2, o2, w2) in other.items():
                m2 = _v2_model(case, weights=w2, fields=f2, order=o2)
                k2 = _kernel(m2)
                if k2 != kern:
                    problems.append("%s / %s: runs %s, the base model %s" % (route, name, k2, kern))
                for B in FO.BATCHES:
                    err = float(np.abs(_scores(torch, m2, feats[B]) - outs[route][B]).max())
                    if not err <= TIGHT:
                        problems.append("%s / %s, B=%d: %.3e from the base model" % (route, name, B, err))
                m2.engine.close()
            if route in MANY:
                # four batches in one launch, bit for bit a launch per batch
                chunks = [SY.synth_fields(4099, fields, seed=seed + 50 + i) for i in range(4)]
                packed = [model.pack(c) for c in chunks]
                ti = [torch.from_numpy(i).cuda() for i, _ in packed]
                td = [torch.from_numpy(d).cuda() for _, d in packed]
                many = [o.cpu().numpy() for o in model.predict_device_many(ti, td)]
                model.engine.check_ids()
                for i in range(4):
                    one = model.predict_device(ti[i], td[i]).cpu().numpy()
                    if not np.array_equal(many[i], one):
                        problems.append("%s: forward_many batch %d differs from its own forward by %.3e" % (route, i, np.abs(many[i] - one).max()))
            model.engine.close()
    for r1, r2 in SAME_BITS:
        if r1 in outs and r2 in outs:
            for B in FO.BATCHES:
                if not np.array_equal(outs[r1][B], outs[r2][B]):
                    problems.append("%s and %s differ at B=%d by %.3e" % (r1, r2, B, np.abs(outs[r1][B] - outs[r2][B]).max()))
    assert not problems, "\n".join(problems)


# ---- pair-dot DeepFM (k_deepfm_pairs) ----------------------------------------------------------------------------------------------
PAIR_ROUTES = {
    "default": {},
    "looped": {"SPRK_V1_ONE": "0"},
    "f32": {"SPRK_DYN_F16": "0"},
    "interpreter": {"SPRK_V1_CHAIN": "0"},
}


@pytest.mark.parametrize("tied", [False, True], ids=["own-deep-tables", "tied-tables"])
@pytest.mark.parametrize("shape", sorted(FO.PAIR_SHAPES))
def test_deepfm_pairs_field_order_routes(torch, shape, tied):
    fields, pairs, D = FO.PAIR_SHAPES[shape]
    nv = (D + 3) // 4
    want = "k_deepfm_pairs<NF=%d,NV=%d>" % (len(fields), nv)
    feats = _batches(fields, 81, "zipf")
    base = M.DeepFM(seed=61, emb_dim=D, fields=fields, pairs=pairs, share_deep_tables=tied)
    w = base.weights
    ref = {B: O.deepfm_forward(f, w, dtype=np.float64, fields=fields, pairs=pairs, share_deep_tables=tied)[:, 0] for B, f in feats.items()}
    assert ref[4099].std() > 0.02
    builds = {"base": (fields, pairs, list(base.deep_emb), w)}
    builds.update(FO.pair_constructions(fields, pairs, w))
    problems, outs = [], {}
    for route, env in PAIR_ROUTES.items():
        with _env(env):
            for name, (f2, p2, de2, w2) in builds.items():
                model = M.DeepFM(weights=w2, emb_dim=D, fields=f2, pairs=p2, deep_emb=de2, share_deep_tables=tied)
                kern = _kernel(model)
                if name == "base":
                    print("%s %s / %s: %s" % (shape, "tied" if tied else "own", route, kern))
                expect = "k_tile_forward" if route == "interpreter" else want
                if kern != expect:
                    problems.append("%s / %s: runs %s, not %s" % (route, name, kern, expect))
                got = {B: _scores(torch, model, f) for B, f in feats.items()}
                model.engine.close()
                if name == "base":
                    outs[route] = got
                for B in FO.BATCHES:
                    err = float(np.abs(got[B] - ref[B]).max())
                    if not err <= TIGHT:
                        problems.append("%s / %s, B=%d: max|p - oracle| %.3e" % (route, name, B, err))
                    err = float(np.abs(got[B] - outs[route][B]).max())
                    if not err <= TIGHT:
                        problems.append("%s / %s, B=%d: %.3e from the base model" % (route, name, B, err))
    for B in FO.BATCHES:
        if not np.array_equal(outs["default"][B], outs["looped"][B]):
            problems.append("one-task and looped kernels differ at B=%d by %.3e" % (B, np.abs(outs["default"][B] - outs["looped"][B]).max()))
    assert not problems, "\n".join(problems)
