"""The off-variant shapes (tests/offvariant_cases.py) without a GPU: the compile layer is right for every one of them, the inputs are worth
comparing, the engine's only refusals are explicit, and the bars the GPU file asserts sit far below the smallest mistake on each axis.

Per case: the model's plan, run by the numpy plan interpreter in float64, reproduces the fp64 oracle (scores at 2e-7; for DIN the attention
weights at 1e-7 and the pooled vector at 1e-6, as test_config3_din_shape) -- so what tests/test_gpu_offvariant_shapes.py leaves open is the
device code alone.  The input CONDITIONS (live share >= 0.9, score standard deviation >= 0.02, fp32 oracle within 1e-5 of the fp64 oracle)
are asserted, not measured: a case that misses one would pass on the GPU for the wrong reason."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L, models as M
from tests import offvariant_cases as OV


@pytest.mark.parametrize("name", OV.NAMES)
def test_plan_matches_the_oracle_and_the_inputs_are_worth_comparing(name):
    r = OV.refs(name)
    c = r.case
    np.testing.assert_allclose(r.plan64, r.o64, atol=2e-7)
    if c.kind == "din":
        pooled, att = OV.plan_parts(r)
        np.testing.assert_allclose(att, r.parts64["att"], atol=1e-7)
        np.testing.assert_allclose(pooled[:, :c.D], r.parts64["pooled"], atol=1e-6)
        assert not pooled[:, c.D:].any()
    assert r.live >= OV.LIVE_MIN, r.live
    assert r.std >= OV.STD_MIN, r.std
    assert r.e32_pool <= OV.ORACLE32_MAX and r.e32 <= OV.ORACLE32_MAX, (r.e32_pool, r.e32)


def test_the_table_holds_what_it_claims():
    """Every axis of the gap is in the table: attention widths on both sides of 32 with an odd and an even block count, histories at every
    MS = 256 / T below 4, rows wider than 32 floats, tails of one, two and three layers, and the three run-time-count forms of k_mlp_rows."""
    din = [c for c in OV.CASES if c.kind == "din"]
    assert {c.H for c in din} >= {16, 20, 32, 48, 64}
    assert {256 // c.T for c in din if c.T > 64} == {3, 2, 1}
    assert {(c.D + 3) // 4 * 4 for c in din if c.D > 32} == {36, 40, 64}
    assert {len(c.kw.get("hidden", (128, 64))) for c in din} == {1, 2, 3}
    assert {len(c.kw.get("hidden", (128, 128))) for c in OV.CASES if c.kind != "din"} == {1, 2, 3}
    assert {c.kernel for c in OV.CASES if c.plan_ref} == {"k_mlp_rows<8,8,NBIG=1,NSMALL=3>", "k_mlp_rows<8,8,NBIG=2,NSMALL=5>", OV._ROWS_28}
    for c in din:                                                          # ragged against the granules: 16-sample tasks, MS-sample passes
        assert c.B == 1 or c.B % 16, c
        assert c.T <= 64 or c.B % (256 // c.T) or 256 // c.T == 1, c
    assert len(set(OV.NAMES)) == len(OV.NAMES) and set(OV.BATCHED) <= set(OV.NAMES) and set(OV.REFUSED) <= set(OV.NAMES)


def test_the_oracle_follows_the_depth_of_the_weights():
    """din_forward / embedding_mlp_forward / wide_n_deep_forward take as many hidden layers as the weight dict holds: a layer more moves the
    scores, and the oracle of a depth-1 / depth-3 model is what its layers compose to (the plan comparison above is the full check)."""
    for name in ("din-tail128", "din-tail128x64x32-D32-T20", "mlp128", "mlp256x128x64"):
        r = OV.refs(name)
        c, w = r.case, r.model.weights
        pre = "fc" if c.kind == "din" else "dense"
        depth = len(c.kw["hidden"])
        assert ("%s%d/kernel" % (pre, depth - 1)) in w and ("%s%d/kernel" % (pre, depth)) not in w
        cut = {k: v for k, v in w.items() if not k.startswith("%s%d" % (pre, depth - 1))}    # the last hidden layer taken out ...
        with pytest.raises(ValueError):                                                     # ... no longer fits the head: the layer WAS applied
            OV.oracle(c, r.feats, cut, np.float64)


@pytest.mark.parametrize("what,slip,name", OV.SLIPS, ids=["%s-%s" % (w.replace(" ", "_"), n) for w, _, n in OV.SLIPS])
def test_bars_sit_ten_times_below_the_smallest_slip(what, slip, name):
    """On the oracle alone: one attention unit, one 16-unit block, one history slot or one embedding dimension lost moves the attention
    weights and the pooled vector by at least ten times the bars tests/test_gpu_offvariant_shapes.py asserts for that case."""
    r = OV.refs(name)
    d_att, d_pooled = slip(r)
    print("%-10s %-24s att moves %.2e (bar %.1e)  pooled moves %.2e (bar %.1e)" % (what, name, d_att, r.att_bar(), d_pooled, r.pooled_bar()))
    assert d_att >= 10 * OV.TIGHT >= 10 * r.att_bar()
    assert d_pooled >= 10 * r.pooled_bar() and d_pooled >= 10 * OV.TIGHT


def _create(lib, plan):
    h = C.c_void_p()
    rc = lib.sprk_create(C.byref(plan), C.byref(h))
    msg = lib.sprk_last_error().decode() if rc else ""
    if rc == 0:
        lib.sprk_destroy(h)
    return rc, msg


@pytest.mark.parametrize("name", OV.NAMES)
def test_create_takes_the_plan_or_refuses_it_in_words(lib, name):
    """sprk_create validates the plan and sizes the interpreter's LDS tile before it touches a device: every case passes, except the ones
    listed as refused, which fail with SPRK_EINVAL and the message the GPU file expects."""
    r = OV.refs(name)
    rc, msg = _create(lib, r.plan)
    if r.case.refused:
        assert rc == L.EINVAL and r.case.refused in msg, (rc, msg)
    else:
        assert rc == 0, msg


def test_hist_len_257_builds_a_plan_the_engine_refuses(lib):
    model = M.DIN(seed=1, hist_len=OV.T_TOO_LONG, movie_buckets=OV.V_MOVIE, user_buckets=OV.V_USER)
    plan, _ = model.build_plan()
    assert plan.din.T == OV.T_TOO_LONG
    rc, msg = _create(lib, plan)
    assert rc == L.EINVAL and "DIN history length 257 outside [1,256]" in msg, (rc, msg)
    plan256, _ = M.DIN(seed=1, hist_len=256, movie_buckets=OV.V_MOVIE, user_buckets=OV.V_USER).build_plan()
    assert _create(lib, plan256)[0] == 0
