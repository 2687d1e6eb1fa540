"""The value-range cases of tests/value_range_cases.py are sound (no GPU): every compared case meets the two input conditions on the oracle
alone, a poison that must not be read leaves the fp64 oracle bit-identical, and an UNGUARDED static split of the poisoned table would fail
the GPU test (the bite check) -- so tests/test_gpu_value_range.py compares live scores and its guard cases can tell a guard from none."""
import numpy as np
import pytest

from tests import value_range_cases as VR

# one route per model shape (routes that share a model share its cases); the route with the most poisoned operands
_BY_MODEL = {}
for _r in VR.ROUTES.values():
    if _r.model.name not in _BY_MODEL or len(_r.after) > len(_BY_MODEL[_r.model.name].after):
        _BY_MODEL[_r.model.name] = _r
REPRESENTATIVES = sorted(r.name for r in _BY_MODEL.values())


def _oracles(route, case):
    m = route.model
    return VR.oracle(m, case.weights, case.feats, np.float64, case.name), VR.oracle(m, case.weights, case.feats, np.float32, case.name)


def test_every_kernel_has_a_route():
    """One route per kernel of EVERY_TILE (tests/test_gpu_stated_sizes.py) plus the two-launch stages and NeuralCF's chain."""
    kernels = [(r.kernel, r.stage) for r in VR.ROUTES.values()]
    for k in ("k_deepfm_v2_joint", "k_deepfm_pairs", "k_din_fused", "k_rows_chain", "k_dien_fused"):
        assert any(kk == k for kk, _ in kernels), k
    assert sum(kk == "k_mlp_rows" for kk, _ in kernels) == 2
    assert ("k_din_tail", "k_din_attn_cols") in kernels and ("k_din_tail", "k_dien_seq_mfma") in kernels
    assert sum(kk == "k_rows_chain" for kk, _ in kernels) == 2            # DeepFM_v2.py as written and NeuralCF
    for r in VR.ROUTES.values():
        for c in VR.guard_cases(r):
            if c.key is not None:
                assert c.key in r.after, (r.name, c.name)                  # every poisoned operand has its expected describe()


def test_live_share_tells_saturated_from_spread():
    assert VR.live_share(np.array([0.5, 0.1, 0.999])) == 1.0
    assert VR.live_share(np.array([0.0, 1.0, 1.0 - 1e-12, 1e-9])) == 0.0          # what ref.std() > 0.02 takes for a spread-out batch
    sat = np.array([0.0, 1.0] * 50)
    assert sat.std() > 0.02 and VR.live_share(sat) == 0.0


def test_static_split_is_fp32_class_on_an_ordinary_table_only():
    t = np.random.default_rng(0).normal(0, 0.3, (1000, 16)).astype(np.float32)
    assert np.abs(VR.static_split(t) - t).max() <= np.abs(t).max() * 2.0 ** -21
    assert not VR.guard_trips([t])
    t[3] *= np.float32(2.0 ** 36)
    q = VR.static_split(t)
    ordinary = np.arange(1000) != 3
    assert np.abs(q[ordinary] - t[ordinary]).max() > 1e-3                            # the ordinary rows lost their lo halves (and more)
    assert VR.guard_trips([t])


@pytest.mark.parametrize("name", REPRESENTATIVES)
def test_compared_cases_meet_the_input_conditions(name):
    route = VR.ROUTES[name]
    for c in VR.compared_cases(route) + [c for c in VR.guard_cases(route) if c.kind != "nonfinite_weight"]:
        r64 = VR.oracle(route.model, c.weights, c.feats, np.float64, c.name)
        if c.clean is not None and c.clean[0] is not None and c.name.startswith(("outlier_row", "nonfinite_row")):
            # the poison is never read: the conditions are the base case's
            base = VR.oracle(route.model, c.clean[0], c.clean[1], np.float64, "base")
            assert np.array_equal(r64, base), (name, c.name)
            continue
        r64, r32 = _oracles(route, c)
        live, e32, ok = VR.conditions(r64, r32)
        print("%s %s: live share %.3f, fp32 oracle %.2e" % (name, c.name, live, e32))
        assert ok, (name, c.name, live, e32)
        if c.clean is not None:                                                      # outlier_weight: the row multiplies zeros
            assert np.array_equal(r64, route.model.oracle(c.clean[1], c.clean[0], np.float64)), (name, c.name)
    print("%s: scale_up factor %d%s" % (name, VR.scale_up_factor(route.model), "" if VR.scale_up_factor(route.model) > 1 else " (no up-scaled case)"))


@pytest.mark.parametrize("name", REPRESENTATIVES)
def test_nonfinite_weight_makes_every_oracle_score_nan(name):
    """0 x NaN: only the build and the route can be pinned for these cases, not scores."""
    route = VR.ROUTES[name]
    for c in VR.guard_cases(route):
        if c.kind == "nonfinite_weight":
            assert np.isnan(VR.oracle(route.model, c.weights, c.feats, np.float64, c.name)).all(), (name, c.name)


@pytest.mark.parametrize("name", [n for n in REPRESENTATIVES if VR.ROUTES[n].row_tables])
def test_unguarded_static_split_would_fail_the_gpu_test(name):
    """The bite check: the x2^36 outlier row, split with the scale of the table's maximum and no guard, moves the oracle's scores by more
    than TIGHT in every table a static scale is taken from."""
    route = VR.ROUTES[name]
    for key in route.row_tables:
        factor, err = VR.outlier_bite_factor(route.model, key)
        print("%s %s: unguarded split of the x%g outlier moves the oracle by %.3g" % (name, key, factor or 0, err))
        assert factor == VR.OUTLIER_FACTORS[1] and err > VR.TIGHT, (name, key, factor, err)


@pytest.mark.parametrize("name", [n for n in REPRESENTATIVES if VR.poisoned_batches(VR.ROUTES[n])])
def test_poisoned_sample_leaves_the_other_oracle_scores_alone(name):
    route = VR.ROUTES[name]
    m = route.model
    base = VR.oracle(m, m.weights(), m.features(), np.float64, "base")
    seen = set()
    for label, poison, pos, feats in VR.poisoned_batches(route):
        if pos != 16:
            continue
        seen.add(poison)
        r = m.oracle(feats, m.weights(), np.float64)
        others = np.arange(VR.B) != pos
        assert np.array_equal(r[others], base[others]), label
        if poison in VR.POISON_ASSERTED:
            assert abs(r[pos] - m.oracle(feats, m.weights(), np.float32)[pos]) <= VR.ORACLE32_MAX, label
    assert seen == {p for p, _ in VR.POISONS}
