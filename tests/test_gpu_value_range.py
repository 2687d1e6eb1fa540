"""Value-range cases through every split-f16 route (``-m gpu``; the cases, the routes and the site table: tests/value_range_cases.py,
their soundness without a GPU: tests/test_value_range_cpu.py).

Every compared case first meets the two input conditions on the oracle alone (live share >= 0.9, fp32 oracle within 1e-5 of the fp64 oracle),
and every route is asserted from describe() -- kernel, stage and ``split_f16`` -- before a score is compared: a route that quietly fell back
would pass for the wrong reason.  Bars: TIGHT = 3e-5 against the fp64 oracle (tests/test_gpu_parity.py), and the split path no worse than
twice its f32 twin + 2e-6 (the rule of test_deepfm_v2_split_f16_is_fp32_class).  One printed line per case:
route, case, kernel, stage, arith, live share, e_split, e_f32, e_oracle32.  docs/value_range_results.md keeps one full run."""
import numpy as np
import pytest

from tests import value_range_cases as VR

pytestmark = pytest.mark.gpu
TIGHT = VR.TIGHT
ROUTES = list(VR.ROUTES)
_SWITCHES = ("SPRK_V2_HALF", "SPRK_DYN_F16", "SPRK_DIN_COLS", "SPRK_DIEN_MFMA", "SPRK_DIN_FUSED", "SPRK_DIEN_FUSED", "SPRK_NCF_CHAIN",
             "SPRK_HALF_RANGE_GUARD")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def _described(d):
    k = d["kernel"]
    return dict(kernel=k.split("<")[0], unf=",UNF" in k, stage=d["stage"], split=frozenset(s for s in d["split_f16"].split(",") if s))


def _matches(d, exp):
    got = _described(d)
    return (got["kernel"] == exp["kernel"] and got["stage"] == exp["stage"] and got["split"] == frozenset(exp["split"])
            and (exp.get("unf") is None or got["unf"] == exp["unf"]))


def _run(monkeypatch, route, weights, feats, extra=None, dense_edit=None):
    """Scores of one model built under the route's switches (+ ``extra``), its describe(); the engine is closed."""
    with monkeypatch.context() as mp:
        for k in _SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in {**route.env, **(extra or {})}.items():
            mp.setenv(k, v)
        model = route.model.build(weights)
        try:
            d = model.engine.describe()
            if dense_edit is None:
                p = [model.predict(feats)[:, 0]]
            else:
                import torch
                ids, dense = model.pack(feats)
                ti = torch.from_numpy(ids).cuda()
                p = []
                for edit in dense_edit:
                    dn = dense.copy()
                    if edit is not None:
                        dn[edit[0], edit[1]] = edit[2]
                    p.append(model.predict_device(ti, torch.from_numpy(dn).cuda()).cpu().numpy().ravel())
            model.engine.check_ids()
        finally:
            model.engine.close()
    return (p[0] if dense_edit is None else p), d


def _line(route, case, d, live, e_split, e_f32, e32):
    g = _described(d)
    print("%-26s %-44s %-18s %-16s split_f16=%-34s live %.3f  e_split %.3g  e_f32 %s  e_oracle32 %.2e"
          % (route.name, case, g["kernel"] + (",UNF" if g["unf"] else ""), g["stage"] or "-", ",".join(sorted(g["split"])) or "(f32)", live, e_split,
             "%.3g" % e_f32 if e_f32 is not None else "-", e32))


def _refs(route, c):
    m = route.model
    r64, r32 = VR.oracle(m, c.weights, c.feats, np.float64, c.name), VR.oracle(m, c.weights, c.feats, np.float32, c.name)
    live, e32, ok = VR.conditions(r64, r32)
    assert ok, (route.name, c.name, live, e32)                                  # the inputs, before anything is compared
    return r64, live, e32


@pytest.mark.parametrize("name", ROUTES)
def test_split_path_holds_fp32_class_over_the_value_range(torch, monkeypatch, name):
    """Cases 1 - 3 (and a small_table the guard need not act on): tables x 2^-12, tables x the largest power of two <= 16 the conditions allow,
    dense columns spread over three / four decades per sample.  The split path stays on, holds TIGHT and the twin rule."""
    route = VR.ROUTES[name]
    bad = []
    print()
    for c in VR.compared_cases(route) + [c for c in VR.guard_cases(route) if c.kind == "split"]:
        r64, live, e32 = _refs(route, c)
        p, d = _run(monkeypatch, route, c.weights, c.feats)
        p0, d0 = _run(monkeypatch, route, c.weights, c.feats, extra=route.twin_env)
        e1, e0 = float(np.abs(p - r64).max()), float(np.abs(p0 - r64).max())
        _line(route, c.name, d, live, e1, e0, e32)
        if not _matches(d, route.expected(c.key)):                             # (c.key: a site's own documented range rule, VR.Case.note)
            bad.append((c.name, "describe", _described(d), route.expected(c.key)))
        if not _matches(d0, route.twin):
            bad.append((c.name, "describe of the f32 twin", _described(d0), route.twin))
        if not (np.isfinite(p).all() and e1 <= TIGHT and e1 <= 2 * e0 + 2e-6):
            bad.append((c.name, e1, e0))
    if VR.scale_up_factor(route.model) == 1:
        print("%-26s scale_up: no power of two above 1 keeps the input conditions -- no up-scaled case for this route" % name)
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", [n for n in ROUTES if VR.guard_cases(VR.ROUTES[n])])
def test_guard_keeps_the_f32_form_of_the_poisoned_site(torch, monkeypatch, name):
    """Cases 4 - 7: an outlier row, a table 2^24 under its neighbours, an outlier weight that multiplies zeros, NaN / Inf in an unreferenced
    row, a NaN weight.  The engine builds, describe() reports the f32 form for THAT site and the other sites unchanged, the scores are finite
    and within TIGHT; once per site, the x2^36 outlier row with SPRK_HALF_RANGE_GUARD=0 errs more than with the guard (the case reaches the site)."""
    route = VR.ROUTES[name]
    bad = []
    print()
    for c in VR.guard_cases(route):
        if c.kind == "split":
            continue
        exp = route.expected(c.key)
        if c.kind == "nonfinite_weight":                                       # the oracle is NaN for every sample: build and route only
            p, d = _run(monkeypatch, route, c.weights, c.feats)
            print("%-26s %-44s %s" % (name, c.name, {k: d[k] for k in ("kernel", "stage", "split_f16")}))
            if not _matches(d, exp):
                bad.append((c.name, "describe", _described(d), exp))
            continue
        r64, live, e32 = _refs(route, c)
        p, d = _run(monkeypatch, route, c.weights, c.feats)
        e1 = float(np.abs(p - r64).max())
        _line(route, c.name, d, live, e1, None, e32)
        if not _matches(d, exp):
            bad.append((c.name, "describe", _described(d), exp))
        if not (np.isfinite(p).all() and e1 <= TIGHT):
            bad.append((c.name, "error", e1))
        if c.guard_off:
            p2, d2 = _run(monkeypatch, route, c.weights, c.feats, extra={"SPRK_HALF_RANGE_GUARD": "0"})
            with np.errstate(invalid="ignore"):
                e2 = float(np.nan_to_num(np.abs(p2 - r64), nan=np.inf).max())
            print("%-26s %-44s   guard off: split_f16=%s e %.3g" % (name, c.name, d2["split_f16"] or "(f32)", e2))
            if not e2 > e1:
                bad.append((c.name, "guard off errs no more", e2, e1))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", [n for n in ROUTES if VR.poisoned_batches(VR.ROUTES[n])])
def test_poisoned_sample_does_not_leak_into_its_tile(torch, monkeypatch, name):
    """Case 8: NaN, +-Inf, 3e38, a subnormal and -0.0 in ONE sample's dense column at the tile edges of the batch (through predict_device: the
    packer of predict(dict) reads NaN as a missing value).  Every OTHER score is bit-identical to the batch without the poison; the subnormal
    and -0.0 samples are within TIGHT of the oracle.  What the poisoned sample scores otherwise is recorded, not asserted."""
    route = VR.ROUTES[name]
    m = route.model
    w, f = m.weights(), m.features()
    col = list(m.build().numeric_keys).index(VR.POISON_COLUMN)
    batches = VR.poisoned_batches(route)
    edits = [None] + [(pos, col, val) for (_, poison, pos, _), val in zip(batches, [v for _, v in VR.POISONS for _ in range(4)])]
    scores, d = _run(monkeypatch, route, w, f, dense_edit=edits)
    print()
    assert _matches(d, route.expected()), (name, d)
    base = scores[0]
    r64 = VR.oracle(m, w, f, np.float64, "base")
    assert np.abs(base - r64).max() <= TIGHT
    bad, recorded = [], {}
    for (label, poison, pos, feats), p in zip(batches, scores[1:]):
        others = np.arange(VR.B) != pos
        leaked = int((p[others] != base[others]).sum())
        if leaked:
            bad.append((label, "%d other scores moved" % leaked))
        recorded.setdefault(poison, []).append(float(p[pos]))
        if poison in VR.POISON_ASSERTED:
            ref = m.oracle(feats, w, np.float64)[pos]
            if not abs(p[pos] - ref) <= TIGHT:
                bad.append((label, float(p[pos]), float(ref)))
    print("%-26s poisoned_sample %s  own score at 0/15/16/B-1: %s" % (name, d["kernel"].split("<")[0], "  ".join(
        "%s %s" % (k, "/".join("%.4g" % x for x in v)) for k, v in recorded.items())))
    assert not bad, (name, bad)
