"""The shapes that fall off the fused kernels, on the device (``-m gpu``; the case table: tests/offvariant_cases.py, its soundness without a
GPU: tests/test_offvariant_cpu.py).

Per case one model is built and scored once.  describe() is asserted first -- ``stage`` exactly, ``kernel`` by its prefix -- so a later
silent re-route shows, and a case that reached the wrong kernel cannot pass for the wrong reason.  Bars, none of them new: the scores
within TIGHT = 3e-5 of the fp64 oracle (tests/test_gpu_parity.py) AND within twice the fp32 oracle's own error + 2e-6 (the second bar of
tests/test_gpu_value_range.py); for DIN the attention weights at the same two bars against the fp32 oracle's attention error, the pooled
vector within twice the fp32 oracle's pooled error + 2e-6 of its magnitude, its padding exactly zero, everything finite, no id flagged.
A shape the engine cannot hold is refused in words (offvariant_cases.REFUSED) and the refusal is what the case asserts.  One printed line per
case: route, e_score, e_att, e_pooled, e_oracle32, live share (``-s``); docs/offvariant_results.md is the place for one full run
(it holds the CPU-side figures until one has been recorded)."""
import numpy as np
import pytest

from sparrowrecsys_amd import models as M
from tests import offvariant_cases as OV

pytestmark = pytest.mark.gpu
_SWITCHES = ("SPRK_DIN_LEGACY", "SPRK_DIN_COLS", "SPRK_DIN_HALF", "SPRK_DIN_FUSED", "SPRK_DIN_FUSED_MIN_T", "SPRK_DIN_TAIL", "SPRK_FORCE_INTERPRETER",
             "SPRK_TILE_FOLD", "SPRK_TAIL_UNF", "SPRK_TAIL_POOLED_F16", "SPRK_MLP_CHAIN", "SPRK_MLP_ROWS_MANY", "SPRK_DYN_F16", "SPRK_HALF_RANGE_GUARD", "SPRK_MANY_STREAMS", "SPRK_PACK_NATIVE")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SPRK_QUIET", "1")                       # (the "no fused kernel" warning is the point of these cases)


def _build(r):
    """A model of the case's shape over the shared weights (the shared Refs object keeps no engine)."""
    return r.case.model(r.model.weights)


def _assert_route(c, d):
    assert d["stage"] == c.stage and d["kernel"].startswith(c.kernel), (c.name, d["stage"], d["kernel"], "expected", c.stage, c.kernel)
    assert d["fused"] == ("0" if c.kernel == "k_tile_forward" else "1")


@pytest.mark.parametrize("name", OV.NAMES)
def test_offvariant_shape_against_the_oracle(torch, name):
    r = OV.refs(name)
    c = r.case
    assert r.conditions_met(), (name, r.live, r.std, r.e32_pool)            # the inputs, before anything is compared
    if c.refused:
        with pytest.raises(RuntimeError, match=c.refused) as e:
            _build(r).engine
        print("\n%-26s refused: %s" % (name, str(e.value).split(": ", 1)[-1]))
        return
    model = _build(r)
    eng = model.engine
    try:
        d = eng.describe()
        _assert_route(c, d)
        got = model.predict(r.feats)[:, 0]                                  # (predict ends in check_ids: a flagged id raises)
        e_att = e_pooled = None
        if c.kind == "din":
            ids = torch.from_numpy(r.ids).cuda()
            pooled = torch.full((c.B, eng.n_aux), float("nan"), dtype=torch.float32, device="cuda")
            att = torch.full((c.B, c.T), float("nan"), dtype=torch.float32, device="cuda")
            eng.din_pool(ids, pooled, att)
            eng.check_ids()
            pooled, att = pooled.cpu().numpy(), att.cpu().numpy()
    finally:
        eng.close()
    e_score = float(np.abs(got - r.ref).max())
    if c.kind == "din":
        assert np.isfinite(att).all() and np.isfinite(pooled).all()
        e_att = float(np.abs(att - r.parts64["att"]).max())
        e_pooled = float(np.abs(pooled[:, :c.D] - r.parts64["pooled"]).max())
    print("\n%-26s %-16s %-32s e_score %.2e (bar %.1e)  e_att %s  e_pooled %s  e_oracle32 %.1e  live %.3f"
          % (name, d["stage"] or "-", d["kernel"], e_score, r.score_bar(),
             "-" if e_att is None else "%.2e (bar %.1e)" % (e_att, r.att_bar()),
             "-" if e_pooled is None else "%.2e (bar %.1e, e32 %.1e, max %.1f)" % (e_pooled, r.pooled_bar(), r.e32_pooled, r.pooled_mag), r.e32, r.live))
    assert np.isfinite(got).all()
    assert e_score <= OV.TIGHT and e_score <= 2 * r.e32 + 2e-6, (name, e_score, r.e32)
    if c.kind == "din":
        assert e_att <= OV.TIGHT and e_att <= 2 * r.e32_att + 2e-6, (name, e_att, r.e32_att)
        assert e_pooled <= r.pooled_bar(), (name, e_pooled, r.e32_pooled, r.pooled_mag)
        assert not pooled[:, c.D:].any()


def test_hist_len_257_is_refused_in_words(torch):
    model = M.DIN(seed=1, hist_len=OV.T_TOO_LONG, movie_buckets=OV.V_MOVIE, user_buckets=OV.V_USER)
    with pytest.raises(RuntimeError, match=r"outside \[1,256\]"):
        model.engine


def test_out_of_range_history_id_raises_on_the_generic_stage(torch):
    """hist_len = 100 (k_din_pool, two samples per pass): a history / candidate id outside the table is flagged, not read
    (as test_din_attention_kernel_bad_ids_raise expects of the fused stages)."""
    r = OV.refs("din-T100-D16")
    c = r.case
    model = _build(r)
    eng = model.engine
    try:
        assert eng.describe()["stage"] == "k_din_pool"
        for row, col, val in ((c.B - 1, 1 + 99, OV.V_MOVIE), (200, 1 + 3, -1), (0, 0, OV.V_MOVIE + 5)):
            bad = r.ids.copy()
            bad[row, col] = val
            pooled = torch.empty((c.B, eng.n_aux), dtype=torch.float32, device="cuda")
            eng.din_pool(torch.from_numpy(bad).cuda(), pooled, None)
            with pytest.raises(ValueError):
                eng.check_ids()
        pooled = torch.empty((c.B, eng.n_aux), dtype=torch.float32, device="cuda")
        eng.din_pool(torch.from_numpy(r.ids).cuda(), pooled, None)
        eng.check_ids()
    finally:
        eng.close()


@pytest.mark.parametrize("name", OV.BATCHED)
def test_batches_and_repeated_launches_give_the_same_bits(torch, name):
    """predict(batch_size=...) over five ragged batches -- four of one size, which go to the several-batches entry point and must fall back
    cleanly where the route has no such kernel, and a shorter last one -- equals predict batch by batch bit for bit; three launches of the
    whole batch are bit-identical."""
    r = OV.refs(name)
    c = r.case
    bs = (c.B + 4) // 5 + 3                                                  # four batches of bs rows and a shorter fifth
    assert 4 * bs < c.B < 5 * bs and bs % 16
    model = _build(r)
    try:
        _assert_route(c, model.engine.describe())
        whole = model.predict(r.feats, batch_size=bs)[:, 0]
        one_by_one = np.concatenate([model.predict({k: v[s:s + bs] for k, v in r.feats.items()})[:, 0] for s in range(0, c.B, bs)])
        ids, dense = torch.from_numpy(r.ids).cuda(), torch.from_numpy(r.dense).cuda()
        runs = [model.predict_device(ids, dense).cpu().numpy() for _ in range(3)]
        model.engine.check_ids()
    finally:
        model.engine.close()
    assert whole.shape == (c.B,) and np.array_equal(whole.view(np.uint32), one_by_one.view(np.uint32))
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)) and np.array_equal(runs[0].view(np.uint32), runs[2].view(np.uint32))
    assert np.abs(runs[0] - r.ref).max() <= OV.TIGHT and np.abs(whole - r.ref).max() <= OV.TIGHT
