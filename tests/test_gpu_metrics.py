"""``model.evaluate``'s accumulators in device memory (``sprk_metrics_*``, csrc/k_metrics.h, ``metrics.DeviceMetrics``) against
their definition, sparrowrecsys_amd/metrics.py: every count exactly, the loss within the bound of a float64 sum (``-m gpu``).

Loss bound (tests/metrics_cases.py loss_bound): every term is non-negative for labels in [0, 1], so any order of N float64 additions
is within N 2^-53 relative of the exact sum and a double log is good to a few ulp; the tests take rel <= max(N, 64) 2^-50."""
import os

import numpy as np
import pytest

from sparrowrecsys_amd import metrics as MT
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import schema as S
from tests import metrics_cases as MC
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
EXCERPT = os.path.join(GOLDEN, "test_samples_512.csv")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


def _counts_equal(dm, y, p, T=200):
    got, want = dm.confusion(), MT._confusion(np.asarray(y), np.asarray(p, dtype=np.float32).astype(np.float64), T)
    for g, w, name in zip(got, want, ("tp", "fp", "tn", "fn")):
        assert g.dtype == np.float64 and np.array_equal(g, w), name
    sd = dm.state_dict()
    assert sd["n"] == len(p)
    assert sd["n_correct"] == int(((np.asarray(p, dtype=np.float64) > 0.5).astype(np.float64) == np.asarray(y, dtype=np.float64)).sum())
    return sd


def _loss_close(got, want, n):
    rel = abs(got - want) / want
    print("loss %.17g against %.17g over %d rows: rel %.3g (bound %.3g)" % (got, want, n, rel, MC.loss_bound(n)))
    assert rel <= MC.loss_bound(n)


@pytest.mark.parametrize("T", [2, 200, 1024])
def test_threshold_table_is_numpys_bit_for_bit(torch, T):
    got = MT.DeviceMetrics(T).thresholds()
    assert np.array_equal(got.view(np.uint64), MC.thresholds(T).view(np.uint64))


@pytest.mark.parametrize("dtype", ["float32", "int32", "int64", "uint8", "bool"])
def test_adversarial_scores_every_label_storage(torch, dtype):
    for with_nan in (True, False):
        y, p = MC.adversarial(with_nan)
        dm = MT.DeviceMetrics(200)
        dm.update(torch.from_numpy(p.copy()).cuda(), torch.from_numpy(y.copy()).cuda().to(getattr(torch, dtype)))
        _counts_equal(dm, y, p)
        got, want = dm.result(), MT.evaluate_scores(y, p)
        assert got[1:] == want[1:]
        if with_nan:
            assert np.isnan(got[0]) and np.isnan(want[0])
        else:
            _loss_close(got[0], want[0], len(p))


def _launch_edge_sizes():
    k = MC.kernel_constants()
    return [1, 63, 64, 65, 255, 4097, 65613, k["MT_MAX_GRID"] * k["MT_SLICE"] + k["MT_SLICE"] + 77]   # the last: past the capped grid's first round


@pytest.mark.parametrize("n", _launch_edge_sizes())
def test_sizes_across_the_launch_shape(torch, n):
    y, p = MC.random_rows(n, 11)
    dm = MT.DeviceMetrics(200)
    dm.update(torch.from_numpy(p.copy()).cuda(), torch.from_numpy(y.copy()).cuda())
    _counts_equal(dm, y, p)
    _loss_close(dm.result()[0], MT.binary_crossentropy(y, p), n)


def test_all_equal_scores(torch):
    """Every lane on one bucket: the contention case."""
    y = MC.random_rows(65536, 7)[0]
    for value in (np.float32(0.5), np.nextafter(np.float32(1.0 / 199.0), np.float32(0))):
        p = np.full(65536, value, dtype=np.float32)
        dm = MT.DeviceMetrics(200)
        dm.update(torch.from_numpy(p).cuda(), torch.from_numpy(y.copy()).cuda())
        _counts_equal(dm, y, p)
        got, want = dm.result(), MT.evaluate_scores(y, p)
        assert got[1:] == want[1:]
        _loss_close(got[0], want[0], len(p))


def test_strided_labels_and_column_scores(torch):
    y, p = MC.random_rows(4097, 5)
    wide = torch.zeros((4097, 7), dtype=torch.float32, device="cuda")
    wide[:, 3] = torch.from_numpy(y.astype(np.float32)).cuda()
    wide[:, 2] = 7.0                                                     # (neighbours that must not be read)
    wide[:, 4] = -1.0
    dm = MT.DeviceMetrics(200)
    dm.update(torch.from_numpy(p.copy()).cuda().reshape(-1, 1), wide[:, 3])
    _counts_equal(dm, y, p)
    # host labels are uploaded; a misaligned score view (4 bytes past a 16-byte boundary) takes the scalar loads
    dm2 = MT.DeviceMetrics(200)
    dm2.update(torch.from_numpy(np.concatenate([[np.float32(9)], p])).cuda()[1:], y.astype(np.float64))
    _counts_equal(dm2, y, p)
    assert dm2.result() == dm.result()


def test_streaming_updates(torch):
    y, p = MC.random_rows()
    n = len(p)
    assert n == 65613 == 1024 + 1 + 64000 + 588
    pd, yd = torch.from_numpy(p.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    one = MT.DeviceMetrics(200)
    one.update(pd, yd)
    whole = _counts_equal(one, y, p)
    want = MT.binary_crossentropy(y, p)
    _loss_close(one.result()[0], want, n)
    bits = set()
    for _ in range(5):
        dm = MT.DeviceMetrics(200)
        lo = 0
        for m in (1024, 1, 64000, 588):
            dm.update(pd[lo:lo + m], yd[lo:lo + m])
            lo += m
        sd = dm.state_dict()
        assert sd["n"] == whole["n"] and sd["n_correct"] == whole["n_correct"]
        assert np.array_equal(sd["pos"], whole["pos"]) and np.array_equal(sd["neg"], whole["neg"])
        _loss_close(sd["loss_sum"] / n, want, n)
        bits.add(np.float64(sd["loss_sum"]).view(np.uint64).item())
    assert len(bits) == 1                                                # no floating-point atomic: the same bits on every run
    # reset starts again; a result without a sample is an error
    dm.reset()
    with pytest.raises(ValueError, match="no sample"):
        dm.result()
    dm.update(pd, yd)
    assert dm.result() == one.result()


def test_evaluate_device_is_evaluate_on_the_trained_neuralcf(torch):
    from tests.test_savedmodel_pins import _ncf_w
    ckpt = np.load(os.path.join(GOLDEN, "neuralcf_ckpt.npz"))
    feats = {"movieId": ckpt["movieId"], "userId": ckpt["userId"], "label": ckpt["label"]}
    n = len(ckpt["label"])
    model = M.NeuralCF(weights=_ncf_w(ckpt, "001"))
    want = model.evaluate(feats)
    got = model.evaluate_device(feats)
    assert got[1:] == want[1:]
    _loss_close(got[0], want[0], n)
    x = {k: v for k, v in feats.items() if k != "label"}
    assert model.evaluate_device(x, feats["label"]) == got and model.evaluate_device(feats, batch_size=500)[1:] == got[1:]

    def halves():
        yield {k: v[:1024] for k, v in x.items()}, feats["label"][:1024]
        yield {k: v[1024:] for k, v in x.items()}, feats["label"][1024:]
    for it in (list(halves()), halves()):                                # a list, and a generator that can be consumed only once
        again = model.evaluate_device(it)
        assert again[1:] == want[1:]
        _loss_close(again[0], want[0], n)
    with pytest.raises(ValueError):
        model.evaluate_device(iter([]))
    with pytest.raises(ValueError):
        model.evaluate_device([x])                                       # batches without labels
    bad = dict(feats, movieId=feats["movieId"].copy())
    bad["movieId"][5] = 10 ** 6
    with pytest.raises(ValueError):
        model.evaluate_device(bad)


@pytest.mark.parametrize("make", [lambda: M.DeepFMv2(seed=3), lambda: M.DIN(seed=5)], ids=["DeepFM_v2", "DIN"])
def test_evaluate_csv_is_evaluate_on_the_parsed_file(torch, make):
    model = make()
    want = model.evaluate(S.read_samples_csv(EXCERPT))
    for got in (model.evaluate_csv(EXCERPT), model.evaluate_csv(open(EXCERPT, "rb").read(), batch_size=200)):
        assert got[1:] == want[1:]
        _loss_close(got[0], want[0], 512)
    part = model.evaluate_csv(EXCERPT, max_rows=100)
    assert part[1:] == model.evaluate(S.read_samples_csv(EXCERPT, limit=100))[1:]
    # an out-of-range id raises what predict_csv raises
    lines = open(EXCERPT).read().split("\n")
    row = lines[3].split(",")
    row[0] = "1000000"
    lines[3] = ",".join(row)
    text = "\n".join(lines)
    with pytest.raises(ValueError) as a:
        model.predict_csv(text.encode())
    with pytest.raises(ValueError) as b:
        model.evaluate_csv(text.encode())
    assert str(a.value) == str(b.value) and "movieId" in str(b.value)
