"""The device metrics' host side (no GPU): ``auc_from_confusion`` is ``keras_auc``'s expression, the bucket rule of
include/sparrow_hip.h reproduces ``metrics._confusion`` exactly, ``sprk_metrics_*`` validate their arguments before any device call,
and ``DeviceMetrics.merge`` adds accumulators."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import metrics as MT
from tests import metrics_cases as MC


def _bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("T", [2, 3, 200, 1024])
def test_auc_from_confusion_is_keras_auc_bit_for_bit(T):
    for y, p in (MC.random_rows(), MC.adversarial(), MC.adversarial(with_nan=True)):
        conf = MT._confusion(y, p.astype(np.float64), T)
        for curve in ("ROC", "PR"):
            assert _bits(MT.auc_from_confusion(*conf, curve)) == _bits(MT.keras_auc(y, p, curve, T)), (T, curve)
    with pytest.raises(ValueError):
        MT.auc_from_confusion(*conf, "XY")


@pytest.mark.parametrize("T", [2, 3, 200, 1024])
def test_the_bucket_rule_reproduces_confusion_exactly(T):
    """Pins the definition: one counter per bucket per class, tp[i] = sum of pos[b] over b > i."""
    for y, p in (MC.adversarial(with_nan=True), MC.adversarial(), MC.random_rows(4097, 5)):
        sd = MC.state_dict_of(y, p, T)
        got = MT.DeviceMetrics._confusion_of(sd)
        want = MT._confusion(y, p.astype(np.float64), T)
        for g, w in zip(got, want):
            assert g.dtype == np.float64 and np.array_equal(g, w)
    # the float32 shortcut floor((T - 1) p) + 1 is NOT the rule: it disagrees on the adversarial set
    y, p = MC.adversarial()
    fin = np.isfinite(p)
    short = np.clip(np.floor(np.float32(199.0) * p[fin]).astype(np.int64) + 1, 0, 200)
    th = MC.thresholds(200)
    rule = (~(p[fin].astype(np.float64)[:, None] <= th[None, :])).sum(1)
    assert 100 < int((short != rule).sum()) < 400


def test_state_bytes(lib):
    assert [lib.sprk_metrics_state_bytes(T) for T in (-1, 0, 1, 1025, 1 << 20)] == [0] * 5
    sizes = [lib.sprk_metrics_state_bytes(T) for T in range(2, 1025)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])) and all(s % 8 == 0 for s in sizes)
    assert sizes[200 - 2] >= 8 * (4 + 2 * 201 + 200)
    assert L.METRICS_MAX_THRESHOLDS == 1024


def _aligned(nbytes, align=16):
    raw = np.zeros(nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw, raw.ctypes.data + off


def test_arguments_are_validated_before_any_device_call(lib):
    """Host memory everywhere: every case below fails validation, so nothing is launched."""
    vp = C.c_void_p
    nbytes = lib.sprk_metrics_state_bytes(200)
    keep, state = _aligned(nbytes)
    keep_s, scores = _aligned(64)
    keep_l, labels = _aligned(64)

    def err():
        return lib.sprk_last_error()
    # reset
    assert lib.sprk_metrics_reset(None, nbytes, 200, None) == L.EINVAL and b"state" in err()
    assert lib.sprk_metrics_reset(vp(state + 8), nbytes, 200, None) == L.EINVAL and b"16-byte" in err()
    assert lib.sprk_metrics_reset(vp(state), nbytes - 8, 200, None) == L.EINVAL and b"state_bytes" in err()
    for T in (1, 0, -5, 1025):
        assert lib.sprk_metrics_reset(vp(state), nbytes, T, None) == L.EINVAL and b"num_thresholds" in err()

    # update
    def upd(state=state, nbytes=nbytes, scores=scores, labels=labels, storage=L.COL_F32, stride=4, n=8):
        return lib.sprk_metrics_update(vp(state) if state else None, nbytes, vp(scores) if scores else None, vp(labels) if labels else None,
                                       storage, stride, n, None)
    assert upd(state=None) == L.EINVAL and b"state" in err()
    assert upd(state=state + 8) == L.EINVAL and b"16-byte" in err()
    assert upd(nbytes=lib.sprk_metrics_state_bytes(2) - 8) == L.EINVAL and b"state_bytes" in err()
    assert upd(scores=None) == L.EINVAL and b"scores" in err()
    assert upd(labels=None) == L.EINVAL and b"labels" in err()
    assert upd(scores=scores + 2) == L.EINVAL and b"scores" in err()
    assert upd(labels=labels + 2) == L.EINVAL and b"labels" in err()
    assert upd(labels=labels + 4, storage=L.COL_I64, stride=8) == L.EINVAL and b"labels" in err()
    for storage in (L.COL_I8, L.COL_I16, L.COL_U16, L.COL_U32, L.COL_F64, L.COL_TEXT, -1, 13):
        assert upd(storage=storage) == L.EINVAL and b"label_storage" in err(), storage
    for storage, stride in ((L.COL_F32, 0), (L.COL_F32, -4), (L.COL_F32, 6), (L.COL_I32, 2), (L.COL_I64, 4), (L.COL_I64, 12), (L.COL_U8, 0), (L.COL_BOOL, -1)):
        assert upd(storage=storage, stride=stride) == L.EINVAL and b"label_stride" in err(), (storage, stride)
    assert upd(n=-1) == L.EINVAL and b"negative n" in err()
    assert upd(n=1 << 62, stride=28) == L.EINVAL
    # nothing to do is not an error, and touches nothing
    assert upd(n=0) == L.OK
    assert not keep.any()


def test_merge_of_two_state_dicts_is_their_sum():
    y, p = MC.random_rows()
    a, b = MC.state_dict_of(y[:30000], p[:30000]), MC.state_dict_of(y[30000:], p[30000:])
    dm = MT.DeviceMetrics(200)                                           # (merged into only: needs no device)
    with pytest.raises(ValueError, match="no sample"):
        dm.result()
    sd = dm.merge(a).merge(b).state_dict()
    assert sd["n"] == a["n"] + b["n"] == len(y) and sd["n_correct"] == a["n_correct"] + b["n_correct"]
    assert sd["loss_sum"] == a["loss_sum"] + b["loss_sum"]
    assert np.array_equal(sd["pos"], a["pos"] + b["pos"]) and np.array_equal(sd["neg"], a["neg"] + b["neg"])
    whole = MC.state_dict_of(y, p)
    assert np.array_equal(sd["pos"], whole["pos"]) and np.array_equal(sd["neg"], whole["neg"]) and sd["n_correct"] == whole["n_correct"]
    got, want = dm.result(), MT.evaluate_scores(y, p)
    assert got[1:] == want[1:]                                           # counts: accuracy and both AUCs are evaluate_scores' bits
    assert abs(got[0] - want[0]) <= MC.loss_bound(len(y)) * want[0]
    # another object merges like its state_dict; a different threshold count does not
    other = MT.DeviceMetrics(200).merge(b)
    assert MT.DeviceMetrics(200).merge(a).merge(other).result() == got
    with pytest.raises(ValueError, match="thresholds"):
        MT.DeviceMetrics(100).merge(a)
    dm.reset()
    assert dm.state_dict()["n"] == 0
    for T in (1, 1025):
        with pytest.raises(ValueError):
            MT.DeviceMetrics(T)
