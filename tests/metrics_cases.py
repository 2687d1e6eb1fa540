"""Inputs shared by tests/test_metrics_device_cpu.py and tests/test_gpu_metrics.py, built once and never modified: the adversarial
scores around every Keras threshold, random rows, and a numpy restatement of the device's bucket rule (include/sparrow_hip.h)."""
import functools
import os
import re

import numpy as np

from sparrowrecsys_amd import metrics as MT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def thresholds(T=200):
    """The table of metrics._confusion."""
    return np.array([0.0 - MT.EPS] + [(i + 1) / (T - 1) for i in range(T - 2)] + [1.0 + MT.EPS])


@functools.lru_cache(maxsize=None)
def _adversarial(with_nan):
    th = thresholds(200)
    vals = []
    for t in th:                                                         # the float32 nearest to each threshold and its two neighbours
        c = np.float32(t)
        vals += [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    tiny, sub_max = np.float32(1e-45), np.nextafter(np.float32(np.finfo(np.float32).tiny), np.float32(0))
    vals += [np.float32(0.0), np.float32(-0.0), np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1)), np.float32(1e-7),
             np.float32(1 - 1e-7), tiny, -tiny, sub_max, -sub_max, np.float32(2.0), np.float32(-1.0)]
    assert len(vals) == 612
    vals += [np.float32(np.inf), np.float32(-np.inf)] + ([np.float32(np.nan)] if with_nan else [])
    p = np.repeat(np.array(vals, dtype=np.float32), 2)                    # every value for both classes
    y = np.tile(np.array([0, 1], dtype=np.int64), len(vals))
    p.setflags(write=False), y.setflags(write=False)
    return y, p


def adversarial(with_nan=False):
    """(labels int64, scores float32): 1 230 rows with the NaN pair, 1 228 without."""
    return _adversarial(bool(with_nan))


@functools.lru_cache(maxsize=None)
def random_rows(n=65613, seed=3):
    """tests/test_metrics.py's _data: labels at 56 % positives, sigmoid scores that know a little about them."""
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.56).astype(np.int64)
    p = (1.0 / (1.0 + np.exp(-(rng.normal(0, 1, n) + 1.2 * (y - 0.5))))).astype(np.float32)
    p.setflags(write=False), y.setflags(write=False)
    return y, p


def bucket_counts(y, p, T=200):
    """The bucket rule in numpy: bucket = the number of thresholds t with !(p <= t); one counter per bucket per class."""
    th = thresholds(T)
    pd = np.asarray(p, dtype=np.float32).astype(np.float64)
    b = np.zeros(len(pd), dtype=np.int64)
    for t in th:
        b += ~(pd <= t)
    pos_class = np.asarray(y).astype(bool)
    return np.bincount(b[pos_class], minlength=T + 1).astype(np.uint64), np.bincount(b[~pos_class], minlength=T + 1).astype(np.uint64)


def state_dict_of(y, p, T=200):
    """What DeviceMetrics.state_dict() holds after an update with these rows, computed on the host."""
    pos, neg = bucket_counts(y, p, T)
    y64, p64 = np.asarray(y, dtype=np.float64), np.asarray(p, dtype=np.float32).astype(np.float64)
    pc = np.clip(p64, MT.EPS, 1.0 - MT.EPS)
    return {"num_thresholds": T, "n": len(p64), "n_correct": int(((p64 > 0.5).astype(np.float64) == y64).sum()),
            "loss_sum": float(np.sum(-(y64 * np.log(pc) + (1.0 - y64) * np.log(1.0 - pc)))), "pos": pos, "neg": neg}


def loss_bound(n):
    """Non-negative terms: any order of n float64 additions is within n 2^-53 relative of the exact sum; eight times that."""
    return max(n, 64) * 2.0 ** -50


def kernel_constants():
    """MT_SLICE (samples of one workgroup slice) and MT_MAX_GRID (the grid cap) of csrc/k_metrics.h."""
    src = open(os.path.join(ROOT, "sparrowrecsys_amd", "csrc", "k_metrics.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(MT_SLICE|MT_MAX_GRID|MT_THREADS)\s+(\d+)", src)}
