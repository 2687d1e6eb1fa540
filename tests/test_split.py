"""The held-out split's definition, featureeng.split_host: the draw against a restatement in Python integers
and its pins, the thresholds, the partition's properties, time mode against an independent np.sort, the shares as a condition, every
error, and the ctypes mirror of the take's column descriptor.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import featureeng as FE
from tests import split_cases as K
from tests.conftest import ROOT


def test_pins_and_the_restatement():
    for (seed, stream, key), u in K.PINS.items():
        assert K.draw(seed, stream, key) == u
        assert int(FE.split_draws(seed, np.array([key], dtype=np.int64), stream)[0]) == u
    rng = np.random.default_rng(3)
    keys = np.concatenate([rng.integers(0, 1 << 62, 300, dtype=np.int64), [0, 1, (1 << 31) - 2, (1 << 63) - 1]])
    for seed in (0, 1, (1 << 64) - 1, (1 << 63) + 7, 987654321):
        for stream in (0, 1):
            got = FE.split_draws(seed, keys, stream)
            assert got.dtype == np.uint64 and got.tolist() == [K.draw(seed, stream, int(k)) for k in keys]
            assert int(got.max()) < 1 << 53
    assert FE.split_draws(5, np.arange(10, dtype=np.int32), 1).tolist() == FE.split_draws(5, np.arange(10, dtype=np.int64), 1).tolist()


def test_thresholds():
    for f, t in K.THRESHOLDS.items():
        assert FE.split_threshold(f) == t
    assert FE.split_threshold(math.nextafter(1.0, 0.0)) == (1 << 53) - 1 and FE.split_threshold(5e-324) == 0
    for bad in (-0.1, 1.0000001, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            FE.split_threshold(bad)


def _by_key(part):
    order = np.argsort(part["source_row"], kind="stable")
    return {k: v[order] for k, v in part.items()}


def _same_part(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("mode", ["random", "time"])
@pytest.mark.parametrize("ts", ["random", "ties"])
def test_partition_properties(mode, ts):
    n = 5000
    cols = K.columns(n, seed=4, ts=ts)
    res = FE.split_host(cols, mode=mode, sample=0.3, train=0.8, seed=9)
    sampled = FE.split_draws(9, cols["source_row"], 0) < np.uint64(FE.split_threshold(0.3))
    assert res.n_sampled == int(sampled.sum()) == len(res.train["userId"]) + len(res.test["userId"]) and 0 < len(res.test["userId"]) < len(res.train["userId"])
    # the union is the sampled rows, the parts are disjoint, both are in input order; every column is cut alike
    position = np.empty(n, dtype=np.int64)
    position[cols["source_row"]] = np.arange(n)                               # (source_row is a permutation here: it names the row)
    at_train, at_test = position[res.train["source_row"]], position[res.test["source_row"]]
    assert (np.diff(at_train) > 0).all() and (np.diff(at_test) > 0).all()
    assert np.array_equal(np.sort(np.concatenate([at_train, at_test])), np.flatnonzero(sampled))
    for part, at in ((res.train, at_train), (res.test, at_test)):
        assert list(part) == list(cols)
        for k in cols:
            assert part[k].dtype == cols[k].dtype and part[k].tobytes() == cols[k][at].tobytes(), k
    # a permutation of the input rows changes nothing but the order
    perm = np.random.default_rng(1).permutation(n)
    other = FE.split_host({k: v[perm] for k, v in cols.items()}, mode=mode, sample=0.3, train=0.8, seed=9)
    assert other.n_sampled == res.n_sampled and other.split_timestamp == res.split_timestamp
    _same_part(_by_key(other.train), _by_key(res.train))
    _same_part(_by_key(other.test), _by_key(res.test))
    # appended rows: the earlier rows are sampled or not as before, and in random mode keep their side
    more = K.columns(n + 700, seed=5, ts=ts)
    more["source_row"] = np.concatenate([cols["source_row"], np.arange(n, n + 700, dtype=np.int32)])
    grown = FE.split_host(more, mode=mode, sample=0.3, train=0.8, seed=9)
    old = lambda part: np.sort(part["source_row"][part["source_row"] < n])
    assert np.array_equal(np.sort(np.concatenate([old(grown.train), old(grown.test)])), np.sort(cols["source_row"][sampled]))
    if mode == "random":
        assert np.array_equal(old(grown.train), np.sort(res.train["source_row"])) and np.array_equal(old(grown.test), np.sort(res.test["source_row"]))
        assert res.split_timestamp is None


def test_key_none_is_the_position_and_other_seeds_differ():
    cols = K.columns(3000, seed=2, key="ordered")
    a, b = FE.split_host(cols, seed=3), FE.split_host(cols, seed=3, key=None)
    _same_part(a.train, b.train)
    _same_part(a.test, b.test)
    c = FE.split_host(dict(cols, source_row=cols["source_row"][::-1].copy()), seed=3, key=None)
    assert c.train["userId"].tobytes() == a.train["userId"].tobytes()       # (only the position counts: the key column is not read)
    assert FE.split_host(cols, seed=4).train["source_row"].tolist() != a.train["source_row"].tolist()
    wide = K.columns(3000, seed=2, key="wide")
    w = FE.split_host(wide, seed=3)
    keep = FE.split_draws(3, wide["source_row"], 0) < np.uint64(K.THRESHOLDS[0.1])
    assert w.n_sampled == int(keep.sum()) > 0 and w.train["source_row"].dtype == np.int64


@pytest.mark.parametrize("ts", ["random", "ties", "equal", "bit63", "top_byte", "low_byte", "extremes"])
@pytest.mark.parametrize("sample,train", [(0.1, 0.8), (1.0, 0.8), (0.5, 0.33), (1.0, 0.0), (1.0, 1.0)])
def test_time_mode_against_np_sort(ts, sample, train):
    n = 4000
    cols = K.columns(n, seed=6, ts=ts)
    res = FE.split_host(cols, mode="time", sample=sample, train=train, seed=1)
    sampled = np.array([K.draw(1, 0, int(k)) < FE.split_threshold(sample) for k in cols["source_row"]])
    m = int(sampled.sum())
    assert res.n_sampled == m > 0
    ordered = np.sort(cols["timestamp"][sampled])
    r = math.ceil(float(train) * float(m))
    assert res.split_timestamp == int(ordered[max(r, 1) - 1])
    assert (res.train["timestamp"] <= res.split_timestamp).all() and (res.test["timestamp"] > res.split_timestamp).all()
    assert len(res.train["timestamp"]) == int((ordered <= res.split_timestamp).sum()) >= max(r, 1)
    # Spark's own tolerance: the value's rank range meets train * m +- 0.05 m
    lo, hi = int(np.searchsorted(ordered, res.split_timestamp, "left")) + 1, int(np.searchsorted(ordered, res.split_timestamp, "right"))
    assert lo - 0.05 * m <= max(train * m, 1) <= hi + 0.05 * m


def test_time_mode_two_values_and_one_sampled_row():
    n = 1000                                                                 # sample = 1: r = 800, the rank is position 799
    for n_low, want in ((800, 100), (799, 200), (1000, 100), (0, 200)):
        cols = K.columns(n, seed=7)
        cols["timestamp"] = K.two_values(n, n_low)
        res = FE.split_host(cols, mode="time", sample=1.0, train=0.8)
        assert res.split_timestamp == want and len(res.train["label"]) == (n_low if want == 100 else n)
    cols = K.columns(40, seed=8)
    seed = next(s for s in range(200) if FE.split_host(cols, mode="time", sample=0.03, seed=s).n_sampled == 1)
    res = FE.split_host(cols, mode="time", sample=0.03, seed=seed)
    assert len(res.train["label"]) == 1 and len(res.test["label"]) == 0 and res.split_timestamp == int(res.train["timestamp"][0])


def test_empty_parts():
    cols = K.columns(500, seed=9)
    for mode in ("random", "time"):
        none = FE.split_host(cols, mode=mode, sample=0.0)
        assert none.n_sampled == 0 and none.split_timestamp is None and len(none.train["label"]) == 0 == len(none.test["label"])
        assert none.train["timestamp"].dtype == np.int64 and list(none.test) == list(cols)
        full = FE.split_host(cols, mode=mode, sample=1.0, train=1.0)
        assert full.n_sampled == 500 == len(full.train["label"]) and len(full.test["label"]) == 0
        _same_part(full.train, cols)
        empty = FE.split_host(K.columns(0), mode=mode)
        assert empty.n_sampled == 0 and empty.split_timestamp is None and len(empty.train["label"]) == 0
    assert len(FE.split_host(cols, sample=1.0, train=0.0).test["label"]) == 500
    low = FE.split_host(cols, mode="time", sample=1.0, train=0.0)            # r = 0: the earliest timestamp, and its ties, are training
    assert low.split_timestamp == int(cols["timestamp"].min()) and len(low.train["label"]) == int((cols["timestamp"] == cols["timestamp"].min()).sum())


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 7])
def test_shares(seed):
    """n = 200 000, keys = the positions: both shares within four standard deviations of the binomial.  The definition gives -0.04, -1.10,
    -0.41, -0.09, +0.07 sigma for the sample and -1.52, -1.32, -0.44, +0.31, +1.10 sigma for the training share at these seeds."""
    n = 200_000
    res = FE.split_host({"source_row": np.arange(n, dtype=np.int32)}, seed=seed)
    n_train = len(res.train["source_row"])
    assert abs(res.n_sampled - 0.1 * n) <= 4 * math.sqrt(n * 0.1 * 0.9)
    assert abs(n_train - 0.8 * res.n_sampled) <= 4 * math.sqrt(res.n_sampled * 0.8 * 0.2)
    print("seed %d: %+.2f sigma, %+.2f sigma" % (seed, (res.n_sampled - 0.1 * n) / math.sqrt(n * 0.09), (n_train - 0.8 * res.n_sampled) / math.sqrt(res.n_sampled * 0.16)))


def test_errors():
    cols = K.columns(100, seed=1)
    for kw in ({"sample": -0.01}, {"sample": 1.01}, {"train": float("nan")}, {"train": float("inf")}, {"sample": float("nan")}, {"train": -1.0}, {"train": 2.0}):
        with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
            FE.split_host(cols, **kw)
    with pytest.raises(ValueError, match="mode"):
        FE.split_host(cols, mode="stratified")
    no_ts = {k: v for k, v in cols.items() if k != "timestamp"}
    with pytest.raises(ValueError, match="int64 timestamp"):
        FE.split_host(no_ts, mode="time")
    with pytest.raises(ValueError, match="int64 timestamp"):
        FE.split_host(dict(cols, timestamp=cols["timestamp"].astype(np.int32)), mode="time")
    assert FE.split_host(no_ts).n_sampled >= 0                                # (random mode needs no timestamp)
    with pytest.raises(ValueError, match="no key column"):
        FE.split_host({k: v for k, v in cols.items() if k != "source_row"})
    with pytest.raises(ValueError, match="no key column"):
        FE.split_host(cols, key="row_id")
    bad = dict(cols, source_row=cols["source_row"].copy())
    bad["source_row"][[17, 60]] = -1
    with pytest.raises(ValueError, match="row 17: negative key"):
        FE.split_host(bad)
    with pytest.raises(ValueError, match="integers"):
        FE.split_host(cols, key="rating")
    with pytest.raises(ValueError, match="differ in length"):
        FE.split_host(dict(cols, label=cols["label"][:-1]))

    class Long:                                                               # a column of 2^31 - 1 rows, of which only the length is asked
        shape, ndim, dtype = ((1 << 31) - 1,), 1, np.dtype(np.int32)
    with pytest.raises(ValueError, match="at most 2\\^31 - 2 rows"):
        FE._split_rows({"source_row": Long()}, "random", "source_row", lambda a: a.dtype.name)


def test_split_device_names_the_host_definition_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError, match="split_host"):
        FE.split_device(K.columns(10))
    with pytest.raises(ValueError, match="mode"):                              # (the arguments are checked first, as on the host)
        FE.split_device(K.columns(10), mode="x")


def test_matrix_groups():
    """Adjacent columns of one row-major matrix form a group, in dict order only, never wider than the matrix; everything else stands alone."""
    import torch
    m, v = torch.zeros((6, 4), dtype=torch.int32), torch.zeros(6, dtype=torch.int32)
    f = torch.zeros((6, 3), dtype=torch.float32)
    cols = {"a": v, "m0": m[:, 0], "m1": m[:, 1], "m2": m[:, 2], "b": v.clone(), "m3": m[:, 3], "f1": f[:, 1], "f2": f[:, 2], "f0": f[:, 0], "t": m[:, 1]}
    assert FE._matrix_groups(cols) == [["a"], ["m0", "m1", "m2"], ["b"], ["m3"], ["f1", "f2"], ["f0"], ["t"]]
    wide = torch.zeros(12, dtype=torch.int32)
    overlap = {"x%d" % k: wide.as_strided((5,), (2,), k) for k in range(3)}      # a stride of 2 holds rows of two words, not three
    assert FE._matrix_groups(overlap) == [["x0", "x1"], ["x2"]]
    assert FE._matrix_groups({}) == []


def test_split_col_mirror_and_argument_checks(lib):
    header = open(os.path.join(ROOT, "include", "sparrow_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} sprk_split_col;", header).group(1)
    fields = [(t.strip(), name) for t, name in re.findall(r"^\s*([a-z0-9_ ]+?\*?)\s*([a-z_]+);", body, re.M)]
    ctype = {"const void*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [(ctype[t], name) for t, name in fields] == [(t, name) for name, t in L.SplitCol._fields_]
    assert C.sizeof(L.SplitCol) == 32 and [getattr(L.SplitCol, name).offset for name, _ in L.SplitCol._fields_] == [0, 8, 16, 20, 24]
    # the checks that come before any device call
    assert lib.sprk_split_plan_workspace_bytes(-1) == 0 and lib.sprk_split_plan_workspace_bytes((1 << 31) - 1) == 0
    sizes = [lib.sprk_split_plan_workspace_bytes(n) for n in (0, 1, 1024, 1025, 1 << 20)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[3] > sizes[2]
    words = (C.c_int64 * 5)(-1, 0, 0, 0, 0)
    plan = lambda **kw: lib.sprk_split_plan(*[kw.get(k, v) for k, v in (("key", None), ("key_kind", 0), ("ts", None), ("n", 0), ("seed", 0), ("t_sample", 1 << 53),
                                                                          ("t_train", 1 << 53), ("train", 0.8), ("mode", 0), ("i0", None), ("i1", None),
                                                                          ("words", C.cast(words, C.c_void_p)), ("ws", None), ("ws_bytes", 0), ("stream", None))])
    for kw, text in (({"n": -1}, b"bad size"), ({"mode": 2}, b"mode"), ({"key_kind": 3}, b"key_kind"), ({"t_sample": (1 << 53) + 1}, b"threshold"), ({"train": 1.5}, b"train"),
                     ({"train": float("nan")}, b"train"), ({"words": None}, b"NULL words"), ({"n": 5, "key_kind": 1}, b"NULL key"), ({"n": 5, "mode": 1}, b"timestamp"),
                     ({"n": 5}, b"NULL index"), ({"words": C.c_void_p(C.addressof(words) + 4)}, b"misaligned"), ({}, b"workspace")):
        assert plan(**kw) == L.EINVAL and text in lib.sprk_last_error(), (kw, lib.sprk_last_error())
    col = lambda **kw: (L.SplitCol * 1)(L.SplitCol(kw.get("src", 64), kw.get("stride", 4), kw.get("row", 4), 0, kw.get("dst", 64)))
    take = lambda c, n_cols=1, index=64, n_index=3, n_rows=3: lib.sprk_take_rows(c, n_cols, C.c_void_p(index), n_index, n_rows, None)
    for args, text in (((col(row=6),), b"row_bytes"), ((col(row=0),), b"row_bytes"), ((col(stride=-4),), b"src_stride"), ((col(stride=6),), b"src_stride"),
                       ((col(src=None),), b"NULL source"), ((col(dst=66),), b"misaligned"), ((col(), 1, 0), b"NULL index"), ((col(), 1, 66), b"misaligned index"),
                       ((col(), -1), b"n_cols"), ((None, 1), b"n_cols"), ((col(), 1, 64, -1), b"bad sizes"), ((col(), 1, 64, 3, 1 << 31), b"bad sizes")):
        assert take(*args) == L.EINVAL and text in lib.sprk_last_error(), (text, lib.sprk_last_error())
    assert take(col(), 1, 64, 0) == 0 and take(col(), 0) == 0                 # nothing to take: no device call
