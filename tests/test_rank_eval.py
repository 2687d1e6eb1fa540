"""Ranking metrics, the host definition (sparrowrecsys_amd/rankeval.py): Spark's documented example, rank_eval_host against Spark's loops
transcribed over Python sets, the properties the rules promise, the error kinds, and every argument check of the C ABI -- all without a
device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import rankeval as RE
from tests import rank_eval_cases as K

P, R_, N, AP, HIT, RR = RE.PRECISION, RE.RECALL, RE.NDCG, RE.AP, RE.HIT, RE.RR


def test_gain_table():
    gain, gain_sum = RE.gain_table()
    assert gain.shape == (1024,) and gain_sum.shape == (1025,) and gain.dtype == gain_sum.dtype == np.float64
    assert gain[0] == 1.0 / np.log(2.0) and gain_sum[0] == 0.0 and gain_sum[1] == gain[0] and gain_sum[3] == (gain[0] + gain[1]) + gain[2]


def test_sparks_documented_example():
    """The example of Spark's RankingMetrics documentation and test suite: three lists, the third user without truth."""
    pred = np.full((3, 10), -1, dtype=np.int32)
    pred[0] = [1, 6, 2, 7, 8, 3, 9, 10, 4, 5]
    pred[1] = [4, 1, 5, 6, 2, 7, 3, 8, 9, 10]
    pred[2, :5] = [1, 2, 3, 4, 5]
    tu = np.array([0] * 5 + [1] * 3, dtype=np.int32)
    ti = np.array([1, 2, 3, 4, 5, 1, 2, 3], dtype=np.int32)
    ks = (1, 2, 3, 4, 5, 10, 15)
    res = RE.rank_eval_host(pred, None, tu, ti, n_users=3, ks=ks)
    m = {k: row for k, row in zip(ks, res.mean("all"))}
    want = {P: {1: 1 / 3, 2: 1 / 3, 3: 1 / 3, 4: 0.25, 5: 0.266667, 10: 0.266667, 15: 0.177778},
            R_: {1: 0.066667, 2: 0.177778, 5: 0.355556, 10: 0.666667},
            N: {3: 1 / 3, 5: 0.328788, 10: 0.487913, 15: 0.487913},
            AP: {1: 1 / 3, 2: 0.25, 10: 0.355026},
            RR: {2: 0.5, 3: 0.5, 10: 0.5, 15: 0.5}}
    for metric, by_k in want.items():
        for k, v in by_k.items():
            assert abs(m[k][metric] - v) <= 1e-6, (RE.METRICS[metric], k, m[k][metric], v)
    assert res.counts.tolist() == [3, 2] and res.n_relevant.tolist() == [5, 3, 0] and res.n_ranked.tolist() == [10, 10, 5]
    assert (res.per_query[2] == 0.0).all() and not np.signbit(res.per_query[2]).any()
    assert np.array_equal(res.mean("truth"), res.sums / 2.0) and np.array_equal(res.mean("all"), res.sums / 3.0)
    with pytest.raises(ValueError, match="over"):
        res.mean("some")


@pytest.mark.parametrize("kw,ks", [
    (dict(), (1, 5, 10, 20, 21, 1024)),
    (dict(Q=300, Lp=7, users="identity", seed=1), (3,)),
    (dict(Q=513, Lp=33, n_users=50, n_items=40, per_truth=12, per_seen=25, seed=2, users="beyond"), (1, 2, 3, 5, 8, 13, 33, 34)),
    (dict(Q=64, Lp=130, n_items=100, per_truth=70, per_seen=0, seed=3), (64, 65, 70, 71, 130, 131)),
])
def test_the_definition_equals_sparks_loops_over_sets(kw, ks):
    c = K.case(**kw)
    res = RE.rank_eval_host(ks=ks, **c)
    per_query, n_relevant, n_ranked = K.spark_per_query(c["pred"], c["query_user"], c["truth_user"], c["truth_item"], c["seen_user"], c["seen_item"], ks)
    assert res.per_query.tobytes() == per_query.tobytes()
    assert res.n_relevant.tobytes() == n_relevant.tobytes() and res.n_ranked.tobytes() == n_ranked.tobytes()
    assert res.sums.tobytes() == K.chunked_sums(per_query).tobytes()
    assert res.counts.tolist() == [len(per_query), int((n_relevant > 0).sum())]
    assert res.per_query.dtype == np.float64 and res.n_relevant.dtype == np.int32 and res.counts.dtype == np.int64
    assert (n_relevant > 0).any() and (n_relevant == 0).any() and (n_ranked < c["pred"].shape[1]).any()


def test_row_order_does_not_matter_and_no_seen_is_an_empty_seen():
    c = K.case(Q=100, seed=4)
    ks = (1, 10, 20)
    want = RE.rank_eval_host(ks=ks, **c)
    rng = np.random.default_rng(0)
    t, s = rng.permutation(len(c["truth_user"])), rng.permutation(len(c["seen_user"]))
    moved = dict(c, truth_user=c["truth_user"][t], truth_item=c["truth_item"][t], seen_user=c["seen_user"][s], seen_item=c["seen_item"][s])
    K.same(RE.rank_eval_host(ks=ks, **moved), want)
    none = dict(c, seen_user=None, seen_item=None)
    empty = dict(c, seen_user=np.zeros(0, np.int32), seen_item=np.zeros(0, np.int32))
    K.same(RE.rank_eval_host(ks=ks, **none), RE.rank_eval_host(ks=ks, **empty))
    assert RE.rank_eval_host(ks=ks, **none).n_ranked.sum() > want.n_ranked.sum()


def test_a_perfect_list_duplicate_truth_rows_and_seen_truth():
    truth = [7, 3, 11, 5]
    tu, ti = np.zeros(4, np.int32), np.array(truth, np.int32)
    perfect = RE.rank_eval_host(np.array([truth + [20, 21]], np.int32), None, tu, ti, n_users=1, ks=(2, 4, 6))
    assert (perfect.per_query[0, :, N] == 1.0).all() and (perfect.per_query[0, :, AP] == 1.0).all() and perfect.per_query[0, :, R_].tolist() == [0.5, 1.0, 1.0]
    # duplicate truth rows: the same R, the same bytes
    twice = RE.rank_eval_host(np.array([truth + [20, 21]], np.int32), None, np.zeros(8, np.int32), np.array(truth + truth, np.int32), n_users=1, ks=(2, 4, 6))
    K.same(twice, perfect)
    # item 3 is truth and seen: it stays in T (R = 4) and leaves the list, so the entries behind it move up
    res = RE.rank_eval_host(np.array([[7, 3, 11, 20]], np.int32), None, tu, ti, np.zeros(1, np.int32), np.array([3], np.int32), n_users=1, ks=(2,))
    assert res.n_relevant.tolist() == [4] and res.n_ranked.tolist() == [3]
    assert res.per_query[0, 0].tolist()[:2] == [1.0, 0.5] and res.per_query[0, 0, N] == 1.0
    # -1 in the middle is no entry: the list behind it moves up; a duplicate entry counts each time
    res = RE.rank_eval_host(np.array([[20, -1, 7, -5, 7]], np.int32), None, tu, ti, n_users=1, ks=(2, 3))
    assert res.n_ranked.tolist() == [3] and res.per_query[0, :, P].tolist() == [0.5, 2 / 3] and res.per_query[0, 0, RR] == 0.5
    gain, gain_sum = RE.gain_table()
    assert res.per_query[0, 1, N] == (gain[1] + gain[2]) / gain_sum[3] and res.per_query[0, 1, AP] == (1 / 2 + 2 / 3) / 3.0


def test_every_error_kind_names_the_smallest_failing_row():
    c = K.case(Q=30, seed=5)
    def broken(**rows):
        d = {k: (None if v is None else np.array(v)) for k, v in c.items() if k != "n_users"}
        for name, (at, value) in rows.items():
            d[name][at] = value
        return dict(d, n_users=c["n_users"])
    n = c["n_users"]
    for rows, kind, row in ((dict(truth_user=([9, 4], n)), 1, 4), (dict(truth_item=([9, 5], -1), truth_user=([7], -1)), 1, 5),
                            (dict(seen_user=([3], -2)), 2, 3), (dict(seen_item=([12, 2], -1)), 2, 2), (dict(query_user=([29, 8], n)), 3, 8),
                            (dict(query_user=([0], -1), seen_item=([6], -1)), 2, 6), (dict(query_user=([0], -1), seen_item=([6], -1), truth_user=([20], n + 5)), 1, 20)):
        with pytest.raises(ValueError, match=r"error kind %d, .* %d\b" % (kind, row)):
            RE.rank_eval_host(ks=(5,), **broken(**rows))
    with pytest.raises(ValueError, match="error kind 3, query 3:"):          # query_user None: query q is user q's, and there is no user 3
        RE.rank_eval_host(np.zeros((5, 2), np.int32), None, np.zeros(0, np.int32), np.zeros(0, np.int32), n_users=3)


def test_python_layer_value_errors():
    pred = np.zeros((2, 3), np.int32)
    e = np.zeros(0, np.int32)
    for ks in ((), (0,), (1025,), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="cut-offs|outside"):
            RE.rank_eval_host(pred, None, e, e, ks=ks)
    with pytest.raises(ValueError, match="pred must be"):
        RE.rank_eval_host(np.zeros((2, 0), np.int32), None, e, e)
    with pytest.raises(ValueError, match="go together"):
        RE.rank_eval_host(pred, None, e, None)
    with pytest.raises(ValueError, match="gain must be"):
        RE.rank_eval_host(pred, None, e, e, gain=np.zeros(10), gain_sum=np.zeros(11))
    with pytest.raises(ValueError, match="query_user must be"):
        RE.rank_eval_host(pred, np.zeros(3, np.int32), e, e)


def test_the_cpu_device_is_the_definition_and_no_device_raises(tmp_path):
    import torch
    c = K.case(Q=50, seed=6)
    K.same(RE.rank_eval_device(ks=(3, 10), device="cpu", **c), RE.rank_eval_host(ks=(3, 10), **c))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a HIP device: no HIP device is visible"):
            RE.rank_eval_device(ks=(3, 10), **c)
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            RE.evaluate(c["pred"], None, {"userId": [0], "movieId": [0], "rating": [4.0]})
    # evaluate: the truth is the test rows with rating >= min_rating; train becomes seen; a CSV path is read
    rating = np.where(np.arange(len(c["truth_user"])) % 3 == 0, 3.0, 4.0).astype(np.float32)
    test = {"userId": c["truth_user"], "movieId": c["truth_item"], "rating": rating}
    train = {"userId": torch.from_numpy(c["seen_user"]), "movieId": torch.from_numpy(c["seen_item"])}
    want = RE.rank_eval_host(c["pred"], c["query_user"], c["truth_user"][rating >= 3.5], c["truth_item"][rating >= 3.5], c["seen_user"], c["seen_item"], c["n_users"], (5,))
    K.same(RE.evaluate(c["pred"], c["query_user"], test, train, ks=(5,), n_users=c["n_users"], device="cpu"), want)
    path = tmp_path / "test.csv"
    path.write_text("userId,movieId,rating,timestamp\n" + "".join("%d,%d,%.1f,0\n" % row for row in zip(c["truth_user"], c["truth_item"], rating)))
    K.same(RE.evaluate(c["pred"], c["query_user"], str(path), train, ks=(5,), n_users=c["n_users"], device="cpu"), want)
    low = RE.evaluate(c["pred"], c["query_user"], test, train, ks=(5,), min_rating=0.0, n_users=c["n_users"], device="cpu")
    assert low.n_relevant.sum() > want.n_relevant.sum()


def test_lists_as_truth_gives_recall_against_exact_lists():
    import torch
    exact = np.array([[4, 9, 2], [7, 1, -1], [5, 5, 6]], dtype=np.int32)
    approx = np.array([[9, 4, 8], [3, 3, 3], [6, -1, 5]], dtype=np.int32)
    tu, ti = RE.lists_as_truth(exact)
    assert tu.tolist() == [0, 0, 0, 1, 1, 2, 2, 2] and ti.tolist() == [4, 9, 2, 7, 1, 5, 5, 6] and tu.dtype == ti.dtype == np.int32
    res = RE.rank_eval_host(approx, None, tu, ti, n_users=3, ks=(3,))
    assert res.per_query[:, 0, R_].tolist() == [2 / 3, 0.0, 1.0] and res.n_relevant.tolist() == [3, 2, 2]
    du, di = RE.lists_as_truth(torch.from_numpy(exact))
    assert du.numpy().tobytes() == tu.tobytes() and di.numpy().tobytes() == ti.tobytes()


# ---------------------------------------------------------------- the C ABI

def test_header_exports_and_prototypes_agree(lib):
    header = open(os.path.join(L.INCLUDE_DIR, "sparrow_hip.h")).read()
    for name, n_args in (("sprk_rank_eval_workspace_bytes", 4), ("sprk_rank_eval", 25)):
        proto = re.search(r"^\w+ %s\(([^;]*)\);" % name, header, re.M | re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == n_args == len(getattr(lib, name).argtypes)
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.sprk_rank_eval_workspace_bytes.restype is C.c_size_t and lib.sprk_rank_eval.restype is C.c_int
    exports = open(os.path.join(os.path.dirname(L.SRC_PATH), "exports.map")).read()
    assert "sprk_*" in exports


def _abi(lib, n_truth=40, n_seen=50, n_users=9, Q=6, Lp=12):
    """The entry point over host memory that stands in for device memory: every refused call returns before it touches any."""
    need = lib.sprk_rank_eval_workspace_bytes(n_truth, n_seen, n_users, Q)
    buf = (C.c_uint64 * (need // 8 + 4096))()
    p = C.c_void_p(C.addressof(buf))
    def call(**kw):
        a = dict(pred=p, Q=Q, Lp=Lp, stride=Lp, qu=p, tu=p, ti=p, n_truth=n_truth, su=p, si=p, n_seen=n_seen, n_users=n_users, ks=(10,), n_ks=None, gain=p, gain_sum=p,
                 per_query=p, n_relevant=p, n_ranked=p, sums=p, counts=p, err=p, ws=p, ws_bytes=need)
        a.update(kw)
        ks = None if a["ks"] is None else (C.c_int32 * max(len(a["ks"]), 1))(*a["ks"])
        n_ks = len(a["ks"]) if a["n_ks"] is None else a["n_ks"]
        return lib.sprk_rank_eval(a["pred"], a["Q"], a["Lp"], a["stride"], a["qu"], a["tu"], a["ti"], a["n_truth"], a["su"], a["si"], a["n_seen"], a["n_users"], ks, n_ks,
                                  a["gain"], a["gain_sum"], a["per_query"], a["n_relevant"], a["n_ranked"], a["sums"], a["counts"], a["err"], a["ws"], a["ws_bytes"], None)
    return need, (lambda k: C.c_void_p(C.addressof(buf) + k)), call


def test_rank_eval_abi_rejects_bad_arguments_before_any_device_call(lib):
    need, off, call = _abi(lib)
    assert need > 0 and need % 16 == 0
    for sizes in ((-1, 0, 1, 1), (0, -1, 1, 1), (2**31 - 1, 0, 1, 1), (0, 2**31 - 1, 1, 1), (0, 0, -1, 1), (0, 0, 2**31 - 1, 1), (0, 0, 1, -1)):
        assert lib.sprk_rank_eval_workspace_bytes(*sizes) == 0, sizes
    assert lib.sprk_rank_eval_workspace_bytes(0, 0, 0, 0) > 0
    table = [dict(Lp=0, stride=0), dict(Lp=-1), dict(Lp=65537, stride=65537), dict(n_ks=0), dict(ks=tuple(range(1, 10))), dict(ks=None, n_ks=1), dict(ks=(0,)), dict(ks=(5, 1025)),
             dict(ks=(-3,)), dict(stride=11), dict(ws_bytes=need - 16), dict(ws_bytes=0), dict(ws=None), dict(ws=off(8)), dict(per_query=None), dict(n_relevant=None),
             dict(n_ranked=None), dict(sums=None), dict(counts=None), dict(err=None), dict(pred=None), dict(gain=None), dict(gain_sum=None), dict(tu=None), dict(ti=None),
             dict(su=None), dict(si=None), dict(n_truth=-1), dict(n_seen=2**31 - 1), dict(n_users=-1), dict(Q=-1), dict(per_query=off(4)), dict(sums=off(4)), dict(counts=off(4)),
             dict(err=off(4)), dict(gain=off(4)), dict(gain_sum=off(4)), dict(pred=off(2)), dict(qu=off(2)), dict(tu=off(1)), dict(ti=off(2)), dict(su=off(2)), dict(si=off(3)),
             dict(n_relevant=off(2)), dict(n_ranked=off(2))]
    for kw in table:
        assert call(**kw) == L.EINVAL, kw
        assert b"rank_eval: " in lib.sprk_last_error()
    assert call(ws_bytes=need - 16) == L.EINVAL
    assert ("needs a workspace of %d bytes (sprk_rank_eval_workspace_bytes)" % need).encode() in lib.sprk_last_error()
    assert call(ks=(5, 1025)) == L.EINVAL and b"ks[1] = 1025" in lib.sprk_last_error()
    import torch
    if not torch.cuda.is_available():                               # a good call reaches the device, and there is none
        assert call() == L.EHIP and call(ks=(1, 2, 3, 4, 5, 6, 7, 1024)) == L.EHIP and call(qu=None) == L.EHIP and call(stride=40) == L.EHIP
        assert call(n_seen=0, su=None, si=None) == L.EHIP and call(n_truth=0, tu=None, ti=None) == L.EHIP
        assert call(Q=0, pred=None, per_query=None, n_relevant=None, n_ranked=None) == L.EHIP          # (sums and counts are still written)
