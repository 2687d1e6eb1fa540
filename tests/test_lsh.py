"""Embedding LSH, the host definition (sparrowrecsys_amd/lsh.py): a hand-worked example, hash_host and approx_nearest_host against a brute
force over Python floats and sets, the count / pad convention, the edge rows, and every argument check of the C ABI and of the Python
layer -- all without a device."""
import ctypes as C
import math

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import lsh
from tests import lsh_cases as K


def test_hand_worked_example():
    assert lsh.hash_host(K.HAND_EMB, K.HAND_VECTORS, K.HAND_LENGTH).tolist() == K.HAND_BUCKETS
    dist, rows, count = lsh.approx_nearest_host(K.HAND_EMB, None, K.HAND_VECTORS, K.HAND_LENGTH, K.HAND_QUERIES, K.HAND_K)
    assert rows.tolist() == K.HAND_ROWS and count.tolist() == K.HAND_COUNT
    K.same((dist, rows, count), (np.array(K.HAND_DIST), np.array(K.HAND_ROWS, np.int32), np.array(K.HAND_COUNT, np.int32)))
    assert dist.dtype == np.float64 and rows.dtype == np.int32 and count.dtype == np.int32
    everything = lsh.approx_nearest_host(K.HAND_EMB, None, K.HAND_VECTORS, K.HAND_LENGTH, K.HAND_QUERIES[:1], 5)
    assert everything[1].tolist() == [K.HAND_ALL_ROWS_QUERY0]
    assert everything[0][0].tolist() == [0.25, 0.25, 1.0, math.sqrt(1.25), math.sqrt(1.625)]
    K.same((dist, rows, count), K.brute_force(K.HAND_EMB, None, K.HAND_VECTORS, K.HAND_LENGTH, K.HAND_QUERIES, K.HAND_K))


def test_hash_host_equals_the_plain_loop():
    emb = K.table(200, 7)
    for T, length in ((3, 0.1), (1, 2.0), (16, 0.013)):
        vec = lsh.random_unit_vectors(7, T, seed=T)
        got = lsh.hash_host(emb, vec, length)
        assert got.dtype == np.int64 and got.shape == (200, T)
        assert got.tolist() == K.loop_hash(emb, vec, length).tolist()
    assert len(np.unique(lsh.hash_host(emb, lsh.random_unit_vectors(7, 3), 0.1))) > 30


@pytest.mark.parametrize("n,D,T,length,k", [(300, 7, 3, 0.1, 5), (300, 7, 1, 0.5, 40), (500, 3, 16, 0.05, 7), (400, 10, 3, 2.0, 300)])
def test_approx_nearest_host_equals_the_brute_force(n, D, T, length, k):
    emb = K.table(n, D)
    rng = np.random.default_rng(1)
    has, qh = (rng.random(n) >= 0.1).astype(np.uint8), (rng.random(60) >= 0.1).astype(np.uint8)
    vec = lsh.random_unit_vectors(D, T, seed=2)
    queries = np.concatenate([emb[:40], K.table(20, D, seed=3)])
    got = lsh.approx_nearest_host(emb, has, vec, length, queries, k, qh)
    K.same(got, K.brute_force(emb, has, vec, length, queries, k, qh))
    assert (got[2][qh == 0] == 0).all() and (got[1][qh == 0] == -1).all() and got[2].max() > 0
    rows = got[1]
    assert all(has[r] for r in rows[rows >= 0].tolist())


def test_count_and_pad_convention():
    """n = 300, D = 7, T = 1, bucket_length 0.1, k = 6, the first 200 rows as queries: some queries have fewer than 6 candidates (NaN / -1
    past count), some more (count > k); a row is its own candidate at distance +0.0."""
    emb = K.table(300, 7)
    vec = lsh.random_unit_vectors(7, 1)
    dist, rows, count = lsh.approx_nearest_host(emb, None, vec, 0.1, emb[:200], 6)
    short, more = count < 6, count > 6
    assert short.any() and more.any() and (count >= 1).all()
    print("fewer than 6 candidates: %.1f %% of the queries" % (100.0 * short.mean()))
    for q in range(200):
        m = min(int(count[q]), 6)
        assert rows[q, 0] == q and dist[q, 0] == 0.0 and not np.signbit(dist[q, 0])
        assert (rows[q, m:] == -1).all() and (dist[q, m:].view(np.uint64) == 0x7ff8000000000000).all()
        assert (rows[q, :m] >= 0).all() and np.isfinite(dist[q, :m]).all() and (np.diff(dist[q, :m]) >= 0).all()
    K.same((dist, rows, count), K.brute_force(emb, None, vec, 0.1, emb[:200], 6))


def test_edge_rows_bucket_edges_clamp_subnormals_and_non_finite():
    emb, has, want = K.edge_rows()
    got = lsh.hash_host(emb, K.EDGE_VECTORS, K.EDGE_LENGTH)
    live = has != 0
    assert got[live].tolist() == want[live].tolist()
    assert got.tolist() == K.loop_hash(emb, K.EDGE_VECTORS, K.EDGE_LENGTH).tolist()
    # with r = e_0 and bucket_length 0.25, 0.5 lies exactly on an edge and opens bucket 2; -0.5 opens bucket -2
    one = lsh.hash_host(np.array([[0.5], [-0.5]], np.float32), np.array([[1.0]]), 0.25)
    assert one.tolist() == [[2], [-2]]
    assert lsh.hash_host(np.array([[1e30], [-1e30]], np.float32), np.array([[1.0]]), 0.1).tolist() == [[1 << 62], [-(1 << 62)]]
    assert lsh.hash_host(np.array([[3e38]], np.float32), np.array([[1.0]]), 1e-300).tolist() == [[1 << 62]]            # the quotient overflows: clamped, not NO_BUCKET
    assert lsh.hash_host(np.array([[3e38, 3e38]], np.float32), np.array([[1e300, 1e300]]), 1.0).tolist() == [[K.NO]]     # the dot overflows


def test_non_finite_rows_and_queries_and_rows_without_embedding():
    emb, has, _ = K.edge_rows()
    queries = np.concatenate([emb, np.array([[0.55, -0.45], [np.nan, np.nan]], np.float32)])
    qh = np.ones(len(queries), np.uint8)
    qh[0] = 0
    got = lsh.approx_nearest_host(emb, has, K.EDGE_VECTORS, K.EDGE_LENGTH, queries, 4, qh)
    K.same(got, K.brute_force(emb, has, K.EDGE_VECTORS, K.EDGE_LENGTH, queries, 4, qh))
    dist, rows, count = got
    bad = [i for i in range(len(emb)) if not np.isfinite(emb[i]).all()]
    assert len(bad) == 3 and not np.isin(rows, bad).any() and not np.isin(rows, np.flatnonzero(has == 0)).any()
    assert count[bad].tolist() == [0, 0, 0] and count[-1] == 0 and count[0] == 0
    # (0.55, -0.45) has buckets (2, -2): rows 0 and 13 by both tables (each counts once), 14 by table 0, 2 by table 1; row 12 has no embedding
    assert count[-2] == 4 and sorted(rows[-2].tolist()[:2]) == [0, 13] and rows[-2].tolist()[2:] == [2, 14]
    assert np.isfinite(dist[rows >= 0]).all()


def test_random_unit_vectors():
    """Unit norm to within 1 ulp at the widths in use (1, the reference's 10, the large table's 64).  The sum of squares is taken in index
    order, so its own rounding grows with D -- up to (D - 1) / 2 ulp of the norm, plus one for the square root and the division --: at
    D = 1024 that bound is what is asserted."""
    for D, T, ulps in ((1, 1, 1), (10, 3, 1), (64, 16, 1), (1024, 2, 1023 / 2 + 1)):
        v = lsh.random_unit_vectors(D, T, seed=5)
        assert v.shape == (T, D) and v.dtype == np.float64
        assert v.tobytes() == lsh.random_unit_vectors(D, T, seed=5).tobytes()
        norm = np.array([math.sqrt(math.fsum(x * x for x in row)) for row in v.tolist()])
        assert (np.abs(norm - 1.0) <= ulps * np.spacing(1.0)).all()
    assert lsh.random_unit_vectors(10, 3, seed=0).tobytes() != lsh.random_unit_vectors(10, 3, seed=1).tobytes()
    raw = np.random.default_rng(0).standard_normal((3, 10))
    assert np.allclose(lsh.random_unit_vectors(10, 3) * np.sqrt((raw * raw).sum(axis=1))[:, None], raw, rtol=1e-15, atol=0)


def test_python_layer_value_errors():
    emb, vec = K.table(20, 4), lsh.random_unit_vectors(4, 3)
    for length in (0.0, -0.1, math.inf, math.nan):
        with pytest.raises(ValueError, match="bucket_length"):
            lsh.hash_host(emb, vec, length)
        with pytest.raises(ValueError, match="bucket_length"):
            lsh.LSHIndex.build(emb, bucket_length=length, device="cpu")
    for bad_vec in (vec[:, :3], vec[0], np.zeros((17, 4)), np.zeros((0, 4))):
        with pytest.raises(ValueError, match="vectors"):
            lsh.hash_host(emb, bad_vec, 0.1)
    with pytest.raises(ValueError, match="emb"):
        lsh.hash_host(emb[0], vec, 0.1)
    with pytest.raises(ValueError, match="emb"):
        lsh.hash_host(np.zeros((3, 1025), np.float32), np.zeros((1, 1025)), 0.1)
    for k in (0, -1, 1025):
        with pytest.raises(ValueError, match="k = "):
            lsh.approx_nearest_host(emb, None, vec, 0.1, emb, k)
    with pytest.raises(ValueError, match="queries"):
        lsh.approx_nearest_host(emb, None, vec, 0.1, emb[:, :3], 2)
    with pytest.raises(ValueError, match="has"):
        lsh.approx_nearest_host(emb, np.ones(19, np.uint8), vec, 0.1, emb, 2)
    with pytest.raises(ValueError, match="has"):
        lsh.approx_nearest_host(emb, None, vec, 0.1, emb, 2, np.ones(3, np.uint8))
    for args in ((0, 3), (1025, 3), (4, 0), (4, 17)):
        with pytest.raises(ValueError):
            lsh.random_unit_vectors(*args)
    with pytest.raises(ValueError, match="has"):
        lsh.LSHIndex.build(emb, has=np.ones(19, np.uint8), device="cpu")
    index = lsh.LSHIndex.build(emb, device="cpu")
    with pytest.raises(ValueError, match="queries"):
        index.approx_nearest(emb[:, :3], 2)
    with pytest.raises(ValueError, match="k = "):
        index.approx_nearest(emb, 0)
    with pytest.raises(ValueError, match="query_has"):
        index.approx_nearest(emb, 2, query_has=np.ones(3, np.uint8))


def test_cpu_index_is_the_host_definition():
    emb = K.table(300, 10)
    has = (np.arange(300) % 7 != 0).astype(np.uint8)
    index = lsh.LSHIndex.build(emb, has, device="cpu")
    assert index.bucket_length == 0.1 and index.vectors.tobytes() == lsh.random_unit_vectors(10, 3, 0).tobytes()
    want = lsh.hash_host(emb, index.vectors, 0.1)
    want[has == 0] = K.NO
    assert index.buckets.tobytes() == want.tobytes()
    K.same(index.approx_nearest(emb[:50], 5), lsh.approx_nearest_host(emb, has, index.vectors, 0.1, emb[:50], 5))
    custom = lsh.LSHIndex.build(emb, vectors=K.HAND_VECTORS.repeat(5, axis=1), bucket_length=0.5, device="cpu")
    assert custom.T == 2 and custom.buckets.shape == (300, 2)


def test_index_without_a_device_raises():
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a HIP device: no HIP device is visible"):
            lsh.LSHIndex.build(K.table(20, 4))
    assert lsh.LSHIndex.build(K.table(20, 4), device="cpu").on_device is False


def _abi(lib, n=8, D=10, T=3, Q=4, K_=5):
    """The three entry points over host memory that stands in for device memory: every refused call returns before it touches any."""
    need = lib.sprk_lsh_build_workspace_bytes(n, T)
    buf = (C.c_uint64 * (need // 8 + 4096))()
    p = C.c_void_p(C.addressof(buf))
    d = C.c_double
    def hash_(**kw):
        a = dict(emb=p, has=p, n=n, D=D, stride=D, vec=p, T=T, length=0.1, out=p)
        a.update(kw)
        return lib.sprk_lsh_hash(a["emb"], a["has"], a["n"], a["D"], a["stride"], a["vec"], a["T"], d(a["length"]), a["out"], None)
    def build(**kw):
        a = dict(buckets=p, n=n, T=T, ib=p, ir=p, ws=p, ws_bytes=need)
        a.update(kw)
        return lib.sprk_lsh_build(a["buckets"], a["n"], a["T"], a["ib"], a["ir"], a["ws"], a["ws_bytes"], None)
    def query(**kw):
        a = dict(emb=p, has=p, n=n, D=D, stride=D, vec=p, T=T, length=0.1, buckets=p, ib=p, ir=p, q=p, qh=p, Q=Q, qstride=D, K=K_, dist=p, rows=p, count=p)
        a.update(kw)
        return lib.sprk_lsh_query(a["emb"], a["has"], a["n"], a["D"], a["stride"], a["vec"], a["T"], d(a["length"]), a["buckets"], a["ib"], a["ir"], a["q"], a["qh"],
                                  a["Q"], a["qstride"], a["K"], a["dist"], a["rows"], a["count"], None)
    return need, (lambda k: C.c_void_p(C.addressof(buf) + k)), hash_, build, query


def test_lsh_abi_rejects_bad_arguments_before_any_device_call(lib, monkeypatch):
    monkeypatch.delenv("SPRK_LSH_CHUNK", raising=False)
    need, off, hash_, build, query = _abi(lib)
    assert need > 0 and need % 16 == 0
    for n, T in ((-1, 3), (2**31 - 1, 3), (8, 0), (8, 17)):
        assert lib.sprk_lsh_build_workspace_bytes(n, T) == 0
    table = [dict(emb=None), dict(vec=None), dict(emb=off(2)), dict(vec=off(4)), dict(n=-1), dict(n=2**31 - 1), dict(D=0), dict(D=1025), dict(stride=9), dict(T=0), dict(T=17),
             dict(length=0.0), dict(length=-0.1), dict(length=math.inf), dict(length=math.nan)]
    for kw in table + [dict(out=None), dict(out=off(4))]:
        assert hash_(**kw) == L.EINVAL, kw
        assert b"lsh_hash" in lib.sprk_last_error()
    for kw in [dict(buckets=None), dict(ib=None), dict(ir=None), dict(ws=None), dict(buckets=off(4)), dict(ib=off(4)), dict(ir=off(2)), dict(ws=off(8)), dict(n=-1),
               dict(n=2**31 - 1), dict(T=0), dict(T=17), dict(ws_bytes=need - 16), dict(ws_bytes=0)]:
        assert build(**kw) == L.EINVAL, kw
        assert b"lsh_build" in lib.sprk_last_error()
    assert build(ws_bytes=need - 16) == L.EINVAL
    assert ("needs a workspace of %d bytes (sprk_lsh_build_workspace_bytes)" % need).encode() in lib.sprk_last_error()
    for kw in table + [dict(buckets=None), dict(ib=None), dict(ir=None), dict(q=None), dict(dist=None), dict(rows=None), dict(count=None), dict(buckets=off(4)),
                       dict(ib=off(4)), dict(ir=off(2)), dict(q=off(2)), dict(dist=off(4)), dict(rows=off(2)), dict(count=off(2)), dict(Q=-1), dict(qstride=9), dict(K=0),
                       dict(K=-1), dict(K=1025)]:
        assert query(**kw) == L.EINVAL, kw
        assert b"lsh_query" in lib.sprk_last_error()
    monkeypatch.setenv("SPRK_LSH_CHUNK", "64")
    for k in (64, 65, 1024):
        assert query(K=k) == L.EINVAL
        assert b"lsh_query: K = " in lib.sprk_last_error()
    monkeypatch.delenv("SPRK_LSH_CHUNK")
    import torch
    if not torch.cuda.is_available():                               # a good call reaches the device, and there is none
        assert hash_() == L.EHIP and build() == L.EHIP and query() == L.EHIP and query(K=1024) == L.EHIP and query(has=None, qh=None) == L.EHIP
        monkeypatch.setenv("SPRK_LSH_CHUNK", "64")
        assert query(K=63) == L.EHIP
    # nothing to do is no error and no device call
    assert hash_(n=0, emb=None, out=None) == L.OK and build(n=0, buckets=None, ib=None, ir=None) == L.OK and query(Q=0, q=None, dist=None, rows=None, count=None) == L.OK
