"""Embedding LSH on the device (sprk_lsh_hash / sprk_lsh_build / sprk_lsh_query, csrc/k_lsh.h) against its definition, lsh.hash_host and
lsh.approx_nearest_host: the buckets, the sorted index, dist, rows and count BYTE FOR BYTE -- no tolerance anywhere -- at the reference's
configuration, past one LDS buffer and past the sort capacity, under every test switch, at the edges of every size, and through
EmbRanker and item2vec.fit."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import lsh
from tests import lsh_cases as K

pytestmark = pytest.mark.gpu

_wanted = {}


def _case(n, D, T, length, n_queries=200, scale=1.0):
    """The table, the vectors, the queries (the first rows) and the definition's buckets, computed once per shape."""
    key = (n, D, T, length, n_queries, scale)
    if key not in _wanted:
        emb = K.table(n, D, scale=scale)
        vec = lsh.random_unit_vectors(D, T)
        _wanted[key] = {"emb": emb, "vec": vec, "length": length, "queries": emb[:n_queries], "buckets": lsh.hash_host(emb, vec, length), "nearest": {}}
    return _wanted[key]


def _want(case, k):
    if k not in case["nearest"]:
        case["nearest"][k] = lsh.approx_nearest_host(case["emb"], None, case["vec"], case["length"], case["queries"], k)
    return case["nearest"][k]


def _host(t):
    return np.ascontiguousarray(t.cpu().numpy())


def _check_index(index, buckets):
    """buckets = the definition's (NO_BUCKET where has == 0 already); the index = every table's (bucket, row) pairs in ascending order."""
    got = _host(index.buckets)
    assert got.dtype == np.int64 and got.tobytes() == buckets.tobytes(), np.flatnonzero((got != buckets).any(axis=1))[:8]
    n = len(buckets)
    ib, ir = _host(index.idx_bucket), _host(index.idx_row)
    assert ib.shape == (index.T, n) and ir.shape == (index.T, n) and ir.dtype == np.int32
    for t in range(index.T):
        order = np.lexsort((np.arange(n), buckets[:, t]))
        assert ir[t].tobytes() == order.astype(np.int32).tobytes(), t
        assert ib[t].tobytes() == np.ascontiguousarray(buckets[order, t]).tobytes(), t


def _run(case, k):
    """Build on the device, search, compare all of it with the definition.  -> (index, (dist, rows, count) on the host)"""
    index = lsh.LSHIndex.build(case["emb"], bucket_length=case["length"], vectors=case["vec"])
    _check_index(index, case["buckets"])
    got = tuple(_host(x) for x in index.approx_nearest(case["queries"], k))
    K.same(got, _want(case, k))
    return index, got


@pytest.mark.parametrize("k", [5, 300])
def test_reference_configuration(lib, k):
    """n = 3000, D = 10, T = 3, bucket_length 0.1 (Embedding.embeddingLSH's settings): 12 to 379 candidates a query, so k = 300 leaves some
    queries short and cuts others."""
    _, (dist, rows, count) = _run(_case(3000, 10, 3, 0.1), k)
    assert count.min() < 300 < count.max() and count.min() > 5
    assert (rows[:, 0] == np.arange(200)).all() and not dist[:, 0].any()


def test_more_than_one_buffer_and_the_long_sort(lib, monkeypatch):
    """n = 6000 with bucket_length 2.0: thousands of candidates a query -- the 4096-pair buffer fills and is cut -- and every table's
    segment is longer than the LDS sort holds: chunks and merge passes.  326 to 5505 candidates a query."""
    monkeypatch.delenv("SPRK_LSH_CHUNK", raising=False)
    monkeypatch.delenv("SPRK_FE_SORT_CAP", raising=False)
    _, (_, _, count) = _run(_case(6000, 10, 3, 2.0), 10)
    assert count.max() > 4096 + 512 and count.min() < 4096
    _run(_case(6000, 10, 3, 2.0), 1024)


@pytest.mark.parametrize("env,value,k", [("SPRK_LSH_CHUNK", 64, 5), ("SPRK_LSH_CHUNK", 64, 63), ("SPRK_LSH_CHUNK", 256, 255), ("SPRK_FE_SORT_CAP", 64, 5),
                                         ("SPRK_FE_MAX_GRID", 3, 5), ("SPRK_FE_MAX_GRID", 1, 5)])
def test_switches(lib, monkeypatch, env, value, k):
    """A buffer of 64 pairs is cut many times, with room for 59 new pairs and for one; a sort capacity of 64 takes the merge passes at
    3000 rows; a grid of 3 and of 1 workgroups takes every loop past one round (one workgroup answers all 200 queries)."""
    monkeypatch.setenv(env, str(value))
    _run(_case(3000, 10, 3, 0.1), k)


def test_k_that_does_not_fit_the_buffer_is_refused(lib, monkeypatch):
    monkeypatch.setenv("SPRK_LSH_CHUNK", "64")
    case = _case(3000, 10, 3, 0.1)
    index = lsh.LSHIndex.build(case["emb"], bucket_length=0.1, vectors=case["vec"])
    with pytest.raises(L.SparrowHipError, match="lsh_query: K = 64"):
        index.approx_nearest(case["queries"], 64)


@pytest.mark.parametrize("n,D,T,length", [(2000, 1, 3, 0.1), (2000, 64, 3, 0.1), (2000, 65, 3, 0.1), (2000, 10, 1, 0.1), (2000, 10, 16, 0.1), (1500, 65, 16, 0.2),
                                          (600, 300, 16, 0.2), (300, 1024, 2, 0.5)])
def test_widths_and_table_counts(lib, n, D, T, length):
    """D = 1, both sides of 64 and the widest row; one table and sixteen; 16 x 65 doubles are more than the query kernel keeps in LDS and
    16 x 300 more than the hash kernel does: both read the vectors from global memory then."""
    _, (_, _, count) = _run(_case(n, D, T, length, n_queries=100), 7)
    assert count.max() > 7


def test_one_row_no_row_no_query(lib):
    one = _case(1, 10, 3, 0.1, n_queries=1)
    _, (dist, rows, count) = _run(one, 4)
    assert rows.tolist() == [[0, -1, -1, -1]] and count.tolist() == [1] and dist[0, 0] == 0.0
    queries = K.table(5, 10, seed=9)
    empty = lsh.LSHIndex.build(np.zeros((0, 10), np.float32), bucket_length=0.1)
    assert tuple(empty.buckets.shape) == (0, 3) and tuple(empty.idx_row.shape) == (3, 0)
    K.same(tuple(_host(x) for x in empty.approx_nearest(queries, 4)), lsh.approx_nearest_host(np.zeros((0, 10), np.float32), None, empty.vectors, 0.1, queries, 4))
    case = _case(3000, 10, 3, 0.1)
    index = lsh.LSHIndex.build(case["emb"], bucket_length=0.1, vectors=case["vec"])
    got = index.approx_nearest(np.zeros((0, 10), np.float32), 4)
    assert [tuple(x.shape) for x in got] == [(0, 4), (0, 4), (0,)]


def test_row_strides_above_D_and_device_tensors_where_they_are(lib):
    import torch
    case = _case(3000, 10, 3, 0.1)
    wide = torch.full((3000, 13), float("nan"), device="cuda")
    wide[:, :10] = torch.from_numpy(case["emb"]).cuda()
    table = wide[:, :10]
    index = lsh.LSHIndex.build(table, bucket_length=0.1, vectors=case["vec"])
    assert index.table.data_ptr() == wide.data_ptr() and index.table.stride(0) == 13
    _check_index(index, case["buckets"])
    qwide = torch.full((200, 17), float("nan"), device="cuda")
    qwide[:, :10] = table[:200]
    K.same(tuple(_host(x) for x in index.approx_nearest(qwide[:, :10], 5)), _want(case, 5))
    K.same(tuple(_host(x) for x in index.approx_nearest(table[:200], 5)), _want(case, 5))


def test_identical_rows_all_ties_go_by_row(lib, monkeypatch):
    """Every row is a candidate of every query at distance +0.0: 4500 candidates through more than one buffer, the first k rows win."""
    monkeypatch.delenv("SPRK_LSH_CHUNK", raising=False)
    emb = np.tile(K.table(1, 10, seed=4), (4500, 1))
    index = lsh.LSHIndex.build(emb, bucket_length=0.1)
    dist, rows, count = (_host(x) for x in index.approx_nearest(emb[:3], 20))
    assert rows.tolist() == [list(range(20))] * 3 and count.tolist() == [4500] * 3 and dist.tobytes() == np.zeros((3, 20)).tobytes()
    K.same((dist, rows, count), lsh.approx_nearest_host(emb, None, index.vectors, 0.1, emb[:3], 20))


def test_edge_rows(lib):
    """Bucket edges, the clamp, subnormal and non-finite coordinates, a row without an embedding (tests/lsh_cases.py edge_rows), as rows and
    as queries, with query_has."""
    emb, has, want = K.edge_rows()
    index = lsh.LSHIndex.build(emb, has, bucket_length=K.EDGE_LENGTH, vectors=K.EDGE_VECTORS)
    assert _host(index.buckets).tolist() == want.tolist()
    buckets = lsh.hash_host(emb, K.EDGE_VECTORS, K.EDGE_LENGTH)
    buckets[has == 0] = K.NO
    _check_index(index, buckets)
    queries = np.concatenate([emb, np.array([[0.55, -0.45], [np.nan, np.nan], [1e-40, -1e-40]], np.float32)])
    qh = np.ones(len(queries), np.uint8)
    qh[0] = 0
    got = tuple(_host(x) for x in index.approx_nearest(queries, 4, query_has=qh))
    K.same(got, lsh.approx_nearest_host(emb, has, K.EDGE_VECTORS, K.EDGE_LENGTH, queries, 4, qh))
    assert got[2][0] == 0 and got[2][-3] == 4 and got[2][-2] == 0 and got[2][-1] >= 1
    one = lsh.LSHIndex.build(np.array([[0.5], [-0.5], [1e30], [-1e30]], np.float32), bucket_length=0.25, vectors=np.array([[1.0]]))
    assert _host(one.buckets).tolist() == [[2], [-2], [1 << 62], [-(1 << 62)]]


def test_rows_without_embedding_on_a_random_table(lib):
    case = _case(3000, 10, 3, 0.1)
    rng = np.random.default_rng(7)
    has, qh = (rng.random(3000) >= 0.2).astype(np.uint8), (rng.random(200) >= 0.2).astype(np.uint8)
    index = lsh.LSHIndex.build(case["emb"], has, bucket_length=0.1, vectors=case["vec"])
    buckets = case["buckets"].copy()
    buckets[has == 0] = K.NO
    _check_index(index, buckets)
    got = tuple(_host(x) for x in index.approx_nearest(case["queries"], 5, query_has=qh))
    K.same(got, lsh.approx_nearest_host(case["emb"], has, case["vec"], 0.1, case["queries"], 5, qh))


FILL = 0xA5
GUARD = 4096


def _is_fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


@pytest.mark.parametrize("n,length,sort_cap,chunk", [(3000, 0.1, None, None), (3000, 0.1, 64, 64), (6000, 2.0, None, None)])
def test_nothing_is_written_outside_the_outputs_or_the_workspace(lib, monkeypatch, n, length, sort_cap, chunk):
    """Guard bands of a fill pattern on both sides of every output and of a workspace of exactly the advertised length keep their fill."""
    import torch
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    if chunk is not None:
        monkeypatch.setenv("SPRK_LSH_CHUNK", str(chunk))
    case = _case(n, 10, 3, length)
    D, T, Q, k = 10, 3, 200, 5
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    def arena(n_bytes):
        a = torch.full((GUARD + n_bytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert a.data_ptr() % 16 == 0
        return a
    ws_bytes = lib.sprk_lsh_build_workspace_bytes(n, T)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    sizes = {"buckets": n * T * 8, "idx_bucket": n * T * 8, "idx_row": n * T * 4, "dist": Q * k * 8, "rows": Q * k * 4, "count": Q * 4, "ws": ws_bytes}
    mem = {name: arena(b) for name, b in sizes.items()}
    at = lambda name: C.c_void_p(mem[name].data_ptr() + GUARD)
    e_d, v_d, q_d = up(case["emb"]), up(case["vec"]), up(case["queries"])
    p = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(lib.sprk_lsh_hash(p(e_d), None, n, D, D, p(v_d), T, length, at("buckets"), stream))
    L.check(lib.sprk_lsh_build(at("buckets"), n, T, at("idx_bucket"), at("idx_row"), at("ws"), ws_bytes, stream))
    L.check(lib.sprk_lsh_query(p(e_d), None, n, D, D, p(v_d), T, length, at("buckets"), at("idx_bucket"), at("idx_row"), p(q_d), None, Q, D, k, at("dist"), at("rows"),
                               at("count"), stream))
    host = {name: a.cpu().numpy() for name, a in mem.items()}
    for name, b in sizes.items():
        assert _is_fill(host[name][:GUARD]) and _is_fill(host[name][GUARD + b:]), name
    body = lambda name, dt: host[name][GUARD:GUARD + sizes[name]].view(dt)
    assert body("buckets", np.int64).tobytes() == case["buckets"].tobytes()
    K.same((body("dist", np.float64).reshape(Q, k), body("rows", np.int32).reshape(Q, k), body("count", np.int32)), _want(case, k))


def test_twenty_calls_give_the_same_bytes(lib):
    case = _case(6000, 10, 3, 2.0)
    index = lsh.LSHIndex.build(case["emb"], bucket_length=2.0, vectors=case["vec"])
    runs = {b"".join(_host(x).tobytes() for x in index.approx_nearest(case["queries"], 10)) for _ in range(20)}
    assert len(runs) == 1
    K.same(tuple(_host(x) for x in index.approx_nearest(case["queries"], 10)), _want(case, 10))


def test_side_stream(lib):
    """Build and search are enqueued behind a spin of some milliseconds on a side stream and return while it is still busy; the event
    recorded after them orders the read."""
    import torch
    case = _case(3000, 10, 3, 0.1)
    table, queries = torch.from_numpy(case["emb"]).cuda(), torch.from_numpy(case["queries"]).cuda()
    torch.cuda.synchronize()
    side, done = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(40_000_000)
        index = lsh.LSHIndex.build(table, bucket_length=0.1, vectors=case["vec"])
        got = index.approx_nearest(queries, 5)
        done.record(side)
        returned_early = not done.query()
    done.synchronize()
    assert returned_early
    _check_index(index, case["buckets"])
    K.same(tuple(_host(x) for x in got), _want(case, 5))


@pytest.fixture(scope="module")
def movies(lib):
    """881 movies (ids 3 i + 1), D = 10, unit-normal rows times 0.4: 8 to 254 candidates a movie at the reference's settings; three movies
    have a vector of the wrong length, so no embedding."""
    from sparrowrecsys_amd import ranker as R
    emb = K.table(881, 10, scale=0.4)
    table = {3 * i + 1: emb[i] for i in range(881)}
    for i in (5, 400, 880):
        table[3 * i + 1] = np.ones(4, np.float32)
    return R.EmbRanker(table)


def test_ranker_lsh_index_and_approx_similar_movies(movies):
    index = movies.lsh_index()
    assert movies.lsh_index(0.1, 3, 0) is index and movies.lsh_index(bucket_length=0.2) is not index
    assert (index.bucket_length, index.T) == (0.1, 3) and index.vectors.tobytes() == lsh.random_unit_vectors(10, 3, 0).tobytes()
    table, has = _host(movies.table), _host(movies.has)
    assert has.sum() == 878
    buckets = lsh.hash_host(table, index.vectors, 0.1)
    buckets[has == 0] = K.NO
    _check_index(index, buckets)
    dist, rows, count = lsh.approx_nearest_host(table, has, index.vectors, 0.1, table, 11, has)
    live = count[has != 0]
    assert 1 <= live.min() < 11 < live.max() < 881                          # some movies have fewer neighbours than are asked for
    assert count[180] < 11                                                     # a movie with fewer neighbours than are asked for
    for row in (0, 1, 5, 77, 180, 400, 879):
        want = [int(movies.ids[r]) for r in rows[row].tolist() if r >= 0 and r != row][:10]
        assert movies.approx_similar_movies(3 * row + 1, 10) == want, row
        assert len(want) == (min(10, count[row] - 1) if has[row] else 0)
    assert movies.approx_similar_movies(2, 10) == [] and movies.approx_similar_movies(1, 0) == []
    # more than the buckets give: every candidate but the movie itself
    everything = movies.approx_similar_movies(1, 1000)
    assert len(everything) == count[0] - 1 < 1000
    wide = movies.approx_similar_movies(1, 10, bucket_length=0.2)
    want = lsh.approx_nearest_host(table, has, index.vectors, 0.2, table[:1], 11)[1][0]
    assert wide == [int(movies.ids[r]) for r in want.tolist() if r > 0][:10]


def test_item2vec_fit_to_lsh_end_to_end(lib):
    """Ratings -> item vectors -> LSH with no further code: item2vec.fit(...).ranker().approx_similar_movies against the definition over the
    trained table."""
    from sparrowrecsys_amd import item2vec as IV
    from tests import item2vec_cases
    model = IV.fit(item2vec_cases.ratings(), n_users=40, n_items=30, D=10, iters=2, round=32)
    ranker = model.ranker()
    table, has = _host(ranker.table), _host(ranker.has)
    index = ranker.lsh_index()
    dist, rows, count = lsh.approx_nearest_host(table, has, index.vectors, 0.1, table, 6, has)
    assert count.max() > 1
    for row, movie in enumerate(ranker.ids.tolist()):
        assert ranker.approx_similar_movies(movie, 5) == [int(ranker.ids[r]) for r in rows[row].tolist() if r >= 0 and r != row][:5], movie
