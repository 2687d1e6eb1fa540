"""ALS on the device (sprk_als_fit / sprk_als_predict / sprk_als_topk, csrc/k_als.h, csrc/k_als_topk.h) against its definition,
als.als_host: all six outputs byte for byte, with error word -1 -- the order of a row's ratings, the Cholesky's operation order and the
rounding to float32 included -- and the scores and the top-K against als.predict_host / als.topk_host."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import als as A
from tests import als_cases as cases

pytestmark = pytest.mark.gpu

NAMES = ("user_factors", "item_factors", "user_has", "item_has", "user_count", "item_count")


def _up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _device(case, rank=10, reg=0.01, iters=1, init=None, seed=0, user_stride=None, item_stride=None):
    """sprk_als_fit through als.als_device -> the six outputs on the host (the factors cut to rank), the error word."""
    init = A.init_factors(case["n_users"], rank, seed) if init is None else init
    out = A.als_device(_up(case["user"], np.int32), _up(case["movie"], np.int32), _up(case["rating"], np.float32), case["n_users"], case["n_items"],
                       rank, reg, iters, _up(init, np.float32), user_stride=user_stride, item_stride=item_stride)
    host = [np.ascontiguousarray(t.cpu().numpy()) for t in out[:6]]
    host[0], host[1] = np.ascontiguousarray(host[0][:, :rank]), np.ascontiguousarray(host[1][:, :rank])
    return host, int(out[6].cpu()[0])


def _assert_same(got, want):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))[:8])


def _check(case, **kw):
    host_kw = {k: v for k, v in kw.items() if k not in ("user_stride", "item_stride")}
    if "init" in host_kw:
        host_kw["init_user"] = host_kw.pop("init")
    want = cases.host(case, **host_kw)
    got, err = _device(case, **kw)
    assert err == -1
    _assert_same(got, want)
    return got


@pytest.fixture(scope="module")
def synthetic_host(lib):
    """The definition's result on the synthetic set, once per (ordered, iters)."""
    return {(ordered, iters): cases.host(cases.synthetic(ordered), iters=iters) for ordered in (False, True) for iters in (1, 3)}


@pytest.mark.parametrize("sort_cap", [None, 64])
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("iters", [1, 3])
def test_synthetic_set_equals_the_host_definition(synthetic_host, monkeypatch, iters, ordered, sort_cap):
    """tests/als_cases.py synthetic: a movie everyone rated and a user of 300 ratings (with SPRK_FE_SORT_CAP = 64 sorted in chunks and
    merge passes), users of one rating, movies of none, repeated pairs; shuffled input and input in key order."""
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    case = cases.synthetic(ordered)
    assert np.bincount(case["user"])[0] == 300 and np.bincount(case["movie"], minlength=80)[0] >= 300 and not np.bincount(case["movie"], minlength=80)[70:].any()
    got, err = _device(case, iters=iters)
    assert err == -1
    _assert_same(got, synthetic_host[(ordered, iters)])


def test_shuffled_and_ordered_input_differ_only_through_the_repeated_pairs(synthetic_host):
    """(a repeated pair goes by input row, and the two inputs number the rows differently: the sets are the same, the results need not be)"""
    a, b = synthetic_host[(False, 1)], synthetic_host[(True, 1)]
    assert a[4].tobytes() == b[4].tobytes() and a[5].tobytes() == b[5].tobytes()


@pytest.mark.parametrize("rank", [1, 2, 5, 6, 7, 10, 11, 16])
def test_rank_classes(lib, rank):
    """Chains per lane: 2 up to rank 6, 5 up to rank 10, 10 up to rank 16 -- every class's ends and their neighbours."""
    _check(cases.low_rank(), rank=rank, iters=2)


@pytest.mark.parametrize("rank", [4, 10])
def test_segment_lengths_around_the_prefetch_chunk(lib, rank):
    """Movies of 0, 1, C-1, C, C+1, 2C, 2C+1 and 100 ratings, C = the half-sweep's chunk."""
    case = cases.segment_lengths()
    assert np.bincount(case["movie"], minlength=case["n_items"]).tolist() == case["lengths"]
    _check(case, rank=rank, iters=2)


def test_hand_worked_systems(lib):
    for reg, want, _ in cases.HAND_RANK1:
        got, err = _device({"user": [0, 1, 2], "movie": [0, 0, 0], "rating": [4, 0, 5], "n_users": 3, "n_items": 1}, rank=1, reg=reg, iters=1,
                           init=np.array([[1], [2], [3]], np.float32))
        assert err == -1 and int(got[1].view(np.uint32)[0, 0]) == want
    got, err = _device({"user": [0, 1, 2], "movie": [0, 0, 0], "rating": cases.HAND2_RATINGS, "n_users": 3, "n_items": 1}, rank=2, reg=cases.HAND2_REG, iters=1,
                       init=cases.HAND2_FACTORS)
    assert err == -1 and got[1].view(np.uint32)[0].tolist() == cases.HAND2_WORDS


def test_the_order_sensitive_set(lib):
    """tests/test_als.py's set on which walking a row backwards changes words: the device walks forwards."""
    rng = np.random.default_rng(3)
    n_users, n_items = 40, 6
    u, m = np.nonzero(rng.random((n_users, n_items)) < 0.7)
    r = cases.half_stars(rng.integers(1, 11, len(u)) / 2.0)
    scale = np.array([1e-3, 1.0, 1e3])[rng.integers(0, 3, n_users)]
    init = (scale[:, None] * np.array([1.0, 0.7, -1.3]) + 1e-3 * rng.standard_normal((n_users, 3))).astype(np.float32)
    case = {"user": u, "movie": m, "rating": r, "n_users": n_users, "n_items": n_items}
    got = _check(case, rank=3, reg=1e-6, iters=1, init=init)
    bwd = cases.host(case, rank=3, reg=1e-6, iters=1, init_user=init, descending=True)
    assert got[1].tobytes() != bwd[1].tobytes()


def test_zero_and_subnormal_factors_and_a_zero_rating(lib):
    """A factor row with an exact 0.0 and a rating of 0.0 are the definition's two skips, which the kernel drops; 1e-40 is a float32
    subnormal, which a kernel that flushes would read as 0."""
    case = dict(cases.segment_lengths())
    rating = case["rating"].copy()
    rating[::5] = 0.0
    case["rating"] = rating
    init = A.init_factors(case["n_users"], 4, 5)
    init[::3, 1] = 0.0
    init[1::7, 2] = 1e-40
    init[2::7] = [1e-40, -1e-40, 0.0, 1e-40]
    assert (np.abs(init[2::7][:, 0]) < np.finfo(np.float32).tiny).all() and (init[2::7][:, 0] != 0).all()
    _check(case, rank=4, reg=0.01, iters=1, init=init)
    _check(case, rank=4, reg=0.01, iters=2, init=init)


def test_empty_inputs_and_no_iterations(lib):
    empty = {"user": np.zeros(0, np.int32), "movie": np.zeros(0, np.int32), "rating": np.zeros(0, np.float32)}
    for n_users, n_items in ((0, 0), (3, 0), (0, 4), (3, 4)):
        got = _check(dict(empty, n_users=n_users, n_items=n_items), rank=3, iters=2)
        assert not got[0].any() and not got[1].any() and got[0].shape == (n_users, 3) and got[1].shape == (n_items, 3)
    case = cases.segment_lengths()
    got = _check(case, rank=5, iters=0, seed=9)
    assert got[0].tobytes() == A.init_factors(case["n_users"], 5, 9).tobytes() and not got[1].any() and got[5].tolist() == case["lengths"]


FILL = 0xA5
GUARD_ROWS, GUARD_BYTES = 64, 4096


def _is_fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


@pytest.mark.parametrize("sort_cap", [None, 64])
def test_nothing_is_written_outside_the_outputs_or_the_workspace(lib, synthetic_host, monkeypatch, sort_cap):
    """Guard bands of a fill pattern after every output, between rank and the stride of every factor row (the sentinel survives), and
    on both sides of a workspace of exactly the advertised length keep their fill."""
    import torch
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    case = cases.synthetic(False)
    n, nu, ni, rank, us, its, ins = len(case["user"]), case["n_users"], case["n_items"], 10, 13, 16, 11
    dev = torch.device("cuda", torch.cuda.current_device())
    def filled(shape, dtype):
        n_bytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        return torch.full((n_bytes,), FILL, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)
    init = np.full((nu, ins), np.nan, dtype=np.float32)                     # (the floats past rank of an init row are not read)
    init[:, :rank] = A.init_factors(nu, rank, 0)
    u_d, m_d, r_d, i_d = _up(case["user"], np.int32), _up(case["movie"], np.int32), _up(case["rating"], np.float32), _up(init, np.float32)
    o_uf, o_if = filled((nu + GUARD_ROWS, us), torch.float32), filled((ni + GUARD_ROWS, its), torch.float32)
    o_uh, o_ih = filled((nu + GUARD_ROWS,), torch.uint8), filled((ni + GUARD_ROWS,), torch.uint8)
    o_uc, o_ic = filled((nu + GUARD_ROWS,), torch.int32), filled((ni + GUARD_ROWS,), torch.int32)
    word = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ws_bytes = lib.sprk_als_workspace_bytes(n, nu, ni, rank)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    arena = torch.full((GUARD_BYTES + ws_bytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device=dev)
    assert arena.data_ptr() % 16 == 0
    p = lambda x: C.c_void_p(x.data_ptr())
    L.check(lib.sprk_als_fit(p(u_d), p(m_d), p(r_d), n, nu, ni, rank, 0.01, 3, p(i_d), ins, p(o_uf), us, p(o_if), its, p(o_uh), p(o_ih), p(o_uc), p(o_ic), p(word),
                             C.c_void_p(arena.data_ptr() + GUARD_BYTES), ws_bytes, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    assert int(word.cpu()[0]) == -1
    arena, uf, itf = arena.cpu().numpy(), o_uf.cpu().numpy(), o_if.cpu().numpy()
    uh, ih, uc, ic = o_uh.cpu().numpy(), o_ih.cpu().numpy(), o_uc.cpu().numpy(), o_ic.cpu().numpy()
    assert _is_fill(arena[:GUARD_BYTES]) and _is_fill(arena[GUARD_BYTES + ws_bytes:])
    assert _is_fill(uf[nu:]) and _is_fill(itf[ni:]) and _is_fill(uf[:nu, rank:]) and _is_fill(itf[:ni, rank:])
    assert _is_fill(uh[nu:]) and _is_fill(ih[ni:]) and _is_fill(uc[nu:]) and _is_fill(ic[ni:])
    got = (np.ascontiguousarray(uf[:nu, :rank]), np.ascontiguousarray(itf[:ni, :rank]), uh[:nu], ih[:ni], uc[:nu], ic[:ni])
    _assert_same(got, synthetic_host[(False, 3)])


def test_strides_through_the_python_surface(lib):
    _check(cases.segment_lengths(), rank=5, iters=1, user_stride=8, item_stride=7)


def test_two_runs_give_the_same_bytes(lib):
    case = cases.synthetic(False)
    runs = [[a.tobytes() for a in _device(case, iters=2)[0]] for _ in range(2)]
    assert runs[0] == runs[1]


def test_side_stream(lib, synthetic_host):
    import torch
    case = cases.synthetic(False)
    args = (_up(case["user"], np.int32), _up(case["movie"], np.int32), _up(case["rating"], np.float32))
    init = _up(A.init_factors(case["n_users"], 10, 0), np.float32)
    torch.cuda.synchronize()
    side, done = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(side):
        out = A.als_device(*args, case["n_users"], case["n_items"], 10, 0.01, 1, init)
        done.record(side)
    done.synchronize()
    assert int(out[6].cpu()[0]) == -1
    _assert_same([np.ascontiguousarray(t.cpu().numpy()) for t in out[:6]], synthetic_host[(False, 1)])


def test_error_words(lib):
    case = cases.synthetic(False)
    user = case["user"].copy()
    user[[4000, 123, 2500]] = [300, 300, -1]
    _, err = _device(dict(case, user=user))
    assert (err >> 32, err & 0xffffffff) == (1, 123)                              # a user id at n_users: kind 1, the smallest such row
    movie = case["movie"].copy()
    movie[[77, 900]] = [80, 1 << 20]
    _, err = _device(dict(case, movie=movie))
    assert (err >> 32, err & 0xffffffff) == (2, 77)
    rating = case["rating"].copy()
    rating[[3000, 555]] = [np.inf, np.nan]
    _, err = _device(dict(case, rating=rating))
    assert (err >> 32, err & 0xffffffff) == (3, 555)
    rating = case["rating"].copy()
    rating[10] = 7.25                                                             # off the half-star scale: no error here
    _, err = _device(dict(case, rating=rating))
    assert err == -1
    init = A.init_factors(case["n_users"], 10, 0)
    init[[200, 41], [3, 9]] = [np.nan, np.inf]
    _, err = _device(case, init=init, iters=2)
    assert (err >> 32, err & 0xffffffff) == (7, 41)
    S = cases.SINGULAR
    _, err = _device({"user": S["user"], "movie": S["movie"], "rating": S["rating"], "n_users": 6, "n_items": 2}, rank=4, reg=0.0, iters=2, init=S["init"])
    assert err == 6 << 32 | 1                                                     # reg = 0 at rank 4 on a movie with 2 ratings
    # with reg > 0 the same set is fine, and a user of too few ratings at reg = 0 is kind 5: users 2 .. 5 have one rating
    _check({"user": S["user"], "movie": S["movie"], "rating": S["rating"], "n_users": 6, "n_items": 2}, rank=4, reg=0.01, iters=2, init=S["init"])
    _, err = _device({"user": S["user"][:6], "movie": S["movie"][:6], "rating": S["rating"][:6], "n_users": 6, "n_items": 1}, rank=4, reg=0.0, iters=1, init=S["init"])
    assert err == 5 << 32 | 0


# ---------------------------------------------------------------- scores and top-K

@pytest.fixture(scope="module")
def model_host(lib):
    case = cases.synthetic(False)
    return case, cases.host(case, iters=2)


def test_predict_equals_the_index_order_dot(model_host):
    case, host = model_host
    rng = np.random.default_rng(2)
    users = np.concatenate([rng.integers(0, 300, 500), [-1, 300, 5, 5, 1 << 30]]).astype(np.int32)
    movies = np.concatenate([rng.integers(0, 80, 500), [3, 3, -1, 80, 3]]).astype(np.int32)
    want = A.predict_host(users, movies, host[0], host[2], host[1], host[3])
    assert np.isnan(want[-5:]).all() and np.isnan(want[:500][movies[:500] >= 70]).all() and not np.isnan(want[:500][movies[:500] < 70]).any()
    pad = lambda f, s: np.concatenate([f, np.full((len(f), s - f.shape[1]), np.nan, np.float32)], axis=1)
    for stride in (10, 13):
        uf, itf = _up(pad(host[0], stride), np.float32), _up(pad(host[1], stride), np.float32)
        got = A.predict_device(_up(users, np.int32), _up(movies, np.int32), uf, _up(host[2], np.uint8), itf, _up(host[3], np.uint8), rank=10).cpu().numpy()
        assert got.tobytes() == want.tobytes()
    none = A.predict_device(_up(users[:0], np.int32), _up(movies[:0], np.int32), uf, _up(host[2], np.uint8), itf, _up(host[3], np.uint8), rank=10)
    assert none.numel() == 0


def _topk(query, query_has, table, table_has, k):
    rows, scores = A.topk_device(_up(query, np.float32), _up(query_has, np.uint8), _up(table, np.float32), _up(table_has, np.uint8), k)
    return rows.cpu().numpy(), scores.cpu().numpy()


@pytest.mark.parametrize("n_items", [1, 63, 64, 65, 300])
def test_topk_equals_sorting_every_score(lib, monkeypatch, n_items):
    """SPRK_EMB_TOPK_CHUNK = 64: 65 rows are two chunks and a merge, 300 rows five chunks; K = 1, 10, the rows available and above them
    (the -1 / NaN padding); some rows and one query without factors."""
    monkeypatch.setenv("SPRK_EMB_TOPK_CHUNK", "64")
    rng = np.random.default_rng(n_items)
    table = rng.standard_normal((n_items, 10)).astype(np.float32)
    has = (rng.random(n_items) < 0.8).astype(np.uint8)
    has[0] = 1
    query = rng.standard_normal((7, 10)).astype(np.float32)
    q_has = np.array([1, 1, 1, 0, 1, 1, 1], dtype=np.uint8)
    available = int(has.sum())
    for k in sorted({1, 10, available, available + 3, min(n_items + 5, 1024)}):
        rows, scores = _topk(query, q_has, table, has, k)
        want_rows, want_scores = A.topk_host(query, q_has, table, has, k)
        assert rows.tobytes() == want_rows.tobytes() and scores.tobytes() == want_scores.tobytes(), k
        assert (rows[3] == -1).all() and (rows[0, :min(k, available)] >= 0).all() and (rows[0, available:] == -1).all()


@pytest.mark.parametrize("chunk", [None, 64])
def test_topk_ties_go_by_ascending_row(lib, monkeypatch, chunk):
    """Half of the table is copies of four rows: their scores tie exactly."""
    if chunk is not None:
        monkeypatch.setenv("SPRK_EMB_TOPK_CHUNK", str(chunk))
    rng = np.random.default_rng(4)
    table = rng.standard_normal((300, 6)).astype(np.float32)
    table[::2] = table[[1, 3, 5, 7]][rng.integers(0, 4, 150)]
    has = np.ones(300, dtype=np.uint8)
    query = rng.standard_normal((5, 6)).astype(np.float32)
    for k in (10, 150, 300):
        rows, scores = _topk(query, np.ones(5, np.uint8), table, has, k)
        want_rows, want_scores = A.topk_host(query, np.ones(5, np.uint8), table, has, k)
        assert rows.tobytes() == want_rows.tobytes() and scores.tobytes() == want_scores.tobytes(), k
    assert (np.diff(want_scores[0]) == 0).sum() > 50
    none = A.topk_device(_up(query[:0], np.float32), _up(np.zeros(0), np.uint8), _up(table, np.float32), _up(has, np.uint8), 5)
    assert none[0].shape == (0, 5)
    rows, scores = _topk(query, np.ones(5, np.uint8), table[:0], has[:0], 3)
    assert (rows == -1).all() and np.isnan(scores).all()


def test_fit_end_to_end(model_host, monkeypatch):
    import torch
    case, host = model_host
    ratings = {"userId": case["user"].astype(np.int64), "movieId": case["movie"].astype(np.int64), "rating": case["rating"]}
    model = A.fit(ratings, iters=2, n_items=80)
    _assert_same(model.to_host(), host)
    on_device = {k: torch.from_numpy(v).cuda() for k, v in ratings.items()}
    _assert_same(A.fit(on_device, iters=2, n_items=80).to_host(), host)
    p = A.predict_host(case["user"], case["movie"], host[0], host[2], host[1], host[3])
    want = float(np.sqrt(np.mean((p - case["rating"]).astype(np.float64) ** 2)))
    assert abs(model.rmse(ratings) - want) <= 1e-9 * want
    assert model.predict([5, 5, 400], [3, 75, 3]).cpu().numpy().tobytes() == A.predict_host([5, 5, 400], [3, 75, 3], host[0], host[2], host[1], host[3]).tobytes()
    monkeypatch.setenv("SPRK_EMB_TOPK_CHUNK", "64")
    rec = model.recommend_for_users()
    want_rows, want_scores = A.topk_host(host[0], host[2], host[1], host[3], 10)
    assert rec.query.cpu().numpy().tolist() == list(range(300))
    assert rec.ids.cpu().numpy().tobytes() == want_rows.tobytes() and rec.scores.cpu().numpy().tobytes() == want_scores.tobytes()
    some = model.recommend_for_users([7, -1, 299, 300], k=5)
    assert some.ids.cpu().numpy()[[0, 2]].tobytes() == want_rows[[7, 299], :5].tobytes() and (some.ids.cpu().numpy()[[1, 3]] == -1).all()
    items = model.recommend_for_items(k=10)
    want_rows, want_scores = A.topk_host(host[1][:70], host[3][:70], host[0], host[2], 10)
    assert items.query.cpu().numpy().tolist() == list(range(70))
    assert items.ids.cpu().numpy().tobytes() == want_rows.tobytes() and items.scores.cpu().numpy().tobytes() == want_scores.tobytes()
    bad = dict(ratings, userId=ratings["userId"].copy())
    bad["userId"][[2000, 17]] = [-3, 2**40]
    with pytest.raises(ValueError) as e:
        A.fit(bad, iters=1)
    assert str(e.value) == "ratings row 17: userId outside the user table"
