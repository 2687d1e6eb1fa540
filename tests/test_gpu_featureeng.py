"""Feature engineering on the device (sprk_feature_eng, csrc/k_feature_eng.h) against its definition, featureeng.samples_host: the
sample columns, the kept-sample count and the store's tables bit for bit; the error word names the row the host error names."""
import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import featureeng as FE
from sparrowrecsys_amd import featurestore as FS
from sparrowrecsys_amd import schema as S
from tests import featureeng_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synthetic(lib):
    ratings, movies = cases.synthetic_ratings(), FE.movie_table(cases.synthetic_movies())
    want = {h: FE.samples_host(ratings, movies, h) for h in (5, 12)}
    return ratings, movies, want


def _assert_same_columns(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, np.flatnonzero(got[k] != want[k])[:8])


def _assert_same_store(store, want_samples, hist_len, n_users, n_movies):
    want = FS.row_images_from_samples(want_samples, hist_len, n_users, n_movies)
    got = [t.cpu().numpy() for t in store.tensors()]
    assert (store.n_users, store.n_movies, store.hist_len) == (n_users, n_movies, hist_len)
    for name, g, w in zip(want._fields, got, want[:4]):
        assert g.dtype == w.dtype and g[:-1].tobytes() == w.tobytes(), name        # (the device tables carry one spare row)
        assert not g[-1].any()
    for a, b in zip(store.images[:4], want[:4]):
        assert np.array_equal(a, b)


def _check(ratings, movies, want, hist_len, n_users=cases.N_USERS, n_movies=cases.N_MOVIES):
    built = FE.build(ratings, movies, hist_len, n_users=n_users, n_movies=n_movies)
    assert built.n_samples == len(want["userId"])
    _assert_same_columns(built.to_host(), want)
    _assert_same_store(built.store(), want, hist_len, n_users, n_movies)
    return built


@pytest.mark.parametrize("hist_len,sort_cap", [(5, None), (5, 64), (12, None)])
def test_synthetic_set_equals_the_host_definition(synthetic, monkeypatch, hist_len, sort_cap):
    """featureeng_cases.synthetic_ratings (tests/test_featureeng.py asserts the cases it holds); with SPRK_FE_SORT_CAP=64 the users of
    100 to 250 ratings take the chunked sort and the merge passes."""
    ratings, movies, want = synthetic
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    _check(ratings, movies, want[hist_len], hist_len)


def test_device_tensors_and_default_table_sizes(synthetic):
    import torch
    ratings, movies, want = synthetic
    dev = {k: torch.from_numpy(v).cuda() for k, v in ratings.items()}
    _check(dev, movies, want[5], 5, n_users=31, n_movies=122)
    built = FE.build(dev, movies)
    assert (built.store().n_users, built.store().n_movies) == (31, 122)
    store = FS.FeatureStore.from_ratings(ratings, movies)
    _assert_same_store(store, want[5], 5, 31, 122)
    assert store.has_user([30, 12, 2, 4]).tolist() == [True, True, False, False]


def test_one_user_longer_than_the_lds_sort():
    """4097 ratings of one user at the default capacity of 4096: two sorted chunks and one merge pass; many equal timestamps."""
    rng = np.random.RandomState(2)
    n = 4097
    ratings = {"userId": np.full(n, 3), "movieId": rng.randint(1, 120, n), "rating": rng.randint(1, 11, n) / 2.0, "timestamp": rng.randint(0, 900, n)}
    movies = FE.movie_table(cases.synthetic_movies())
    want = FE.samples_host(ratings, movies)
    assert len(want["userId"]) == n - 2
    _check(ratings, movies, want, 5, n_users=5, n_movies=120)


def test_two_runs_give_the_same_bytes(synthetic):
    ratings, movies, _ = synthetic
    runs = []
    for _ in range(2):
        built = FE.build(ratings, movies, 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
        runs.append([v.tobytes() for v in built.to_host().values()] + [t.cpu().numpy().tobytes() for t in built.store().tensors()])
    assert runs[0] == runs[1]


def test_error_word_names_the_row_of_the_host_error(synthetic):
    ratings, movies, _ = synthetic
    def both(r, **kw):
        with pytest.raises(ValueError) as host:
            FE.samples_host(r, movies, **kw)
        with pytest.raises(ValueError) as device:
            FE.build(r, movies, **kw)
        assert str(host.value) == str(device.value)
        return str(host.value)
    r = {k: v.copy() for k, v in ratings.items()}
    r["rating"][[800, 40]] = [3.7, np.nan]
    assert both(r).startswith("ratings row 40: rating")
    r["movieId"][[700, 77]] = [150, -1]
    assert both(r, n_users=cases.N_USERS, n_movies=cases.N_MOVIES).startswith("ratings row 77: movieId")
    r["userId"][[820, 300]] = [-5, 2**31 + 7]
    assert both(r, n_users=cases.N_USERS, n_movies=cases.N_MOVIES).startswith("ratings row 300: userId")
    assert both(r).startswith("ratings row 300: userId")


# ---- the kernels' tile, grid and width edges (docs/feature_eng_results.md, "Test coverage") ----
@pytest.fixture(scope="module")
def synthetic_table():
    return FE.movie_table(cases.synthetic_movies())


def test_all_32_genre_counters(lib):
    """Every dictionary id 0 .. 31 leads a top five, and ids of different counter registers tie (tests/test_featureeng.py asserts both)."""
    ratings, movies = cases.all_genres_ratings(), FE.movie_table(cases.all_genres_movies())
    _check(ratings, movies, FE.samples_host(ratings, movies, 5), 5, n_users=cases.ALL_GENRES_USERS, n_movies=cases.ALL_GENRES_MOVIES)


@pytest.fixture(scope="module")
def merge_shapes(lib, synthetic_table):
    ratings = cases.merge_shapes_ratings()
    return ratings, FE.samples_host(ratings, synthetic_table, 5)


@pytest.mark.parametrize("sort_cap", [64, 128, None])
def test_merge_shapes(merge_shapes, synthetic_table, monkeypatch, sort_cap):
    """Segments of exactly 1, 2, 3 and 5 chunks and of one rating more, 16 chunks, one timestamp throughout, descending timestamps, INT64_MAX
    (the LDS sort's padding) and INT64_MIN as timestamps.  Capacity 64: six merge passes; 128: five, so the copy back runs too."""
    ratings, want = merge_shapes
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    _check(ratings, synthetic_table, want, 5, n_users=cases.MERGE_USERS)


def test_rating_scale_ends(lib, synthetic_table):
    """0.0, -0.0 and 10.0; the window {0.0, 10.0} (stddev 7.07); a window of a hundred 10.0."""
    ratings = cases.scale_ends_ratings()
    _check(ratings, synthetic_table, FE.samples_host(ratings, synthetic_table, 5), 5, n_users=cases.SCALE_USERS)


@pytest.mark.parametrize("hist_len", [1, 100])
def test_shortest_and_longest_history(synthetic, hist_len):
    ratings, movies, _ = synthetic
    _check(ratings, movies, FE.samples_host(ratings, movies, hist_len), hist_len)


def test_users_across_scan_tiles_and_rounds(lib, synthetic_table):
    """300 000 user ids, about fifty of them with ratings, on both sides of the 1024-user scan tiles and of the 256-tile round of
    k_fe_scan_tops: a wrong tile base or a lost carry puts two users' segments, or their samples, on top of each other."""
    n_users = 300_000
    ratings = cases.sparse_users_ratings(n_users)
    built = _check(ratings, synthetic_table, FE.samples_host(ratings, synthetic_table, 5), 5, n_users=n_users)
    lens = np.bincount(ratings["userId"], minlength=n_users)
    assert int(built.store().tensors()[1].sum()) == int((lens >= 3).sum())


@pytest.fixture(scope="module")
def singletons(lib, synthetic_table):
    case = cases.singletons_ratings()
    return case, cases.singletons_expectation(case, synthetic_table, 5)


def test_one_movie_of_4_5_million_ratings_and_users_past_the_sort_grid(singletons, synthetic_table):
    """The popular movie's stddev needs the 128-bit products (64-bit ones give another value: tests/test_featureeng.py); the ordinary
    users sit in the first, second and third stride of k_fe_sort_short's grid; k_fe_hist and k_fe_scatter stride over the ratings."""
    case, want = singletons
    n, s, q = case["popular"]
    built = _check(case["ratings"], synthetic_table, want, 5, n_users=case["n_users"], n_movies=case["n_movies"])
    user_rows, user_has, movie_rows, movie_has = built.store().tensors()
    assert np.array_equal(np.flatnonzero(user_has.cpu().numpy()), case["ordinary_users"])
    row = movie_rows[cases.POPULAR_MOVIE].cpu().numpy()
    assert movie_has[cases.POPULAR_MOVIE] == 1
    assert row[4:7].view(np.float32).tolist() == [np.float32(n), FE.hundredths(FE.avg_h(n, s)), FE.hundredths(FE.sd_h(n, s, q))]


@pytest.fixture(scope="module")
def one_long_user(lib, synthetic_table):
    ratings = cases.one_long_user_ratings()
    return ratings, FE.samples_host(ratings, synthetic_table, 5)


@pytest.mark.parametrize("sort_cap", [64, 128])
def test_one_user_longer_than_the_capped_grids(one_long_user, synthetic_table, monkeypatch, sort_cap):
    """530 000 ratings of one user: more than 2048 x 256 positions, so k_fe_merge_pass strides, and more than 2048 chunks, so
    k_fe_sort_long_chunks does.  Capacity 64: 8 282 chunks, fourteen merge passes; 128: 4 141 chunks, thirteen passes, after which
    k_fe_long_copy runs, and strides."""
    ratings, want = one_long_user
    monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    _check(ratings, synthetic_table, want, 5, n_users=4)


def _same_error(ratings, movies, **kw):
    with pytest.raises(ValueError) as host:
        FE.samples_host(ratings, movies, **kw)
    with pytest.raises(ValueError) as device:
        FE.build(ratings, movies, **kw)
    assert str(host.value) == str(device.value)
    return str(host.value)


@pytest.mark.parametrize("bad", [1e-45, np.inf, -np.inf, 10.5, -0.5, 0.25])
def test_ratings_next_to_the_scale_are_errors(synthetic, bad):
    """The neighbours of the valid values: a float32 denormal (a flush-to-zero compare would take it for 0.0), the infinities, half a
    star beyond either end, a quarter star."""
    ratings, movies, _ = synthetic
    r = {k: v.copy() for k, v in ratings.items()}
    r["rating"][123] = bad
    assert np.float32(bad) != 0
    assert _same_error(r, movies, n_users=cases.N_USERS, n_movies=cases.N_MOVIES) == "ratings row 123: rating off the half-star scale 0, 0.5 .. 10"


def test_error_word_names_the_lower_of_two_rows_in_different_grid_strides(singletons, synthetic_table):
    case, _ = singletons
    r = dict(case["ratings"], rating=case["ratings"]["rating"].copy())
    low, high = 1_000_003, 4_000_001                           # more than 2048 x 256 apart: k_fe_hist meets them in different strides
    assert high - low > 2048 * 256
    r["rating"][[low, high]] = [0.75, np.nan]
    assert _same_error(r, synthetic_table, n_users=case["n_users"], n_movies=case["n_movies"]).startswith("ratings row %d: rating" % low)


def _empty_ratings():
    return {"userId": np.zeros(0, np.int64), "movieId": np.zeros(0, np.int64), "rating": np.zeros(0, np.float64), "timestamp": np.zeros(0, np.int64)}


@pytest.mark.parametrize("shape", ["no ratings", "no users", "no user of three ratings"])
def test_empty_inputs(lib, synthetic_table, shape):
    """No rating at all with a movie table, a user table of no rows, and ratings none of which becomes a sample."""
    n_users = 0 if shape == "no users" else cases.N_USERS
    ratings = _empty_ratings()
    if shape == "no user of three ratings":
        ratings = {"userId": np.array([3, 9, 9, 5, 39, 39]), "movieId": np.array([1, 3, 5, 7, 9, 1]), "rating": np.array([4.0, 5.0, 0.5, 3.5, 4.0, 4.5]),
                   "timestamp": np.array([5, 4, 3, 2, 1, 0])}
    want = FE.samples_host(ratings, synthetic_table, 5, n_users=n_users, n_movies=cases.N_MOVIES)
    assert len(want["userId"]) == 0
    built = _check(ratings, synthetic_table, want, 5, n_users=n_users)
    assert built.n_samples == 0 and all(v.shape[0] == 0 for v in built.to_host().values())
    user_rows, user_has, movie_rows, movie_has = (t.cpu().numpy() for t in built.store().tensors())
    assert user_rows.shape[0] == n_users + 1 and not user_has.any() and not movie_has.any()
    assert (user_rows[:n_users, 5:10] == -1).all() and not user_rows[:n_users, :5].any() and not user_rows[:n_users, 10:].any()
    assert (movie_rows[:-1, :3] == -1).all() and not movie_rows[:-1, 3:].any()


FILL = 0xA5
GUARD_ROWS, GUARD_BYTES = 64, 4096


def _call_with_guards(lib, ratings, table, hist_len, n_users, n_movies):
    """sprk_feature_eng through ctypes with featureeng.build's argument list; every output column has GUARD_ROWS rows past n, the
    workspace is a slice of exactly the advertised length with GUARD_BYTES on either side, everything filled with FILL beforehand.
    -> (kept, the output columns as numpy arrays of n + GUARD_ROWS rows, the bytes before and after the workspace)."""
    import ctypes as C

    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    u, m, r, t = FE._rating_columns(ratings)
    n = len(u)
    table = FE._padded(table, n_movies)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    u_d, m_d, r_d, t_d = up(u.astype(np.int32)), up(m.astype(np.int32)), up(r), up(t)
    year_d, genre_d, mask_d = up(table.year), up(table.genre), up(table.mask.view(np.int32))
    def filled(shape, dtype):
        n_bytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        return torch.full((n_bytes,), FILL, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)
    rows = n + GUARD_ROWS
    outs = {"user": filled((rows,), torch.int32), "movie": filled((rows,), torch.int32), "rating": filled((rows,), torch.float32),
            "ts": filled((rows,), torch.int64), "label": filled((rows,), torch.int32), "src": filled((rows,), torch.int32),
            "genres": filled((rows, 8), torch.int32), "hist": filled((rows, hist_len), torch.int32), "dense": filled((rows, 7), torch.float32)}
    pitch = FS.user_pitch(hist_len)
    user_rows, user_has = filled((n_users + GUARD_ROWS, pitch), torch.int32), filled((n_users + GUARD_ROWS,), torch.uint8)
    movie_rows, movie_has = filled((n_movies + GUARD_ROWS, 8), torch.int32), filled((n_movies + GUARD_ROWS,), torch.uint8)
    words = torch.tensor([-1, 0], dtype=torch.int64, device=dev)
    ws_bytes = lib.sprk_feature_eng_workspace_bytes(n, n_users, n_movies)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    arena = torch.full((GUARD_BYTES + ws_bytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device=dev)
    assert arena.data_ptr() % 16 == 0
    p = lambda x: C.c_void_p(x.data_ptr())
    o = outs
    L.check(lib.sprk_feature_eng(p(u_d), p(m_d), p(r_d), p(t_d), n, n_users, n_movies, p(year_d), p(genre_d), p(mask_d), S.N_GENRES, hist_len,
                                 p(o["user"]), p(o["movie"]), p(o["rating"]), p(o["ts"]), p(o["label"]), p(o["src"]), p(o["genres"]), p(o["hist"]), p(o["dense"]),
                                 p(user_rows), p(user_has), pitch, p(movie_rows), p(movie_has),
                                 C.c_void_p(words.data_ptr()), C.c_void_p(words.data_ptr() + 8), C.c_void_p(arena.data_ptr() + GUARD_BYTES), ws_bytes,
                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    err, kept = (int(v) for v in words.cpu().numpy())
    assert err == -1
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    tables = [x.cpu().numpy() for x in (user_rows, user_has, movie_rows, movie_has)]
    arena = arena.cpu().numpy()
    return kept, host, tables, arena[:GUARD_BYTES], arena[GUARD_BYTES + ws_bytes:]


def _is_fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


@pytest.mark.parametrize("which,sort_cap", [("synthetic", 64), ("synthetic", None), ("merge_shapes", 64)])
def test_nothing_is_written_outside_the_workspace_or_past_the_kept_rows(lib, synthetic, merge_shapes, synthetic_table, monkeypatch, which, sort_cap):
    """The sixteen arrays carved from the workspace stay inside sprk_feature_eng_workspace_bytes, the sample columns inside their kept
    rows and the store's tables inside n_users / n_movies rows: the guard bands around each keep their fill."""
    if which == "synthetic":
        ratings, want, n_users = synthetic[0], synthetic[2][5], cases.N_USERS
    else:
        (ratings, want), n_users = merge_shapes, cases.MERGE_USERS
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    n = len(ratings["userId"])
    kept, outs, tables, before, after = _call_with_guards(lib, ratings, synthetic_table, 5, n_users, cases.N_MOVIES)
    assert _is_fill(before) and _is_fill(after)
    assert kept == len(want["userId"]) and kept < n
    for name, a in outs.items():
        assert a.shape[0] == n + GUARD_ROWS and _is_fill(a[kept:]), name
    got = FE._columns_dict(5, *(outs[k][:kept] for k in ("user", "movie", "rating", "ts", "label", "src", "genres", "hist", "dense")))
    _assert_same_columns(got, want)
    images = FS.row_images_from_samples(want, 5, n_users, cases.N_MOVIES)
    for a, w, rows in zip(tables, images[:4], (n_users, n_users, cases.N_MOVIES, cases.N_MOVIES)):
        assert a[:rows].tobytes() == w.tobytes() and _is_fill(a[rows:])
