"""Feature engineering on the device (sprk_feature_eng, csrc/k_feature_eng.h) against its definition, featureeng.samples_host: the
sample columns, the kept-sample count and the store's tables bit for bit; the error word names the row the host error names."""
import numpy as np
import pytest

from sparrowrecsys_amd import featureeng as FE
from sparrowrecsys_amd import featurestore as FS
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
