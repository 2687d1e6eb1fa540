"""Feature engineering on the host (sparrowrecsys_amd/featureeng.py): the definition the device path must equal.  The movie side and
the rounding rules are pinned by the reference's own data (tests/golden/test_samples_512.csv and the matching lines of its movies.csv);
the reference ships no ratings.csv, so the user windows are pinned by a hand-worked example."""
import ctypes as C
import decimal
import itertools
import os

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import featureeng as FE
from sparrowrecsys_amd import featurestore as FS
from sparrowrecsys_amd import schema as S
from tests import featureeng_cases as cases
from tests.conftest import GOLDEN

MOVIES_CSV = os.path.join(GOLDEN, "movies_for_samples_512.csv")
SAMPLES_CSV = os.path.join(GOLDEN, "test_samples_512.csv")


@pytest.fixture(scope="module")
def excerpt():
    return S.read_samples_csv(SAMPLES_CSV)


def test_movie_table_reproduces_the_reference_movie_columns(excerpt):
    table = FE.movie_table(MOVIES_CSV)
    assert int(table.has.sum()) == 255 and table.dictionary[:S.N_GENRES] == S.GENRE_VOCAB
    for i in range(len(excerpt["movieId"])):
        m = int(excerpt["movieId"][i])
        assert table.has[m]
        assert table.year[m] == int(excerpt["releaseYear"][i]), (i, m)
        for k, key in enumerate(S.MOVIE_GENRE_KEYS):
            assert table.genre[m, k] == S._GENRE_INDEX.get(excerpt[key][i], -1), (i, m, key)


def _hundredths_of(text):
    return int(decimal.Decimal(text).scaleb(2).to_integral_exact())


def _reachable(n, population):
    """Every (avg_h, sd_h) that n half-star ratings 0.5 .. 5.0 can give under the rounding rules (sample stddev), or with a population
    stddev rounded the same way."""
    out = set()
    for ms in itertools.combinations_with_replacement(range(1, 11), n):
        s, q = sum(ms), sum(x * x for x in ms)
        if population:
            with decimal.localcontext() as ctx:
                ctx.prec = 60
                sd = int((100 * (decimal.Decimal(n * q - s * s) / (4 * n * n)).sqrt()).quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_EVEN))
        else:
            sd = FE.sd_h(n, s, q)
        out.add((FE.avg_h(n, s), sd))
    return out


def test_rounding_rules_explain_the_reference_user_columns(excerpt):
    rows = [i for i in range(len(excerpt["userId"])) if int(excerpt["userRatingCount"][i]) <= 7]
    assert len(rows) == 77
    sample = {n: _reachable(n, False) for n in range(2, 8)}
    population = {n: _reachable(n, True) for n in range(2, 8)}
    unexplained = 0
    for i in rows:
        n = int(excerpt["userRatingCount"][i])
        got = (_hundredths_of(excerpt["userAvgRating"][i]), _hundredths_of(excerpt["userRatingStddev"][i]))
        assert got in sample[n], (i, n, got)
        unexplained += got not in population[n]
    assert unexplained >= 1                                   # the check tells a sample stddev from a population stddev


def test_stored_float_equals_the_two_decimal_text():
    h = np.arange(100_001)
    text = np.array(["%.2f" % (v / 100) for v in h]).astype(np.float32)
    assert np.array_equal(FE.hundredths(h).view(np.int32), text.view(np.int32))


def _decimal_avg_sd(n, s, q):
    with decimal.localcontext() as ctx:
        ctx.prec = 200
        one = decimal.Decimal(1)
        avg = (decimal.Decimal(50 * s) / n).quantize(one, rounding=decimal.ROUND_HALF_EVEN)
        sd = decimal.Decimal(0) if n < 2 else (100 * (decimal.Decimal(n * q - s * s) / (4 * n * (n - 1))).sqrt()).quantize(one, rounding=decimal.ROUND_HALF_EVEN)
        return int(avg), int(sd)


def test_integer_rounding_against_decimal_arithmetic():
    for n in range(1, 5):
        for ms in itertools.combinations_with_replacement(range(0, 21), n):
            s, q = sum(ms), sum(x * x for x in ms)
            assert (FE.avg_h(n, s), FE.sd_h(n, s, q)) == _decimal_avg_sd(n, s, q), ms
    rng = np.random.RandomState(3)
    for trial in range(300):
        n = int(rng.choice([2, 3, 100, 101, 65_537, 2**31 - 1])) if trial % 2 else int(rng.randint(2, 2**31 - 1))
        cuts = np.sort(rng.randint(0, n + 1, size=20))
        counts = np.diff(np.concatenate([[0], cuts, [n]]))    # n ratings over the 21 values 0, 0.5 .. 10
        s = sum(int(c) * k for k, c in enumerate(counts))
        q = sum(int(c) * k * k for k, c in enumerate(counts))
        assert (FE.avg_h(n, s), FE.sd_h(n, s, q)) == _decimal_avg_sd(n, s, q), (n, s, q)
        if n <= 100:
            a = np.array([n], dtype=np.int64)
            assert (int(FE._avg_h_vec(a, np.array([s]))[0]), int(FE._sd_h_vec(a, np.array([s]), np.array([q]))[0])) == (FE.avg_h(n, s), FE.sd_h(n, s, q))
    # exact ties.  Average: seven 3.0 and one 3.5 -> 3.0625 -> 3.06; 3.0, 3.0, 3.5, 3.5 -> 3.25 stays, 4 x 3.0 + 3.5 ... 362.5 -> 362, 363.5 -> 364
    assert FE.avg_h(8, 7 * 6 + 7) == 306 == _decimal_avg_sd(8, 49, 7 * 36 + 49)[0]
    assert FE.avg_h(4, 29) == 362 and FE.avg_h(20, 20 * 7 + 11) == 378      # 362.5 -> 362 (even), 377.5 -> 378 (even)
    # Stddev: fifteen ratings a and one a + 0.5 -> exactly 0.125 -> 0.12 (even); one a + 1.5 instead -> exactly 0.375 -> 0.38 (to even, up)
    assert FE.sd_h(16, 15 * 6 + 7, 15 * 36 + 49) == 12 == _decimal_avg_sd(16, 97, 15 * 36 + 49)[1]
    assert FE.sd_h(16, 15 * 6 + 9, 15 * 36 + 81) == 38 == _decimal_avg_sd(16, 99, 15 * 36 + 81)[1]
    a = np.array([16, 16], dtype=np.int64)
    assert FE._sd_h_vec(a, np.array([97, 99]), np.array([15 * 36 + 49, 15 * 36 + 81])).tolist() == [12, 38]


def test_hand_worked_user():
    """User 7 of featureeng_cases.HAND_RATINGS.  In (timestamp, input row) order its ratings are
         p0 movie 1  4.0 t100 (row 3)   p1 movie 2  2.0 t200 (row 5)   p2 movie 3  5.0 t300 (row 1)   p3 movie 5  3.5 t300 (row 4)
         p4 movie 9  4.5 t400 (row 6)   p5 movie 4  1.5 t500 (row 0)   p6 movie 1  3.0 t600 (row 2)
    p0 and p1 are dropped (windows of 0 and 1 ratings).  Dictionary ids: Film-Noir 0, Adventure 2, Comedy 6, Drama 10, Fantasy 13,
    Animation 14, Children 17, Zydeco 19 (outside the vocabulary).  Windows:
      p2: {4.0, 2.0}: avg 3.00, sd sqrt(2) = 1.41; positives: movie 1; its five genres once each -> by id 2, 6, 13, 14, 17
      p3: {4.0, 2.0, 5.0}: avg 3.667 -> 3.67, sd 1.5275 -> 1.53; positives 3, 1; seven genres once each -> 2, 6, 10, 13, 14
      p4: + 3.5: avg 3.625 -> 3.62 (tie, to even), sd exactly 1.25; positives 5, 3, 1; Zydeco twice, then 0, 2, 6, 10
      p5: + 4.5: avg 3.80, sd 1.1511 -> 1.15; positives 9, 5, 3, 1 (movie 9 has no genres)
      p6: + 1.5: avg 3.4167 -> 3.42, sd 1.3934 -> 1.39
    Movie 1 is rated 4.0, 3.0 and (user 3) 5.0: count 3, avg 4.00, sd 1.00; the others once: sd 0."""
    got = FE.samples_host(cases.HAND_RATINGS, cases.HAND_MOVIES)
    f = np.float32
    want = {
        "userId": [7] * 5, "movieId": [3, 5, 9, 4, 1], "rating": [5.0, 3.5, 4.5, 1.5, 3.0], "timestamp": [300, 300, 400, 500, 600],
        "label": [1, 1, 1, 0, 0], "source_row": [1, 4, 6, 0, 2],
        "movieGenre1": [-1, 0, -1, 6, 2], "movieGenre2": [10, -1, -1, -1, 14], "movieGenre3": [-1, -1, -1, -1, 17],
        "userGenre1": [2, 2, -1, -1, -1], "userGenre2": [6, 6, 0, 0, 0], "userGenre3": [13, 10, 2, 2, 2], "userGenre4": [14, 13, 6, 6, 6],
        "userGenre5": [17, 14, 10, 10, 10],
        "userRatedMovie1": [1, 3, 5, 9, 9], "userRatedMovie2": [0, 1, 3, 5, 5], "userRatedMovie3": [0, 0, 1, 3, 3],
        "userRatedMovie4": [0, 0, 0, 1, 1], "userRatedMovie5": [0, 0, 0, 0, 0],
        "releaseYear": [2001, 1950, 1990, 1990, 1995], "movieRatingCount": [1, 1, 1, 1, 3],
        "movieAvgRating": [f("5.00"), f("3.50"), f("4.50"), f("1.50"), f("4.00")], "movieRatingStddev": [0, 0, 0, 0, f("1.00")],
        "userRatingCount": [2, 3, 4, 5, 6], "userAvgRating": [f("3.00"), f("3.67"), f("3.62"), f("3.80"), f("3.42")],
        "userRatingStddev": [f("1.41"), f("1.53"), f("1.25"), f("1.15"), f("1.39")],
    }
    assert list(got) == FE.sample_keys(5) and set(got) == set(want)
    for k, v in want.items():
        assert got[k].dtype == (np.float32 if k in FE.DENSE_KEYS + ["rating"] else np.int64 if k == "timestamp" else np.int32), k
        assert np.array_equal(got[k], np.asarray(v, dtype=got[k].dtype)), (k, got[k])
    # a longer history keeps the same values and adds empty places
    got12 = FE.samples_host(cases.HAND_RATINGS, cases.HAND_MOVIES, hist_len=12)
    assert got12["userRatedMovie4"].tolist() == [0, 0, 0, 1, 1] and not got12["userRatedMovie12"].any()
    # hist_len 2 = the two most recent positives
    got2 = FE.samples_host(cases.HAND_RATINGS, cases.HAND_MOVIES, hist_len=2)
    assert got2["userRatedMovie2"].tolist() == [0, 1, 3, 5, 5] and "userRatedMovie3" not in got2


def test_samples_are_accepted_by_the_column_packer_and_the_store():
    from sparrowrecsys_amd import models as M
    got = FE.samples_host(cases.synthetic_ratings(), cases.synthetic_movies())
    for model in (M.DeepFM(seed=1), M.DIN(seed=1)):
        ids, dense = model.pack(got)
        assert ids.shape[0] == dense.shape[0] == len(got["userId"])
    store = FS.FeatureStore.from_samples(got, device="cpu")
    assert store.has_user([30, 12, 2, 4, 5]).tolist() == [True, True, False, False, True]


def test_title_rule():
    assert FE.release_year("Heat (1995)") == 1995
    assert FE.release_year("Short") == 1990 and FE.release_year("  ab   ") == 1990 and FE.release_year(None) == 1990
    for title in ("Toy Story (1995) ", "Toy Story (199x)", "Toy Story 1995", " Toy Story (1995)"):
        with pytest.raises(ValueError, match="movie 12"):
            FE.movie_table({"movieId": [12], "title": [title], "genres": ["Comedy"]})


def test_validation():
    r = {k: v.copy() for k, v in cases.HAND_RATINGS.items()}
    r["rating"][5] = 3.7
    r["rating"][6] = 11.0
    with pytest.raises(ValueError, match="ratings row 5: rating"):
        FE.samples_host(r, cases.HAND_MOVIES)
    r["movieId"][6] = -2
    with pytest.raises(ValueError, match="ratings row 6: movieId"):        # the kind comes first, then the row
        FE.samples_host(r, cases.HAND_MOVIES)
    r["userId"][7] = -1
    with pytest.raises(ValueError, match="ratings row 7: userId"):
        FE.samples_host(r, cases.HAND_MOVIES)
    with pytest.raises(ValueError, match="ratings row 0: userId"):
        FE.samples_host(cases.HAND_RATINGS, cases.HAND_MOVIES, n_users=7)
    with pytest.raises(ValueError, match="ratings row 6: movieId"):
        FE.samples_host(cases.HAND_RATINGS, cases.HAND_MOVIES, n_movies=9)
    many = {"movieId": list(range(14)), "title": ["T (2000)"] * 14, "genres": ["G%d" % k for k in range(14)]}
    with pytest.raises(ValueError, match="more than 32"):
        FE.movie_table(many)
    assert len(FE.movie_table({k: v[:13] for k, v in many.items()}).dictionary) == 32
    with pytest.raises(ValueError, match="hist_len"):
        FE.samples_host(cases.HAND_RATINGS, cases.HAND_MOVIES, hist_len=101)


@pytest.mark.parametrize("hist_len", [5, 12])
def test_store_from_ratings_equals_the_images_of_the_host_samples(hist_len):
    ratings, movies = cases.synthetic_ratings(), cases.synthetic_movies()
    store = FS.FeatureStore.from_ratings(ratings, movies, hist_len=hist_len, device="cpu", n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    want = FS.row_images_from_samples(FE.samples_host(ratings, movies, hist_len), hist_len, cases.N_USERS, cases.N_MOVIES)
    assert store.images.hist_len == hist_len and store.n_users == cases.N_USERS and store.n_movies == cases.N_MOVIES
    for a, b in zip(store.images[:4], want[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # users with fewer than three ratings have no sample, hence no row; movie 121 (not in the movie table) has one
    assert store.images.user_has[[2, 4, 5, 12, 39]].tolist() == [0, 0, 1, 1, 0]
    assert store.images.movie_has[[117, 121, 149]].tolist() == [1, 1, 0]
    # default sizes: the greatest id of the ratings + 1
    small = FS.FeatureStore.from_ratings(ratings, movies, hist_len=hist_len, device="cpu")
    assert (small.n_users, small.n_movies) == (31, 122)


def test_synthetic_set_holds_the_cases_it_names():
    """The GPU tests rely on these properties of featureeng_cases.synthetic_ratings."""
    ratings, movies = cases.synthetic_ratings(), cases.synthetic_movies()
    table = FE.movie_table(movies)
    assert "Zydeco" in table.dictionary[S.N_GENRES:]
    lens = np.bincount(ratings["userId"], minlength=cases.N_USERS)
    assert [int(lens[u]) for u in (0, 2, 4, 5, 8, 9, 10, 12)] == [0, 1, 2, 3, 100, 101, 102, 250]
    got = FE.samples_host(ratings, movies)
    assert len(got["userId"]) == int(np.maximum(lens - 2, 0).sum())
    of = lambda u: got["userId"] == u
    assert got["userRatingCount"][of(10)].tolist() == list(range(2, 100)) + [100, 100]
    assert got["userRatingCount"][of(9)].max() == 100 and got["userRatingCount"][of(8)].max() == 99
    assert not got["userRatedMovie1"][of(15)].any() and (got["userGenre1"][of(15)] == -1).all()
    h17 = np.stack([got["userRatedMovie%d" % k][of(17)] for k in range(1, 6)], axis=1)
    n_hist = (h17 != 0).sum(axis=1)
    assert n_hist.max() == 5 and set(n_hist[-14:].tolist()) == {4, 3, 2, 1, 0}
    assert (got["userGenre1"][of(20)] == -1).all() and (got["userGenre2"][of(20)] >= 0).all()   # Zydeco leads, unnamed
    assert (got["releaseYear"][got["movieId"] == 121] == 1990).all() and (got["movieGenre1"][got["movieId"] == 121] == -1).all()
    assert got["movieRatingCount"][got["movieId"] == 117].tolist() == [1.0]
    ts14 = got["source_row"][of(14)]
    assert (np.diff(ts14) > 0).all()                           # one timestamp: input row order


def test_feature_eng_abi_rejects_bad_arguments_before_any_device_call(lib):
    n, nu, nm, H = 8, 4, 4, 5
    need = lib.sprk_feature_eng_workspace_bytes(n, nu, nm)
    assert need > 0 and need % 16 == 0
    assert lib.sprk_feature_eng_workspace_bytes(-1, nu, nm) == 0 and lib.sprk_feature_eng_workspace_bytes(n, -1, nm) == 0
    assert lib.sprk_feature_eng_workspace_bytes(2**31 - 1, nu, nm) == 0
    # host memory stands in for device memory: every call below must return before it touches any of it
    buf = (C.c_uint64 * (need // 8 + 64))()
    p = C.c_void_p(C.addressof(buf))
    def call(**kw):
        a = dict(user=p, movie=p, rating=p, ts=p, n=n, nu=nu, nm=nm, year=p, g3=p, mask=p, vocab=S.N_GENRES, H=H, out=p, ur=p, uh=p, pitch=FS.user_pitch(H),
                 mr=p, mh=p, err=p, kept=p, ws=p, ws_bytes=need)
        a.update(kw)
        return lib.sprk_feature_eng(a["user"], a["movie"], a["rating"], a["ts"], a["n"], a["nu"], a["nm"], a["year"], a["g3"], a["mask"], a["vocab"], a["H"],
                                    a["out"], a["out"], a["out"], a["out"], a["out"], a["out"], a["out"], a["out"], a["out"],
                                    a["ur"], a["uh"], a["pitch"], a["mr"], a["mh"], a["err"], a["kept"], a["ws"], a["ws_bytes"], None)
    bad = [dict(user=None), dict(ts=None), dict(year=None), dict(mask=None), dict(out=None), dict(err=None), dict(kept=None), dict(ws=None),
           dict(n=-1), dict(nu=-1), dict(nm=-1), dict(n=2**31 - 1), dict(H=0), dict(H=101), dict(vocab=33), dict(vocab=-1),
           dict(ws_bytes=need - 16), dict(ws_bytes=0), dict(ws=C.c_void_p(C.addressof(buf) + 8)), dict(uh=None), dict(mr=None), dict(pitch=H + 7),
           dict(rating=C.c_void_p(C.addressof(buf) + 2))]
    for kw in bad:
        assert call(**kw) == L.EINVAL, kw
        assert b"feature_eng" in lib.sprk_last_error()
    import torch
    if not torch.cuda.is_available():
        assert call() == L.EHIP                                 # a good call reaches the device, and there is none


# ---- the definition against its row-by-row restatement, and the properties of the rating sets the device tests rely on ----
def _assert_same_bytes(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, np.flatnonzero(got[k] != want[k])[:8])


def _restated_sets():
    synthetic = (cases.synthetic_ratings(), cases.synthetic_movies())
    return {
        "hand": (cases.HAND_RATINGS, cases.HAND_MOVIES, 5),
        "synthetic-5": synthetic + (5,),
        "synthetic-12": synthetic + (12,),
        "synthetic-1": synthetic + (1,),
        "synthetic-100": synthetic + (100,),
        "all_genres": (cases.all_genres_ratings(), cases.all_genres_movies(), 5),
        "merge_shapes": (cases.merge_shapes_ratings(), cases.synthetic_movies(), 5),
        "scale_ends": (cases.scale_ends_ratings(), cases.synthetic_movies(), 5),
        "scale_ends-100": (cases.scale_ends_ratings(), cases.synthetic_movies(), 100),
        "sparse_users": (cases.sparse_users_ratings(), cases.synthetic_movies(), 5),
    }


@pytest.mark.parametrize("name", ["hand", "synthetic-5", "synthetic-12", "synthetic-1", "synthetic-100", "all_genres", "merge_shapes", "scale_ends",
                                  "scale_ends-100", "sparse_users"])
def test_definition_equals_its_restatement_row_by_row(name):
    """samples_host (prefix sums, searchsorted, a sort of packed keys) against featureeng_cases.definition_by_rows (DESIGN.md section 5.7
    with loops, fractions and a dict), every column byte for byte.  The restatement loops over the users that have ratings."""
    ratings, movies, hist_len = _restated_sets()[name]
    _assert_same_bytes(FE.samples_host(ratings, movies, hist_len), cases.definition_by_rows(ratings, movies, hist_len))


def _top_fives(got, user):
    return np.stack([got["userGenre%d" % k][got["userId"] == user] for k in range(1, 6)], axis=1)


def test_all_genres_set_holds_the_cases_it_names():
    ratings, movies = cases.all_genres_ratings(), cases.all_genres_movies()
    table = FE.movie_table(movies)
    assert len(table.dictionary) == 32 and table.dictionary[:S.N_GENRES] == S.GENRE_VOCAB
    assert [int(table.mask[g]) for g in range(32)] == [1 << g for g in range(32)]
    assert [int(table.mask[32 + k]) for k in range(8)] == [0x01010101 << k for k in range(8)]
    assert int(ratings["userId"].max()) < cases.ALL_GENRES_USERS and int(ratings["movieId"].max()) < cases.ALL_GENRES_MOVIES
    got = FE.samples_host(ratings, movies)
    name = lambda g: g if g < S.N_GENRES else -1
    for g in range(32):                                        # id g leads with count 3; vocabulary genres follow, so losing g's count shows
        last = _top_fives(got, g)[-1].tolist()
        others = [x for x in range(4) if x != g]
        assert last == ([name(g)] + others + [-1] * 5)[:5], (g, last)
        assert last != (others + [-1] * 5)[:5]
    registers = set()
    for k, (a, b) in enumerate(cases.ALL_GENRES_TIES):
        assert a < b and a // 8 != b // 8                      # a tie across two counter registers: the lower id wins
        registers.add((a // 8, b // 8))
        lead = _top_fives(got, 40 + k)[-1].tolist()
        assert lead == [name(a), name(b), -1, -1, -1], (a, b, lead)
        fifth = _top_fives(got, 50 + k)[-1].tolist()
        assert fifth == [1, 2, 3, 4, name(a)], (a, b, fifth)
        if a < S.N_GENRES <= b:                                # the other order would write -1 here
            assert lead[0] != name(b) and fifth[4] != name(b)
    assert {(0, 1), (1, 2), (2, 3), (0, 3)} <= registers
    for k in range(8):                                         # four registers in one window: ids k (3), k + 8, k + 16 (2 each; k + 24 is unnamed)
        assert _top_fives(got, 60 + k)[-1].tolist() == [k, k + 8, name(k + 16), -1, -1]


def test_merge_shapes_set_holds_the_cases_it_names():
    ratings = cases.merge_shapes_ratings()
    lens = np.bincount(ratings["userId"], minlength=cases.MERGE_USERS)
    assert lens[1:12].tolist() == [64, 65, 128, 129, 192, 320, 321, 1000, 300, 200, 70]
    of = lambda u: ratings["timestamp"][ratings["userId"] == u]
    assert len(set(of(9).tolist())) == 1
    assert (np.diff(of(10)) < 0).all()
    t11 = of(11)
    assert (t11 == cases.INT64_MAX).sum() == 2 and (t11 == cases.INT64_MIN).sum() == 2 and len(set(t11.tolist())) > 20
    got = FE.samples_host(ratings, cases.synthetic_movies())
    assert len(got["userId"]) == int(np.maximum(lens - 2, 0).sum())
    src = lambda u: got["source_row"][got["userId"] == u]
    assert (np.diff(src(9)) > 0).all() and (np.diff(src(10)) < 0).all()
    assert got["timestamp"][got["userId"] == 11][-2:].tolist() == [cases.INT64_MAX] * 2 and (np.diff(src(11)[-2:]) > 0).all()
    assert not np.array_equal(ratings["userId"], np.sort(ratings["userId"]))                  # shuffled


def test_scale_ends_set_holds_the_cases_it_names():
    ratings = cases.scale_ends_ratings()
    one = ratings["rating"][ratings["userId"] == 1]
    assert set(one.tolist()) == {0.0, 10.0} and np.signbit(one).any() and (one == 0).sum() > np.signbit(one).sum()
    got = FE.samples_host(ratings, cases.synthetic_movies())
    first = np.flatnonzero(got["userId"] == 1)[0]
    assert got["userRatingCount"][first] == 2 and got["userAvgRating"][first] == np.float32(5.0) and got["userRatingStddev"][first] == np.float32(7.07)
    assert np.signbit(got["rating"][got["userId"] == 1]).any()                               # -0.0 is written as it came
    two = got["userId"] == 2
    full = two & (got["userRatingCount"] == 100) & (got["userAvgRating"] == np.float32(10.0)) & (got["userRatingStddev"] == 0)
    assert full.sum() == 2 and two.sum() == 110               # positions 100 and 101: windows of a hundred 10.0, S = 2000, Q = 40000


def test_sparse_users_set_holds_the_cases_it_names():
    n_users = 300_000
    ratings = cases.sparse_users_ratings(n_users)
    lens = np.bincount(ratings["userId"], minlength=n_users)
    assert len(lens) == n_users and 2000 <= len(ratings["userId"]) <= 6000
    for u in cases.SPARSE_EDGE_IDS + [n_users - 1]:
        assert 3 <= lens[u] <= 150, u
    assert 50 <= (lens >= 3).sum() <= 55 and (lens == 1).sum() >= 1 and (lens == 2).sum() >= 1
    assert (n_users + 1 + 1023) // 1024 > 256                 # the scan over the tiles' totals takes a second round


def test_singletons_popular_movie_tells_64_bit_products_from_128():
    """The (n, S, Q) of the popular movie of the device test: the exact rule and the same steps wrapped to 64 bits differ."""
    case = cases.singletons_ratings()
    n, s, q = case["popular"]
    assert n >= 4_500_000 and 4 * 512 * 512 * n * (n - 1) > 2**64
    exact, narrow = FE.sd_h(n, s, q), cases.sd_h_in_64_bits(n, s, q)
    print("popular movie: n = %d, S = %d, Q = %d: exact h = %d, 64-bit h = %d" % (n, s, q, exact, narrow))
    assert exact == _decimal_avg_sd(n, s, q)[1] and exact != narrow
    assert cases.sd_h_in_64_bits(100, 1234, 20000) == FE.sd_h(100, 1234, 20000)              # (the emulation is the rule where nothing wraps)
    # the issue's alternating 0.0 / 10.0 figures
    assert [(FE.sd_h(k, 10 * k, 200 * k), cases.sd_h_in_64_bits(k, 10 * k, 200 * k)) for k in (4_000_000, 4_300_000)] == [(500, 500), (500, 24)]
    users = case["ordinary_users"]
    grid = cases.SHORT_SORT_GRID
    assert (users < grid).sum() >= 9 and ((users >= grid) & (users < 2 * grid)).sum() >= 9 and (users >= 2 * grid).sum() >= 9
    lens = np.bincount(case["ratings"]["userId"][case["ordinary_rows"]], minlength=case["n_users"])[users]
    assert lens.min() >= 3 and lens.max() <= 300
    popular = case["ratings"]["movieId"][case["ordinary_rows"]] == cases.POPULAR_MOVIE
    assert 5 <= popular.sum() and n == 4_500_000 + popular.sum()


def test_singletons_expectation_equals_the_definition_on_a_reduced_copy():
    case = cases.singletons_ratings(n_single=20_000)
    movies = cases.synthetic_movies()
    whole = FE.samples_host(case["ratings"], movies, 5, n_users=case["n_users"], n_movies=case["n_movies"])
    _assert_same_bytes(cases.singletons_expectation(case, movies, 5), whole)
    assert len(whole["userId"]) > 1000 and (whole["movieId"] == cases.POPULAR_MOVIE).sum() >= 5
