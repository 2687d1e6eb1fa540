"""The feature store's host side (no GPU): the two tables' row images against a test-side oracle, ``join_plan`` for every model class,
and the argument checks of ``sprk_join_features`` / ``sprk_rank_scores``, which return SPRK_EINVAL before any device call."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import schema as S
from sparrowrecsys_amd.featurestore import (MOVIE_NUMERIC_KEYS, USER_NUMERIC_KEYS, FeatureStore, row_images_from_feature_maps,
                                            row_images_from_samples)
from tests import featurestore_cases as FC

ANY = (1 << 31) - 1
HIST = ["userRatedMovie%d" % i for i in range(1, 6)]
USER_IDS = [S.IdColumn(k, "id", ANY) for k in HIST] + [S.IdColumn(k, "genre", S.N_GENRES) for k in S.USER_GENRE_KEYS]
MOVIE_IDS = [S.IdColumn(k, "genre", S.N_GENRES) for k in S.MOVIE_GENRE_KEYS]


def _oracle_rows(cols, which):
    """{id: the row's dwords (int32)} for every entity of the samples, packed by schema.pack_ids / pack_dense from its latest row."""
    rows = FC.latest_rows(cols, which)
    ids = sorted(rows)
    d = {k: np.array([cols[k][rows[i]] for i in ids], dtype=object) for k in cols}
    a = S.pack_ids(d, USER_IDS if which == "userId" else MOVIE_IDS)
    b = S.pack_dense(d, USER_NUMERIC_KEYS if which == "userId" else MOVIE_NUMERIC_KEYS)
    packed = np.concatenate([a, b.view(np.int32)], axis=1)
    return {i: packed[n] for n, i in enumerate(ids)}


def _check_images(im, cols):
    for which, rows, has, pitch, default in (("userId", im.user_rows, im.user_has, 16, [0] * 5 + [-1] * 5 + [0] * 6),
                                             ("movieId", im.movie_rows, im.movie_has, 8, [-1] * 3 + [0] * 5)):
        want = _oracle_rows(cols, which)
        assert rows.dtype == np.int32 and rows.shape == (max(want) + 1, pitch) and has.dtype == np.uint8
        assert sorted(np.flatnonzero(has).tolist()) == sorted(want)
        expect = np.tile(np.array(default, dtype=np.int32), (rows.shape[0], 1))
        for i, r in want.items():
            expect[i, :r.size] = r
        assert rows.tobytes() == expect.tobytes()


def test_from_samples_row_images_are_the_latest_rows(lib):
    cols = FC.samples()
    im = row_images_from_samples(cols)
    assert im.hist_len == 5
    _check_images(im, cols)
    assert row_images_from_samples(FC.CSV).user_rows.tobytes() == im.user_rows.tobytes()
    # user 25375 has two rows with timestamp 938817779: the later line (userRatingCount 24) wins
    ts = np.array([int(t) for t in cols["timestamp"]])
    mine = np.flatnonzero((cols["userId"] == "25375") & (ts == 938817779))
    assert mine.size == 2 and ts[cols["userId"] == "25375"].max() == 938817779
    assert [cols["userRatingCount"][i] for i in mine][-1] == "24"
    assert im.user_rows[25375, 10:11].view(np.float32)[0] == np.float32(24.0)


def test_timestamp_ties_keep_the_last_input_row(lib):
    cols = {k: np.array(["1", "1", "1"], dtype=object) for k in ("userId", "movieId")}
    cols["timestamp"] = np.array(["5", "9", "9"], dtype=object)
    for k in HIST + S.USER_GENRE_KEYS + S.MOVIE_GENRE_KEYS:
        cols[k] = np.array(["", "", ""], dtype=object)
    for k in USER_NUMERIC_KEYS + MOVIE_NUMERIC_KEYS:
        cols[k] = np.array(["1", "2", "3"], dtype=object)
    im = row_images_from_samples(cols)
    assert im.user_rows[1, 10:13].view(np.float32).tolist() == [3.0, 3.0, 3.0]
    assert im.movie_rows[1, 3:7].view(np.float32).tolist() == [3.0] * 4
    assert im.user_has.tolist() == [0, 1] and im.user_rows[0].tolist() == [0] * 5 + [-1] * 5 + [0] * 6


def test_typed_columns_and_history_matrix_give_the_same_images(lib):
    cols = FC.samples()
    typed = dict(cols)
    for k in ("userId", "movieId", "timestamp", "releaseYear", "movieRatingCount", "userRatingCount"):
        typed[k] = np.array([int(v) if v else 0 for v in cols[k]], dtype=np.int64)
    typed["userRatedMovies"] = np.array([[int(cols[k][i]) if cols[k][i] else 0 for k in HIST] for i in range(len(cols["userId"]))], dtype=np.int32)
    for k in HIST:
        del typed[k]
    a, b = row_images_from_samples(cols), row_images_from_samples(typed)
    assert a.user_rows.tobytes() == b.user_rows.tobytes() and a.movie_rows.tobytes() == b.movie_rows.tobytes()


def test_from_feature_maps_on_string_maps_is_identical(lib):
    cols = FC.samples()
    urow, mrow = FC.latest()
    ukeys = HIST + S.USER_GENRE_KEYS + USER_NUMERIC_KEYS
    mkeys = S.MOVIE_GENRE_KEYS + MOVIE_NUMERIC_KEYS
    # the hashes' own shape: strings; a missing value is an absent key for every other entity, an empty string for the rest
    umaps = {u: {k: cols[k][r] for k in ukeys if cols[k][r] != "" or n % 2} for n, (u, r) in enumerate(urow.items())}
    mmaps = {str(m): {k: cols[k][r] for k in mkeys if cols[k][r] != "" or n % 2} for n, (m, r) in enumerate(mrow.items())}
    a, b = row_images_from_samples(cols), row_images_from_feature_maps(umaps, mmaps)
    assert a.user_rows.tobytes() == b.user_rows.tobytes() and a.user_has.tobytes() == b.user_has.tobytes()
    assert a.movie_rows.tobytes() == b.movie_rows.tobytes() and a.movie_has.tobytes() == b.movie_has.tobytes()


def test_missing_values_are_the_na_defaults(lib):
    im = row_images_from_feature_maps({3: {"userRatedMovie1": "7", "userGenre2": "Drama", "userGenre3": "", "userAvgRating": 3.5, "userGenre4": "NoSuchGenre"},
                                       5: {}}, {2: {"releaseYear": 1995, "movieGenre1": "IMAX"}})
    g = S.GENRE_VOCAB.index
    assert im.user_rows.shape == (6, 16) and im.user_has.tolist() == [0, 0, 0, 1, 0, 1]
    assert im.user_rows[3, :10].tolist() == [7, 0, 0, 0, 0, -1, g("Drama"), -1, -1, -1]
    assert im.user_rows[3, 10:13].view(np.float32).tolist() == [0.0, 3.5, 0.0] and im.user_rows[3, 13:].tolist() == [0, 0, 0]
    assert im.user_rows[5].tolist() == im.user_rows[0].tolist() == [0] * 5 + [-1] * 5 + [0] * 6
    assert im.movie_rows[2, :3].tolist() == [g("IMAX"), -1, -1] and im.movie_rows[2, 3:7].view(np.float32).tolist() == [1995.0, 0.0, 0.0, 0.0]
    assert im.movie_rows[1].tolist() == [-1] * 3 + [0] * 5 and im.movie_has.tolist() == [0, 0, 1]


def test_numbers_next_to_missing_values_keep_one_rounding(lib):
    """A numeric column of a feature map that also has missing entries stays numeric: 16777217 is (float32) 16777216 by one rounding of the
    integer, 0.1 + 2^-27 rounds to float32(0.1)'s neighbour only if it is first cut to a short decimal string."""
    x = 0.1 + 2.0 ** -27
    im = row_images_from_feature_maps({1: {"userRatingCount": 16777217, "userAvgRating": x, "userGenre1": 3, "userRatedMovie2": 9}, 2: {"userGenre2": 4}},
                                      {1: {"movieAvgRating": np.float32(3.3)}, 2: {}})
    assert im.user_rows[1, 10:13].view(np.float32).tolist() == [16777216.0, float(np.float32(x)), 0.0]
    assert im.user_rows[1, :10].tolist() == [0, 9, 0, 0, 0, 3, -1, -1, -1, -1] and im.user_rows[2, :10].tolist() == [0] * 5 + [-1, 4, -1, -1, -1]
    assert im.user_rows[2, 10:13].tolist() == [0, 0, 0]
    assert im.movie_rows[1, 3:7].view(np.float32).tolist() == [0.0, 0.0, float(np.float32(3.3)), 0.0] and im.movie_rows[2].tolist() == [-1] * 3 + [0] * 5


def test_store_attributes_and_wide_history(lib):
    st = FeatureStore.from_samples(FC.samples(), device="cpu")
    assert (st.n_users, st.n_movies, st.hist_len, st.user_pitch, st.movie_pitch) == (st.images.user_rows.shape[0], st.images.movie_rows.shape[0], 5, 16, 8)
    assert st.table_bytes() == st.n_users * 65 + st.n_movies * 33
    with pytest.raises(RuntimeError):
        st.tensors()
    st.close()
    n = 7
    cols = {"userId": np.arange(n), "movieId": np.arange(n), "timestamp": np.arange(n), "userRatedMovies": np.arange(n * 50).reshape(n, 50)}
    for k in S.USER_GENRE_KEYS + S.MOVIE_GENRE_KEYS:
        cols[k] = np.array(["Drama"] * n, dtype=object)
    for k in USER_NUMERIC_KEYS + MOVIE_NUMERIC_KEYS:
        cols[k] = np.ones(n, dtype=np.float32)
    im = row_images_from_samples(cols, hist_len=50)
    assert im.user_rows.shape == (n, 60) and im.user_rows[3, :50].tolist() == list(range(150, 200)) and im.user_rows[3, 58:].tolist() == [0, 0]


# ---- join_plan --------------------------------------------------------------------------------------------------------------------
U, MV = L.JOIN_USER_ROW, L.JOIN_MOVIE_ROW
WANT = {"userId": (L.JOIN_PAIR_USER, 0), "movieId": (L.JOIN_PAIR_MOVIE, 0),
        "userRatedMovie1": (U, 0), "userRatedMovie2": (U, 1), "userRatedMovie3": (U, 2), "userRatedMovie4": (U, 3), "userRatedMovie5": (U, 4),
        "userGenre1": (U, 5), "userGenre2": (U, 6), "userGenre3": (U, 7), "userGenre4": (U, 8), "userGenre5": (U, 9),
        "userRatingCount": (U, 10), "userAvgRating": (U, 11), "userRatingStddev": (U, 12),
        "movieGenre1": (MV, 0), "movieGenre2": (MV, 1), "movieGenre3": (MV, 2),
        "releaseYear": (MV, 3), "movieRatingCount": (MV, 4), "movieAvgRating": (MV, 5), "movieRatingStddev": (MV, 6)}


@pytest.mark.parametrize("cls", [M.NeuralCF, M.EmbeddingMLP, M.WideNDeep, M.DeepFM, M.DeepFMv2, M.DIN, M.DIEN])
def test_join_plan_sources_and_offsets(lib, cls):
    st = FeatureStore.from_samples(FC.samples(), device="cpu")
    model = cls(seed=1)
    plan = model.join_plan(st)
    assert plan.n_id == len(model.id_columns) and plan.n_dense == len(model.numeric_keys)
    for c, got in zip(model.id_columns, plan.id_cols):
        assert got == WANT[c.key] + (L.RULE_GENRE if c.kind == "genre" else L.RULE_IDENTITY, c.vocab), c.key
    for k, got in zip(model.numeric_keys, plan.dense_cols):
        assert got == WANT[k] + (L.RULE_DENSE, 0), k
    for j, t in enumerate(plan.id_cols):
        a = plan.id_array[j]
        assert (a.source, a.offset, a.rule, a.vocab) == t
    for j, t in enumerate(plan.dense_cols):
        a = plan.dense_array[j]
        assert (a.source, a.offset, a.rule, a.vocab) == t


def test_join_plan_refuses_what_the_store_does_not_hold(lib):
    st = FeatureStore.from_samples(FC.samples(), device="cpu")
    with pytest.raises(ValueError, match="userRatedMovie6"):
        M.DIN(seed=1, hist_len=6).join_plan(st)

    class Odd(M.NeuralCF):
        def _id_columns(self):
            return super()._id_columns() + [S.IdColumn("userAge", "id", 100)]
    with pytest.raises(ValueError, match="userAge"):
        Odd(seed=1).join_plan(st)

    class WrongRole(M.NeuralCF):                                   # a numeric of the store read as an identity column
        def _id_columns(self):
            return super()._id_columns() + [S.IdColumn("userRatingCount", "id", 100)]
    with pytest.raises(ValueError, match="userRatingCount"):
        WrongRole(seed=1).join_plan(st)


# ---- argument checks: SPRK_EINVAL before any device call --------------------------------------------------------------------------
def _join_args(**over):
    """A valid call's arguments over host memory (nothing is launched: every case below fails validation)."""
    keep = {"ur": np.zeros((4, 16), np.int32), "uh": np.ones(4, np.uint8), "mr": np.zeros((4, 8), np.int32), "mh": np.ones(4, np.uint8),
            "u": np.zeros(2, np.int32), "m": np.zeros(2, np.int32), "ids": np.zeros((2, 2), np.int32), "dense": np.zeros((2, 1), np.float32),
            "key": np.full(1, -1, np.int64)}
    p = {k: v.ctypes.data for k, v in keep.items()}
    a = dict(user_rows=p["ur"], user_has=p["uh"], n_users=4, user_pitch=16, movie_rows=p["mr"], movie_has=p["mh"], n_movies=4, movie_pitch=8,
             user_ids=p["u"], movie_ids=p["m"], Q=2, C=1, shared=0,
             id_cols=(L.JoinCol * 2)(L.JoinCol(L.JOIN_PAIR_USER, 0, L.RULE_IDENTITY, 10), L.JoinCol(L.JOIN_USER_ROW, 5, L.RULE_GENRE, 19)), n_id=2,
             dense_cols=(L.JoinCol * 1)(L.JoinCol(L.JOIN_MOVIE_ROW, 3, L.RULE_DENSE, 0)), n_dense=1,
             ids_out=p["ids"], dense_out=p["dense"], key=p["key"])
    a.update(over)
    return keep, a


def _join_rc(lib, **over):
    keep, a = _join_args(**over)
    vp = C.c_void_p
    return lib.sprk_join_features(vp(a["user_rows"]), vp(a["user_has"]), a["n_users"], a["user_pitch"], vp(a["movie_rows"]), vp(a["movie_has"]),
                                  a["n_movies"], a["movie_pitch"], vp(a["user_ids"]), vp(a["movie_ids"]), a["Q"], a["C"], a["shared"],
                                  a["id_cols"], a["n_id"], a["dense_cols"], a["n_dense"], vp(a["ids_out"]), vp(a["dense_out"]), vp(a["key"]), None)


def test_join_features_arguments_are_validated_before_any_device_call(lib):
    for name in ("user_rows", "user_has", "movie_rows", "movie_has", "user_ids", "movie_ids", "ids_out", "dense_out", "key"):
        assert _join_rc(lib, **{name: None}) == L.EINVAL, name
    assert _join_rc(lib, id_cols=None) == L.EINVAL and _join_rc(lib, dense_cols=None) == L.EINVAL
    assert _join_rc(lib, Q=-1) == L.EINVAL and _join_rc(lib, C=-1) == L.EINVAL
    assert _join_rc(lib, n_id=-1) == L.EINVAL and _join_rc(lib, n_dense=-1) == L.EINVAL
    many = (L.JoinCol * 129)(*[L.JoinCol(L.JOIN_USER_ROW, 0, L.RULE_IDENTITY, 10)] * 129)
    assert _join_rc(lib, id_cols=many, n_id=129, n_dense=0) == L.EINVAL and b"128" in lib.sprk_last_error()
    assert _join_rc(lib, id_cols=many, n_id=128, n_dense=1) == L.EINVAL

    def ids(*cols):
        return dict(id_cols=(L.JoinCol * len(cols))(*[L.JoinCol(*c) for c in cols]), n_id=len(cols))
    assert _join_rc(lib, **ids((4, 0, L.RULE_IDENTITY, 10))) == L.EINVAL and b"source" in lib.sprk_last_error()
    assert _join_rc(lib, **ids((-1, 0, L.RULE_IDENTITY, 10))) == L.EINVAL
    assert _join_rc(lib, **ids((L.JOIN_USER_ROW, 0, 3, 10))) == L.EINVAL and b"rule" in lib.sprk_last_error()
    assert _join_rc(lib, **ids((L.JOIN_USER_ROW, 0, L.RULE_DENSE, 10))) == L.EINVAL           # a dense rule among the id columns
    assert _join_rc(lib, dense_cols=(L.JoinCol * 1)(L.JoinCol(L.JOIN_MOVIE_ROW, 3, L.RULE_GENRE, 19))) == L.EINVAL
    assert _join_rc(lib, **ids((L.JOIN_USER_ROW, 16, L.RULE_IDENTITY, 10))) == L.EINVAL        # past the row
    assert _join_rc(lib, **ids((L.JOIN_MOVIE_ROW, 8, L.RULE_GENRE, 19))) == L.EINVAL
    assert _join_rc(lib, **ids((L.JOIN_USER_ROW, -1, L.RULE_IDENTITY, 10))) == L.EINVAL
    assert _join_rc(lib, **ids((L.JOIN_USER_ROW, 0, L.RULE_IDENTITY, 0))) == L.EINVAL          # vocab
    assert _join_rc(lib, user_pitch=13) == L.EINVAL and _join_rc(lib, movie_pitch=0) == L.EINVAL
    assert _join_rc(lib, n_users=-1) == L.EINVAL and _join_rc(lib, shared=2) == L.EINVAL
    assert _join_rc(lib, Q=1 << 20, C=1 << 12) == L.EINVAL                                     # Q * C beyond int32
    keep, a = _join_args()
    assert _join_rc(lib, ids_out=a["ids_out"] + 4) == L.EINVAL                                 # outputs start on 16 bytes
    # nothing to do is not an error, and touches nothing
    assert _join_rc(lib, Q=0) == L.OK and _join_rc(lib, C=0) == L.OK and _join_rc(lib, n_id=0, n_dense=0) == L.OK


def test_rank_scores_arguments_are_validated_before_any_device_call(lib):
    s, o = np.zeros(8, np.float32), np.zeros(8, np.int32)
    sp, op = C.c_void_p(s.ctypes.data), C.c_void_p(o.ctypes.data)
    assert lib.sprk_rank_scores(None, 1, 8, op, None) == L.EINVAL
    assert lib.sprk_rank_scores(sp, 1, 8, None, None) == L.EINVAL
    assert lib.sprk_rank_scores(sp, 1, 0, op, None) == L.EINVAL
    assert lib.sprk_rank_scores(sp, 1, 4097, op, None) == L.EINVAL and b"4096" in lib.sprk_last_error()
    assert lib.sprk_rank_scores(sp, 1, -3, op, None) == L.EINVAL
    assert lib.sprk_rank_scores(sp, -1, 8, op, None) == L.EINVAL
    assert lib.sprk_rank_scores(sp, 0, 8, op, None) == L.OK
    assert L.RANK_MAX_SORT == 4096


def test_rank_oracle_is_float_compare_descending():
    s = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, 1.0, -np.nan]], dtype=np.float32)
    assert FC.rank_oracle(s).tolist() == [[2, 7, 3, 5, 6, 0, 1, 4]]
