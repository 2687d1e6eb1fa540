"""The grid-stride loops and the work queues of the ratings pipelines and the trainers past their first round (``-m gpu``).

Part 1, under ``SPRK_FE_MAX_GRID`` = 3 and 1 (csrc/host_segments.h fe_max_grid): every entry point on the sets of its own test file, against
its host definition with that file's equalities.  3: several workgroups and a stride that is no power of two -- a loop that steps by 256 in
place of ``gridDim.x * 256`` does work twice; 1: one workgroup drains every queue alone, so each of its waves draws many times.  Every test
first asserts through ``sprk_segments_grid`` that a loop of its entry point has more items than one round of its grid covers, or that a queue
has more rows than its groups take at once: a switch that is ignored fails the test.

Part 2, at the real cap of 2048 workgroups, where the host definition is cheap: 530 000 ratings (524 289 is the first count that strides) and
40 000 ALS rows (32 769 is the first count at which a wave of k_als_half_sweep draws again).  These catch what a small cap cannot: 64-bit
index arithmetic, FE_MAX_GRID itself, scans over more than one tile."""
import functools

import numpy as np
import pytest

from sparrowrecsys_amd import als as A
from sparrowrecsys_amd import catalog as CT
from sparrowrecsys_amd import featureeng as FE
from sparrowrecsys_amd import item2vec as IV
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_fm as TF
from sparrowrecsys_amd import userembedding as UE
from tests import als_cases
from tests import catalog_cases
from tests import featureeng_cases
from tests import item2vec_cases
from tests import train_cases as TC
from tests import train_fm_cases as TFC
from tests import userembedding_cases
from tests import test_gpu_als as GA
from tests import test_gpu_catalog as GC
from tests import test_gpu_featureeng as GF
from tests import test_gpu_item2vec as GI
from tests import test_gpu_train as GT
from tests import test_gpu_train_fm as GTF
from tests import test_gpu_userembedding as GU

pytestmark = pytest.mark.gpu

THREADS = 256                     # FE_THREADS: the workgroup of every strided loop
ALS_ROWS_PER_GROUP = 16           # k_als_half_sweep: rows a workgroup draws at once
UE_USERS_PER_GROUP = {True: 16, False: 4}    # k_ue_sum: D <= 16, and above
REAL_CAP = 2048                   # FE_MAX_GRID

caps = pytest.mark.parametrize("cap", ["3", "1"])
sort_caps = pytest.mark.parametrize("sort_cap", [None, "64"])


def _set(monkeypatch, lib, cap, sort_cap=None):
    """The two switches; -> the cap as the library reads it."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", cap)
    if sort_cap is None:
        monkeypatch.delenv("SPRK_FE_SORT_CAP", raising=False)
    else:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", sort_cap)
    assert lib.sprk_segments_grid(1 << 30) == int(cap)
    return int(cap)


def _unset(monkeypatch, lib):
    monkeypatch.delenv("SPRK_FE_MAX_GRID", raising=False)
    monkeypatch.delenv("SPRK_FE_SORT_CAP", raising=False)
    assert lib.sprk_segments_grid(1 << 30) == REAL_CAP


def strides(lib, items):
    """A loop over ``items`` elements, launched with fe_grid_capped(items) workgroups, makes a second trip."""
    return items > lib.sprk_segments_grid(items) * THREADS


def draws_again(lib, rows, per_group):
    """A queue of ``rows`` rows, ``per_group`` to a workgroup at once, is drawn from more than once by some workgroup."""
    groups = (rows + per_group - 1) // per_group
    return rows > min(groups, lib.sprk_segments_grid(1 << 30)) * per_group


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


# ================================================================ part 1: every pipeline under a small cap

# ---------------------------------------------------------------- sprk_feature_eng

@pytest.fixture(scope="module")
def fe_sets(lib):
    table = FE.movie_table(featureeng_cases.synthetic_movies())
    synthetic, merge = featureeng_cases.synthetic_ratings(), featureeng_cases.merge_shapes_ratings()
    return table, (synthetic, FE.samples_host(synthetic, table, 5)), (merge, FE.samples_host(merge, table, 5))


@caps
@sort_caps
def test_feature_eng(lib, fe_sets, monkeypatch, cap, sort_cap):
    """The synthetic set (837 ratings) and the merge shapes (2 789 ratings, a user of 1 024): samples and store byte for byte.  k_fe_hist and
    k_fe_scatter stride over the ratings, k_fe_sort_short over the users, and with the sort capped at 64 k_fe_sort_long_chunks over 16
    chunks and k_fe_merge_pass over 1 024 positions."""
    c = _set(monkeypatch, lib, cap, sort_cap)
    table, (synthetic, want), (merge, merge_want) = fe_sets
    assert strides(lib, len(synthetic["userId"])) and strides(lib, len(merge["userId"])) and featureeng_cases.MERGE_USERS > c
    GF._check(synthetic, table, want, 5)
    GF._check(merge, table, merge_want, 5, n_users=featureeng_cases.MERGE_USERS)


# ---------------------------------------------------------------- sprk_user_emb

@functools.lru_cache(maxsize=None)
def _ue_case(D, grouped):
    return userembedding_cases.synthetic(D=D, stride=D + 2, grouped=grouped)


@caps
@sort_caps
@pytest.mark.parametrize("D", [10, 17])
def test_user_emb(lib, monkeypatch, cap, sort_cap, D):
    """The synthetic set (5 000 ratings, 97 users) shuffled and grouped, mean and sum: emb, has, count.  k_ue_count and k_ue_scatter stride;
    k_ue_sum's queue holds 7 groups of 16 users at D = 10 and 25 groups of 4 at D = 17."""
    _set(monkeypatch, lib, cap, sort_cap)
    for grouped in (False, True):
        case = _ue_case(D, grouped)
        assert strides(lib, len(case["user"])) and draws_again(lib, case["n_users"], UE_USERS_PER_GROUP[D <= 16])
        for mode in ("mean", "sum"):
            GU._check(case, mode, D=D)


# ---------------------------------------------------------------- sprk_catalog_build, sprk_catalog_similar

@pytest.fixture(scope="module")
def cat_sets(lib):
    out = {}
    for grouped in (False, True):
        ratings, movies, info = catalog_cases.synthetic(grouped=grouped)
        out[grouped] = (ratings, movies, info, CT.catalog_host(ratings, movies))
    ratings, movies, queries = catalog_cases.counts_table()
    out["counts"] = (ratings, movies, queries, CT.catalog_host(ratings, movies))
    return out


@caps
@sort_caps
def test_catalog_build(lib, cat_sets, monkeypatch, cap, sort_cap):
    """The synthetic set (20 000 ratings, 340 ids, lists of 2 142 entries) shuffled and grouped: averages, counts and all lists.  The ratings
    side strides at both caps; the movie side (k_cat_avg_short, k_cat_list_count, k_cat_list_scatter: 340 ids) at cap 1; k_cat_avg_wave
    gives every wave many movies; k_cat_list_write strides over the lists."""
    c = _set(monkeypatch, lib, cap, sort_cap)
    for grouped in (False, True):
        ratings, movies, info, want = cat_sets[grouped]
        assert strides(lib, len(ratings["rating"])) and strides(lib, len(want["list_movies"])) and catalog_cases.N_TABLE > c * 4
        assert c > 1 or strides(lib, catalog_cases.N_TABLE)
        got = CT.build(ratings, movies).to_host()
        GC._assert_same(got, want)
        for m, n in info["fixed"].items():
            assert got["rating_count"][m] == n and got["avg"][m] == catalog_cases.loop_average(ratings["rating"][ratings["movieId"] == m]), (m, n)


@caps
@pytest.mark.parametrize("mode", [0, 1])
def test_catalog_similar(lib, cat_sets, monkeypatch, cap, mode):
    """The table of candidate counts (1 793 ids, lists of 7 048 entries: the movie side strides at cap 3 too), built under the cap, then the
    similar lists of both modes."""
    _set(monkeypatch, lib, cap)
    ratings, movies, queries, host = cat_sets["counts"]
    assert strides(lib, len(host["has"])) and strides(lib, len(host["list_movies"])) and strides(lib, len(ratings["rating"]))
    cat = CT.build(ratings, movies)
    GC._assert_same(cat.to_host(), host)
    counts = GC._similar_equals_host(cat, host, list(queries.values()), mode, 2000)
    if mode == 0:
        assert counts.tolist() == list(queries)
    GC._similar_equals_host(cat, host, np.flatnonzero(host["has"])[::7], mode, 20)


# ---------------------------------------------------------------- sprk_als_fit, sprk_als_predict, sprk_als_topk

@functools.lru_cache(maxsize=None)
def _als_host(rank, iters=2):
    return als_cases.host(als_cases.synthetic(False), rank=rank, iters=iters)


@caps
@sort_caps
@pytest.mark.parametrize("rank", [2, 10, 16])
def test_als_fit(lib, monkeypatch, cap, sort_cap, rank):
    """The synthetic set (5 326 ratings, 300 users, 80 movies), one rank per chain class, two iterations: factors, has, counts.
    k_als_count and k_als_scatter stride; k_als_half_sweep's queue holds 19 groups of 16 users and 5 of 16 movies."""
    _set(monkeypatch, lib, cap, sort_cap)
    case = als_cases.synthetic(False)
    assert strides(lib, len(case["user"])) and draws_again(lib, case["n_users"], ALS_ROWS_PER_GROUP) and draws_again(lib, case["n_items"], ALS_ROWS_PER_GROUP)
    got, err = GA._device(case, rank=rank, iters=2)
    assert err == -1
    GA._assert_same(got, _als_host(rank))


@caps
def test_als_predict_and_topk(lib, monkeypatch, cap):
    """2 005 pairs over the fitted tables, ids outside either table and movies without a factor among them; the top-K of seven queries over
    300 rows in chunks of 64."""
    _set(monkeypatch, lib, cap)
    host = _als_host(10)
    rng = np.random.default_rng(2)
    users = np.concatenate([rng.integers(0, 300, 2000), [-1, 300, 5, 5, 1 << 30]]).astype(np.int32)
    movies = np.concatenate([rng.integers(0, 80, 2000), [3, 3, -1, 80, 3]]).astype(np.int32)
    assert strides(lib, len(users))
    want = A.predict_host(users, movies, host[0], host[2], host[1], host[3])
    assert np.isnan(want[-5:]).all() and np.isnan(want[:2000][movies[:2000] >= 70]).all() and not np.isnan(want[:2000][movies[:2000] < 70]).any()
    got = A.predict_device(GA._up(users, np.int32), GA._up(movies, np.int32), GA._up(host[0], np.float32), GA._up(host[2], np.uint8), GA._up(host[1], np.float32),
                           GA._up(host[3], np.uint8), rank=10).cpu().numpy()
    assert got.tobytes() == want.tobytes()
    monkeypatch.setenv("SPRK_EMB_TOPK_CHUNK", "64")
    n_items = 300
    rng = np.random.default_rng(n_items)
    table = rng.standard_normal((n_items, 10)).astype(np.float32)
    has = (rng.random(n_items) < 0.8).astype(np.uint8)
    has[0] = 1
    query = rng.standard_normal((7, 10)).astype(np.float32)
    q_has = np.array([1, 1, 1, 0, 1, 1, 1], dtype=np.uint8)
    available = int(has.sum())
    for k in sorted({1, 10, available, available + 3, min(n_items + 5, 1024)}):
        rows, scores = GA._topk(query, q_has, table, has, k)
        want_rows, want_scores = A.topk_host(query, q_has, table, has, k)
        assert rows.tobytes() == want_rows.tobytes() and scores.tobytes() == want_scores.tobytes(), k
        assert (rows[3] == -1).all() and (rows[0, :min(k, available)] >= 0).all() and (rows[0, available:] == -1).all()


# ---------------------------------------------------------------- sprk_item_sequences, sprk_item_walks, sprk_skipgram_fit

I2V_USERS, I2V_ITEMS = GI.NU, GI.NI


@pytest.fixture(scope="module")
def i2v_sets(lib):
    """item2vec_cases.ratings(long_user=7, long_len=260): 1 160 ratings, 708 kept, a user of more than 64 kept rows; its sequences and
    300 walks of 10 on the host."""
    cols = item2vec_cases.ratings(seed=1, long_user=7, long_len=260)
    seq = GI._host_sequences(cols)
    walks = IV.walks_host(IV.transitions_host(seq[0], seq[1], I2V_ITEMS), 300, 10, seed=5)
    return cols, seq, walks


@caps
@sort_caps
def test_item_sequences(lib, i2v_sets, monkeypatch, cap, sort_cap):
    """k_i2v_seq_count, k_i2v_seq_scatter and k_i2v_seq_emit stride over 1 160 rows."""
    _set(monkeypatch, lib, cap, sort_cap)
    cols, want, _ = i2v_sets
    assert strides(lib, len(cols["userId"])) and np.diff(want[0]).max() > 64
    off, items, cnt, err = GI._dev_sequences(cols)
    assert err == -1
    GI._same(off, want[0], "seq_offsets"); GI._same(items, want[1], "seq_items"); GI._same(cnt, want[2], "item_count")


@caps
@sort_caps
def test_item_walks(lib, i2v_sets, monkeypatch, cap, sort_cap):
    """300 walks of 10 over the transitions of 708 sequence items: k_fe_sort_short strides over the 30 items' segments at both caps;
    k_i2v_pair_count, k_i2v_pair_scatter (708 items), k_i2v_walk and k_i2v_walk_emit (300 and 301 samples) stride at cap 1."""
    c = _set(monkeypatch, lib, cap, sort_cap)
    _, (off, items, _), want = i2v_sets
    assert I2V_ITEMS > c and (c > 1 or (strides(lib, len(items)) and strides(lib, 300)))
    woff, witems, word = IV.walks_device(GI._up(off, np.int32), GI._up(items, np.int32), I2V_ITEMS, 300, 10, seed=5)
    assert int(word.cpu()[0]) == -1
    woff = woff.cpu().numpy()
    GI._same(woff, want[0], "walk_offsets"); GI._same(witems.cpu().numpy()[:woff[-1]], want[1], "walk_items")


@caps
@sort_caps
@pytest.mark.parametrize("D", [10, 17])
def test_skipgram_fit(lib, i2v_sets, monkeypatch, cap, sort_cap, D):
    """Two iterations in rounds of 7 over the 708 words: vectors, syn1, the loss' bits, error word -1.  k_fe_sort_short strides over the
    2 V = 60 record segments at both caps; k_i2v_init (V D cells), k_i2v_mark, k_i2v_corpus and k_i2v_records (708 items) at cap 1."""
    c = _set(monkeypatch, lib, cap, sort_cap)
    _, (off, items, _), _ = i2v_sets
    vocab, corpus, _ = GI._check_fit(("grid rounds", D), off, items, I2V_ITEMS, D=D, iters=2, round=7)
    assert 2 * len(vocab.ids) > c and (c > 1 or (strides(lib, len(items)) and strides(lib, len(vocab.ids) * D)))
    assert len(corpus.word) % 7


# ---------------------------------------------------------------- sprk_train_fit, sprk_train_fm_fit

@caps
@sort_caps
def test_train_fit(torch, lib, monkeypatch, cap, sort_cap):
    """``small(50)``, batch 12, tile 8, three epochs, a shuffled order: k_fe_sort_short strides over the 5 batches' segments.  No element
    loop of that family is long enough to stride (150 entries, 60 table floats), so a second family follows: 300 rows of (90, 5, 200) x 3
    with one layer of 80, batch 64 -- k_tr_count and k_tr_scatter over 900 entries, k_tr_table_adam over 885 floats, k_tr_dense_adam over
    1 041."""
    c = _set(monkeypatch, lib, cap, sort_cap)
    fam, w, ids, dense, y = GT.small(50, seed=4)
    assert (50 + 11) // 12 > c
    GT.both(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8, order=np.random.default_rng(1).permutation(50))
    fam, w, ids, dense, y = GT.small(300, seed=1, vocabs=(90, 5, 200), widths=(80,))
    shapes = T.param_shapes(fam)
    table = sum(int(np.prod(shapes[k])) for k in fam.tables)
    assert strides(lib, ids.size) and strides(lib, table) and strides(lib, sum(int(np.prod(s)) for s in shapes.values()) - table)
    GT.both(fam, w, ids, dense, y, batch_size=64, epochs=2, tile=8, order=np.random.default_rng(2).permutation(300))


@caps
@sort_caps
def test_train_fm_fit(torch, lib, monkeypatch, cap, sort_cap):
    """``TFC.small(50)`` as above, and the reference shape at 40 rows: k_tf_table_adam strides over 1 188 floats (``fo_cat/kernel`` behind the
    ``emb/`` tables) and k_tf_dense_adam over the Dense parameters."""
    c = _set(monkeypatch, lib, cap, sort_cap)
    fam, w, ids, dense, y = TFC.small(50, seed=4)
    assert (50 + 11) // 12 > c
    GTF.both(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8, order=np.random.default_rng(1).permutation(50))
    fam, w, ids, dense, y = TFC.small(40, seed=5, **TFC.REFERENCE_SHAPE)
    shapes = TF.param_shapes(fam)
    table = sum(int(np.prod(shapes[k])) for k in shapes if k.startswith("emb/") or k == "fo_cat/kernel")
    assert strides(lib, table) and strides(lib, sum(int(np.prod(s)) for s in shapes.values()) - table) and (40 + 11) // 12 > c
    GTF.both(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8, order=np.random.default_rng(3).permutation(40))


# ---------------------------------------------------------------- the error word across rounds: cap 3, a round is 768 rows

BAD_THIRD, BAD_SECOND = 1600, 800            # rows of the third round and of the second; the later one is written first in each test


def _rounds(lib, monkeypatch, n):
    _set(monkeypatch, lib, "3")
    assert lib.sprk_segments_grid(n) == 3 and n > BAD_THIRD >= 2 * 3 * THREADS > BAD_SECOND >= 3 * THREADS


def test_error_word_feature_eng(lib, fe_sets, monkeypatch):
    table, _, (merge, _) = fe_sets
    _rounds(lib, monkeypatch, len(merge["userId"]))
    bad = {k: v.copy() for k, v in merge.items()}
    bad["rating"][[BAD_THIRD, BAD_SECOND]] = [np.nan, 3.7]
    assert GF._same_error(bad, table, n_users=featureeng_cases.MERGE_USERS).startswith("ratings row %d: rating" % BAD_SECOND)


def test_error_word_user_emb(lib, monkeypatch):
    case = _ue_case(10, False)
    _rounds(lib, monkeypatch, len(case["user"]))
    user = case["user"].copy()
    user[[BAD_THIRD, BAD_SECOND]] = [97, -1]
    _, err = GU._device(user, case["row"], case["emb"], case["has"], 97, D=10)
    assert (err >> 32, err & 0xffffffff) == (1, BAD_SECOND)


def test_error_word_catalog(lib, cat_sets, monkeypatch):
    ratings, movies, _, _ = cat_sets[False]
    _rounds(lib, monkeypatch, len(ratings["rating"]))
    bad = {k: v.copy() for k, v in ratings.items()}
    bad["rating"][[BAD_THIRD, BAD_SECOND]] = [np.nan, np.inf]
    _, _, err, _ = GC._raw_build(bad, movies)
    assert (err >> 32, err & 0xffffffff) == (CT.ERR_RATING, BAD_SECOND)


def test_error_word_als(lib, monkeypatch):
    case = als_cases.synthetic(False)
    _rounds(lib, monkeypatch, len(case["user"]))
    movie = case["movie"].copy()
    movie[[BAD_THIRD, BAD_SECOND]] = [80, -1]
    _, err = GA._device(dict(case, movie=movie))
    assert (err >> 32, err & 0xffffffff) == (2, BAD_SECOND)


def test_error_word_item_sequences(lib, monkeypatch):
    cols = item2vec_cases.ratings(seed=2, n=1800)
    _rounds(lib, monkeypatch, len(cols["userId"]))
    bad = dict(cols, rating=cols["rating"].copy())
    bad["rating"][[BAD_THIRD, BAD_SECOND]] = [np.inf, np.nan]
    assert GI._dev_sequences(bad)[3] == 3 << 32 | BAD_SECOND
    with pytest.raises(ValueError, match="row %d" % BAD_SECOND):
        GI._host_sequences(bad)


def _train_error(torch, raw_fit, fit_device, fit_host, names, fam, w, ids, dense, y):
    bad = y.copy()
    bad[[BAD_THIRD, BAD_SECOND]] = [-np.inf, np.nan]
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, dense, bad, 256, 8, 1)
    assert rc == 0 and intact and word == (T.ERR_LABEL << 32 | BAD_SECOND), (word >> 32, word & 0xffffffff)
    assert TC.same_bits(params, np.concatenate([w[k].reshape(-1) for k in names])) and not m.any() and not v.any()
    for fit in (fit_device, fit_host):
        with pytest.raises(ValueError, match="samples row %d: the label" % BAD_SECOND):
            fit(fam, w, ids, dense, bad, batch_size=256, epochs=1, tile=8)


def test_error_word_train(torch, lib, monkeypatch):
    fam, w, ids, dense, y = GT.small(1700, seed=11)
    _rounds(lib, monkeypatch, len(y))
    _train_error(torch, GT.raw_fit, T.train_device, T.train_host, T.param_names(fam), fam, w, ids, dense, y)


def test_error_word_train_fm(torch, lib, monkeypatch):
    fam, w, ids, dense, y = TFC.small(1700, seed=11)
    _rounds(lib, monkeypatch, len(y))
    _train_error(torch, GTF.raw_fit, TF.train_device, TF.train_host, TF.param_names(fam), fam, w, ids, dense, y)


# ================================================================ part 2: the same loops at the real cap

MANY = 530_000                    # > 2048 x 256 = 524 288: every loop over the ratings makes a second trip


@functools.lru_cache(maxsize=None)
def _many_ratings(n_users=3000, n_items=500, seed=23):
    """530 000 shuffled half-star ratings of 3 000 users on 500 items, timestamps from 200 000 values."""
    rng = np.random.default_rng(seed)
    return {"user": rng.integers(0, n_users, MANY).astype(np.int32), "movie": rng.integers(0, n_items, MANY).astype(np.int32),
            "rating": als_cases.half_stars(rng.integers(1, 11, MANY) / 2.0), "timestamp": rng.integers(1_000_000, 1_200_000, MANY).astype(np.int64),
            "n_users": n_users, "n_items": n_items}


@pytest.mark.parametrize("rank,iters", [(3, 1), (10, 2)])
def test_als_with_more_rows_than_the_queue_hands_out_at_once(lib, monkeypatch, rank, iters):
    """40 000 users x 300 items, 120 000 shuffled ratings, so some users have none: 40 000 > 2048 x 16 (32 769 rows are the fewest), every
    workgroup of k_als_half_sweep's user side draws again.  A user without ratings has no factor."""
    _unset(monkeypatch, lib)
    rng = np.random.default_rng(31)
    n_users, n_items, n = 40_000, 300, 120_000
    case = {"user": rng.integers(0, n_users, n).astype(np.int32), "movie": rng.integers(0, n_items, n).astype(np.int32),
            "rating": als_cases.half_stars(rng.integers(1, 11, n) / 2.0), "n_users": n_users, "n_items": n_items}
    assert draws_again(lib, n_users, ALS_ROWS_PER_GROUP) and (np.bincount(case["user"], minlength=n_users) == 0).sum() > 100
    got, err = GA._device(case, rank=rank, iters=iters)
    assert err == -1
    GA._assert_same(got, als_cases.host(case, rank=rank, iters=iters))
    assert not got[2][np.bincount(case["user"], minlength=n_users) == 0].any()


def test_als_with_more_ratings_than_one_round(lib, monkeypatch):
    """530 000 ratings, 3 000 users, 500 items, rank 2, one iteration: k_als_count and k_als_scatter stride."""
    _unset(monkeypatch, lib)
    case = _many_ratings()
    assert strides(lib, MANY)
    got, err = GA._device(case, rank=2, iters=1)
    assert err == -1
    GA._assert_same(got, als_cases.host(case, rank=2, iters=1))


def test_als_predict_with_more_pairs_than_one_round(lib, monkeypatch):
    """530 000 pairs, a hundredth of them with an id outside its table, a tenth of the rows of either table without a factor."""
    _unset(monkeypatch, lib)
    rng = np.random.default_rng(37)
    n_users, n_items, rank = 3000, 500, 7
    uf, itf = rng.standard_normal((n_users, rank)).astype(np.float32), rng.standard_normal((n_items, rank)).astype(np.float32)
    uh, ih = (rng.random(n_users) >= 0.1).astype(np.uint8), (rng.random(n_items) >= 0.1).astype(np.uint8)
    users, movies = rng.integers(0, n_users, MANY).astype(np.int32), rng.integers(0, n_items, MANY).astype(np.int32)
    odd = rng.permutation(MANY)[:MANY // 100]
    users[odd[::2]] = rng.choice([-1, n_users, 1 << 30], len(odd[::2]))
    movies[odd[1::2]] = rng.choice([-1, n_items, 1 << 30], len(odd[1::2]))
    users[-1], movies[-1] = n_users, 0                                          # the last pair, in the second trip
    assert strides(lib, MANY)
    want = A.predict_host(users, movies, uf, uh, itf, ih)
    assert np.isnan(want[odd]).all() and np.isnan(want[-1]) and 0.1 < np.isnan(want).mean() < 0.3
    got = A.predict_device(GA._up(users, np.int32), GA._up(movies, np.int32), GA._up(uf, np.float32), GA._up(uh, np.uint8), GA._up(itf, np.float32), GA._up(ih, np.uint8),
                           rank=rank).cpu().numpy()
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("grouped", [False, True])
def test_user_emb_with_more_ratings_than_one_round(lib, monkeypatch, grouped):
    """530 000 ratings, 3 000 users, 500 items, D = 10, both modes: k_ue_count strides, and on shuffled input k_ue_scatter."""
    _unset(monkeypatch, lib)
    r = _many_ratings()
    rng = np.random.default_rng(41)
    emb = rng.standard_normal((r["n_items"], 10)).astype(np.float32)
    has = (rng.random(r["n_items"]) >= 0.1).astype(np.uint8)
    emb[has == 0] = np.nan
    user, row = r["user"], r["movie"]
    if grouped:
        by_user = np.argsort(user, kind="stable")
        user, row = user[by_user], row[by_user]
    case = {"user": user, "row": row, "emb": emb, "has": has, "n_users": r["n_users"]}
    assert strides(lib, MANY)
    for mode in ("mean", "sum"):
        GU._check(case, mode)


@pytest.mark.parametrize("all_kept", [False, True])
def test_item_sequences_with_more_ratings_than_one_round(lib, monkeypatch, all_kept):
    """530 000 ratings of which about 40 % are kept (rating >= 3.5), and with every rating kept: k_i2v_seq_count, k_i2v_seq_scatter and
    k_i2v_seq_emit stride; with all kept the emitted items do too."""
    _unset(monkeypatch, lib)
    r = _many_ratings()
    rating = np.full(MANY, 4.0, dtype=np.float32) if all_kept else r["rating"]
    cols = {"userId": r["user"], "movieId": r["movie"], "rating": rating, "timestamp": r["timestamp"]}
    want = IV.sequences_host(cols["userId"], cols["movieId"], cols["rating"], cols["timestamp"], r["n_users"], r["n_items"])
    kept = int(want[0][-1])
    assert strides(lib, MANY) and (kept == MANY if all_kept else 0.3 * MANY < kept < 0.5 * MANY)
    off, items, cnt, err = GI._dev_sequences(cols, r["n_users"], r["n_items"])
    assert err == -1
    GI._same(off, want[0], "seq_offsets"); GI._same(items, want[1], "seq_items"); GI._same(cnt, want[2], "item_count")


def test_catalog_with_more_ratings_than_one_round(lib, monkeypatch):
    """530 000 shuffled ratings on 600 movies: k_cat_count and k_cat_scatter stride; averages, counts and lists."""
    _unset(monkeypatch, lib)
    ratings, movies = catalog_cases.many_ratings(MANY, 600)
    assert strides(lib, len(ratings["rating"]))
    want = CT.catalog_host(ratings, movies)
    assert want["rating_count"].sum() > 0.99 * MANY and want["rating_count"].sum() < MANY
    GC._assert_same(CT.build(ratings, movies).to_host(), want)
