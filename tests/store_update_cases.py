"""Inputs shared by tests/test_store_update.py (CPU) and tests/test_gpu_store_update.py: rating sets from tests/featureeng_cases.py's
generators, sorted by timestamp, cut into batches and shuffled inside each batch, and a hand-built set (EDGES) that holds the cases an
update distinguishes.  The expectation after every batch is the REBUILD: featurestore.row_images_from_samples(featureeng.samples_host(
the concatenation of the batches so far))."""
import collections
import functools

import numpy as np

from sparrowrecsys_amd import featureeng as FE
from sparrowrecsys_amd import featurestore as FS
from tests import featureeng_cases as cases

Case = collections.namedtuple("Case", "batches movies n_users n_movies")      # batches: [ratings dict], movies: a featureeng.MovieTable


def empty_batch():
    return {"userId": np.zeros(0, np.int64), "movieId": np.zeros(0, np.int64), "rating": np.zeros(0, np.float64), "timestamp": np.zeros(0, np.int64)}


def concatenation(batches):
    """R: the batches in call order."""
    return {k: np.concatenate([b[k] for b in batches]) if batches else empty_batch()[k] for k in FE.RATING_KEYS}


def split_in_time(ratings, n_batches, seed):
    """The ratings sorted by timestamp (equal timestamps keep their order), cut at random places into n_batches non-empty batches, the
    rows of each batch shuffled.  A cut may fall between two equal timestamps of one user: the tie then crosses a batch boundary."""
    rng = np.random.RandomState(seed)
    n = len(ratings["userId"])
    order = np.argsort(ratings["timestamp"], kind="stable")
    cuts = np.sort(rng.choice(np.arange(1, n), n_batches - 1, replace=False)) if n_batches > 1 else np.zeros(0, np.int64)
    out = []
    for lo, hi in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [n]])):
        rows = order[lo:hi][rng.permutation(hi - lo)]
        out.append({k: np.asarray(v)[rows] for k, v in ratings.items()})
    return out


# ---- the hand-built set: four batches and an empty one, synthetic movie table, N_USERS x N_MOVIES tables ----
EDGES_AFTER = {"b1": 0, "b2": 1, "empty": 2, "b3": 3, "b4": 4}               # index of the update after which a batch is applied
RING_USER, LONG_BATCH_USER, FLIP_USER, NO_FLIP_USER, ONE_STAMP_USER, FIRST_TWO_USER, LATE_USER = 1, 2, 3, 4, 5, 6, 7
RING_COUNTS = [99, 100, 101, 230]                                            # RING_USER's ratings after b1 .. b4: the ring wraps, twice
FLAGGED_LATER, DROPPED_ONLY, OUTSIDE_TABLE = 101, 103, 121                   # movies no random draw names
DROPPED_ONLY_COUNTS = [1, 2, 3, 4]                                           # DROPPED_ONLY's ratings after b1 .. b4; flagged by b4 alone


def edges_batches(seed=41):
    """By user, ratings per batch b1 .. b4 (timestamps 1000 b + 0 .. 29: ties inside a batch, none across):
      RING_USER        99, 1, 1, 129     the counts of RING_COUNTS; b2's rating names FLAGGED_LATER at position 99
      LONG_BATCH_USER  5, 0, 0, 130      130 new ratings in one batch, DROPPED_ONLY and OUTSIDE_TABLE among them
      FLIP_USER        2, 1, 0, 0        2 -> 3 ratings: user_has flips with b2
      NO_FLIP_USER     1, 1, 0, 0        1 -> 2: it does not
      ONE_STAMP_USER   3, 4, 2, 50       every rating at timestamp 777: ties inside a batch and across every boundary
      FIRST_TWO_USER   2, 0, 0, 0        FLAGGED_LATER at position 0, DROPPED_ONLY at position 1: counted, not flagged
      LATE_USER        0, 1, 1, 0        DROPPED_ONLY at positions 0 and 1: its count grows, its row stays NA until b4
    """
    rng = np.random.RandomState(seed)
    pool = np.arange(1, 100, 2)
    plan = {RING_USER: [99, 1, 1, 129], LONG_BATCH_USER: [5, 0, 0, 130], FLIP_USER: [2, 1, 0, 0], NO_FLIP_USER: [1, 1, 0, 0], ONE_STAMP_USER: [3, 4, 2, 50],
            FIRST_TWO_USER: [2, 0, 0, 0], LATE_USER: [0, 1, 1, 0]}
    out = []
    for b in range(4):
        u, m, r, t = [], [], [], []
        for user, sizes in plan.items():
            n = sizes[b]
            mm, rr = rng.choice(pool, n), rng.randint(1, 11, n) / 2.0
            tt = np.full(n, 777) if user == ONE_STAMP_USER else 1000 * (b + 1) + rng.randint(0, 30, n)
            if user == RING_USER and b == 1:
                mm[0] = FLAGGED_LATER
            if user == LONG_BATCH_USER and b == 3:
                mm[[17, 90]] = [DROPPED_ONLY, OUTSIDE_TABLE]
            if user == FIRST_TWO_USER and b == 0:
                mm[:], tt[:] = [FLAGGED_LATER, DROPPED_ONLY], [1001, 1002]
            if user == LATE_USER:
                mm[:] = DROPPED_ONLY
            u.extend([user] * n); m.extend(mm); r.extend(rr); t.extend(tt)
        order = rng.permutation(len(u))
        out.append({"userId": np.asarray(u, np.int64)[order], "movieId": np.asarray(m, np.int64)[order], "rating": np.asarray(r, np.float64)[order],
                    "timestamp": np.asarray(t, np.int64)[order]})
    return out[:2] + [empty_batch()] + out[2:]


WIDE_SHIFT, WIDE_USERS, WIDE_MOVIES = 800, 850, 1000                         # "wide-2": ids and batches past three workgroups' first round (3 x 256)
CASES = ["synthetic-1", "synthetic-3", "synthetic-6", "edges", "all-genres", "wide-2"]
# (case, hist_len) pairs the CPU and the GPU tests run
RUNS = [("synthetic-1", 5), ("synthetic-3", 5), ("synthetic-6", 5), ("synthetic-3", 1), ("synthetic-6", 100), ("edges", 5), ("edges", 100), ("all-genres", 5),
        ("wide-2", 5)]


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    if name.startswith("synthetic-"):
        k = int(name.split("-")[1])
        return Case(split_in_time(cases.synthetic_ratings(), k, seed=100 + k), FE.movie_table(cases.synthetic_movies()), cases.N_USERS, cases.N_MOVIES)
    if name == "wide-2":          # the synthetic set whole, then once more with another seed and later timestamps; every user and movie id WIDE_SHIFT higher
        movies = cases.synthetic_movies()
        movies["movieId"] = [i + WIDE_SHIFT for i in movies["movieId"]]
        again = cases.synthetic_ratings(seed=12)
        batches = [cases.synthetic_ratings(), dict(again, timestamp=again["timestamp"] + 10**7)]
        batches = [dict(b, userId=b["userId"] + WIDE_SHIFT, movieId=b["movieId"] + WIDE_SHIFT) for b in batches]
        assert all(len(b["userId"]) > 3 * 256 for b in batches)
        return Case(batches, FE.movie_table(movies), WIDE_USERS, WIDE_MOVIES)
    if name == "edges":
        return Case(edges_batches(), FE.movie_table(cases.synthetic_movies()), cases.N_USERS, cases.N_MOVIES)
    if name == "all-genres":                                                   # featureeng_cases' ties between genre counters, split in two
        return Case(split_in_time(cases.all_genres_ratings(), 2, seed=7), FE.movie_table(cases.all_genres_movies()), cases.ALL_GENRES_USERS, cases.ALL_GENRES_MOVIES)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, hist_len):
    """Per update of the case: the four arrays of the rebuild from the batches so far, as bytes.  Computed once; read-only."""
    c = case(name)
    out = []
    for k in range(len(c.batches)):
        samples = FE.samples_host(concatenation(c.batches[:k + 1]), c.movies, hist_len, n_users=c.n_users, n_movies=c.n_movies)
        images = FS.row_images_from_samples(samples, hist_len, c.n_users, c.n_movies)
        out.append(tuple(a.tobytes() for a in images[:4]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def host_states(name, hist_len):
    """Per update of the case: featureeng.update_host's state and tables (StoreState.to_host()), the definition of the device's."""
    c = case(name)
    store = FS.FeatureStore.empty(c.movies, c.n_users, c.n_movies, hist_len, device="cpu")
    out = []
    for b in c.batches:
        store.update(b)
        out.append(store._state.to_host())
    return tuple(out)


def bad_batches(last_ts_user, latest):
    """kind -> (a batch of four rows of which rows 1 and 3 are wrong in that kind, the message of row 1).  last_ts_user: a user whose
    latest applied timestamp is `latest`."""
    good = {"userId": np.array([RING_USER, FLIP_USER, LATE_USER, last_ts_user]), "movieId": np.array([1, 3, 5, 7]), "rating": np.array([4.0, 0.5, 3.5, 5.0]),
            "timestamp": np.full(4, latest + 10**6)}
    def wrong(key, values):
        b = {k: v.copy() for k, v in good.items()}
        b[key] = b[key].astype(np.float64 if key == "rating" else np.int64)
        b[key][[1, 3]] = values
        return b
    return {FE.ERR_USER: (wrong("userId", [cases.N_USERS, -1]), "ratings row 1: userId outside the user table"),
            FE.ERR_MOVIE: (wrong("movieId", [-7, cases.N_MOVIES]), "ratings row 1: movieId outside the movie table"),
            FE.ERR_RATING: (wrong("rating", [3.7, np.nan]), "ratings row 1: rating off the half-star scale 0, 0.5 .. 10"),
            FE.ERR_OLDER: (dict(good, userId=np.array([RING_USER, last_ts_user, LATE_USER, last_ts_user]), timestamp=np.array([latest + 10**6, latest - 1, latest + 10**6, 0])),
                           "ratings row 1: older than its user's latest rating")}
