"""Inputs shared by tests/test_featureeng.py (CPU) and tests/test_gpu_featureeng.py: a hand-worked user, one synthetic rating set
that holds every case the feature-engineering rules distinguish, rating sets aimed at the device kernels' tile, grid and width edges,
and a row-by-row restatement of the definition (definition_by_rows)."""
import fractions
import math

import numpy as np

# ---- the hand-worked example (expected values: tests/test_featureeng.py) ----
HAND_MOVIES = {
    "movieId": [1, 2, 3, 4, 5],
    "title": ["Toy Story (1995)", "Heat (1995)", "Odd (2001)", "Short", "Noir (1950)"],
    "genres": ["Adventure|Animation|Children|Comedy|Fantasy", "Action|Crime|Thriller", "Zydeco|Drama", "Comedy", "Film-Noir|Zydeco"],
}
# user 7: seven ratings in no order, two of them at timestamp 300 (input rows 1 and 4); movie 9 is not in the table; user 3: one rating
HAND_RATINGS = {
    "userId": np.array([7, 7, 7, 7, 7, 7, 7, 3]),
    "movieId": np.array([4, 3, 1, 1, 5, 2, 9, 1]),
    "rating": np.array([1.5, 5.0, 3.0, 4.0, 3.5, 2.0, 4.5, 5.0]),
    "timestamp": np.array([500, 300, 600, 100, 300, 200, 400, 50]),
}


def synthetic_movies():
    """60 movies with ids 1 .. 119 (odd ids only: gaps): genre lists of 1-5 entries drawn so that ties are common; 'Zydeco' and 'IMAX 3D' are
    outside the vocabulary, and movies 1, 3, 5 carry 'Zydeco' so that it reaches a top five; titles with and without a year."""
    from sparrowrecsys_amd import schema as S
    rng = np.random.RandomState(5)
    ids, titles, genres = [], [], []
    for k in range(60):
        mid = 2 * k + 1
        ids.append(mid)
        titles.append("Movie %d (%d)" % (mid, 1930 + (mid * 7) % 90) if k % 9 else "M%d" % (mid % 10))
        pool = S.GENRE_VOCAB[:6] + ["Zydeco", "IMAX 3D"]
        g = list(rng.choice(pool, size=1 + k % 5, replace=False))
        if mid in (1, 3, 5):
            g = ["Zydeco", S.GENRE_VOCAB[mid]]               # Action, Horror, War
        genres.append("|".join(g))
    return {"movieId": ids, "title": titles, "genres": genres}


N_USERS, N_MOVIES = 40, 150            # both above the greatest id (user 30, movie 121)


def synthetic_ratings(seed=11):
    """A few thousand ratings, shuffled, user ids with gaps.  By user:
      2: 1 rating   4: 2   5: 3   (0, 1, 3, ...: none)
      8: 100   9: 101   10: 102   12: 250        the window starts to slide at position 100
      14: 40 ratings, all at one timestamp        ordered by input row alone
      15: 30 ratings, none positive               no history, no genres
      17: 130 ratings: positions 0-19 positive, then none     more than hist_len positives in the window, fewer after it slides
      20: 12 ratings of movies 1, 3, 5 only, all positive     'Zydeco' (outside the vocabulary) leads the top five
      21: 6 ratings, each positive, of movie 121 (not in the movie table) and movie 119
      30: 60 ordinary ratings
    Movie 117 is rated exactly once (user 5's latest rating, the only one of that user that becomes a sample)."""
    rng = np.random.RandomState(seed)
    movie_ids = np.arange(1, 116, 2)                       # 1 .. 115; 117, 119, 121 are placed by hand
    u, m, r, t = [], [], [], []
    def add(user, movies, ratings, stamps):
        u.extend([user] * len(movies)); m.extend(movies); r.extend(ratings); t.extend(stamps)
    def ordinary(user, n):
        add(user, rng.choice(movie_ids, n), rng.randint(1, 11, n) / 2.0, rng.randint(1_000_000, 1_000_400, n))    # few distinct timestamps: many ties
    ordinary(2, 1)
    ordinary(4, 2)
    add(5, [7, 117, 9], [4.0, 2.5, 5.0], [10, 30, 20])
    for user, n in ((8, 100), (9, 101), (10, 102), (12, 250), (30, 60)):
        ordinary(user, n)
    add(14, rng.choice(movie_ids, 40), rng.randint(1, 11, 40) / 2.0, [777] * 40)
    add(15, rng.choice(movie_ids, 30), rng.randint(1, 7, 30) / 2.0, rng.randint(0, 50, 30))
    add(17, rng.choice(movie_ids, 130), [4.5] * 20 + [2.0] * 110, np.arange(130) * 3)
    add(20, [1, 3, 5] * 4, [5.0] * 12, rng.randint(0, 5, 12))
    add(21, [121, 119] * 3, [4.0] * 6, np.arange(6) - 3)                                    # (negative timestamps sort too)
    order = rng.permutation(len(u))
    return {"userId": np.asarray(u, dtype=np.int64)[order], "movieId": np.asarray(m, dtype=np.int64)[order],
            "rating": np.asarray(r, dtype=np.float64)[order], "timestamp": np.asarray(t, dtype=np.int64)[order]}


# ---- the definition, row by row ----
def _rhe(x: fractions.Fraction) -> int:
    """Round half to even of an exact rational."""
    f = math.floor(x)
    twice = 2 * (x - f)
    return f + (1 if twice > 1 or (twice == 1 and f % 2) else 0)


def _rhe_sqrt(x: fractions.Fraction) -> int:
    """Round half to even of sqrt(x), x an exact rational >= 0: h = floor(sqrt(x)), then (h + 1/2)^2 against x."""
    h = math.isqrt(math.floor(x))
    half = fractions.Fraction(2 * h + 1, 2) ** 2
    return h + (1 if half < x or (half == x and h % 2) else 0)


def definition_by_rows(ratings, table, hist_len):
    """DESIGN.md section 5.7 restated one row at a time: Python integers and fractions, a sorted() per user, a loop over the previous
    100 rows per position, a dict of genre counts.  Returns the dict featureeng.samples_host returns.  For a few thousand ratings."""
    from sparrowrecsys_amd import featureeng as FE
    from sparrowrecsys_amd import schema as S
    table = FE.movie_table(table)
    users = [int(v) for v in np.asarray(ratings["userId"]).tolist()]
    movies = [int(v) for v in np.asarray(ratings["movieId"]).tolist()]
    stored = np.asarray(ratings["rating"]).astype(np.float32)
    stamps = [int(v) for v in np.asarray(ratings["timestamp"]).tolist()]
    r2 = []
    for v in stored.tolist():
        twice = 2 * fractions.Fraction(v)
        assert twice.denominator == 1 and 0 <= twice <= 20, v
        r2.append(int(twice))
    hundredth = lambda h: np.float32(h / 100.0)
    # movie side: count, S, Q over all ratings
    m_n, m_s, m_q = {}, {}, {}
    for m, x in zip(movies, r2):
        m_n[m] = m_n.get(m, 0) + 1
        m_s[m] = m_s.get(m, 0) + x
        m_q[m] = m_q.get(m, 0) + x * x
    def average(n, s):
        return _rhe(fractions.Fraction(50 * s, n))
    def stddev(n, s, q):
        return 0 if n < 2 else _rhe_sqrt(fractions.Fraction(10000 * (n * q - s * s), 4 * n * (n - 1)))
    in_table = lambda m: m < len(table.has) and table.has[m]
    by_user = {}
    for row, u in enumerate(users):
        by_user.setdefault(u, []).append(row)
    keys = FE.sample_keys(hist_len)
    out = {k: [] for k in keys}
    for u in sorted(by_user):
        rows = sorted(by_user[u], key=lambda row: (stamps[row], row))
        for p, row in enumerate(rows):
            window = rows[max(0, p - 100):p]
            if len(window) <= 1:
                continue
            n = s = q = 0
            for w in window:
                n += 1
                s += r2[w]
                q += r2[w] * r2[w]
            history, genre_count = [], {}
            for w in reversed(window):                          # most recent first
                if r2[w] >= 7:
                    history.append(movies[w])
                    if in_table(movies[w]):
                        for g in range(32):
                            if (int(table.mask[movies[w]]) >> g) & 1:
                                genre_count[g] = genre_count.get(g, 0) + 1
            top = sorted(genre_count, key=lambda g: (-genre_count[g], g))[:5]
            top = [g if g < S.N_GENRES else -1 for g in top] + [-1] * (5 - len(top))
            history = history[:hist_len] + [0] * max(0, hist_len - len(history))
            m = movies[row]
            out["userId"].append(u); out["movieId"].append(m); out["rating"].append(stored[row]); out["timestamp"].append(stamps[row])
            out["label"].append(1 if r2[row] >= 7 else 0); out["source_row"].append(row)
            for k in range(3):
                out["movieGenre%d" % (k + 1)].append(int(table.genre[m, k]) if in_table(m) else -1)
            for k in range(5):
                out["userGenre%d" % (k + 1)].append(top[k])
            for k in range(hist_len):
                out["userRatedMovie%d" % (k + 1)].append(history[k])
            out["releaseYear"].append(np.float32(int(table.year[m]) if in_table(m) else 1990))
            out["movieRatingCount"].append(np.float32(m_n[m]))
            out["movieAvgRating"].append(hundredth(average(m_n[m], m_s[m])))
            out["movieRatingStddev"].append(hundredth(stddev(m_n[m], m_s[m], m_q[m])))
            out["userRatingCount"].append(np.float32(n))
            out["userAvgRating"].append(hundredth(average(n, s)))
            out["userRatingStddev"].append(hundredth(stddev(n, s, q)))
    floats = set(FE.DENSE_KEYS + ["rating"])
    return {k: np.asarray(out[k], dtype=np.float32 if k in floats else np.int64 if k == "timestamp" else np.int32) for k in keys}


def _shuffled(rng, u, m, r, t):
    order = rng.permutation(len(u))
    return {"userId": np.asarray(u, dtype=np.int64)[order], "movieId": np.asarray(m, dtype=np.int64)[order],
            "rating": np.asarray(r, dtype=np.float64)[order], "timestamp": np.asarray(t, dtype=np.int64)[order]}


def _ordinary(rng, n):
    """n ratings of the synthetic movies: movie ids, half-star ratings 0.5 .. 5.0, timestamps from a range of 400 (many ties)."""
    return rng.choice(np.arange(1, 116, 2), n), rng.randint(1, 11, n) / 2.0, rng.randint(1_000_000, 1_000_400, n)


# ---- all 32 genre counters ----
ALL_GENRES_TIES = [(7, 8), (15, 16), (23, 24), (18, 24), (5, 31), (12, 20)]     # dictionary ids with equal counts, from different counter registers
ALL_GENRES_USERS, ALL_GENRES_MOVIES = 80, 48


def all_genres_movies():
    """Movie g (g = 0 .. 31) carries dictionary id g alone: the 19 vocabulary genres, then 13 further strings in this order.  Movies
    32 .. 39 carry four genres, one per counter register: ids k, k + 8, k + 16, k + 24."""
    from sparrowrecsys_amd import schema as S
    names = list(S.GENRE_VOCAB) + ["Extra%02d" % k for k in range(13)]
    ids, titles, genres = [], [], []
    for g in range(32):
        ids.append(g); titles.append("One genre %d (2000)" % g); genres.append(names[g])
    for k in range(8):
        ids.append(32 + k); titles.append("Four genres %d (2001)" % k); genres.append("|".join(names[k + 8 * j] for j in range(4)))
    return {"movieId": ids, "title": titles, "genres": genres}


def all_genres_ratings(seed=17):
    """Goes with all_genres_movies.  Users:
      g (0 .. 31): movie g three times, each of the movies 0 .. 3 other than g once, all positive, then two low ratings: dictionary id g
                   leads the top five with count 3 and vocabulary genres follow, so a lost count of g changes a written genre
      40 + k, pair (a, b) = ALL_GENRES_TIES[k]: movies a and b twice each, then two low ratings: a tie for the lead
      50 + k: four vocabulary movies outside the pair three times each, movies a and b twice each: a tie for the fifth place
      60 + k (k = 0 .. 7): the four-genre movie 32 + k twice and movie k once: every register counts in one window
    Timestamps ascend in the order written here; the rows are shuffled."""
    rng = np.random.RandomState(seed)
    u, m, r, t = [], [], [], []
    def add(user, movies, ratings):
        stamps = 100 * np.arange(len(movies)) + user
        u.extend([user] * len(movies)); m.extend(movies); r.extend(ratings); t.extend(stamps)
    for g in range(32):
        liked = [g] * 3 + [x for x in range(4) if x != g]
        add(g, liked + [1, 2], [4.0] * len(liked) + [1.0, 2.5])
    for k, (a, b) in enumerate(ALL_GENRES_TIES):
        add(40 + k, [b, a, b, a, 0, 1], [5.0] * 4 + [1.0, 1.5])
        leaders = [x for x in (1, 2, 3, 4, 6, 9) if x not in (a, b)][:4]
        add(50 + k, leaders * 3 + [b, a, b, a] + [0, 1], [3.5] * 16 + [0.5, 3.0])
    for k in range(8):
        add(60 + k, [32 + k, k, 32 + k, 0, 1], [4.5, 4.5, 4.5, 2.0, 2.0])
    return _shuffled(rng, u, m, r, t)


# ---- merge shapes (SPRK_FE_SORT_CAP = 64 and 128) ----
MERGE_LENGTHS = {1: 64, 2: 65, 3: 128, 4: 129, 5: 192, 6: 320, 7: 321, 8: 1000}
MERGE_ONE_STAMP, MERGE_DESCENDING, MERGE_EXTREMES = (9, 300), (10, 200), (11, 70)
MERGE_USERS = 13
INT64_MAX, INT64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def merge_shapes_ratings(seed=23):
    """Users 1 .. 8 of MERGE_LENGTHS ratings (at capacity 64: exactly one, two, three and five chunks, one more than one, two and five
    chunks, sixteen chunks with a short last one), user 9 with 300 ratings at one timestamp, user 10 with 200 ratings whose timestamps
    descend with the input row, user 11 with 70 ratings: INT64_MAX twice, INT64_MIN twice, ordinary values.  Shuffled."""
    rng = np.random.RandomState(seed)
    u, m, r, t = [], [], [], []
    for user, n in list(MERGE_LENGTHS.items()) + [MERGE_ONE_STAMP, MERGE_DESCENDING, MERGE_EXTREMES]:
        mm, rr, tt = _ordinary(rng, n)
        u.extend([user] * n); m.extend(mm); r.extend(rr); t.extend(tt)
    out = _shuffled(rng, u, m, r, t)
    out["timestamp"][out["userId"] == MERGE_ONE_STAMP[0]] = 4242
    out["timestamp"][out["userId"] == MERGE_DESCENDING[0]] = 5_000_000 - 7 * np.arange(MERGE_DESCENDING[1])
    rows = np.flatnonzero(out["userId"] == MERGE_EXTREMES[0])
    out["timestamp"][rows[[3, 40, 12, 66]]] = [INT64_MAX, INT64_MAX, INT64_MIN, INT64_MIN]
    return out


# ---- the rating scale's ends ----
SCALE_USERS = 4


def scale_ends_ratings(seed=29):
    """User 1: ratings 0.0, -0.0 and 10.0 only; in time order the first two are 0.0 and 10.0, so the third's window is exactly {0.0, 10.0}
    (stddev 7.07, the greatest there is).  User 2: 100 ratings of 10.0, then 12 more: the window sums reach S = 2000, Q = 40000.  Shuffled."""
    rng = np.random.RandomState(seed)
    one = [0.0, 10.0, -0.0, 10.0, 10.0, -0.0, 0.0, 0.0, 10.0, -0.0, 10.0, 0.0, -0.0, 10.0]
    two = [10.0] * 100 + [10.0, 0.0, 5.0, 10.0, -0.0, 0.5, 9.5, 10.0, 0.0, 10.0, 3.5, 10.0]
    u = [1] * len(one) + [2] * len(two)
    m = list(rng.choice(np.arange(1, 116, 2), len(u)))
    t = list(50 * np.arange(len(one))) + list(1000 + np.arange(len(two)) // 2)         # (user 2: pairs of equal timestamps, input row decides)
    out = _shuffled(rng, u, m, one + two, t)
    rows = np.flatnonzero(out["userId"] == 2)                  # user 2's ratings in input-row order, so that equal timestamps keep it
    out["rating"][rows] = two
    out["timestamp"][rows] = 1000 + np.arange(len(two)) // 2
    return out


# ---- users far apart: the scans over more than one tile ----
SPARSE_EDGE_IDS = [0, 1022, 1023, 1024, 1025, 2047, 2048, 262_142, 262_143, 262_144, 262_145]


def sparse_users_ratings(n_users=300_000, seed=31):
    """Users of 3 - 150 ratings at SPARSE_EDGE_IDS (both sides of the scan tile of 1024 users and of the 256-tile round of the scan over
    the tiles' totals), at n_users - 1 and at 40 random ids; three more users of 1 and 2 ratings; every other id is empty.  Shuffled."""
    rng = np.random.RandomState(seed)
    ids = sorted(set(SPARSE_EDGE_IDS + [n_users - 1] + [int(v) for v in rng.randint(0, n_users, 40)]))
    u, m, r, t = [], [], [], []
    for user in ids:
        n = int(rng.randint(3, 151))
        mm, rr, tt = _ordinary(rng, n)
        u.extend([user] * n); m.extend(mm); r.extend(rr); t.extend(tt)
    for user, n in ((1021, 1), (262_146, 2), (n_users - 2, 2)):
        if user not in ids:
            mm, rr, tt = _ordinary(rng, n)
            u.extend([user] * n); m.extend(mm); r.extend(rr); t.extend(tt)
    return _shuffled(rng, u, m, r, t)


# ---- one movie with millions of ratings, users past the short sort's grid ----
POPULAR_MOVIE = 7
SHORT_SORT_GRID = 1_048_576            # k_fe_sort_short's greatest grid: users beyond it are reached by its stride


def singletons_ratings(n_single=4_500_000, seed=0):
    """n_single users with one rating each, all of POPULAR_MOVIE, uniformly random half-stars 0.0 .. 10.0; 30 ordinary users of 3 - 300
    ratings, ten in each third of the id range (at the full size: below SHORT_SORT_GRID, up to twice that, above), every third of which also
    rates the popular movie.  Shuffled.  Returns a dict: ratings, n_users, n_movies, ordinary_users, ordinary_rows (the input rows of
    the ordinary users' ratings, ascending) and popular = the popular movie's (n, S, Q) over all ratings."""
    rng = np.random.RandomState(seed)
    n_users = n_single + 40
    third = SHORT_SORT_GRID if n_users > 3 * SHORT_SORT_GRID else n_users // 3
    ordinary = np.sort(np.concatenate([z * third + rng.choice(third, 10, replace=False) for z in range(3)]))
    ordinary[[0, 10, 20]] = [0, third, 2 * third]              # the first user of each stride of the grid
    ordinary = np.unique(ordinary)
    single_ids = np.setdiff1d(np.arange(n_users, dtype=np.int64), ordinary)[:n_single]
    u, m, r, t = [single_ids], [np.full(n_single, POPULAR_MOVIE)], [rng.randint(0, 21, n_single) / 2.0], [rng.randint(0, 1 << 40, n_single)]
    for k, user in enumerate(ordinary):
        n = int(rng.randint(3, 301))
        mm, rr, tt = _ordinary(rng, n)
        if k % 3 == 0:
            mm[n // 2] = POPULAR_MOVIE
        u.append(np.full(n, user)); m.append(mm); r.append(rr); t.append(tt)
    ratings = _shuffled(rng, np.concatenate(u), np.concatenate(m), np.concatenate(r), np.concatenate(t))
    r2 = np.rint(2 * ratings["rating"][ratings["movieId"] == POPULAR_MOVIE]).astype(np.int64)
    popular = (int(r2.size), int(r2.sum()), int((r2 * r2).sum()))
    return {"ratings": ratings, "n_users": int(n_users), "n_movies": N_MOVIES, "ordinary_users": ordinary, "popular": popular,
            "ordinary_rows": np.flatnonzero(np.isin(ratings["userId"], ordinary))}


def singletons_expectation(case, movies, hist_len=5):
    """What samples_host gives for a singletons_ratings case, without its per-rating work on the single ratings (they give no sample):
    the definition on the ordinary users' ratings alone, source_row mapped back to the whole set's rows, and the three per-movie
    columns replaced by the exact scalar rules (featureeng.avg_h, sd_h) on the sums over ALL ratings."""
    from sparrowrecsys_amd import featureeng as FE
    ratings, rows = case["ratings"], case["ordinary_rows"]
    want = FE.samples_host({k: v[rows] for k, v in ratings.items()}, movies, hist_len, n_users=case["n_users"], n_movies=case["n_movies"])
    want["source_row"] = rows[want["source_row"]].astype(np.int32)
    r2 = np.rint(2 * ratings["rating"]).astype(np.int64)
    count = np.bincount(ratings["movieId"], minlength=case["n_movies"])
    s = np.bincount(ratings["movieId"], weights=r2, minlength=case["n_movies"]).astype(np.int64)           # (exact in float64: below 2^53)
    q = np.bincount(ratings["movieId"], weights=r2 * r2, minlength=case["n_movies"]).astype(np.int64)
    seen = np.unique(want["movieId"])
    avg, sd = np.zeros(case["n_movies"], dtype=np.int64), np.zeros(case["n_movies"], dtype=np.int64)
    for i in seen:
        avg[i], sd[i] = FE.avg_h(count[i], s[i]), FE.sd_h(count[i], s[i], q[i])
    mk = want["movieId"]
    want["movieRatingCount"] = count[mk].astype(np.float32)
    want["movieAvgRating"] = FE.hundredths(avg[mk])
    want["movieRatingStddev"] = FE.hundredths(sd[mk])
    return want


def sd_h_in_64_bits(n, s, q):
    """featureeng.sd_h's steps with every product wrapped to 64 bits: what a device evaluation without 128-bit products would give."""
    wrap = lambda v: v & ((1 << 64) - 1)
    if n < 2:
        return 0
    N, d = wrap(wrap(n * q) - wrap(s * s)), wrap(n * (n - 1))
    R = wrap(N * 10000)
    h = 0
    for bit in (512, 256, 128, 64, 32, 16, 8, 4, 2, 1):
        c = h | bit
        if wrap(wrap(4 * c * c) * d) <= R:
            h = c
    t = wrap(wrap((2 * h + 1) * (2 * h + 1)) * d)
    if t < R or (t == R and h & 1):
        h += 1
    return h


# ---- one user longer than the capped grids ----
def one_long_user_ratings(n=530_000, seed=37):
    """One user (id 2 of 4) with n ratings, timestamps from a range of 5000: about a hundred ratings per timestamp."""
    rng = np.random.RandomState(seed)
    return {"userId": np.full(n, 2, dtype=np.int64), "movieId": rng.choice(np.arange(1, 116, 2), n).astype(np.int64),
            "rating": rng.randint(1, 11, n) / 2.0, "timestamp": rng.randint(0, 5000, n).astype(np.int64)}
