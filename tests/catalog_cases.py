"""Inputs of the catalogue tests (sparrowrecsys_amd/catalog.py, sprk_catalog_build, sprk_catalog_similar) and the row-by-row restatement
of the average they are checked against.  tests/test_catalog.py asserts the properties the device tests rely on."""
import numpy as np

from sparrowrecsys_amd import schema as S

WAVE_MIN = 128           # k_catalog.h CAT_WAVE_MIN: a movie of this many ratings gets a wave of its own
SORT_CAP = 64            # the SPRK_FE_SORT_CAP the device tests lower the LDS sort to


def loop_average(ratings) -> float:
    """Movie.addRating as a plain loop over Python floats (IEEE doubles, every operation rounded on its own)."""
    avg, n = 0.0, 0
    for s in ratings:
        avg = (avg * float(n) + float(np.float32(s))) / float(n + 1)
        n += 1
    return avg


# ---- the hand-worked movie: the recurrence ends one ulp above sum / n ----
TWELVE = [2.0, 3.5, 3.0, 4.5, 2.5, 4.5, 0.5, 2.0, 1.0, 2.0, 5.0, 1.0]
TWELVE_AVG_HEX = "0x1.5000000000001p+1"
TWELVE_SUM_OVER_N_HEX = "0x1.5000000000000p+1"


# ---- the hand-worked catalogue: nine movies, three genres, in this file order (ids below 16: the HashMap iterates in id order) ----
#   pos id title          genres                 ratings (input order)   average              year
#    0   7 Seven (1995)   Action|Drama           4.0 3.0                 (4 * 1 + 3) / 2 = 3.5   1995
#    1   3 Three (2001)   Comedy                 3.5                     3.5                  2001
#    2   5 Five (1995)    Action|Comedy          5.0 2.0                 3.5                  1995
#    3   2 Two (1987)     Drama                  4.5                     4.5                  1987
#    4   9 Nine           Action                 none                    0.0                  0 (shorter than 6)
#    5   4 Four (20xx)    Comedy|Drama           1.0 2.0 3.0             1, 1.5, 2.0          0 (no integer)
#    6   1 One (2001)     none                   3.5                     3.5                  2001
#    7   6 Six (1999)     Action|Comedy|Drama    0.5                     0.5                  1999
#    8   8 Eight (2010)   none                   none                    0.0                  2010
HAND_MOVIES = {"movieId": [7, 3, 5, 2, 9, 4, 1, 6, 8],
               "title": ["Seven (1995)", "Three (2001)", "Five (1995)", "Two (1987)", "Nine", "Four (20xx)", "One (2001)", "Six (1999)", "Eight (2010)"],
               "genres": ["Action|Drama", "Comedy", "Action|Comedy", "Drama", "Action", "Comedy|Drama", "", "Action|Comedy|Drama", ""]}
HAND_RATINGS = {"movieId": [7, 4, 3, 5, 4, 2, 7, 1, 5, 6, 4, 12, -1, 0],      # (the last three: outside the table, and a movie it does not hold)
                "rating": [4.0, 1.0, 3.5, 5.0, 2.0, 4.5, 3.0, 3.5, 2.0, 0.5, 3.0, 5.0, 5.0, 5.0]}
HAND_AVG = {1: 3.5, 2: 4.5, 3: 3.5, 4: 2.0, 5: 3.5, 6: 0.5, 7: 3.5, 8: 0.0, 9: 0.0}
HAND_COUNT = {1: 1, 2: 1, 3: 1, 4: 3, 5: 2, 6: 1, 7: 2, 8: 0, 9: 0}
HAND_YEAR = {1: 2001, 2: 1987, 3: 2001, 4: 0, 5: 1995, 6: 1999, 7: 1995, 8: 2010, 9: 0}
# equal averages (3.5: movies 7, 3, 5, 1) fall back to the file position in a genre list and to the bucket (= id) order in the whole
# catalogue's; the unrated movies 8 and 9 come last
HAND_LISTS = {
    ("Action", "rating"): [7, 5, 6, 9], ("Comedy", "rating"): [3, 5, 4, 6], ("Drama", "rating"): [2, 7, 4, 6],
    (None, "rating"): [2, 1, 3, 5, 7, 4, 6, 8, 9],
    ("Action", "releaseYear"): [6, 7, 5, 9], ("Comedy", "releaseYear"): [3, 6, 5, 4], ("Drama", "releaseYear"): [6, 7, 2, 4],
    (None, "releaseYear"): [8, 1, 3, 6, 5, 7, 2, 4, 9],
}
# (query, mode, extra_n, size) -> the ranked ids and their scores, the score written as the Java computes it
HAND_SIMILAR = {
    # Action | Drama: movie 6 is in both lists and counts once, the query is removed
    (7, 0, 100, 10): ([2, 5, 4, 6, 9], [(1.0 / 3.0) / 2.0 * 0.7 + (4.5 / 5.0) * 0.3, (1.0 / 4.0) / 2.0 * 0.7 + (3.5 / 5.0) * 0.3,
                                        (1.0 / 4.0) / 2.0 * 0.7 + (2.0 / 5.0) * 0.3, (2.0 / 5.0) / 2.0 * 0.7 + (0.5 / 5.0) * 0.3,
                                        (1.0 / 3.0) / 2.0 * 0.7 + (0.0 / 5.0) * 0.3]),
    # Action: movies 5 and 7 score the same and come in id order
    (9, 0, 100, 10): ([5, 7, 6], [(1.0 / 3.0) / 2.0 * 0.7 + (3.5 / 5.0) * 0.3, (1.0 / 3.0) / 2.0 * 0.7 + (3.5 / 5.0) * 0.3,
                                  (1.0 / 4.0) / 2.0 * 0.7 + (0.5 / 5.0) * 0.3]),
    (9, 0, 100, 2): ([5, 7], None),
    # no genres, mode 1: the whole catalogue through the two heads; movie 8 has no genres either: 0 / 0 = NaN, the greatest
    (1, 1, 100, 20): ([8, 2, 3, 5, 7, 4, 6, 9], [float("nan"), (4.5 / 5.0) * 0.3, (3.5 / 5.0) * 0.3, (3.5 / 5.0) * 0.3, (3.5 / 5.0) * 0.3, (2.0 / 5.0) * 0.3,
                                                 (0.5 / 5.0) * 0.3, 0.0]),
    (1, 1, 2, 20): ([8, 2], None),                                             # heads [2, 1] and [8, 1]
    (1, 0, 100, 10): ([], None),                                               # mode 0, no genres: no candidates
    (10, 0, 100, 10): ([], None),                                              # a movie the table does not hold
}


GENRES_20 = list(S.GENRE_VOCAB) + ["(no genres listed)"]
GENRES_32 = list(S.GENRE_VOCAB) + ["Extra%d" % k for k in range(13)]


def _titles(rng, n):
    years = rng.randint(1990, 2000, n)                                          # ten years: many equal keys
    titles = np.array(["Movie %d (%d)" % (k, y) for k, y in enumerate(years)], dtype=object)
    titles[rng.permutation(n)[:n // 20]] = "Untitled"                          # no year: 0
    return titles.tolist()


# ---- the synthetic set: 300 movies, 20 genres, 20 000 ratings ----
N_TABLE, N_HELD, N_RATINGS = 340, 300, 20000
GENRE_MEMBERS = {0: 99, 1: 100, 2: 101, 3: 0, 4: 1, 5: SORT_CAP, 6: SORT_CAP + 1}     # against top_n = 100 and the LDS sort capacity 64
RATING_COUNTS = [0, 1, 2, SORT_CAP, SORT_CAP + 1, WAVE_MIN - 1, WAVE_MIN, WAVE_MIN + 1, 700]    # of the first held movies, in file order


def synthetic(grouped=False, seed=7, rated=True):
    """-> (ratings, movies, info).  300 of the ids below 340 are held, in a shuffled file order; genres 0 .. 6 of 20 have the member counts
    of GENRE_MEMBERS, the others a tenth of the movies each (some movies have none); years from ten values, a twentieth of the titles
    without one.  The first movies of the file have the RATING_COUNTS; the other ratings fall at random, 300 of them on ids that are
    negative, past the table or not held.  Half-star ratings.  Fully shuffled; grouped=True: the same rows sorted by movie id (stable:
    every movie's rows keep their order, so the result is the same).  rated=False: no ratings at all."""
    rng = np.random.RandomState(seed)
    ids = rng.permutation(N_TABLE)[:N_HELD]
    member = rng.rand(N_HELD, 20) < 0.1
    for g, k in GENRE_MEMBERS.items():
        member[:, g] = False
        member[rng.permutation(N_HELD)[:k], g] = True
    genres = ["|".join(GENRES_20[g] for g in np.flatnonzero(row)) for row in member]
    movies = {"movieId": ids.tolist(), "title": _titles(rng, N_HELD), "genres": genres}
    fixed = np.repeat(ids[:len(RATING_COUNTS)], RATING_COUNTS)
    others = ids[len(RATING_COUNTS):]
    rest = N_RATINGS - len(fixed)
    movie = np.concatenate([fixed, others[rng.randint(0, len(others), rest)]])
    not_held = np.setdiff1d(np.arange(N_TABLE), ids)
    odd = len(fixed) + rng.permutation(rest)[:300]
    movie[odd[:100]] = -1 - rng.randint(0, 1000, 100)
    movie[odd[100:200]] = N_TABLE + rng.randint(0, 10 ** 6, 100)
    movie[odd[200:]] = not_held[rng.randint(0, len(not_held), 100)]
    rating = (rng.randint(1, 11, N_RATINGS) * 0.5).astype(np.float32)
    order = rng.permutation(N_RATINGS)
    movie, rating = movie[order], rating[order]
    if grouped:
        by_movie = np.argsort(movie, kind="stable")
        movie, rating = movie[by_movie], rating[by_movie]
    if not rated:
        movie, rating = movie[:0], rating[:0]
    info = {"ids": ids, "fixed": dict(zip(ids[:len(RATING_COUNTS)].tolist(), RATING_COUNTS))}
    return {"movieId": movie.astype(np.int64), "rating": rating}, movies, info


# ---- many ratings on few movies: the ratings side past one round of its grid ----
def many_ratings(n=530_000, n_movies=600, seed=19):
    """-> (ratings, movies).  ``n`` shuffled half-star ratings on ``n_movies`` movies of one to three of 20 genres, ids 0 .. n_movies - 1 in a
    shuffled file order; a thousandth of the ratings fall on ids outside the table.  530 000 > 2048 x 256: k_cat_count and k_cat_scatter
    stride, and the per-movie sort takes every segment (about 880 ratings each) in LDS."""
    rng = np.random.RandomState(seed)
    ids = rng.permutation(n_movies)
    genres = ["|".join(GENRES_20[g] for g in np.sort(rng.permutation(20)[:rng.randint(1, 4)])) for _ in range(n_movies)]
    movies = {"movieId": ids.tolist(), "title": _titles(rng, n_movies), "genres": genres}
    movie = rng.randint(0, n_movies, n)
    odd = rng.permutation(n)[:n // 1000]
    movie[odd] = np.where(rng.rand(len(odd)) < 0.5, -1 - rng.randint(0, 1000, len(odd)), n_movies + rng.randint(0, 10 ** 6, len(odd)))
    rating = (rng.randint(1, 11, n) * 0.5).astype(np.float32)
    return {"movieId": movie.astype(np.int64), "rating": rating}, movies


# ---- a table for candidate counts: disjoint one-genre movies and eight query movies ----
COUNT_GENRES = {10: 24, 11: 25, 12: 1, 13: 2, 14: 63, 15: 64, 16: 65, 17: 0}   # genre -> its members next to the query
COUNT_QUERIES = {1024: 10, 1025: 11, 1: 12, 2: 13, 63: 14, 64: 15, 65: 16, 0: 17}   # the mode-0 candidate count -> the query's own genre


def counts_table(seed=11):
    """-> (ratings, movies, queries {count: movie id}).  Genres 0 .. 9 have 150 rated members each, genres 10 .. 17 the COUNT_GENRES; every
    such movie has one genre and between one and three ratings.  Eight unrated query movies: the 1024 and 1025 ones carry genres 0 .. 9
    (they are at the end of those lists, outside the heads of 100) and genre 10 or 11 (where they are inside the head), the others one
    small genre each."""
    rng = np.random.RandomState(seed)
    genre_of = np.concatenate([np.repeat(np.arange(10), 150)] + [np.repeat(g, k) for g, k in COUNT_GENRES.items()])
    n = len(genre_of)
    ids = 1 + rng.permutation(n + len(COUNT_QUERIES) + 40)[:n + len(COUNT_QUERIES)]
    genres = [GENRES_20[g] for g in genre_of]
    queries = {}
    for k, (count, g) in enumerate(COUNT_QUERIES.items()):
        own = [GENRES_20[g]]
        genres.append("|".join(GENRES_20[:10] + own if count >= 1024 else own))
        queries[count] = int(ids[n + k])
    movies = {"movieId": ids.tolist(), "title": _titles(rng, len(ids)), "genres": genres}
    movie = np.repeat(ids[:n], rng.randint(1, 4, n))
    rating = (rng.randint(1, 11, len(movie)) * 0.5).astype(np.float32)
    order = rng.permutation(len(movie))
    return {"movieId": movie[order].astype(np.int64), "rating": rating[order]}, movies, queries


def all_genres_table(seed=13):
    """-> (ratings, movies, query).  700 movies with six of 32 genres each (every genre has more than 100 members) and one movie that
    carries all 32: 3 200 gathered entries in mode 0, 3 400 in mode 1."""
    rng = np.random.RandomState(seed)
    n = 700
    ids = 1 + rng.permutation(n + 60)[:n + 1]
    genres = ["|".join(GENRES_32[g] for g in np.sort(rng.permutation(32)[:6])) for _ in range(n)] + ["|".join(GENRES_32)]
    movies = {"movieId": ids.tolist(), "title": _titles(rng, n + 1), "genres": genres}
    movie = ids[rng.randint(0, n + 1, 4000)]
    rating = (rng.randint(1, 11, len(movie)) * 0.5).astype(np.float32)
    return {"movieId": movie.astype(np.int64), "rating": rating}, movies, int(ids[n])
