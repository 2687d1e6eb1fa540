"""Inputs shared by tests/test_featureeng.py (CPU) and tests/test_gpu_featureeng.py: a hand-worked user and one synthetic rating set
that holds every case the feature-engineering rules distinguish."""
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
