"""Inputs of the user-embedding tests (sparrowrecsys_amd/userembedding.py, sprk_user_emb) and the row-by-row restatement of the
definition they are checked against.  tests/test_userembedding.py asserts the properties the device tests rely on."""
import numpy as np

NAN = np.float32(np.nan)


def loop_reference(user, row, emb, has, n_users, mode="mean", forward=False):
    """The definition as a plain loop: per user, from the LAST input row to the first (forward=True: the wrong way round),
    acc = acc + emb[row] in float32 for the rows that have an embedding; mean: / float32(all the user's rows); sum: as it is."""
    D = emb.shape[1]
    acc = np.zeros((n_users, D), dtype=np.float32)
    rows_all, rows_emb = np.zeros(n_users, dtype=np.int64), np.zeros(n_users, dtype=np.int64)
    order = range(len(user)) if forward else range(len(user) - 1, -1, -1)
    for i in order:
        u, r = int(user[i]), int(row[i])
        rows_all[u] += 1
        if 0 <= r < len(has) and has[r]:
            rows_emb[u] += 1
            acc[u] = acc[u] + emb[r].astype(np.float32)
    count = rows_all if mode == "mean" else rows_emb
    out = np.zeros_like(acc)
    for u in range(n_users):
        if count[u]:
            out[u] = acc[u] / np.float32(count[u]) if mode == "mean" else acc[u]
    return out, (count > 0).astype(np.uint8), count.astype(np.int32)


# ---- the hand-worked user ----
# One user (id 0 of a table of one), four ratings in this file order; the item table has four rows, row 1 without an embedding:
#   input row 0: item row 0 = (1.0,   3.0,  2^24)
#   input row 1: item row 1 = no embedding (has = 0, the row holds NaN): skipped, but counted
#   input row 2: item row 2 = (2^-24, -1.5, 1.0)
#   input row 3: item row 3 = (2^-24, 0.25, 1.0)
# The definition sums from input row 3 back to input row 0:
#   dim 0: 2^-24 + 2^-24 = 2^-23;  2^-23 + 1.0 = 1 + 2^-23, one ulp above 1.0            (forward: 1.0 + 2^-24 ties to 1.0, twice: 1.0)
#   dim 1: 0.25 + -1.5 = -1.25;  -1.25 + 3.0 = 1.75                                      (exact either way)
#   dim 2: 1.0 + 1.0 = 2.0;  2.0 + 2^24 = 16777218, one ulp above 2^24                   (forward: 2^24 + 1.0 ties to 2^24, twice: 2^24)
# movieCount = 4, so the mean is the sum's exponent less two: 0.25 + 2^-25, 0.4375, 4194304.5.
HAND_USER = np.array([0, 0, 0, 0], dtype=np.int32)
HAND_ROW = np.array([0, 1, 2, 3], dtype=np.int32)
HAND_EMB = np.array([[1.0, 3.0, 2.0 ** 24], [NAN, NAN, NAN], [2.0 ** -24, -1.5, 1.0], [2.0 ** -24, 0.25, 1.0]], dtype=np.float32)
HAND_HAS = np.array([1, 0, 1, 1], dtype=np.uint8)
HAND_MEAN_WORDS = np.array([[0x3E800001, 0x3EE00000, 0x4A800001]], dtype=np.uint32)
HAND_SUM_WORDS = np.array([[0x3F800001, 0x3FE00000, 0x4B800001]], dtype=np.uint32)
HAND_FORWARD_SUM_WORDS = np.array([[0x3F800000, 0x3FE00000, 0x4B800000]], dtype=np.uint32)
HAND_COUNT = {"mean": 4, "sum": 3}


def hand_worked():
    return {"user": HAND_USER, "row": HAND_ROW, "emb": HAND_EMB, "has": HAND_HAS, "n_users": 1}


# ---- the synthetic set ----
N_RATINGS, N_USERS, N_ITEMS = 5000, 97, 211
NO_RATING_USERS = (5, 50, 96)
NO_EMBEDDING_USER = 7          # every rating names a movie without an embedding
LONG_USER, LONG_LEN = 11, 300  # with SPRK_FE_SORT_CAP = 64: chunks and merge passes
COUNT_3_USER, COUNT_7_USER = 2, 3
PAD = np.float32(7e7)          # the columns between D and the stride: never read


def synthetic(D=10, stride=12, grouped=False, seed=3):
    """5 000 ratings of 97 users over a table of 211 rows of D floats at `stride`; row magnitudes from {1e-3, 1, 1e3}; a fifth of the
    table rows have has = 0 and hold NaN; some ratings name row -1 or a row past the table; users 5, 50 and 96 have no rating, user 7
    only rows without an embedding, user 11 has 300 ratings, users 2 and 3 have 3 and 7.  Fully shuffled; grouped=True: the same ratings
    sorted by user (stable: every user's rows keep their order, so the result is the same)."""
    rng = np.random.RandomState(seed)
    has = np.ones(N_ITEMS, dtype=np.uint8)
    has[rng.permutation(N_ITEMS)[:N_ITEMS // 5]] = 0
    emb = np.full((N_ITEMS, stride), PAD, dtype=np.float32)
    scale = np.array([1e-3, 1.0, 1e3])[rng.randint(0, 3, N_ITEMS)]
    emb[:, :D] = (rng.standard_normal((N_ITEMS, D)) * scale[:, None]).astype(np.float32)
    emb[has == 0, :D] = NAN
    lens = np.zeros(N_USERS, dtype=np.int64)
    fixed = {LONG_USER: LONG_LEN, COUNT_3_USER: 3, COUNT_7_USER: 7, NO_EMBEDDING_USER: 9}
    for u, n in fixed.items():
        lens[u] = n
    free = [u for u in range(N_USERS) if u not in fixed and u not in NO_RATING_USERS]
    rest = N_RATINGS - int(lens.sum())
    lens[free] = 1
    extra = rng.multinomial(rest - len(free), np.ones(len(free)) / len(free))
    lens[free] += extra
    user = np.repeat(np.arange(N_USERS), lens)
    row = rng.randint(0, N_ITEMS, N_RATINGS)
    odd = rng.permutation(N_RATINGS)[:150]
    row[odd[:50]] = -1
    row[odd[50:100]] = N_ITEMS
    row[odd[100:]] = N_ITEMS + rng.randint(1, 10 ** 6, 50)
    row[user == NO_EMBEDDING_USER] = np.flatnonzero(has == 0)[:9]
    order = rng.permutation(N_RATINGS)
    user, row = user[order], row[order]
    if grouped:
        by_user = np.argsort(user, kind="stable")
        user, row = user[by_user], row[by_user]
    return {"user": user.astype(np.int32), "row": row.astype(np.int32), "emb": emb, "has": has, "n_users": N_USERS, "D": D}
