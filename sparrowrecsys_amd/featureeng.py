"""Feature engineering: ``ratings.csv`` + ``movies.csv`` -> the training samples and the feature store, without Spark.

The reference builds its samples (``testSamples.csv``) and its ``uf:`` / ``mf:`` feature hashes with a Spark job,
``FeatureEngForRecModel`` (FeatureEngForRecModel.scala:21-130; the PySpark twin is the same).  This module is that job's arithmetic:
:func:`samples_host` is the DEFINITION, in numpy and integer arithmetic, and :func:`build` computes the same bits on the device
(``sprk_feature_eng``, csrc/k_feature_eng.h).  The rules (DESIGN.md section 5.7 has them with their sources):

* ``label = rating >= 3.5``.
* Movie side: ``releaseYear`` from the title -- with ``t = title.trim``: 1990 if ``len(t) < 6``, else ``int(t[len(title) - 5 : len(title) - 1])``,
  the indices taken from the UNTRIMMED length as the reference does; ``movieGenre1..3`` = the first three ``|``-separated genres; a rating
  whose movie the table does not hold gets 1990 and no genres.  Per movie over ALL ratings: ``movieRatingCount``, ``movieAvgRating``,
  ``movieRatingStddev`` (sample stddev; 0 for a single rating).
* User side: within a user the ratings are ordered by timestamp; the window of the rating at position p is positions
  ``[max(0, p - 100), p - 1]`` (rows, not time).  ``userRatingCount`` is its size, ``userAvgRating`` / ``userRatingStddev`` its ratings' average
  and sample stddev, ``userRatedMovie1..`` its label-1 movies, most recent first, ``userGenre1..5`` the genres of its label-1 movies (a
  movie's WHOLE genre list counts) by count descending.  Rows with ``userRatingCount <= 1`` are dropped.
* ``userAvgReleaseYear`` and ``userReleaseYearStddev``, which the reference also writes, are no columns of ``schema.py`` and no model
  reads them: they are left out.

Two places where Spark leaves the result open are fixed here (deviations):

* equal timestamps within a user are ordered by input row: the sort key ``(userId, timestamp, input row)`` is total;
* equal genre counts: the genre with the lower id in the genre dictionary wins (Scala iterates a hash map).  The dictionary is
  ``schema.GENRE_VOCAB`` in its order, then every other genre string of the movie table in order of first appearance ("(no genres
  listed)" in MovieLens); at most 32 entries.  A genre outside the vocabulary competes for its place as in the reference and is
  written as -1, which is what the column packer makes of it.

Rounding is decided in integers.  Ratings are on the half-star scale, ``r2 = 2 rating`` an integer in [0, 20]; for n ratings with
``S = sum r2``, ``Q = sum r2^2``: :func:`avg_h` ``= RHE(50 S / n)`` and :func:`sd_h` ``= RHE(100 sqrt(N / (4 d)))``, ``N = n Q - S^2``,
``d = n (n - 1)``, both in hundredths, RHE = round half to even of the exact value; the stored float32 is ``float32(h / 100.0)``, which
equals ``float32("%.2f" % (h / 100))``.  Counts and ``releaseYear`` are ``float32(int)``; missing history is 0, a missing genre -1.

Parity with the reference: the movie side and the rounding are pinned by the reference's own data (tests/test_featureeng.py); the
reference does not ship ``ratings.csv``, so the user windows are pinned by this definition and hand-worked examples.

New ratings are applied to an existing store by :func:`update_host` (the definition) and :func:`update_device` (``sprk_store_update``,
csrc/k_store_update.h): the store's tables afterwards are byte for byte the tables built from all ratings applied so far, given
that a user's new ratings are not older than the user's latest.  They keep a :class:`StoreState`.

The held-out split between ``build`` and ``model.fit`` -- the reference's 10 % sample cut 80 / 20 at random or at the 0.8 quantile of
the timestamps (FeatureEngForRecModel.scala:176-205) -- is :func:`split_host` (the definition, integers only), :func:`split_device` and
:meth:`DeviceSamples.split` (``sprk_split_plan`` + ``sprk_take_rows``, csrc/k_split.h): DESIGN.md section 5.17.

Out of scope: feeding the device-resident samples straight into ``evaluate_device`` (use ``.to_host()``).
"""
from __future__ import annotations

import csv
import re
from collections import namedtuple
from typing import Mapping, Optional

import numpy as np

from . import schema as S

WINDOW = 100
POSITIVE_R2 = 7                       # label = rating >= 3.5
DEFAULT_YEAR = 1990
MAX_GENRES = 32
_ID_LIMIT = (1 << 31) - 1
_JAVA_BLANKS = "".join(chr(c) for c in range(33))          # String.trim strips every char <= U+0020
DENSE_KEYS = ["releaseYear", "movieRatingCount", "movieAvgRating", "movieRatingStddev", "userRatingCount", "userAvgRating", "userRatingStddev"]
ERR_USER, ERR_MOVIE, ERR_RATING = 1, 2, 3                   # the device error word's kinds, in the order the host checks them
ERR_OLDER = 4                                               # (updates only: a rating older than its user's latest applied one)

# year [n] int32, genre [n, 3] int32 (vocabulary index or -1), mask [n] uint32 (bit g = dictionary id g), has [n] uint8, dictionary [str];
# row = movieId; a movie the table does not hold: 1990, -1, 0, 0
MovieTable = namedtuple("MovieTable", "year genre mask has dictionary")


def avg_h(n: int, s: int) -> int:
    """Round-half-to-even of 50 S / n: the average of n half-star ratings (S = the sum of 2 * rating) in hundredths.  Exact."""
    n, s = int(n), int(s)
    if n == 0:
        return 0
    q, r = divmod(50 * s, n)
    return q + (1 if 2 * r > n or (2 * r == n and q & 1) else 0)


def sd_h(n: int, s: int, q: int) -> int:
    """Round-half-to-even of 100 sqrt(N / (4 d)), N = n Q - S^2, d = n (n - 1): the sample stddev in hundredths.  Exact for any n."""
    n, s, q = int(n), int(s), int(q)
    if n < 2:
        return 0
    N, d = n * q - s * s, n * (n - 1)
    h = 0
    for bit in (512, 256, 128, 64, 32, 16, 8, 4, 2, 1):       # floor: the greatest h with (2 h)^2 d <= 10^4 N (h <= 708)
        if 4 * (h | bit) * (h | bit) * d <= 10000 * N:
            h |= bit
    t = (2 * h + 1) * (2 * h + 1) * d
    if t < 10000 * N or (t == 10000 * N and h & 1):
        h += 1
    return h


def hundredths(h) -> np.ndarray:
    """The stored float32 of h hundredths: ``float32(h / 100.0)``, dividing in double."""
    return (np.asarray(h, dtype=np.float64) / 100.0).astype(np.float32)


def _avg_h_vec(n, s):
    a = 50 * s
    nn = np.maximum(n, 1)
    q, r = a // nn, a % nn
    return np.where(n == 0, 0, q + ((2 * r > nn) | ((2 * r == nn) & (q & 1 == 1))))


def _sd_h_vec(n, s, q):
    """:func:`sd_h` for int64 arrays with n <= 100 (a window): every product fits 64 bits."""
    N, d = n * q - s * s, np.maximum(n * (n - 1), 1)
    R = 10000 * N
    h = np.zeros_like(n)
    for bit in (512, 256, 128, 64, 32, 16, 8, 4, 2, 1):
        c = h | bit
        h = np.where(4 * c * c * d <= R, c, h)
    t = (2 * h + 1) * (2 * h + 1) * d
    h = h + ((t < R) | ((t == R) & (h & 1 == 1)))
    return np.where(n < 2, 0, h)


def release_year(title, movie_id=None) -> int:
    """``extractReleaseYearUdf`` (FeatureEngForRecModel.scala:36-44), its untrimmed indices included; where the reference's UDF throws
    (no number at that place) this raises ``ValueError`` naming the movie."""
    if title is None:
        return DEFAULT_YEAR
    t = title.strip(_JAVA_BLANKS)
    if len(t) < 6:
        return DEFAULT_YEAR
    b, e = len(title) - 5, len(title) - 1
    text = t[b:e] if e <= len(t) else None
    if text is None or not re.fullmatch(r"[+-]?[0-9]+", text):
        raise ValueError("movie %s: no release year at the end of the title %r" % (movie_id, title))
    return int(text)


def _host_column(col):
    if hasattr(col, "detach"):
        col = col.detach().cpu().numpy()
    return np.asarray(col)


def _read_csv_columns(path, names):
    with open(path, newline="", encoding="utf-8") as f:
        reader = csv.reader(f)
        header = next(reader)
        at = [header.index(k) for k in names]
        cols = [[] for _ in names]
        for row in reader:
            if len(row) != len(header):
                continue
            for c, j in zip(cols, at):
                c.append(row[j])
    return dict(zip(names, cols))


def movie_table(movies) -> MovieTable:
    """The per-movie inputs of the job from ``movies.csv`` (a path) or ``{movieId, title, genres}`` columns."""
    if isinstance(movies, MovieTable):
        return movies
    cols = _read_csv_columns(movies, ["movieId", "title", "genres"]) if isinstance(movies, str) else movies
    ids = [int(v) for v in _host_column(cols["movieId"]).tolist()]
    titles, genres = list(_host_column(cols["title"]).tolist()), list(_host_column(cols["genres"]).tolist())
    if any(i < 0 or i >= _ID_LIMIT for i in ids):
        raise ValueError("movieId %d cannot index a table" % next(i for i in ids if i < 0 or i >= _ID_LIMIT))
    if len(set(ids)) != len(ids):
        raise ValueError("the movie table names a movieId twice")
    n = max(ids) + 1 if ids else 0
    dictionary = list(S.GENRE_VOCAB)
    index = {g: i for i, g in enumerate(dictionary)}
    year = np.full(n, DEFAULT_YEAR, dtype=np.int32)
    genre = np.full((n, 3), -1, dtype=np.int32)
    mask = np.zeros(n, dtype=np.uint32)
    has = np.zeros(n, dtype=np.uint8)
    for i, title, g in zip(ids, titles, genres):
        title = None if title is None else (title.decode() if isinstance(title, bytes) else str(title))
        year[i] = release_year(title, i)
        pieces = [] if g is None else (g.decode() if isinstance(g, bytes) else str(g)).split("|")
        bits = 0
        for k, piece in enumerate(pieces):
            if piece == "":
                continue                                     # (an empty piece is a missing genre)
            if piece not in index:
                if len(dictionary) == MAX_GENRES:
                    raise ValueError("more than %d distinct genres (movie %d: %r)" % (MAX_GENRES, i, piece))
                index[piece] = len(dictionary)
                dictionary.append(piece)
            gid = index[piece]
            bits |= 1 << gid
            if k < 3 and gid < S.N_GENRES:
                genre[i, k] = gid
        mask[i] = bits
        has[i] = 1
    return MovieTable(year, genre, mask, has, dictionary)


def _padded(table: MovieTable, n_movies: int) -> MovieTable:
    n = len(table.year)
    if n_movies <= n:
        return MovieTable(table.year[:n_movies], table.genre[:n_movies], table.mask[:n_movies], table.has[:n_movies], table.dictionary)
    extra = n_movies - n
    return MovieTable(np.concatenate([table.year, np.full(extra, DEFAULT_YEAR, np.int32)]), np.concatenate([table.genre, np.full((extra, 3), -1, np.int32)]),
                      np.concatenate([table.mask, np.zeros(extra, np.uint32)]), np.concatenate([table.has, np.zeros(extra, np.uint8)]), table.dictionary)


RATING_KEYS = ["userId", "movieId", "rating", "timestamp"]


def _rating_columns(ratings):
    """-> userId, movieId (int64), rating (float32: the sample column's type), timestamp (int64) as numpy arrays."""
    cols = _read_csv_columns(ratings, RATING_KEYS) if isinstance(ratings, str) else ratings
    for k in RATING_KEYS:
        if k not in cols:
            raise KeyError("missing ratings column %r" % k)
    def ints(col):
        a = _host_column(col)
        return a.astype(np.int64) if a.dtype.kind in "iub" else np.array([int(v) for v in a.tolist()], dtype=np.int64)
    def floats(col):
        a = _host_column(col)
        return a.astype(np.float32) if a.dtype.kind in "iubf" else np.array([float(v) for v in a.tolist()], dtype=np.float64).astype(np.float32)
    u, m, r, t = ints(cols["userId"]), ints(cols["movieId"]), floats(cols["rating"]), ints(cols["timestamp"])
    if not (len(u) == len(m) == len(r) == len(t)):
        raise ValueError("the ratings columns differ in length")
    if len(u) >= _ID_LIMIT:
        raise ValueError("at most 2^31 - 2 ratings")
    return u, m, r, t


def _error_message(kind: int, row: int) -> str:
    what = {ERR_USER: "userId outside the user table", ERR_MOVIE: "movieId outside the movie table",
            ERR_RATING: "rating off the half-star scale 0, 0.5 .. 10", ERR_OLDER: "older than its user's latest rating"}[kind]
    return "ratings row %d: %s" % (row, what)


def _half_stars(r: np.ndarray) -> np.ndarray:
    """2 * rating as int64, -1 where the float32 rating is off the half-star scale."""
    t = r.astype(np.float32) * np.float32(2.0)
    ok = (t >= 0) & (t <= 20) & (np.floor(t) == t)             # (NaN fails every comparison)
    return np.where(ok, np.where(ok, t, 0).astype(np.int64), -1)


def _validate(u, m, r2, n_users, n_movies, older=None):
    """Raises the ValueError the device's error word names: the lowest kind, then the first input row.  ``older``: an update's rows
    that precede their user's latest rating."""
    checks = [(ERR_USER, (u < 0) | (u >= n_users)), (ERR_MOVIE, (m < 0) | (m >= n_movies)), (ERR_RATING, r2 < 0)]
    for kind, bad in checks if older is None else checks + [(ERR_OLDER, older)]:
        if bad.any():
            raise ValueError(_error_message(kind, int(np.flatnonzero(bad)[0])))


def _greatest_id(col) -> int:
    """The greatest id of a column (a numpy array or a tensor) that can index a table, -1 for none."""
    ok = (col >= 0) & (col < _ID_LIMIT)
    return int(col[ok].max()) if bool(ok.any()) else -1


def _table_sizes(u, m, table: MovieTable, n_users, n_movies):
    """Default table sizes: the greatest id + 1 (the movie table's rows at least); a given size that does not hold the movie table is an error."""
    if n_users is None:
        n_users = int(u.max()) + 1 if len(u) and int(u.max()) >= 0 else 0
    if n_movies is None:
        n_movies = max(len(table.year), int(m.max()) + 1 if len(m) and int(m.max()) >= 0 else 0)
    if not 0 <= n_users < _ID_LIMIT or not 0 <= n_movies <= _ID_LIMIT:
        raise ValueError("n_users / n_movies outside [0, 2^31 - 1)")
    if n_movies < len(table.year) and table.has[n_movies:].any():
        raise ValueError("movieId %d of the movie table does not fit a table of %d rows" % (int(np.flatnonzero(table.has)[-1]), n_movies))
    return int(n_users), int(n_movies)


def sample_keys(hist_len: int = 5):
    """The columns of a samples dict, in order."""
    return (["userId", "movieId", "rating", "timestamp", "label"] + S.MOVIE_GENRE_KEYS + S.USER_GENRE_KEYS
            + ["userRatedMovie%d" % (k + 1) for k in range(hist_len)] + DENSE_KEYS + ["source_row"])


def _columns_dict(hist_len, user, movie, rating, ts, label, src, genres, hist, dense):
    out = {"userId": user, "movieId": movie, "rating": rating, "timestamp": ts, "label": label}
    for k, key in enumerate(S.MOVIE_GENRE_KEYS + S.USER_GENRE_KEYS):
        out[key] = genres[:, k]
    for k in range(hist_len):
        out["userRatedMovie%d" % (k + 1)] = hist[:, k]
    for k, key in enumerate(DENSE_KEYS):
        out[key] = dense[:, k]
    out["source_row"] = src
    return out


def samples_host(ratings, movies, hist_len: int = 5, n_users: Optional[int] = None, n_movies: Optional[int] = None) -> dict:
    """The definition (module docstring): ``ratings`` = ``{userId, movieId, rating, timestamp}`` columns or a CSV path, ``movies`` a
    :class:`MovieTable` (or what :func:`movie_table` takes) -> a dict of columns in ``(userId, timestamp, input row)`` order, the dropped
    rows removed: ``userId, movieId, rating, timestamp, label``, ``movieGenre1..3`` and ``userGenre1..5`` as vocabulary indices (-1 = none),
    ``userRatedMovie1..hist_len`` (0 = none), the seven numeric columns as float32 and ``source_row``, the input row.  ``model.predict``,
    ``model.evaluate`` and ``FeatureStore.from_samples`` accept it as it is.  A rating off the half-star scale, or an id outside
    ``[0, n_users)`` / ``[0, n_movies)`` (default: any non-negative id), raises ``ValueError`` naming the first such input row."""
    if not 1 <= hist_len <= WINDOW:
        raise ValueError("hist_len = %d outside [1, %d]" % (hist_len, WINDOW))
    table = movie_table(movies)
    u, m, r, t = _rating_columns(ratings)
    r2 = _half_stars(r)
    _validate(u, m, r2, _ID_LIMIT if n_users is None else n_users, _ID_LIMIT if n_movies is None else n_movies)
    n_users, n_movies = _table_sizes(u, m, table, n_users, n_movies)
    table = _padded(table, n_movies)
    n = len(u)
    # movie side, over ALL ratings (bincount sums in float64: exact, S <= 20 n and Q <= 400 n stay below 2^53)
    cnt = np.bincount(m, minlength=n_movies).astype(np.int64)
    sm = np.bincount(m, weights=r2, minlength=n_movies).astype(np.int64)
    qm = np.bincount(m, weights=r2 * r2, minlength=n_movies).astype(np.int64)
    m_avg, m_sd = np.zeros(n_movies, dtype=np.int64), np.zeros(n_movies, dtype=np.int64)
    for i in np.flatnonzero(cnt):
        m_avg[i], m_sd[i] = avg_h(cnt[i], sm[i]), sd_h(cnt[i], sm[i], qm[i])
    # user side: one sort, then every window as a difference of prefix sums over the sorted order
    order = np.lexsort((np.arange(n), t, u))
    us, ms, r2s = u[order], m[order], r2[order]
    pos = np.arange(n, dtype=np.int64)
    new = np.ones(n, dtype=bool)
    new[1:] = us[1:] != us[:-1]
    start = np.maximum.accumulate(np.where(new, pos, 0))
    first = np.maximum(start, pos - WINDOW)                                  # the window is [first, pos)
    count = pos - first
    def window_sum(v):
        c = np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
        return c[pos] - c[first]
    s_w, q_w = window_sum(r2s), window_sum(r2s * r2s)
    positive = r2s >= POSITIVE_R2
    bits = ((table.mask[ms].astype(np.int64)[:, None] >> np.arange(MAX_GENRES)) & 1) * positive[:, None]
    prefix = np.concatenate([np.zeros((1, MAX_GENRES), np.int64), np.cumsum(bits, axis=0, dtype=np.int64)])
    counts = prefix[pos] - prefix[first]                                     # [n, 32]
    key = np.where(counts > 0, counts * MAX_GENRES + (MAX_GENRES - 1 - np.arange(MAX_GENRES)), 0)   # count desc, dictionary id asc
    top = -np.sort(-key, axis=1)[:, :5]
    gid = MAX_GENRES - 1 - top % MAX_GENRES
    user_genres = np.where((top > 0) & (gid < S.N_GENRES), gid, -1)
    where_pos = np.flatnonzero(positive)
    hi, lo = np.searchsorted(where_pos, pos), np.searchsorted(where_pos, first)    # the window's positives: where_pos[lo:hi]
    hist = np.zeros((n, hist_len), dtype=np.int64)
    for k in range(hist_len):
        at = hi - 1 - k
        ok = at >= lo
        if where_pos.size:
            hist[:, k] = np.where(ok, ms[where_pos[np.clip(at, 0, where_pos.size - 1)]], 0)
    keep = count > 1
    sel = order[keep]
    genres = np.concatenate([table.genre[ms[keep]], user_genres[keep]], axis=1).astype(np.int32)
    mk = ms[keep]
    dense = np.stack([table.year[mk].astype(np.float32), cnt[mk].astype(np.float32), hundredths(m_avg[mk]), hundredths(m_sd[mk]),
                      count[keep].astype(np.float32), hundredths(_avg_h_vec(count[keep], s_w[keep])),
                      hundredths(_sd_h_vec(count[keep], s_w[keep], q_w[keep]))], axis=1) if n else np.zeros((0, 7), np.float32)
    return _columns_dict(hist_len, u[sel].astype(np.int32), m[sel].astype(np.int32), r[sel], t[sel], positive[keep].astype(np.int32), sel.astype(np.int32),
                         genres, hist[keep].astype(np.int32), dense.astype(np.float32))


class DeviceSamples:
    """What :func:`build` returns: the sample columns as device tensors (``columns``: the dict of :func:`samples_host`, every tensor cut to
    ``n_samples`` rows) and the feature store's tables, which were written by the same call and never left the device."""

    def __init__(self, columns, n_samples, hist_len, store_tensors, device, n_sampled=None, split_timestamp=None):
        self.columns, self.n_samples, self.hist_len, self.device = columns, int(n_samples), int(hist_len), device
        self._store_tensors = store_tensors
        self.n_sampled, self.split_timestamp = n_sampled, split_timestamp      # (set on the two parts of a split)

    def split(self, mode: str = "random", sample: float = 0.1, train: float = 0.8, seed: int = 0, key="source_row"):
        """-> ``(train, test)``: :func:`split_device` over ``columns``, as two :class:`DeviceSamples` whose columns are exactly ``n_train`` /
        ``n_test`` rows long and which carry ``n_sampled`` and ``split_timestamp``.  Both share this build's store tables: the reference's
        store is built from all samples.  ``model.fit(train.columns)`` and ``model.evaluate_device(test.columns)`` take them as they are."""
        res = split_device(self.columns, mode=mode, sample=sample, train=train, seed=seed, key=key, device=self.device)
        part = lambda cols: DeviceSamples(cols, len(next(iter(cols.values()))) if cols else 0, self.hist_len, self._store_tensors, self.device,
                                          res.n_sampled, res.split_timestamp)
        return part(res.train), part(res.test)

    def to_host(self) -> dict:
        """The dict :func:`samples_host` returns, bit for bit."""
        return {k: v.cpu().numpy() for k, v in self.columns.items()}

    def store(self):
        """A :class:`~sparrowrecsys_amd.featurestore.FeatureStore` over the tables this build wrote on the device."""
        from .featurestore import FeatureStore
        return FeatureStore._from_device_tables(self._store_tensors, self.hist_len, self.device)


def _device_rating_columns(ratings, dev):
    """-> userId, movieId (int32), rating (float32), timestamp (int64) as contiguous tensors on ``dev``, their length, and the greatest
    userId and movieId where the columns came from the host (-1 for none; None for device tensors, which are used where they are)."""
    import torch
    if isinstance(ratings, Mapping) and all(hasattr(ratings.get(k), "detach") for k in RATING_KEYS):
        cols = [ratings[k].detach().to(dev) for k in RATING_KEYS]
        if not all(c.ndim == 1 and c.numel() == cols[0].numel() for c in cols):
            raise ValueError("the ratings columns differ in length")
        if any(c.dtype.is_floating_point for c in (cols[0], cols[1], cols[3])):
            raise TypeError("userId, movieId and timestamp must be integer tensors")
        # (an id beyond int32 must not wrap into range: it becomes -1, which the kernel reports)
        ids = [torch.where((c < 0) | (c >= _ID_LIMIT), torch.full_like(c, -1), c).to(torch.int32).contiguous() for c in cols[:2]]
        u_d, m_d, r_d, t_d = ids[0], ids[1], cols[2].to(torch.float32).contiguous(), cols[3].to(torch.int64).contiguous()
        n, greatest = u_d.numel(), None
    else:
        u, m, r, t = _rating_columns(ratings)
        n = len(u)
        clip = lambda a: np.where((a < 0) | (a >= _ID_LIMIT), -1, a).astype(np.int32)
        u, m = clip(u), clip(m)
        greatest = (int(u.max()), int(m.max())) if n else (-1, -1)
        u_d, m_d = torch.from_numpy(u).to(dev), torch.from_numpy(m).to(dev)
        r_d, t_d = torch.from_numpy(np.ascontiguousarray(r)).to(dev), torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    if n >= _ID_LIMIT:
        raise ValueError("at most 2^31 - 2 ratings")
    return u_d, m_d, r_d, t_d, n, greatest


def build(ratings, movies, hist_len: int = 5, device=None, n_users: Optional[int] = None, n_movies: Optional[int] = None) -> DeviceSamples:
    """Samples and store on the device.  ``ratings``: a CSV path or ``{userId, movieId, rating, timestamp}`` columns, numpy arrays or
    device tensors (tensors on ``device`` are used where they are); ``movies``: what :func:`movie_table` takes.  ``n_users`` /
    ``n_movies`` size the store's tables (default: the greatest id + 1, which costs one reduction over the id columns).  Errors are the
    ``ValueError`` of :func:`samples_host`.  One host synchronisation: the error word and the sample count."""
    import ctypes as C

    import torch

    from . import _lib as L
    from .featurestore import user_pitch
    if not 1 <= hist_len <= WINDOW:
        raise ValueError("hist_len = %d outside [1, %d]" % (hist_len, WINDOW))
    lib = L.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError("featureeng.build needs a HIP device: no HIP device is visible (samples_host is the host definition)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    table = movie_table(movies)
    u_d, m_d, r_d, t_d, n, greatest = _device_rating_columns(ratings, dev)
    if greatest is None:
        greatest = (int(u_d.max()), int(m_d.max())) if n and (n_users is None or n_movies is None) else (-1, -1)
    um, mm = greatest
    n_users, n_movies = _table_sizes(np.array([um]), np.array([mm]), table, n_users, n_movies)
    table = _padded(table, n_movies)
    pitch = user_pitch(hist_len)
    with torch.cuda.device(dev):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        year_d, genre_d, mask_d = up(table.year), up(table.genre), up(table.mask.view(np.int32))
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        rows = max(n, 1)
        o_user, o_movie, o_rating, o_ts = new(rows, torch.int32), new(rows, torch.int32), new(rows, torch.float32), new(rows, torch.int64)
        o_label, o_src = new(rows, torch.int32), new(rows, torch.int32)
        o_genres, o_hist, o_dense = new((rows, 8), torch.int32), new((rows, hist_len), torch.int32), new((rows, 7), torch.float32)
        # (one spare row each, zero: an empty table still has an address -- FeatureStore's convention)
        user_rows, user_has = torch.zeros((n_users + 1, pitch), dtype=torch.int32, device=dev), torch.zeros(n_users + 1, dtype=torch.uint8, device=dev)
        movie_rows, movie_has = torch.zeros((n_movies + 1, 8), dtype=torch.int32, device=dev), torch.zeros(n_movies + 1, dtype=torch.uint8, device=dev)
        words = torch.tensor([-1, 0], dtype=torch.int64, device=dev)            # the error word (~0), the sample count
        ws_bytes = lib.sprk_feature_eng_workspace_bytes(n, n_users, n_movies)
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)   # (torch's allocations are 512-byte aligned)
        p = lambda x: C.c_void_p(x.data_ptr())
        L.check(lib.sprk_feature_eng(p(u_d), p(m_d), p(r_d), p(t_d), n, n_users, n_movies, p(year_d), p(genre_d), p(mask_d), S.N_GENRES, hist_len,
                                     p(o_user), p(o_movie), p(o_rating), p(o_ts), p(o_label), p(o_src), p(o_genres), p(o_hist), p(o_dense),
                                     p(user_rows), p(user_has), pitch, p(movie_rows), p(movie_has),
                                     C.c_void_p(words.data_ptr()), C.c_void_p(words.data_ptr() + 8), p(ws), ws.numel() * 8,
                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        err, kept = (int(v) for v in words.cpu().numpy())                        # the one synchronisation
    if err != -1:
        raise ValueError(_error_message((err >> 32) & 0xffffffff, err & 0xffffffff))
    cut = lambda x: x[:kept]
    columns = _columns_dict(hist_len, cut(o_user), cut(o_movie), cut(o_rating), cut(o_ts), cut(o_label), cut(o_src), cut(o_genres), cut(o_hist), cut(o_dense))
    return DeviceSamples(columns, kept, hist_len, (user_rows, user_has, movie_rows, movie_has), dev)


# ---- new ratings applied to an existing store ----
TS_MIN = int(np.iinfo(np.int64).min)
# name, dtype, per-row shape; the first four have one row per user, the others one per movie
STATE_ARRAYS = [("user_count", np.uint32, ()), ("user_last_ts", np.int64, ()), ("ring_movie", np.int32, (WINDOW,)), ("ring_r2", np.uint8, (WINDOW,)),
                ("movie_count", np.uint32, ()), ("movie_sum", np.uint64, ()), ("movie_sumsq", np.uint64, ()), ("movie_flag", np.uint8, ())]
TABLE_NAMES = ["user_rows", "user_has", "movie_rows", "movie_has"]


class StoreState:
    """What an updatable store keeps next to its four tables so that new ratings can be applied without the old ones.

    Per user: ``user_count`` (ratings applied), ``user_last_ts`` (the latest timestamp applied, ``TS_MIN`` for none), ``ring_movie`` /
    ``ring_r2`` ``[n_users, 100]``: the user's last 100 ratings as movie id and 2 * rating, the rating at position p of the user's
    ``(timestamp, input row)`` order in slot ``p % 100``.  Per movie: ``movie_count`` / ``movie_sum`` / ``movie_sumsq`` (n, S, Q over all
    ratings) and ``movie_flag`` (a rating of the movie sits at a user position >= 2: a kept sample names it).  ``table``: the movie table
    padded to ``n_movies``.  ``tables``: the store's ``user_rows, user_has, movie_rows, movie_has``, changed in place.  ``n_ratings``: all
    ratings applied.  On the host (``device`` None) everything is a numpy array of exactly ``n_users`` / ``n_movies`` rows; on a device
    everything is a tensor with one spare row (an empty array still has an address), and ``movie_dev`` holds the movie table's columns."""

    def __init__(self, table, n_users, n_movies, hist_len, arrays, tables, device=None, movie_dev=None):
        self.table, self.n_users, self.n_movies, self.hist_len = table, int(n_users), int(n_movies), int(hist_len)
        self.arrays, self.tables, self.device, self.movie_dev = dict(arrays), tuple(tables), device, movie_dev
        self.n_ratings = 0

    def __getattr__(self, name):                                               # state.user_count is state.arrays["user_count"]
        arrays = self.__dict__.get("arrays", {})
        if name in arrays:
            return arrays[name]
        raise AttributeError(name)

    def to_host(self) -> dict:
        """The state arrays and the tables as numpy arrays of ``n_users`` / ``n_movies`` rows (copies), by name."""
        rows = [self.n_users] * 4 + [self.n_movies] * 4 + [self.n_users] * 2 + [self.n_movies] * 2
        named = [(k, self.arrays[k], dt) for k, dt, _ in STATE_ARRAYS] + [(k, v, None) for k, v in zip(TABLE_NAMES, self.tables)]
        out = {}
        for (k, v, dt), n in zip(named, rows):
            a = v.cpu().numpy() if hasattr(v, "detach") else v
            out[k] = (a if dt is None else a.view(dt))[:n].copy()              # (a device array stores an unsigned word as the signed type of its width)
        return out

    def state_bytes(self) -> int:
        """Bytes of the state arrays, the tables not counted."""
        return sum((self.n_users if k < 4 else self.n_movies) * int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
                   for k, (_, dt, shape) in enumerate(STATE_ARRAYS))


def empty_state(movies, n_users: int, n_movies: int, hist_len: int = 5, device=None) -> StoreState:
    """The state and the tables of no ratings: what ``sprk_feature_eng`` writes for an empty ``ratings.csv``.  ``device`` None or
    ``"cpu"``: on the host."""
    from .featurestore import MOVIE_PITCH, user_pitch
    if not 1 <= hist_len <= WINDOW:
        raise ValueError("hist_len = %d outside [1, %d]" % (hist_len, WINDOW))
    table = movie_table(movies)
    n_users, n_movies = _table_sizes(np.array([-1]), np.array([-1]), table, int(n_users), int(n_movies))
    table = _padded(table, n_movies)
    pitch = user_pitch(hist_len)
    if device is None or str(device) == "cpu":
        arrays = {k: np.zeros((n_users if i < 4 else n_movies,) + shape, dtype=dt) for i, (k, dt, shape) in enumerate(STATE_ARRAYS)}
        arrays["user_last_ts"][:] = TS_MIN
        user_rows, movie_rows = np.zeros((n_users, pitch), np.int32), np.zeros((n_movies, MOVIE_PITCH), np.int32)
        user_rows[:, hist_len:hist_len + 5] = -1
        movie_rows[:, :3] = -1
        return StoreState(table, n_users, n_movies, hist_len, arrays, (user_rows, np.zeros(n_users, np.uint8), movie_rows, np.zeros(n_movies, np.uint8)))
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("an updatable store on a device needs a HIP device: none is visible (device=\"cpu\" runs the host definition)")
    dev = torch.device(device)
    storage = {np.uint32: torch.int32, np.uint64: torch.int64, np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}   # (the same bits)
    arrays = {k: torch.zeros((n_users + 1 if i < 4 else n_movies + 1,) + shape, dtype=storage[dt], device=dev) for i, (k, dt, shape) in enumerate(STATE_ARRAYS)}
    arrays["user_last_ts"][:n_users] = TS_MIN
    user_rows, movie_rows = torch.zeros((n_users + 1, pitch), dtype=torch.int32, device=dev), torch.zeros((n_movies + 1, MOVIE_PITCH), dtype=torch.int32, device=dev)
    user_rows[:n_users, hist_len:hist_len + 5] = -1
    movie_rows[:n_movies, :3] = -1
    tables = (user_rows, torch.zeros(n_users + 1, dtype=torch.uint8, device=dev), movie_rows, torch.zeros(n_movies + 1, dtype=torch.uint8, device=dev))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return StoreState(table, n_users, n_movies, hist_len, arrays, tables, dev, (up(table.year), up(table.genre), up(table.mask.view(np.int32))))


def _user_row(movies, r2s, table: MovieTable, hist_len: int, pitch: int) -> np.ndarray:
    """The store's user row of one window, ``movies`` / ``r2s`` in position order (oldest first): history | userGenre1..5 | count avg
    stddev | zeros -- the columns of the sample whose window this is."""
    n, s, q = len(r2s), int(r2s.sum()), int((r2s * r2s).sum())
    liked = movies[r2s >= POSITIVE_R2][::-1]                                   # most recent first
    counts = [0] * MAX_GENRES
    for bits in table.mask[liked].tolist():
        for g in range(MAX_GENRES):
            counts[g] += (bits >> g) & 1
    top = sorted((g for g in range(MAX_GENRES) if counts[g]), key=lambda g: (-counts[g], g))[:5]    # count desc, dictionary id asc
    row = np.zeros(pitch, dtype=np.int32)
    row[:min(hist_len, len(liked))] = liked[:hist_len]
    row[hist_len:hist_len + 5] = [g if g < S.N_GENRES else -1 for g in top] + [-1] * (5 - len(top))
    row[hist_len + 5:hist_len + 8] = np.array([np.float32(n), hundredths(avg_h(n, s)), hundredths(sd_h(n, s, q))], dtype=np.float32).view(np.int32)
    return row


def update_host(state: StoreState, ratings) -> int:
    """The definition of an update: ``ratings`` (what :func:`build` takes) applied to ``state`` and its tables in place, in numpy and
    integers; returns their number.  Afterwards the tables are the tables of ``samples_host`` over ALL ratings applied, in call order,
    provided no new rating is older than the latest rating of its user applied by an earlier call -- then the new ratings sort after
    the old ones of their user (a timestamp tie goes by input row), so no old position moves: the user row is the window before the new
    last position, read from the ring and the sorted new ratings; a movie row is a function of the movie's n / S / Q and of its flag.
    Errors are ``ValueError`` as for :func:`samples_host`, and "older than its user's latest rating"; an error leaves every byte as it was."""
    from .featurestore import user_pitch
    if state.device is not None:
        raise TypeError("update_host takes a host state (update_device applies ratings to a state on a device)")
    u, m, r, t = _rating_columns(ratings)
    n = len(u)
    if state.n_ratings + n >= _ID_LIMIT:
        raise ValueError("at most 2^31 - 2 ratings")
    r2 = _half_stars(r)
    known = (u >= 0) & (u < state.n_users)
    older = np.zeros(n, dtype=bool)
    older[known] = t[known] < state.user_last_ts[u[known]]
    _validate(u, m, r2, state.n_users, state.n_movies, older)
    if n == 0:
        return 0
    table, H, pitch = state.table, state.hist_len, user_pitch(state.hist_len)
    user_rows, user_has, movie_rows, movie_has = state.tables
    state.arrays["movie_count"] += np.bincount(m, minlength=state.n_movies).astype(np.uint32)
    state.arrays["movie_sum"] += np.bincount(m, weights=r2, minlength=state.n_movies).astype(np.uint64)            # (exact in float64: below 2^53)
    state.arrays["movie_sumsq"] += np.bincount(m, weights=r2 * r2, minlength=state.n_movies).astype(np.uint64)
    order = np.lexsort((np.arange(n), t, u))
    us = u[order]
    starts = np.flatnonzero(np.concatenate([[True], us[1:] != us[:-1]]))
    for lo, hi in zip(starts, np.concatenate([starts[1:], [n]])):
        rows, user = order[lo:hi], int(us[lo])                                 # the user's new ratings by (timestamp, row in the batch)
        k, old = int(hi - lo), int(state.user_count[user])
        mv, rr = m[rows], r2[rows]
        state.movie_flag[mv[max(0, 2 - old):]] = 1                             # new position j is the user's position old + j
        last = old + k - 1
        if last >= 2:                                                          # the last kept sample: the window before the last position
            pos = np.arange(max(0, last - WINDOW), last)
            new = np.clip(pos - old, 0, k - 1)
            w_movie = np.where(pos < old, state.ring_movie[user, pos % WINDOW], mv[new])
            w_r2 = np.where(pos < old, state.ring_r2[user, pos % WINDOW], rr[new]).astype(np.int64)
            user_rows[user] = _user_row(w_movie, w_r2, table, H, pitch)
            user_has[user] = 1
        tail = np.arange(max(0, k - WINDOW), k)
        state.ring_movie[user, (old + tail) % WINDOW] = mv[tail]
        state.ring_r2[user, (old + tail) % WINDOW] = rr[tail]
        state.user_count[user] = old + k
        state.user_last_ts[user] = t[rows[-1]]
    for movie in np.unique(m).tolist():
        cnt, sm, sq = int(state.movie_count[movie]), int(state.movie_sum[movie]), int(state.movie_sumsq[movie])
        if state.movie_flag[movie]:
            movie_rows[movie, :3] = table.genre[movie]
            movie_rows[movie, 3:7] = np.array([np.float32(table.year[movie]), np.float32(cnt), hundredths(avg_h(cnt, sm)), hundredths(sd_h(cnt, sm, sq))],
                                              dtype=np.float32).view(np.int32)
            movie_has[movie] = 1
    state.n_ratings += n
    return n


def update_device(state: StoreState, ratings) -> int:
    """:func:`update_host` on the device (``sprk_store_update``): the same bytes in the state and in the tables.  ``ratings`` as for
    :func:`build`; tensors on the state's device are used where they are.  Everything is enqueued on the current stream; one host
    synchronisation, for the error word."""
    import ctypes as C

    import torch

    from . import _lib as L
    if state.device is None:
        raise TypeError("update_device takes a state on a device (update_host is the host definition)")
    lib, dev = L.load_library(), state.device
    u_d, m_d, r_d, t_d, n, _ = _device_rating_columns(ratings, dev)
    if state.n_ratings + n >= _ID_LIMIT:
        raise ValueError("at most 2^31 - 2 ratings")
    if n == 0:
        return 0
    with torch.cuda.device(dev):
        word = torch.tensor([-1], dtype=torch.int64, device=dev)               # the error word (~0)
        ws_bytes = lib.sprk_store_update_workspace_bytes(n, state.n_users, state.n_movies)
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)   # (torch's allocations are 512-byte aligned)
        p = lambda x: C.c_void_p(x.data_ptr())
        user_rows, user_has, movie_rows, movie_has = state.tables
        L.check(lib.sprk_store_update(p(u_d), p(m_d), p(r_d), p(t_d), n, state.n_users, state.n_movies, *(p(x) for x in state.movie_dev), S.N_GENRES, state.hist_len,
                                      *(p(state.arrays[k]) for k, _, _ in STATE_ARRAYS),
                                      p(user_rows), p(user_has), int(user_rows.shape[1]), p(movie_rows), p(movie_has),
                                      p(word), p(ws), ws.numel() * 8, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        err = int(word.cpu().numpy()[0])                                       # the one synchronisation
    if err != -1:
        raise ValueError(_error_message((err >> 32) & 0xffffffff, err & 0xffffffff))
    state.n_ratings += n
    return n


# ---- the held-out split: a sample, cut at random or at a time quantile ----
SplitResult = namedtuple("SplitResult", "train test n_sampled split_timestamp")
SPLIT_MODES = {"random": 0, "time": 1}
STREAM_SAMPLE, STREAM_SPLIT = 0, 1
_MASK64 = (1 << 64) - 1


def split_threshold(f: float) -> int:
    """``T(f)``: ``floor(f * 2^53)`` for ``f < 1`` and ``2^53`` for ``f = 1`` -- one exact float64 scaling.  A draw ``u`` succeeds where ``u < T(f)``."""
    import math
    f = float(f)
    if not 0.0 <= f <= 1.0:                                                  # (NaN fails both comparisons)
        raise ValueError("a fraction of %r is outside [0, 1]" % f)
    return int(math.floor(math.ldexp(f, 53)))


def split_draws(seed: int, keys, stream: int) -> np.ndarray:
    """The 53-bit draws of the rows with the non-negative integer ``keys`` on ``stream`` (0 = sample, 1 = split) as uint64: splitmix64's
    finalizer over ``seed + 0x9E3779B97F4A7C15 (2 k + s + 1)``, all modulo 2^64.  A function of (seed, key, stream) alone."""
    k = np.asarray(keys).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(int(seed) & _MASK64) + np.uint64(0x9E3779B97F4A7C15) * (k * np.uint64(2) + np.uint64(int(stream) + 1))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x >> np.uint64(11)


def _split_arguments(mode, sample, train):
    """-> T(sample), T(train); the ``ValueError`` of a bad fraction or mode."""
    if mode not in SPLIT_MODES:
        raise ValueError("mode = %r (\"random\" or \"time\")" % (mode,))
    return split_threshold(sample), split_threshold(train)


def _split_rows(columns, mode, key, dtype_of):
    """The row count of a dict of equal-length columns; the ``ValueError`` of unequal lengths, too many rows, a missing key column or,
    in time mode, a missing or non-int64 ``timestamp``.  ``dtype_of``: a column's dtype by name ("int64", ...)."""
    lengths = {int(v.shape[0]) if getattr(v, "ndim", 1) else -1 for v in columns.values()}
    if len(lengths) > 1 or -1 in lengths:
        raise ValueError("the columns differ in length")
    n = lengths.pop() if lengths else 0
    if n >= _ID_LIMIT:
        raise ValueError("at most 2^31 - 2 rows")
    if mode == "time" and ("timestamp" not in columns or dtype_of(columns["timestamp"]) != "int64"):
        raise ValueError("mode \"time\" needs an int64 timestamp column")
    if key is not None:
        if key not in columns:
            raise ValueError("no key column %r" % (key,))
        if dtype_of(columns[key]) not in ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"):
            raise ValueError("the key column %r must hold integers" % (key,))
    return n


def split_host(samples, mode: str = "random", sample: float = 0.1, train: float = 0.8, seed: int = 0, key="source_row") -> SplitResult:
    """The definition of the held-out split (FeatureEngForRecModel.scala:176-205: a 10 % sample, cut 80 / 20), in numpy and integers.

    ``samples``: a dict of equal-length columns (what :func:`samples_host` returns) -> ``SplitResult(train, test, n_sampled,
    split_timestamp)``; ``train`` / ``test`` are dicts of the same keys and dtypes, their rows in input order.  ``sample`` and ``train``
    default to the reference's 0.1 and 0.8.

    The generator is the project's own, not Spark's ``XORShiftRandom``: a row's draws are :func:`split_draws` of ``seed``, the row's
    value in the ``key`` column (``key=None``: the row's position) and a stream number, and of nothing else -- not of the row's position
    nor of which other rows exist, so a rating keeps its side when ratings are appended and the samples rebuilt.  A row is sampled where
    its stream-0 draw is below ``T(sample)`` (:func:`split_threshold`); ``n_sampled`` counts these rows.

    ``mode="random"``: a sampled row is training where its stream-1 draw is below ``T(train)``, otherwise test; ``split_timestamp`` is None.

    ``mode="time"`` (needs an int64 ``timestamp`` column): with ``r = ceil(float64(train) * float64(n_sampled))`` -- one product, one ceil
    -- ``split_timestamp`` is the sampled rows' timestamp at ascending position ``max(r, 1) - 1``; sampled rows with ``timestamp <=
    split_timestamp`` are training (ties too, the reference's ``<=``), the others test; no sampled row gives two empty parts and None.
    Deviation: this is the EXACT quantile where the reference takes ``approxQuantile(..., 0.05)``, which may return any value whose rank
    lies within 0.05 n of 0.8 n; the exact quantile is one of those values.

    ``ValueError``, before anything is computed: ``sample`` or ``train`` outside [0, 1] or not finite, an unknown mode, ``"time"`` without
    an int64 timestamp, a missing or negative key, columns of unequal length, 2^31 - 1 rows or more."""
    t_sample, t_train = _split_arguments(mode, sample, train)
    cols = {k: _host_column(v) for k, v in samples.items()}
    n = _split_rows(cols, mode, key, lambda a: a.dtype.name)
    keys = np.arange(n, dtype=np.int64) if key is None else cols[key]
    if key is not None and keys.dtype.kind == "i" and n and int(keys.min()) < 0:
        raise ValueError("row %d: negative key" % int(np.flatnonzero(keys < 0)[0]))
    sampled = split_draws(seed, keys, STREAM_SAMPLE) < np.uint64(t_sample)
    n_sampled = int(sampled.sum())
    split_timestamp = None
    if mode == "random":
        to_train = sampled & (split_draws(seed, keys, STREAM_SPLIT) < np.uint64(t_train))
    elif n_sampled == 0:
        to_train = sampled
    else:
        ts = cols["timestamp"]
        r = int(np.ceil(np.float64(train) * np.float64(n_sampled)))
        split_timestamp = int(np.sort(ts[sampled])[max(r, 1) - 1])
        to_train = sampled & (ts <= split_timestamp)
    to_test = sampled & ~to_train
    return SplitResult({k: v[to_train] for k, v in cols.items()}, {k: v[to_test] for k, v in cols.items()}, n_sampled, split_timestamp)


def _matrix_groups(cols) -> list:
    """The columns' names in groups: a run of columns that are the adjacent columns of ONE row-major matrix (``DeviceSamples.columns``'
    genre, history and numeric columns) is one group, taken as one row-wide column; every other column is a group of its own."""
    groups, last = [], None
    for k, v in cols.items():
        where = (v.untyped_storage().data_ptr(), v.dtype, v.stride(0))
        if last is not None and where == last[0] and v.stride(0) > len(groups[-1]) and v.storage_offset() == last[1] + 1:
            groups[-1].append(k)
        else:
            groups.append([k])
        last = (where, v.storage_offset())
    return groups


def split_device(columns, mode: str = "random", sample: float = 0.1, train: float = 0.8, seed: int = 0, key="source_row", device=None,
                 group_matrices: bool = True) -> SplitResult:
    """:func:`split_host` on the device, byte for byte: ``columns`` is a dict of equal-length one-dimensional columns of 4- or 8-byte
    elements -- device tensors (``DeviceSamples.columns``; strided views are read where they are) or numpy arrays, which are uploaded --
    and ``train`` / ``test`` are dicts of dense device tensors exactly ``n_train`` / ``n_test`` rows long.  ``sprk_split_plan`` writes the
    two index lists and five words; one host synchronisation reads the words; then one ``sprk_take_rows`` per part.  Columns that are
    adjacent columns of one matrix are taken as one row-wide column, and come back as the columns of a dense matrix of their own
    (``group_matrices=False`` takes every column singly, into a dense vector: the same values; docs/split_results.md has both).  Errors are
    :func:`split_host`'s; a negative key in a device column is found by the plan and raised after the synchronisation."""
    import ctypes as C

    import torch

    from . import _lib as L
    t_sample, t_train = _split_arguments(mode, sample, train)
    lib = L.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError("featureeng.split_device needs a HIP device: no HIP device is visible (split_host is the host definition)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    cols = {k: (v.detach().to(dev) if hasattr(v, "detach") else torch.from_numpy(np.ascontiguousarray(_host_column(v))).to(dev)) for k, v in columns.items()}
    n = _split_rows(cols, mode, key, lambda t: str(t.dtype).replace("torch.", ""))
    for k, v in cols.items():
        if v.ndim != 1 or v.element_size() % 4:
            raise ValueError("column %r: split_device takes one-dimensional columns of 4- or 8-byte elements" % (k,))
    key_kind, key_col = 0, None
    if key is not None:
        key_col = cols[key] if cols[key].dtype in (torch.int32, torch.int64) else cols[key].to(torch.int64)
        key_col, key_kind = key_col.contiguous(), 1 if key_col.dtype == torch.int32 else 2
    ts_col = cols["timestamp"].contiguous() if mode == "time" else None
    with torch.cuda.device(dev):
        rows = max(n, 1)
        index = torch.empty((2, rows), dtype=torch.int32, device=dev)
        words = torch.tensor([-1, 0, 0, 0, 0], dtype=torch.int64, device=dev)  # the error word (~0), n_sampled, n_train, n_test, split_timestamp
        ws_bytes = lib.sprk_split_plan_workspace_bytes(n)
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)   # (torch's allocations are 512-byte aligned)
        p = lambda x: C.c_void_p(None if x is None else x.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(lib.sprk_split_plan(p(key_col), key_kind, p(ts_col), n, int(seed) & _MASK64, t_sample, t_train, float(train), SPLIT_MODES[mode],
                                    p(index[0]), p(index[1]), p(words), p(ws), ws.numel() * 8, stream))
        err, n_sampled, n_train, n_test, split_timestamp = (int(v) for v in words.cpu().numpy())     # the one synchronisation
        if err != -1:
            raise ValueError("row %d: negative key" % (err & 0xffffffff))
        groups = _matrix_groups(cols) if group_matrices else [[k] for k in cols]
        parts = []
        for which, count in ((0, n_train), (1, n_test)):
            out, desc = {}, []
            for names in groups:
                first = cols[names[0]]
                block = torch.empty((count, len(names)), dtype=first.dtype, device=dev)
                desc.append(L.SplitCol(first.data_ptr(), first.stride(0) * first.element_size(), len(names) * first.element_size(), 0, block.data_ptr()))
                for j, k in enumerate(names):
                    out[k] = block[:, j]
            L.check(lib.sprk_take_rows((L.SplitCol * len(desc))(*desc), len(desc), p(index[which]), count, n, stream))
            parts.append({k: out[k] for k in cols})
    return SplitResult(parts[0], parts[1], n_sampled, split_timestamp if mode == "time" and n_sampled else None)
