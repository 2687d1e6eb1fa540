"""Feature store in HBM: the per-user and per-movie feature maps behind a ``{"userId": u, "movieId": m}`` request.

The reference's Jetty server sends the ranking model nothing but pairs of ids (``RecForYouProcess.java:113-138``); every other model
input comes from two per-entity maps, the ``uf:<userId>`` and ``mf:<movieId>`` hashes, which hold the columns of each user's and each
movie's LATEST sample (``FeatureEngForRecModel.extractAndSave{User,Movie}FeaturesToRedis``, FeatureEngForRecModel.scala:127-174,208-259:
``row_number() over (partitionBy id orderBy timestamp desc) == 1``; read by RecForYouProcess.java:46-52 and
``DataManager.loadMovieFeatures``).  :class:`FeatureStore` is those two maps as device tables indexed by id, like the embedding
tables (row = id, one ``has`` byte per row), in the bits ``schema.pack_ids`` / ``pack_dense`` produce -- so that joining a pair of ids
with its two rows (``sprk_join_features``, csrc/k_feature_join.h) IS packing the assembled sample row, with nothing left to convert.

User row, int32 / float32 dwords, pitch rounded up to a multiple of 4::

    userRatedMovie1..H | userGenre1..5 | userRatingCount userAvgRating userRatingStddev

Movie row, pitch 8::

    movieGenre1..3 | releaseYear movieRatingCount movieAvgRating movieRatingStddev

Identity values: missing -> 0; genres: index in the 19-entry vocabulary, else -1; numerics: float32, missing -> 0.0, ints cast with one
rounding.  History ids are stored as they are (any int32 >= 0): the range check belongs to the model that reads them.  The row of an id
without an entry is the NA defaults 0 / -1 / 0.0.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Mapping, Optional, Tuple

import numpy as np

from . import schema as S

USER_NUMERIC_KEYS = ["userRatingCount", "userAvgRating", "userRatingStddev"]
MOVIE_NUMERIC_KEYS = ["releaseYear", "movieRatingCount", "movieAvgRating", "movieRatingStddev"]
MOVIE_PITCH = 8
_ANY_ID = (1 << 31) - 1                 # "vocabulary" of a column stored unchecked: every non-negative int32

# user_rows [n_users, user_pitch] int32, user_has [n_users] uint8, movie_rows [n_movies, 8] int32, movie_has [n_movies] uint8, hist_len
RowImages = namedtuple("RowImages", "user_rows user_has movie_rows movie_has hist_len")


def history_keys(hist_len: int):
    return ["userRatedMovie%d" % (i + 1) for i in range(hist_len)]


def user_pitch(hist_len: int) -> int:
    return (hist_len + len(S.USER_GENRE_KEYS) + len(USER_NUMERIC_KEYS) + 3) // 4 * 4


def user_layout(hist_len: int):
    """{column: (dword offset in the user row, role)}; role 'id' | 'genre' | 'dense'."""
    out, o = {}, 0
    for k in history_keys(hist_len):
        out[k] = (o, "id"); o += 1
    for k in S.USER_GENRE_KEYS:
        out[k] = (o, "genre"); o += 1
    for k in USER_NUMERIC_KEYS:
        out[k] = (o, "dense"); o += 1
    return out


def movie_layout():
    out, o = {}, 0
    for k in S.MOVIE_GENRE_KEYS:
        out[k] = (o, "genre"); o += 1
    for k in MOVIE_NUMERIC_KEYS:
        out[k] = (o, "dense"); o += 1
    return out


def _pack(features: Mapping, id_columns, numeric_keys) -> Tuple[np.ndarray, np.ndarray]:
    """The project's column packer, route by route as ``CTRModel.pack`` takes them (host native, else the Python packer: same bits)."""
    from . import ingest
    if not ingest.force_python():
        got = ingest.pack_columns(features, id_columns, list(numeric_keys))
        if got is not None:
            return got
    return S.pack_ids(features, id_columns), S.pack_dense(features, numeric_keys)


def _default_row(pitch: int, layout) -> np.ndarray:
    row = np.zeros(pitch, dtype=np.int32)
    for off, role in layout.values():
        if role == "genre":
            row[off] = -1
    return row


def _table(keys: np.ndarray, order_by: Optional[np.ndarray], ids: np.ndarray, dense: np.ndarray, pitch: int, layout, n_rows: Optional[int],
           what: str):
    """rows [n, pitch] int32 + has [n] uint8 from one packed row per sample: per key the sample with the greatest ``order_by`` stays,
    among equal ones the last in input order."""
    keys = np.asarray(keys, dtype=np.int64)
    if keys.size and (keys.min() < 0 or keys.max() >= _ANY_ID):
        raise ValueError("%s %d cannot index a table" % (what, int(keys[(keys < 0) | (keys >= _ANY_ID)][0])))
    n = int(keys.max()) + 1 if keys.size else 0
    if n_rows is not None:
        if n_rows < n:
            raise ValueError("%s %d does not fit a table of %d rows" % (what, n - 1, n_rows))
        n = int(n_rows)
    rows = np.tile(_default_row(pitch, layout), (n, 1))
    has = np.zeros(n, dtype=np.uint8)
    if keys.size:
        o = np.argsort(order_by, kind="stable") if order_by is not None else np.arange(keys.size)
        ko = keys[o]
        _, first_rev = np.unique(ko[::-1], return_index=True)    # per key: its LAST position in (order_by, input order)
        pick = o[ko.size - 1 - first_rev]
        k = keys[pick]
        rows[k, :ids.shape[1]] = ids[pick]
        rows[k, ids.shape[1]:ids.shape[1] + dense.shape[1]] = dense[pick].view(np.int32)
        has[k] = 1
    return rows, has


def _split_history(features: Mapping, hist_len: int) -> Mapping:
    """``userRatedMovies [n, H]`` as H column views, as ``DIN._columns`` accepts it."""
    keys = history_keys(hist_len)
    if "userRatedMovies" in features and keys[0] not in features:
        hist = features["userRatedMovies"]
        hist = hist.detach().cpu().numpy() if hasattr(hist, "detach") else np.asarray(hist)
        if hist.ndim != 2 or hist.shape[1] != hist_len:
            raise ValueError("userRatedMovies must be [n, %d]" % hist_len)
        features = dict(features)
        for i, k in enumerate(keys):
            features[k] = hist[:, i]
    return features


def _user_columns(hist_len):
    return ([S.IdColumn(k, "id", _ANY_ID) for k in history_keys(hist_len)]
            + [S.IdColumn(k, "genre", S.N_GENRES) for k in S.USER_GENRE_KEYS])


def _movie_columns():
    return [S.IdColumn(k, "genre", S.N_GENRES) for k in S.MOVIE_GENRE_KEYS]


def row_images_from_samples(features_or_csv_path, hist_len: int = 5, n_users: Optional[int] = None, n_movies: Optional[int] = None) -> RowImages:
    """The two tables' host images from sample columns (a dict as ``schema.read_samples_csv`` returns it, any column types the column
    packer accepts, or a CSV path): per user, and independently per movie, the row with the greatest ``timestamp``; among equal
    timestamps the last row in input order (Spark leaves that open; this is fixed here).  A store column the samples do not carry
    (synthetic.synth_din has one user genre) is missing in every row.  ``n_users`` / ``n_movies`` size the tables beyond the greatest id
    seen (default: that id + 1; an id past a table reads the default row anyway).  No GPU involved."""
    feats = S.read_samples_csv(features_or_csv_path) if isinstance(features_or_csv_path, str) else features_or_csv_path
    feats = _split_history(feats, hist_len)
    for k in ("userId", "movieId", "timestamp"):
        if k not in feats:
            raise KeyError("missing input feature %r" % k)
    n = len(feats["userId"])
    absent = [k for k in history_keys(hist_len) + S.USER_GENRE_KEYS + S.MOVIE_GENRE_KEYS + USER_NUMERIC_KEYS + MOVIE_NUMERIC_KEYS if k not in feats]
    if absent:                                                     # a column the samples do not carry is missing in every row
        feats = dict(feats)
        for k in absent:
            feats[k] = np.full(n, -1, dtype=np.int64) if "Genre" in k else np.zeros(n, dtype=np.float32 if k in S.NUMERIC_KEYS else np.int64)
    ts = S.to_int_column(feats["timestamp"], "timestamp")
    uid = S.to_int_column(feats["userId"], "userId")
    mid = S.to_int_column(feats["movieId"], "movieId")
    u_ids, u_dense = _pack(feats, _user_columns(hist_len), USER_NUMERIC_KEYS)
    m_ids, m_dense = _pack(feats, _movie_columns(), MOVIE_NUMERIC_KEYS)
    user_rows, user_has = _table(uid, ts, u_ids, u_dense, user_pitch(hist_len), user_layout(hist_len), n_users, "userId")
    movie_rows, movie_has = _table(mid, ts, m_ids, m_dense, MOVIE_PITCH, movie_layout(), n_movies, "movieId")
    return RowImages(user_rows, user_has, movie_rows, movie_has, int(hist_len))


def _map_columns(maps: Mapping, keys):
    """``{id: {column: str-or-number}}`` -> (ids, {column: array}) for ``keys`` = ``[(column, role)]``; absent keys, None and empty
    strings are missing values.  A column whose present values are all numbers keeps them as numbers -- a missing one is the packer's
    own missing value of that role (genre index -1, NaN otherwise) -- so a float reaches float32 in one rounding; a column that holds any
    string is handed over as strings, the hashes' own form."""
    ids = np.fromiter((int(i) for i in maps), dtype=np.int64, count=len(maps))
    entries = list(maps.values())
    cols = {}
    for k, role in keys:
        vals = [e.get(k) for e in entries]
        missing = [v is None or (isinstance(v, (str, bytes)) and len(v) == 0) for v in vals]
        if vals and not any(isinstance(v, (str, bytes)) and len(v) for v in vals) and not all(missing):
            if not any(missing):
                cols[k] = np.asarray(vals)                           # numbers throughout: their own storage kind
            elif role == "genre":
                cols[k] = np.array([-1 if m else int(v) for v, m in zip(vals, missing)], dtype=np.int64)
            else:
                cols[k] = np.array([np.nan if m else float(v) for v, m in zip(vals, missing)], dtype=np.float64)
        else:
            cols[k] = np.array(["" if m else (v.decode() if isinstance(v, bytes) else str(v)) for v, m in zip(vals, missing)], dtype=object)
    return ids, cols


def row_images_from_feature_maps(user_maps: Mapping, movie_maps: Mapping, hist_len: int = 5, n_users: Optional[int] = None,
                                 n_movies: Optional[int] = None) -> RowImages:
    """The same images from ``{id: {column: str-or-number}}`` maps, the shape of the reference's ``uf:`` / ``mf:`` hashes.  ``n_users`` /
    ``n_movies`` size the tables (default: the greatest id + 1), as in :func:`row_images_from_samples`."""
    ucols, mcols = _user_columns(hist_len), _movie_columns()
    uid, uf = _map_columns(user_maps, [(c.key, c.kind) for c in ucols] + [(k, "dense") for k in USER_NUMERIC_KEYS])
    mid, mf = _map_columns(movie_maps, [(c.key, c.kind) for c in mcols] + [(k, "dense") for k in MOVIE_NUMERIC_KEYS])
    u_ids, u_dense = (_pack(uf, ucols, USER_NUMERIC_KEYS) if uid.size
                      else (np.zeros((0, len(ucols)), np.int32), np.zeros((0, len(USER_NUMERIC_KEYS)), np.float32)))
    m_ids, m_dense = (_pack(mf, mcols, MOVIE_NUMERIC_KEYS) if mid.size
                      else (np.zeros((0, len(mcols)), np.int32), np.zeros((0, len(MOVIE_NUMERIC_KEYS)), np.float32)))
    user_rows, user_has = _table(uid, None, u_ids, u_dense, user_pitch(hist_len), user_layout(hist_len), n_users, "userId")
    movie_rows, movie_has = _table(mid, None, m_ids, m_dense, MOVIE_PITCH, movie_layout(), n_movies, "movieId")
    return RowImages(user_rows, user_has, movie_rows, movie_has, int(hist_len))


class FeatureStore:
    """The two tables on a device.  ``device="cpu"`` keeps the host images only (layout, ``join_plan``; nothing can be joined from it).

    ``n_users``, ``n_movies``, ``hist_len``, ``user_pitch``, ``movie_pitch`` (dwords) describe the tables; ``images`` is the host copy
    they were uploaded from (a :class:`RowImages`), ``user_layout`` / ``movie_layout`` map a column to its dword and role."""

    _state = None                       # an updatable store's featureeng.StoreState (empty, from_ratings(updatable=True))

    def __init__(self, images: RowImages, device=None):
        self._images = images
        self.hist_len = int(images.hist_len)
        self.n_users, self.user_pitch = int(images.user_rows.shape[0]), int(images.user_rows.shape[1])
        self.n_movies, self.movie_pitch = int(images.movie_rows.shape[0]), int(images.movie_rows.shape[1])
        if self.user_pitch != user_pitch(self.hist_len) or self.movie_pitch != MOVIE_PITCH:
            raise ValueError("row images do not have the store's pitches")
        self.user_layout, self.movie_layout = user_layout(self.hist_len), movie_layout()
        self.device = None
        self._tensors = None
        if device is None or str(device) != "cpu":
            import torch
            if not torch.cuda.is_available():
                raise RuntimeError("FeatureStore needs a HIP device (device=\"cpu\" keeps the host images only)")
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            # (one spare row each: an empty table still has an address)
            def up(a, pad_shape):
                t = torch.from_numpy(np.concatenate([a, np.zeros(pad_shape, dtype=a.dtype)])).to(dev)
                return t
            self._tensors = (up(images.user_rows, (1, self.user_pitch)), up(images.user_has, (1,)),
                             up(images.movie_rows, (1, self.movie_pitch)), up(images.movie_has, (1,)))
            self.device = dev

    @property
    def images(self) -> RowImages:
        """The host copy of the tables; a store whose tables were written on the device (:meth:`from_ratings`) downloads it at first use."""
        if self._images is None:
            ur, uh, mr, mh = (t.cpu().numpy() for t in self.tensors())
            self._images = RowImages(ur[:self.n_users], uh[:self.n_users], mr[:self.n_movies], mh[:self.n_movies], self.hist_len)
        return self._images

    @classmethod
    def _from_device_tables(cls, tensors, hist_len: int, device):
        """A store over tables that are on the device already, one spare row each: ``(user_rows, user_has, movie_rows, movie_has)``."""
        self = cls.__new__(cls)
        self._images = None
        self.hist_len = int(hist_len)
        self.n_users, self.user_pitch = int(tensors[0].shape[0]) - 1, int(tensors[0].shape[1])
        self.n_movies, self.movie_pitch = int(tensors[2].shape[0]) - 1, int(tensors[2].shape[1])
        if self.user_pitch != user_pitch(self.hist_len) or self.movie_pitch != MOVIE_PITCH:
            raise ValueError("the tables do not have the store's pitches")
        self.user_layout, self.movie_layout = user_layout(self.hist_len), movie_layout()
        self._tensors, self.device = tuple(tensors), device
        return self

    @classmethod
    def from_ratings(cls, ratings, movies, hist_len: int = 5, device=None, n_users: Optional[int] = None, n_movies: Optional[int] = None,
                     updatable: bool = False):
        """From ``ratings.csv`` and ``movies.csv`` (paths or columns, as ``featureeng.build`` takes them) without the reference's Spark
        job: the samples are computed on ``device`` and the tables written there (``sprk_feature_eng``).  ``device="cpu"`` builds the images
        from the host definition ``featureeng.samples_host``: no GPU involved, like the other constructors.  ``n_users`` / ``n_movies``
        default to the greatest id of the RATINGS + 1 (the movie table's rows at least).  ``updatable=True``: the same tables, byte for
        byte, as :meth:`empty` followed by :meth:`update`: the store keeps the state that later updates need, and its table sizes are
        capacities."""
        from . import featureeng as FE
        if updatable:
            table = FE.movie_table(movies)
            on_device = isinstance(ratings, Mapping) and all(hasattr(ratings.get(k), "detach") for k in FE.RATING_KEYS)
            cols = ratings if on_device else dict(zip(FE.RATING_KEYS, FE._rating_columns(ratings)))
            sized = n_users is not None and n_movies is not None
            greatest = [np.array([-1 if sized else FE._greatest_id(cols[k])]) for k in ("userId", "movieId")]
            n_users, n_movies = FE._table_sizes(greatest[0], greatest[1], table, n_users, n_movies)
            store = cls.empty(table, n_users, n_movies, hist_len, device)
            store.update(cols)
            return store
        if device is not None and str(device) == "cpu":
            table = FE.movie_table(movies)
            u, m, _, _ = cols = FE._rating_columns(ratings)
            samples = FE.samples_host(dict(zip(FE.RATING_KEYS, cols)), table, hist_len, n_users, n_movies)
            n_users, n_movies = FE._table_sizes(u, m, table, n_users, n_movies)
            return cls(row_images_from_samples(samples, hist_len, n_users, n_movies), "cpu")
        return FE.build(ratings, movies, hist_len, device, n_users, n_movies).store()

    @classmethod
    def from_samples(cls, features_or_csv_path, hist_len: int = 5, device=None, n_users: Optional[int] = None, n_movies: Optional[int] = None):
        """Every user's and every movie's latest sample (:func:`row_images_from_samples`), uploaded to ``device``."""
        return cls(row_images_from_samples(features_or_csv_path, hist_len, n_users, n_movies), device)

    @classmethod
    def from_feature_maps(cls, user_maps, movie_maps, hist_len: int = 5, device=None, n_users: Optional[int] = None,
                          n_movies: Optional[int] = None):
        """``{id: {column: str-or-number}}`` maps, the shape of the ``uf:`` / ``mf:`` hashes (:func:`row_images_from_feature_maps`)."""
        return cls(row_images_from_feature_maps(user_maps, movie_maps, hist_len, n_users, n_movies), device)

    @classmethod
    def empty(cls, movies, n_users: int, n_movies: int, hist_len: int = 5, device=None):
        """An updatable store with no ratings: no entry, every row the NA defaults.  ``movies``: what ``featureeng.movie_table`` takes;
        ``n_users`` / ``n_movies`` are capacities that do not grow: an id beyond them in a later batch is :meth:`update`'s error.
        ``device="cpu"``: the host images and the host definition of the update, no GPU involved."""
        from . import featureeng as FE
        if device is not None and str(device) == "cpu":
            state = FE.empty_state(movies, n_users, n_movies, hist_len, "cpu")
            self = cls(RowImages(*state.tables, int(hist_len)), "cpu")         # (the images ARE the state's tables: updated in place)
        else:
            import torch
            if not torch.cuda.is_available():
                raise RuntimeError("FeatureStore needs a HIP device (device=\"cpu\" keeps the host images only)")
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            state = FE.empty_state(movies, n_users, n_movies, hist_len, dev)
            self = cls._from_device_tables(state.tables, hist_len, dev)
        self._state = state
        return self

    @property
    def updatable(self) -> bool:
        """:meth:`update` applies new ratings to this store."""
        return self._state is not None

    @property
    def n_ratings(self) -> int:
        """The ratings an updatable store has been given so far, the ones it was built from included."""
        if self._state is None:
            raise RuntimeError("this FeatureStore does not count its ratings: it is not updatable")
        return self._state.n_ratings

    def update(self, ratings) -> int:
        """Applies new ratings -- a CSV path or ``{userId, movieId, rating, timestamp}`` columns, numpy arrays or device tensors, which
        are used where they are -- and returns their number.  Afterwards the four tables are byte for byte the tables of
        ``from_ratings(R, ...)`` with the same table sizes, R = every batch this store has been given, in call order, PROVIDED no
        rating is older than the latest rating of its user in an EARLIER batch (a nearline stream is in time order per user; the rows
        of one batch may come in any order).  A rating that is older, an id beyond the tables or a rating off the half-star scale raises
        ``ValueError`` naming the batch's row, and the store is as it was.  On a device: the kernels of ``sprk_store_update`` on the
        current stream and one host synchronisation, for the error word; the tables are changed in place, so :meth:`tensors`, join plans
        and engines made earlier stay valid, and the cached host image is dropped."""
        from . import featureeng as FE
        if self._state is None:
            raise RuntimeError("this FeatureStore is not updatable: build it with FeatureStore.empty or from_ratings(..., updatable=True)")
        if self._state.device is None:
            return FE.update_host(self._state, ratings)
        n = FE.update_device(self._state, ratings)
        self._images = None
        return n

    def tensors(self):
        """Device tensors ``(user_rows, user_has, movie_rows, movie_has)``."""
        if self._tensors is None:
            raise RuntimeError("this FeatureStore holds no device tables (closed, or built with device=\"cpu\")")
        return self._tensors

    def has_user(self, ids) -> np.ndarray:
        """Per id: the store holds a row for this user (from the host image: no device call)."""
        ids = np.asarray(ids, dtype=np.int64)
        ok = (ids >= 0) & (ids < self.n_users)
        out = np.zeros(ids.shape, dtype=bool)
        out[ok] = self.images.user_has[ids[ok]] != 0
        return out

    def table_bytes(self) -> int:
        """Bytes of the two tables and their ``has`` flags."""
        return self.n_users * (self.user_pitch * 4 + 1) + self.n_movies * (self.movie_pitch * 4 + 1)

    def close(self):
        """Drops the device tables (the host images stay) and, with them, an updatable store's state on the device."""
        if self._state is not None and self._state.device is not None:
            self._state = None
        self._tensors = None
        self.device = None
