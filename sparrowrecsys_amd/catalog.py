"""The movie catalogue: average ratings, the sorted lists, candidate generation and the default similarity ranker, without the JVM.

The reference's online server keeps every movie in a ``DataManager`` and asks it which movies to rank: ``RecForYouProcess.getRecList``
ranks ``getMovies(800, "rating")``, ``SimilarMovieProcess.getRecList`` ranks the union of ``getMoviesByGenre(g, 100, "rating")`` over the
movie's genres, by default with ``calculateSimilarScore``.  This module is that arithmetic: :func:`catalog_host` and :func:`similar_host`
are the DEFINITION, in numpy, and :func:`build` / :class:`Catalog` compute the same bits on the device (``sprk_catalog_build``,
``sprk_catalog_similar``, csrc/k_catalog.h).  The rules:

* Movie table (``DataManager.loadMovieData``, DataManager.java:53-87).  Rows are indexed by movie id; the genre dictionary, ``mask`` and
  ``has`` are ``featureeng.movie_table``'s.  ``n_genres`` is ``genres.size()``: the number of ``|`` pieces of a genre field that is not
  blank; a field that repeats a genre raises ``ValueError`` naming the movie, which keeps ``sameGenreCount`` a popcount.  ``file_pos`` is
  the movie's position in the file.  ``year`` is ``parseReleaseYear`` (:167-178), not the Spark job's: with ``t = title.trim()``, 0 if
  ``len(t) < 6``, else ``int(t[len(t) - 5 : len(t) - 1])``, and 0 where that is no integer (Java leaves the field at its default; it
  neither throws nor gives 1990).
* Average rating (``Movie.addRating``, Movie.java:93-98).  Per movie the table holds, over its ratings in input order from ``avg = 0.0``,
  ``n = 0``: ``avg = (avg * (double)n + (double)score) / (double)(n + 1); n++`` with ``score`` a float32 -- one double multiply, one add
  and one IEEE division per rating, nothing fused or reassociated.  This is a recurrence and NOT ``sum / n`` in general.  A rating on a
  movie id outside the table, or on a movie the table does not hold, is skipped (``movieMap.get == null``); a rating that is not finite
  is an error, ``ValueError`` naming the first such row.  ``rating_count`` is an int32.
* Lists (``getMovies`` / ``getMoviesByGenre``, :253-283).  With G dictionary genres there are 2 (G + 1) lists: list ``g < G`` = genre g
  by ``"rating"``, list ``G`` = the whole catalogue by rating, list ``G + 1 + g`` = genre g by ``"releaseYear"``, list ``2 G + 1`` = the
  whole catalogue by year.  ``"rating"`` is ``Double.compare`` on the average, descending (0.0 before -0.0, every NaN one greatest
  value: ``k_emb_rank.h``'s keys); ``"releaseYear"`` is the year, descending.  Ties keep the pre-sort order, as Java's stable sort
  does: a genre list starts in file order, so its ties fall back to ``file_pos``; the whole catalogue starts in the iteration order of a
  ``HashMap<Integer, Movie>``, defined here as the order of ``(bucket, file_pos)`` with ``cap`` the least power of two ``>= 16`` with
  ``n <= 0.75 cap`` for n movies held and ``bucket = (id ^ (id >>> 16)) & (cap - 1)`` (``hash_pos``, computed on the host).  Every list
  is thus a total order on (key, tie position): any correct sort gives the same bytes.
* Candidates (SimilarMovieProcess.java:39-83).  Mode 0 (``candidateGenerator``): the union over the query's genres of the first
  ``top_n`` (100) entries of that genre's rating list, minus the query.  Mode 1 (``multipleRetrievalCandidates``): the same with
  ``top_n`` 20, plus the first ``extra_n`` (100) entries of the whole catalogue's rating list and of its year list, minus the query.
  A query the table does not hold has no candidates.
* Default score (``calculateSimilarScore``, :145-159), in doubles, every operation rounded on its own: ``same = popcount(mask_q &
  mask_c)``, ``gs = ((double)same / (double)(n_genres_q + n_genres_c)) / 2.0``, ``rs = avg_c / 5.0``, ``score = gs * 0.7 + rs * 0.3``;
  ``0 / 0`` is NaN (mode 1, a query and a candidate without genres), which sorts as the greatest value, as in Java.
* Ranking: scores descending in ``Double.compare`` order, equal scores in candidate order, cut to ``size``.

Deviations, where Java leaves the result open or the project chooses otherwise:

* CSV parsing: by default the project's CSV reader is used and no movie is dropped.  Java's ``split(",")`` drops every line that does
  not give exactly three pieces -- every title with a quoted comma; ``reference_lines=True`` reproduces that (755 of the reference's 982
  movies remain).
* Candidate and tie order: Java iterates a ``HashMap`` over identity hashes, which differs from run to run.  Candidates are returned in
  ascending movie id order here, and that is the order equal scores fall back to.
* Tree bins: a ``HashMap`` bucket that eight or more ids share becomes a tree in Java and iterates differently; not reproduced.
* An unknown genre gives an empty list, where Java throws.  An empty ``|`` piece is no genre, as in ``featureeng.movie_table``.

Parity with the reference: it ships no ``ratings.csv``, so the averages are pinned by this definition and a hand-worked movie
(tests/catalog_cases.py: twelve ratings whose recurrence differs from ``sum / n`` in the last bit); the movie side is pinned by the
reference's own data through the excerpt fixture (tests/test_catalog.py).

Out of scope: REST endpoints, movie JSON, Redis, updating a built catalogue from new ratings.
"""
from __future__ import annotations

import re
from collections import namedtuple
from typing import Mapping, Optional

import numpy as np

from . import featureeng as FE

MAX_CANDIDATES = 4096
ERR_RATING, ERR_LISTS = 3, 4
SORT_KEYS = ("rating", "releaseYear")
_ID_LIMIT = (1 << 31) - 1
_CANONICAL_NAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]

# row = movieId: year int32, n_genres uint8, mask uint32, has uint8, file_pos / hash_pos int32 (-1 = not held); dictionary [str]
CatalogTable = namedtuple("CatalogTable", "year n_genres mask has file_pos hash_pos dictionary")


def release_year(title) -> int:
    """``DataManager.parseReleaseYear`` (DataManager.java:167-178) with the field's default where it gives -1: 0."""
    if title is None:
        return 0
    t = (title.decode() if isinstance(title, bytes) else str(title)).strip(FE._JAVA_BLANKS)
    if len(t) < 6:
        return 0
    text = t[len(t) - 5:len(t) - 1]
    return int(text) if re.fullmatch(r"[+-]?[0-9]+", text) else 0


def hashmap_capacity(n: int) -> int:
    """The table length of a ``HashMap`` after n insertions: the least power of two >= 16 with n <= 0.75 cap."""
    cap = 16
    while 4 * int(n) > 3 * cap:
        cap *= 2
    return cap


def hashmap_positions(ids) -> np.ndarray:
    """ids in insertion (file) order -> each one's place in the map's iteration order: the order of ``(bucket, insertion)``."""
    ids = np.asarray(ids, dtype=np.int64)
    bucket = (ids ^ (ids >> 16)) & (hashmap_capacity(len(ids)) - 1)
    pos = np.empty(len(ids), dtype=np.int32)
    pos[np.lexsort((np.arange(len(ids)), bucket))] = np.arange(len(ids), dtype=np.int32)
    return pos


def _java_split(text: str, sep: str) -> list:
    """``String.split`` with a literal separator: trailing empty strings are removed; a string without the separator is one piece."""
    parts = text.split(sep)
    if len(parts) == 1:
        return parts
    while parts and parts[-1] == "":
        parts.pop()
    return parts


def reference_lines_columns(path: str) -> dict:
    """``movies.csv`` as ``DataManager.loadMovieData`` reads it: the first line skipped, every other line ``split(",")`` and kept only
    when that gives exactly three pieces."""
    ids, titles, genres = [], [], []
    with open(path, encoding="utf-8") as f:
        for k, line in enumerate(f.read().splitlines()):
            if k == 0:
                continue
            pieces = _java_split(line, ",")
            if len(pieces) == 3:
                ids.append(int(pieces[0]))
                titles.append(pieces[1])
                genres.append(pieces[2])
    return {"movieId": ids, "title": titles, "genres": genres}


def catalog_table(movies, reference_lines: bool = False) -> CatalogTable:
    """The catalogue's movie table from ``movies.csv`` (a path) or ``{movieId, title, genres}`` columns."""
    if isinstance(movies, CatalogTable):
        return movies
    if reference_lines:
        if not isinstance(movies, str):
            raise ValueError("reference_lines reads the file's lines: movies must be a path")
        cols = reference_lines_columns(movies)
    else:
        cols = FE._read_csv_columns(movies, ["movieId", "title", "genres"]) if isinstance(movies, str) else movies
    text = lambda v: None if v is None else (v.decode() if isinstance(v, bytes) else str(v))
    ids = [int(v) for v in FE._host_column(cols["movieId"]).tolist()]
    titles = [text(v) for v in FE._host_column(cols["title"]).tolist()]
    fields = []
    for i, g in zip(ids, FE._host_column(cols["genres"]).tolist()):
        g = text(g)
        if g is None or g.strip(FE._JAVA_BLANKS) == "":          # genres.trim().isEmpty(): no genre
            fields.append([])
            continue
        pieces = [p for p in _java_split(g, "|") if p != ""]
        if len(set(pieces)) != len(pieces):
            raise ValueError("movie %d names a genre twice: %r" % (i, g))
        fields.append(pieces)
    base = FE.movie_table({"movieId": ids, "title": [None] * len(ids), "genres": ["|".join(p) for p in fields]})   # (its year is not used)
    n = len(base.has)
    year, n_genres = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    file_pos, hash_pos = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    if ids:
        at = np.asarray(ids, dtype=np.int64)
        year[at] = [release_year(t) for t in titles]
        n_genres[at] = [len(p) for p in fields]
        file_pos[at] = np.arange(len(ids), dtype=np.int32)
        hash_pos[at] = hashmap_positions(at)
    return CatalogTable(year, n_genres, base.mask, base.has, file_pos, hash_pos, base.dictionary)


def _error_message(kind: int, row: int) -> str:
    if kind == ERR_LISTS:
        return "the lists do not fit list_capacity"
    return "ratings row %d: the rating is not finite" % row


def _rating_columns(ratings):
    """-> movieId (int64) and rating (float32) as numpy arrays, in input order."""
    cols = FE._read_csv_columns(ratings, ["movieId", "rating"]) if isinstance(ratings, str) else ratings
    for k in ("movieId", "rating"):
        if k not in cols:
            raise KeyError("missing ratings column %r" % k)
    m, r = FE._host_column(cols["movieId"]), FE._host_column(cols["rating"])
    m = m.astype(np.int64) if m.dtype.kind in "iub" else np.array([int(v) for v in m.tolist()], dtype=np.int64)
    r = r.astype(np.float32) if r.dtype.kind in "iubf" else np.array([float(v) for v in r.tolist()], dtype=np.float64).astype(np.float32)
    if m.ndim != 1 or m.shape != r.shape:
        raise ValueError("the ratings columns differ in length")
    if len(m) >= _ID_LIMIT:
        raise ValueError("at most 2^31 - 2 ratings")
    return m, r


def double_compare_key(x) -> np.ndarray:
    """``Double.compare`` order as unsigned 64-bit keys: 0.0 above -0.0, every NaN one greatest value (k_emb_rank.h's er_key)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64)
    key = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(x), np.uint64(0xffffffffffffffff), key)


def average_ratings(movie_id, rating, has):
    """The recurrence of ``Movie.addRating`` for every movie of the table at once -> ``(avg float64, count int32)``.  Step k runs over
    all movies that have more than k ratings, each operation a numpy operation of its own (numpy fuses nothing)."""
    n_movies = len(has)
    m, r = np.asarray(movie_id, dtype=np.int64), np.asarray(rating, dtype=np.float32)
    bad = ~np.isfinite(r)
    if bad.any():
        raise ValueError(_error_message(ERR_RATING, int(np.flatnonzero(bad)[0])))
    inside = (m >= 0) & (m < n_movies)
    ok = inside & (np.asarray(has)[np.where(inside, m, 0)] != 0) if n_movies else np.zeros(len(m), dtype=bool)
    m, score = m[ok], r[ok].astype(np.float64)
    count = np.bincount(m, minlength=n_movies).astype(np.int64)
    score = score[np.argsort(m, kind="stable")]                               # grouped by movie, input order within
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    by_len = np.argsort(-count, kind="stable")                                 # the movies with more than k ratings are a prefix of this
    start_l, len_l = start[by_len], count[by_len]
    avg_l = np.zeros(n_movies, dtype=np.float64)
    live = int((len_l > 0).sum())
    k = 0
    while live:
        avg_l[:live] = (avg_l[:live] * np.float64(k) + score[start_l[:live] + k]) / np.float64(k + 1)
        k += 1
        while live and len_l[live - 1] <= k:
            live -= 1
    avg = np.zeros(n_movies, dtype=np.float64)
    avg[by_len] = avg_l
    return avg, count.astype(np.int32)


def catalog_host(ratings, movies, reference_lines: bool = False) -> dict:
    """The definition (module docstring): ``ratings`` = ``{movieId, rating, ..}`` columns or a CSV path, in input order; ``movies`` what
    :func:`catalog_table` takes.  -> a dict: the table's columns ``year, n_genres, mask, has, file_pos, hash_pos`` and ``dictionary``,
    ``avg`` float64 and ``rating_count`` int32 per movie id, and the 2 (G + 1) lists as ``list_offsets`` int32 ``[2 (G + 1) + 1]`` into
    ``list_movies`` int32."""
    table = catalog_table(movies, reference_lines)
    m, r = _rating_columns(ratings)
    avg, count = average_ratings(m, r, table.has)
    G = len(table.dictionary)
    held = np.flatnonzero(table.has)
    by_rating = ~double_compare_key(avg)                                       # ascending in this = descending in Double.compare
    by_year = -table.year.astype(np.int64)
    lists = []
    for key in (by_rating, by_year):
        for g in range(G):
            members = held[((table.mask[held] >> np.uint32(g)) & np.uint32(1)) != 0]
            lists.append(members[np.lexsort((table.file_pos[members], key[members]))])
        lists.append(held[np.lexsort((table.hash_pos[held], key[held]))])
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    out = dict(table._asdict())
    out.update(avg=avg, rating_count=count, list_offsets=offsets,
               list_movies=np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32))
    return out


def _popcount32(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint32)
    return sum(((x >> np.uint32(g)) & np.uint32(1)).astype(np.int64) for g in range(32))


def _heads(top_n, mode):
    return (100 if mode == 0 else 20) if top_n is None else int(top_n)


def _check_similar_arguments(mode, top_n, extra_n, size):
    if mode not in (0, 1):
        raise ValueError("mode = %r (0 = candidateGenerator, 1 = multipleRetrievalCandidates)" % (mode,))
    if top_n < 0 or extra_n < 0 or 32 * top_n + 2 * extra_n > MAX_CANDIDATES:
        raise ValueError("top_n = %d, extra_n = %d: need both >= 0 and 32 top_n + 2 extra_n <= %d" % (top_n, extra_n, MAX_CANDIDATES))
    if size < 0:
        raise ValueError("size = %d" % size)


def candidate_width(cat, mode: int = 0, top_n: Optional[int] = None, extra_n: int = 100) -> int:
    """The columns of a candidate matrix: the most candidates any movie of this table can have, one at the least."""
    n_genres, has = np.asarray(cat["n_genres"]), np.asarray(cat["has"])
    most = int(n_genres.max()) * _heads(top_n, mode) + (2 * int(extra_n) if mode == 1 else 0) if len(n_genres) else 0
    return max(1, min(most, int(has.sum())))


def similar_host(cat, movie_ids, size: int = 10, mode: int = 0, top_n: Optional[int] = None, extra_n: int = 100, model: str = "default"):
    """The definition of candidate generation and the default ranker over :func:`catalog_host`'s dict (or a :class:`Catalog`).
    ``model="default"`` -> ``(ids [Q, size] int32 best first, padded -1; scores [Q, size] float64, padded 0.0, NaN as Java's
    Double.NaN; counts [Q] int32 = min(size, candidates))``.  ``model="candidates"`` -> ``(ids [Q, candidate_width] ascending, padded -1;
    None; counts)``: the candidate generator alone."""
    if isinstance(cat, Catalog):
        cat = cat.to_host()
    if model not in ("default", "candidates"):
        raise ValueError("model = %r (similar_host knows \"default\" and \"candidates\")" % (model,))
    top_n, extra_n, size = _heads(top_n, mode), int(extra_n), int(size)
    _check_similar_arguments(mode, top_n, extra_n, size)
    mask, has, n_genres, avg = cat["mask"], cat["has"], cat["n_genres"], cat["avg"]
    off, movies, G = cat["list_offsets"], cat["list_movies"], len(cat["dictionary"])
    head = lambda l, k: movies[off[l]:off[l] + min(k, off[l + 1] - off[l])]
    queries = np.asarray(list(movie_ids) if not hasattr(movie_ids, "shape") else FE._host_column(movie_ids), dtype=np.int64).reshape(-1)
    W = size if model == "default" else candidate_width(cat, mode, top_n, extra_n)
    ids = np.full((len(queries), W), -1, dtype=np.int32)
    scores = np.zeros((len(queries), W), dtype=np.float64) if model == "default" else None
    counts = np.zeros(len(queries), dtype=np.int32)
    for j, q in enumerate(queries.tolist()):
        if not (0 <= q < len(has) and has[q]):
            continue
        parts = [head(g, top_n) for g in range(G) if int(mask[q]) >> g & 1]
        if mode == 1:
            parts += [head(G, extra_n), head(2 * G + 1, extra_n)]
        c = np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.int32)     # ascending, each id once
        c = c[c != q]
        if model == "candidates":
            ids[j, :len(c)], counts[j] = c, len(c)
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            same = _popcount32(mask[q] & mask[c]).astype(np.float64)
            gs = (same / (int(n_genres[q]) + n_genres[c].astype(np.int64)).astype(np.float64)) / np.float64(2.0)
            rs = avg[c] / np.float64(5.0)
            s = gs * np.float64(0.7) + rs * np.float64(0.3)
        s = np.where(np.isnan(s), _CANONICAL_NAN, s)
        order = np.lexsort((c, ~double_compare_key(s)))[:size]
        ids[j, :len(order)], scores[j, :len(order)], counts[j] = c[order], s[order], len(order)
    return ids, scores, counts


HOST_KEYS = ("year", "n_genres", "mask", "has", "file_pos", "hash_pos", "avg", "rating_count", "list_offsets", "list_movies")


class Catalog:
    """What :func:`build` returns: the movie table (host copy ``table`` and device columns), ``avg`` float64 and ``rating_count`` int32 per
    movie id, and the lists (``list_offsets``, ``list_movies``) as device tensors; the offsets are kept on the host as well."""

    def __init__(self, table: CatalogTable, columns: dict, avg, rating_count, list_offsets, list_movies, offsets_host, device):
        self.table, self.columns, self.device = table, columns, device
        self.avg, self.rating_count, self.list_offsets, self.list_movies = avg, rating_count, list_offsets, list_movies
        self.offsets = np.asarray(offsets_host, dtype=np.int64)
        self.dictionary = list(table.dictionary)
        self.G, self.n_movies = len(self.dictionary), len(table.has)

    def to_host(self) -> dict:
        """The dict :func:`catalog_host` returns, bit for bit."""
        out = dict(self.table._asdict())
        for k, v in (("avg", self.avg), ("rating_count", self.rating_count), ("list_offsets", self.list_offsets), ("list_movies", self.list_movies)):
            out[k] = np.ascontiguousarray(FE._host_column(v))
        return out

    def _list(self, l: int, size: int):
        lo, hi = int(self.offsets[l]), int(self.offsets[l + 1])
        return self.list_movies[lo:lo + max(0, min(int(size), hi - lo))]       # subList(0, size) of a longer list, the list itself otherwise

    @staticmethod
    def _sort(sort_by: str) -> int:
        if sort_by not in SORT_KEYS:
            raise ValueError("sort_by = %r (\"rating\" or \"releaseYear\")" % (sort_by,))
        return SORT_KEYS.index(sort_by)

    def top(self, size: int, sort_by: str = "rating"):
        """``getMovies(size, sortBy)``: the first ``size`` movie ids of the whole catalogue's list, a device tensor."""
        return self._list(self._sort(sort_by) * (self.G + 1) + self.G, size)

    def by_genre(self, genre: str, size: int, sort_by: str = "rating"):
        """``getMoviesByGenre(genre, size, sortBy)``; a genre the dictionary does not know gives an empty list (Java throws)."""
        k = self._sort(sort_by)
        if genre not in self.dictionary:
            return self.list_movies[:0]
        return self._list(k * (self.G + 1) + self.dictionary.index(genre), size)

    def _queries(self, movie_ids):
        import torch
        if hasattr(movie_ids, "detach"):
            q = movie_ids.detach().to(self.device).to(torch.int64).reshape(-1)
        else:
            q = torch.from_numpy(np.asarray(list(movie_ids), dtype=np.int64).reshape(-1)).to(self.device)
        return torch.where((q < 0) | (q >= _ID_LIMIT), torch.full_like(q, -1), q).to(torch.int32).contiguous()

    def similar_device(self, queries, mode: int, top_n: int, extra_n: int, score_kind: int, size: int, width: int):
        """``sprk_catalog_similar`` on an int32 device column of movie ids, enqueued on the current stream; no synchronisation.
        -> ``(ids [Q, width], scores [Q, width] | None, counts [Q])``: device tensors."""
        import ctypes as C

        import torch

        from . import _lib as L
        lib = L.load_library()
        Q, c = int(queries.numel()), self.columns
        with torch.cuda.device(self.device):
            ids = torch.empty((max(Q, 1), width), dtype=torch.int32, device=self.device)
            scores = torch.empty((max(Q, 1), width), dtype=torch.float64, device=self.device) if score_kind else None
            counts = torch.empty(max(Q, 1), dtype=torch.int32, device=self.device)
            p = lambda x: C.c_void_p(None if x is None else x.data_ptr())
            L.check(lib.sprk_catalog_similar(p(queries), Q, self.n_movies, p(c["mask"]), p(c["has"]), p(c["n_genres"]), p(self.avg), self.G,
                                             p(self.list_offsets), p(self.list_movies), int(self.list_movies.numel()), mode, top_n, extra_n, score_kind, size,
                                             p(ids), p(scores), width, p(counts), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return ids[:Q], None if scores is None else scores[:Q], counts[:Q]

    def candidates(self, movie_ids, mode: int = 0, top_n: Optional[int] = None, extra_n: int = 100):
        """The candidate generator alone, for many movies at once -> ``(ids [Q, Cmax] int32 ascending, padded -1; counts [Q])`` on the
        device, where ``EmbRanker.score_many`` and ``model.recommend`` consume them.  ``Cmax`` is :func:`candidate_width`."""
        top_n, extra_n = _heads(top_n, mode), int(extra_n)
        _check_similar_arguments(mode, top_n, extra_n, 0)
        ids, _, counts = self.similar_device(self._queries(movie_ids), mode, top_n, extra_n, 0, 0, candidate_width(self.table._asdict(), mode, top_n, extra_n))
        return ids, counts

    def similar_movies(self, movie_ids, size: int, model: str = "default", mode: int = 0, ranker=None, top_n: Optional[int] = None, extra_n: int = 100,
                       return_scores: bool = False):
        """``SimilarMovieProcess.getRecList`` for many movies at once: per id of ``movie_ids`` the ``size`` best candidates, best first,
        as a list of lists of movie ids; ``[]`` for a movie the catalogue does not hold.  ``model="default"`` is the fused kernel
        (candidates, ``calculateSimilarScore``, the sort); ``model="emb"`` generates the candidates on the device and ranks them with
        ``ranker.score_many`` on ``ranker.row_lut()[candidates]`` -- a candidate, or a query, without an embedding scores -1 and keeps
        candidate order.  ``return_scores=True``: ``(lists, scores)``, the float64 scores as one array per movie.  One copy to the host."""
        import torch
        size = int(size)
        top_n, extra_n = _heads(top_n, mode), int(extra_n)
        _check_similar_arguments(mode, top_n, extra_n, size)
        q = self._queries(movie_ids)
        Q = int(q.numel())
        if model == "default":
            width = max(1, min(size, MAX_CANDIDATES))
            ids, scores, counts = self.similar_device(q, mode, top_n, extra_n, 1, min(size, width), width)
            ids, counts = ids.cpu().numpy(), counts.cpu().numpy()
            lists = [ids[j, :counts[j]].tolist() for j in range(Q)]
            if not return_scores:
                return lists
            scores = scores.cpu().numpy()
            return lists, [scores[j, :counts[j]].copy() for j in range(Q)]
        if model != "emb":
            raise ValueError("model = %r (\"default\" or \"emb\")" % (model,))
        if ranker is None:
            raise ValueError("model=\"emb\" needs the EmbRanker that holds the movie embeddings")
        if Q == 0:
            return ([], []) if return_scores else []
        cand, _ = self.candidates(q, mode, top_n, extra_n)
        lut = ranker.row_lut().to(self.device)
        last = lut.numel() - 1                                                 # (the entry for every id the table does not reach: -1)
        at = lambda ids: torch.where((ids < 0) | (ids >= last), torch.full_like(ids, last), ids).long()
        rows, q_row = lut[at(cand)].contiguous(), lut[at(q)].long()
        q_has = (q_row >= 0).to(torch.uint8) * ranker.has.to(self.device)[q_row.clamp(min=0)]
        s, order = ranker.score_many(ranker.table.to(self.device)[q_row.clamp(min=0)], rows, q_has)
        ranked = torch.gather(cand, 1, order.long())
        ranked_h, s_h = ranked.cpu().numpy(), (torch.gather(s, 1, order.long()).cpu().numpy() if return_scores else None)
        lists, scores = [], []
        for j in range(Q):
            real = ranked_h[j] >= 0                                            # the padding scores -1 like a movie without an embedding: taken out here
            lists.append(ranked_h[j][real][:size].tolist())
            if return_scores:
                scores.append(s_h[j][real][:size].copy())
        return (lists, scores) if return_scores else lists

    def rec_for_you(self, users, size: int, model, store=None, ranker=None, user_emb=None, candidate_size: int = 800):
        """``RecForYouProcess.getRecList`` for many users at once: the candidates are ``top(candidate_size, "rating")``, where they lie on
        the device.  ``model`` a ``CTRModel``: ``model.recommend(store, users, candidates, size)``; ``"emb"``:
        ``ranker.score_many(user_emb.table[users], ..)``; ``"default"``: the candidates' own order cut to ``size``.  Who is a known user
        is the delegate's answer (``store.has_user`` / ``user_emb.has``): an unknown user gets ``[]``."""
        import torch
        users = [int(u) for u in (FE._host_column(users).reshape(-1).tolist() if hasattr(users, "shape") else users)]
        cand = self.top(candidate_size, "rating")
        C = int(cand.numel())
        size = max(0, min(int(size), C))
        if not users or C == 0:
            return [[] for _ in users]
        if isinstance(model, str) and model == "default":
            head = cand[:size].cpu().tolist()
            return [list(head) for _ in users]
        if isinstance(model, str) and model == "emb":
            if ranker is None or user_emb is None:
                raise ValueError("model=\"emb\" needs ranker and user_emb")
            dev = ranker.device
            at = torch.tensor(users, dtype=torch.int64, device=dev)
            inside = (at >= 0) & (at < user_emb.n_users)
            at = torch.where(inside, at, torch.zeros_like(at))
            table, has = torch.as_tensor(user_emb.table).to(dev), torch.as_tensor(user_emb.has).to(dev)
            if user_emb.n_users == 0:
                return [[] for _ in users]
            q_has = has[at] * inside.to(has.dtype)
            lut = ranker.row_lut().to(dev)
            last = lut.numel() - 1
            c = cand.to(dev)
            rows = lut[torch.where(c >= last, torch.full_like(c, last), c).long()]
            _, order = ranker.score_many(table[at], rows[None, :].expand(len(users), C).contiguous(), q_has)
            got = torch.cat([c[order[:, :size].long()].to(torch.int64), q_has.to(torch.int64)[:, None]], dim=1).cpu().numpy()
            return [row[:size].tolist() if row[size] else [] for row in got]
        if isinstance(model, str):
            raise ValueError("model = %r (\"default\", \"emb\" or a CTRModel)" % (model,))
        if store is None:
            raise ValueError("a CTRModel needs the feature store")
        return model.recommend(store, np.asarray(users, dtype=np.int64), cand, size)


def catalog_device(movie_id, rating, columns: dict, G: int, list_capacity: int):
    """``sprk_catalog_build`` on device tensors, enqueued on the current stream; no synchronisation.  ``movie_id`` int32 / ``rating``
    float32 ``[n]``, ``columns`` the table's device columns (``mask`` as int32 bits).  -> ``(avg, rating_count, list_offsets,
    list_movies, error word)``: tensors; the error word (int64, -1 = none) is the caller's to read."""
    import ctypes as C

    import torch

    from . import _lib as L
    lib = L.load_library()
    dev = columns["has"].device
    n, n_movies = int(movie_id.numel()), int(columns["has"].numel()) - 1       # (one spare row each: an empty table still has an address)
    for t, dt in ((movie_id, torch.int32), (rating, torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError("catalog_device takes contiguous int32 / float32 tensors on the table's device")
    L_lists = 2 * (G + 1)
    with torch.cuda.device(dev):
        avg = torch.zeros(n_movies + 1, dtype=torch.float64, device=dev)
        count = torch.zeros(n_movies + 1, dtype=torch.int32, device=dev)
        offsets = torch.zeros(L_lists + 1, dtype=torch.int32, device=dev)
        movies = torch.empty(max(list_capacity, 1), dtype=torch.int32, device=dev)
        word = torch.full((1,), -1, dtype=torch.int64, device=dev)                 # the error word, ~0
        ws_bytes = lib.sprk_catalog_build_workspace_bytes(n, n_movies, list_capacity)
        ws = torch.empty(max(ws_bytes, 16) // 8 + 2, dtype=torch.int64, device=dev)   # (torch's allocations are 512-byte aligned)
        p = lambda x: C.c_void_p(x.data_ptr())
        L.check(lib.sprk_catalog_build(p(movie_id), p(rating), n, n_movies, p(columns["mask"]), p(columns["has"]), p(columns["year"]), p(columns["file_pos"]),
                                       p(columns["hash_pos"]), G, p(avg), p(count), p(offsets), p(movies), list_capacity, p(word), p(ws), ws.numel() * 8,
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return avg[:n_movies], count[:n_movies], offsets, movies[:list_capacity], word


def table_to_device(table: CatalogTable, dev) -> dict:
    """The table's columns as device tensors, one spare row each."""
    import torch
    def up(a, fill):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(np.concatenate([a, np.full(1, fill, dtype=a.dtype)])).to(dev)
    return {"year": up(table.year, 0), "n_genres": up(table.n_genres, 0), "mask": up(table.mask.view(np.int32), 0), "has": up(table.has, 0),
            "file_pos": up(table.file_pos, -1), "hash_pos": up(table.hash_pos, -1)}


def list_total(table: CatalogTable) -> int:
    """The entries of all 2 (G + 1) lists."""
    return 2 * (int(table.n_genres[table.has != 0].astype(np.int64).sum()) + int((table.has != 0).sum()))


def build(ratings, movies, device=None, reference_lines: bool = False) -> Catalog:
    """The catalogue on the device.  ``ratings``: a CSV path or ``{movieId, rating, ..}`` columns, numpy arrays or device tensors
    (tensors on ``device`` are used where they are), in input order; ``movies``: what :func:`catalog_table` takes.  Errors are the
    ``ValueError`` of :func:`catalog_host`.  One host synchronisation: the error word and the lists' offsets."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("catalog.build needs a HIP device: no HIP device is visible (catalog_host is the host definition)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    table = catalog_table(movies, reference_lines)
    if isinstance(ratings, Mapping) and all(hasattr(ratings.get(k), "detach") for k in ("movieId", "rating")):
        m, r = ratings["movieId"].detach().to(dev), ratings["rating"].detach().to(dev)
        if m.dtype.is_floating_point:
            raise TypeError("movieId must be an integer tensor")
        if m.ndim != 1 or m.shape != r.shape:
            raise ValueError("the ratings columns differ in length")
        # (an id beyond int32 must not wrap into range: it becomes -1, which the kernel skips)
        m_d = torch.where((m < 0) | (m >= _ID_LIMIT), torch.full_like(m, -1), m).to(torch.int32).contiguous()
        r_d = r.to(torch.float32).contiguous()
    else:
        m, r = _rating_columns(ratings)
        m_d = torch.from_numpy(np.where((m < 0) | (m >= _ID_LIMIT), -1, m).astype(np.int32)).to(dev)
        r_d = torch.from_numpy(np.ascontiguousarray(r)).to(dev)
    if m_d.numel() >= _ID_LIMIT:
        raise ValueError("at most 2^31 - 2 ratings")
    columns = table_to_device(table, dev)
    avg, count, offsets, list_movies, word = catalog_device(m_d, r_d, columns, len(table.dictionary), list_total(table))
    got = torch.cat([word, offsets.to(torch.int64)]).cpu().numpy()              # the one synchronisation
    err = int(got[0])
    if err != -1:
        raise ValueError(_error_message((err >> 32) & 0xffffffff, err & 0xffffffff))
    return Catalog(table, columns, avg, count, offsets, list_movies, got[1:], dev)
