"""The reference's "emb" ranker on the MI355X: cosine similarity of a user (or movie) embedding against candidate
movies and the ranked candidate list -- `RecForYouProcess.ranker(user, candidates, "emb")`
(RecForYouProcess.java:69-92,100-105), `SimilarMovieProcess.ranker(movie, candidates, "emb")`
(SimilarMovieProcess.java:121-136,167-172), `Embedding.calculateSimilarity` (Embedding.java:33-47).

Host side only parses the reference's embedding files and moves arrays; the scores and the ranking come from
`sprk_emb_rank` (HIP, include/sparrow_hip.h).  There is no CPU fallback: without the library / a GPU it raises.

Recall -- the step in front of the ranker -- is `EmbRanker.topk` / `retrieve` / `similar_movies`: the K table rows closest to a
query over the WHOLE table, exact (`sprk_emb_topk`; `SimilarMovieProcess.retrievalCandidatesByEmbedding`,
SimilarMovieProcess.java:91-112).  `EmbRanker.lsh_index` / `approx_similar_movies` are the approximate recall next to it: the rows that
share an LSH bucket with the query (`lsh.py`, `sprk_lsh_query`; Embedding.embeddingLSH, Embedding.scala:230-252).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


def parse_emb_str(s: str) -> np.ndarray:
    """Utility.parseEmbStr (Utility.java:6-13): whitespace-separated floats."""
    return np.array(s.split(" "), dtype=np.float32)


def load_emb_file(path: str) -> Dict[int, np.ndarray]:
    """`id:f f f ...` per line -- DataManager.loadMovieEmb / loadUserEmb (DataManager.java:92-108,146-162):
    lines that do not split into exactly two parts on ':' are skipped."""
    out: Dict[int, np.ndarray] = {}
    with open(path, "r") as fh:
        for line in fh:
            parts = line.rstrip("\r\n").split(":")
            if len(parts) == 2:
                out[int(parts[0])] = parse_emb_str(parts[1])
    return out


class EmbRanker:
    """Movie embedding table resident in HBM + the ranker over it.

    `movie_emb`: {movieId: vector} (e.g. load_emb_file('item2vecEmb.csv')).  Movies passed as candidates that are
    not in the table score -1.0, like a Movie whose getEmb() is null (Embedding.java:34-37)."""

    def __init__(self, movie_emb: Dict[int, np.ndarray], device: str = "cuda:0"):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("EmbRanker needs an MI355X (no CPU fallback)")
        self._torch = torch
        self._lib = L.load_library()
        self.device = torch.device(device)
        ids = sorted(movie_emb)
        if not ids:
            raise ValueError("empty embedding table")
        self.D = len(movie_emb[ids[0]])
        table = np.zeros((len(ids), self.D), dtype=np.float32)
        has = np.ones(len(ids), dtype=np.uint8)
        for i, m in enumerate(ids):
            v = np.asarray(movie_emb[m], dtype=np.float32)
            if v.shape != (self.D,):
                has[i] = 0                       # size mismatch -> -1 (Embedding.java:35)
            else:
                table[i] = v
        self.row_of = {m: i for i, m in enumerate(ids)}
        self.ids = np.array(ids, dtype=np.int64)                         # movie id of every table row
        self._topk_ws = None
        self._row_lut = None
        self._lsh = {}
        self.table = torch.from_numpy(table).to(self.device)
        self.has = torch.from_numpy(has).to(self.device)

    def rows(self, movie_ids: Iterable[int]) -> np.ndarray:
        return np.array([self.row_of.get(int(m), -1) for m in movie_ids], dtype=np.int32)

    def row_lut(self):
        """`rows` for columns that live on the device: an int32 device tensor of (greatest movie id + 2) entries, entry m = the table
        row of movie m, -1 for a movie the table does not hold; the last entry is -1, for every id beyond it.  Built once.  Dense in
        the id, not in the table: 4 bytes x the greatest movie id (MovieLens: 131 262 -> 0.5 MB); ids above 2^28 (1 GiB of table) raise."""
        if self._row_lut is None:
            ids = self.ids[self.ids >= 0]
            if len(ids) and int(ids.max()) >= 1 << 28:
                raise ValueError("movie id %d: the dense id -> row table would need more than 1 GiB" % int(ids.max()))
            lut = np.full(int(ids.max()) + 2 if len(ids) else 1, -1, dtype=np.int32)
            lut[ids] = np.flatnonzero(self.ids >= 0).astype(np.int32)
            self._row_lut = self._torch.from_numpy(lut).to(self.device)
        return self._row_lut

    @classmethod
    def from_ratings_and_items(cls, item_emb, ratings, n_users: Optional[int] = None, mode: str = "mean", device: str = "cuda:0"):
        """The reference's "emb" route from its two inputs: `item_emb` = {movieId: vector} or the path of an `item2vecEmb.csv`,
        `ratings` = what `userembedding.build` takes -> (ranker, user_embeddings); `user_embeddings.recommend(ranker, users, size)`
        is then the recommendation, with nothing leaving the device in between."""
        from . import userembedding
        ranker = cls(load_emb_file(item_emb) if isinstance(item_emb, str) else item_emb, device=device)
        return ranker, userembedding.build(ratings, ranker, n_users=n_users, mode=mode)

    def score_many(self, query_emb, cand_rows, query_has=None, want_order: bool = True) -> Tuple[object, Optional[object]]:
        """query_emb [Q, D] float32, cand_rows [Q, C] int32 table rows (-1 = no embedding) -- numpy or device tensors.
        Returns (scores [Q, C] float64, order [Q, C] int32 | None) as device tensors."""
        torch = self._torch
        q = torch.as_tensor(query_emb, dtype=torch.float32).to(self.device).contiguous()
        c = torch.as_tensor(cand_rows, dtype=torch.int32).to(self.device).contiguous()
        if q.dim() != 2 or c.dim() != 2 or q.shape[0] != c.shape[0] or q.shape[1] != self.D:
            raise ValueError("query_emb must be [Q, %d] and cand_rows [Q, C]" % self.D)
        qh = None if query_has is None else torch.as_tensor(query_has, dtype=torch.uint8).to(self.device).contiguous()
        Q, Cn = c.shape
        scores = torch.empty((Q, Cn), dtype=torch.float64, device=self.device)
        order = torch.empty((Q, Cn), dtype=torch.int32, device=self.device) if want_order else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(self._lib.sprk_emb_rank(
            C.c_void_p(self.table.data_ptr()), C.c_void_p(self.has.data_ptr()), C.c_int32(self.table.shape[0]), C.c_int32(self.D),
            C.c_int32(self.D), C.c_void_p(q.data_ptr()), C.c_void_p(qh.data_ptr() if qh is not None else None),
            C.c_int32(Q), C.c_int32(self.D), C.c_void_p(c.data_ptr()), C.c_int32(Cn), C.c_void_p(scores.data_ptr()),
            C.c_void_p(order.data_ptr() if order is not None else None), C.c_void_p(stream)))
        return scores, order

    def rank(self, query: Optional[np.ndarray], candidate_ids: Sequence[int]) -> list:
        """ranker(user, candidates, "emb") (RecForYouProcess.java:69-92): the candidate movie ids, best first.
        `query` None = the user has no embedding (every score -1, candidates keep their order)."""
        cand = self.rows(candidate_ids)[None, :]
        if query is None:
            q, qh = np.zeros((1, self.D), dtype=np.float32), np.zeros(1, dtype=np.uint8)
        else:
            q, qh = np.asarray(query, dtype=np.float32)[None, :], np.ones(1, dtype=np.uint8)
            if q.shape[1] != self.D:
                q, qh = np.zeros((1, self.D), dtype=np.float32), np.zeros(1, dtype=np.uint8)    # size mismatch -> -1
        _, order = self.score_many(q, cand, qh)
        ids = list(candidate_ids)
        return [ids[i] for i in order[0].cpu().tolist()]

    # ---- recall: the K closest rows of the whole table (sprk_emb_topk) ----
    TOPK_WORKSPACE_BYTES = 256 << 20

    def topk(self, query_emb, k: int, query_has=None, largest: bool = True) -> Tuple[object, object]:
        """The first `k` entries of every query's ranking of the WHOLE table: query_emb [Q, D] float32 (numpy or a device
        tensor) -> (scores [Q, k] float64, rows [Q, k] int32) as device tensors -- what `score_many(q, arange(N))` gives, cut to
        k, for a table of any size.  largest=False: ascending order (the least similar rows first).  1 <= k <= min(1024, N),
        else SparrowHipError; a wrong shape is a ValueError.

        A table above one chunk of 4 096 rows merges through a workspace this object owns (a cached device tensor that
        grows as needed): 12 bytes x about min(k, 4096) x N / 4096 per query for the first level, 5/4 of it with the next.  The
        queries are walked in tiles of as many as fit TOPK_WORKSPACE_BYTES (256 MiB), one at the least, so the workspace is
        max(256 MiB, one query's need) at the most -- 101 MB per query for 27 M rows at k = 1024."""
        torch = self._torch
        q = torch.as_tensor(query_emb, dtype=torch.float32).to(self.device).contiguous()
        if q.dim() != 2 or q.shape[1] != self.D:
            raise ValueError("query_emb must be [Q, %d]" % self.D)
        Q, N = q.shape[0], self.table.shape[0]
        qh = None if query_has is None else torch.as_tensor(query_has, dtype=torch.uint8).to(self.device).contiguous()
        if qh is not None and tuple(qh.shape) != (Q,):
            raise ValueError("query_has must be [Q]")
        k = int(k)
        kk = k if 1 <= k <= 1024 else 1                                  # (a k the library refuses: it says so below, nothing is written)
        scores = torch.empty((Q, kk), dtype=torch.float64, device=self.device)
        rows = torch.empty((Q, kk), dtype=torch.int32, device=self.device)
        per_query = int(self._lib.sprk_emb_topk_workspace_bytes(N, 1, k))
        tile = max(1, Q if per_query == 0 else min(Q, self.TOPK_WORKSPACE_BYTES // per_query))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for u0 in range(0, Q, tile):
            n = min(tile, Q - u0)
            need = int(self._lib.sprk_emb_topk_workspace_bytes(N, n, k))
            if need and (self._topk_ws is None or self._topk_ws.numel() < need):
                self._topk_ws = None                                     # free before growing
                self._topk_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            L.check(self._lib.sprk_emb_topk(
                C.c_void_p(self.table.data_ptr()), C.c_void_p(self.has.data_ptr()), C.c_int32(N), C.c_int32(self.D), C.c_int32(self.D),
                C.c_void_p(q.data_ptr() + u0 * self.D * 4), C.c_void_p(qh.data_ptr() + u0 if qh is not None else None),
                C.c_int32(n), C.c_int32(self.D), C.c_int32(k), C.c_int32(1 if largest else 0),
                C.c_void_p(scores.data_ptr() + u0 * kk * 8), C.c_void_p(rows.data_ptr() + u0 * kk * 4),
                C.c_void_p(self._topk_ws.data_ptr() if need else None), C.c_size_t(self._topk_ws.numel() if need else 0),
                C.c_void_p(stream)))
        return scores, rows

    def retrieve(self, query: Optional[np.ndarray], size: int, reference_order: bool = False) -> Optional[list]:
        """retrievalCandidatesByEmbedding (SimilarMovieProcess.java:91-112): the `size` movie ids closest to `query` over the
        whole table, best first; None when the query is None or has the wrong length (Java: null for a movie without an
        embedding); `size` is clamped to the table as `subList(0, Math.min(candidates.size(), size))` does.
        reference_order=True is the Java to the letter: it sorts ASCENDING (`comparingByValue()` without reverseOrder, :104)
        and so returns the `size` LEAST similar movies.  The reference scores "the first 10 000 movies by rating" (:96): which
        movies are candidates is the caller's choice of the dict this EmbRanker is built from."""
        n = _retrieve_size(query, size, self.D, len(self.ids))
        if n is None:
            return None
        if n == 0:
            return []
        _, rows = self.topk(np.asarray(query, dtype=np.float32)[None, :], n, largest=not reference_order)
        return self.ids[rows[0].cpu().numpy()].tolist()

    def similar_movies(self, movie_id: int, size: int) -> list:
        """The `size` movies closest to `movie_id`'s own embedding, the movie itself left out (asked for as size + 1 rows and
        dropped on the host, as `candidateMap.remove(movie.getMovieId())` does in the reference's candidate generators); [] for
        a movie the table does not know (getRecList, SimilarMovieProcess.java:22-24)."""
        row = self.row_of.get(int(movie_id))
        if row is None or int(size) <= 0:
            return []
        n = min(int(size) + 1, len(self.ids))
        _, rows = self.topk(self.table[row:row + 1], n, query_has=self.has[row:row + 1])
        out = [int(m) for m in self.ids[rows[0].cpu().numpy()].tolist() if m != int(movie_id)]
        return out[:int(size)]

    # ---- approximate recall: the rows that share an LSH bucket with the query (lsh.py, sprk_lsh_query) ----
    def lsh_index(self, bucket_length: float = 0.1, num_hash_tables: int = 3, seed: int = 0):
        """The :class:`~sparrowrecsys_amd.lsh.LSHIndex` over this table (Embedding.embeddingLSH's configuration by default), built on
        first use and kept per argument triple."""
        from . import lsh
        key = (float(bucket_length), int(num_hash_tables), int(seed))
        if key not in self._lsh:
            self._lsh[key] = lsh.LSHIndex.build(self.table, self.has, bucket_length=key[0], num_hash_tables=key[1], seed=key[2])
        return self._lsh[key]

    def approx_similar_movies(self, movie_id: int, size: int, **index_args) -> list:
        """`similar_movies` through the LSH index (`index_args`: `lsh_index`'s): the movies that share a bucket with `movie_id` in at
        least one hash table, closest first by Euclidean distance, the movie itself left out (asked for as size + 1 rows and dropped on
        the host); [] for a movie the table does not know, and however many candidates the buckets give when that is fewer than
        `size`.  The exact search reads every row of the table for a query; this one reads the rows of the query's buckets."""
        row = self.row_of.get(int(movie_id))
        if row is None or int(size) <= 0:
            return []
        _, rows, _ = self.lsh_index(**index_args).approx_nearest(self.table[row:row + 1], int(size) + 1, query_has=self.has[row:row + 1])
        out = [int(self.ids[r]) for r in rows[0].cpu().tolist() if r >= 0 and r != row]
        return out[:int(size)]


def _retrieve_size(query, size: int, D: int, n_rows: int) -> Optional[int]:
    """How many rows `retrieve` asks for: None = the Java's null (no query embedding / wrong length), else size clamped to
    [0, table rows]."""
    if query is None or np.asarray(query).shape != (D,):
        return None
    return max(0, min(int(size), n_rows))
