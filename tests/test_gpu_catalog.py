"""The movie catalogue on the device (sprk_catalog_build, sprk_catalog_similar, csrc/k_catalog.h) against its definition,
catalog.catalog_host / similar_host: averages, counts, lists, candidates, scores and rankings byte for byte -- on both routes of the
grouping (input grouped by movie: walked where it lies; any other input: scattered and sorted by input row), on both sides of the
lane-per-movie / wave-per-movie switch and of the LDS sort capacity -- and the calls built on them."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import catalog as CT
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import ranker as R
from sparrowrecsys_amd import userembedding as UE
from sparrowrecsys_amd.featurestore import FeatureStore
from tests import catalog_cases as cases
from tests import featurestore_cases as FC

pytestmark = pytest.mark.gpu


def _assert_same(got: dict, want: dict):
    for k in CT.HOST_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert g.tobytes() == w.tobytes(), (k, np.flatnonzero(g != w)[:8])
    assert got["dictionary"] == want["dictionary"]


@pytest.fixture(scope="module")
def synthetic(lib):
    out = {}
    for grouped in (False, True):
        ratings, movies, info = cases.synthetic(grouped=grouped)
        out[grouped] = (ratings, movies, info, CT.catalog_host(ratings, movies))
    return out


@pytest.mark.parametrize("sort_cap", [None, cases.SORT_CAP])
@pytest.mark.parametrize("grouped", [False, True])
def test_synthetic_set_equals_the_host_definition(synthetic, monkeypatch, grouped, sort_cap):
    """tests/test_catalog.py asserts what the set holds: movies of 0, 1, 2, 64, 65, 127, 128, 129 and 700 ratings, their rows interleaved
    with all others' (64 / 65: the LDS sort's capacity and one past it at SPRK_FE_SORT_CAP = 64; 127 / 128 / 129: around the switch to a
    wave per movie), genre lists of 0, 1, 64, 65, 99, 100 and 101 members, ratings on ids outside the table and on movies it does not
    hold, and movies whose average is not sum / n."""
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    ratings, movies, info, want = synthetic[grouped]
    got = CT.build(ratings, movies).to_host()
    _assert_same(got, want)
    for m, n in info["fixed"].items():
        assert got["rating_count"][m] == n and got["avg"][m] == cases.loop_average(ratings["rating"][ratings["movieId"] == m]), (m, n)


@pytest.mark.parametrize("sort_cap", [None, cases.SORT_CAP])
def test_every_movie_unrated_and_few_distinct_averages(lib, monkeypatch, sort_cap):
    """No rating at all: every average is 0.0 and the rating lists are the tie order alone; whole ratings 1 .. 3 on one-rating movies:
    three distinct averages over 300 movies."""
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    ratings, movies, info = cases.synthetic(rated=False)
    got = CT.build(ratings, movies).to_host()
    _assert_same(got, CT.catalog_host(ratings, movies))
    assert not got["avg"].any() and not got["rating_count"].any()
    ids = info["ids"]
    ratings = {"movieId": ids, "rating": (1 + np.arange(len(ids)) % 3).astype(np.float32)}
    _assert_same(CT.build(ratings, movies).to_host(), CT.catalog_host(ratings, movies))


def test_hand_worked_catalogue_and_the_list_calls(lib):
    import torch
    cat = CT.build(cases.HAND_RATINGS, cases.HAND_MOVIES)
    _assert_same(cat.to_host(), CT.catalog_host(cases.HAND_RATINGS, cases.HAND_MOVIES))
    for (genre, sort_by), want in cases.HAND_LISTS.items():
        for size in (0, 2, len(want), 100):
            got = cat.top(size, sort_by) if genre is None else cat.by_genre(genre, size, sort_by)
            assert got.is_cuda and got.dtype == torch.int32 and got.cpu().tolist() == want[:size], (genre, sort_by, size)
    assert cat.by_genre("Western", 10).numel() == 0 and cat.by_genre("No such genre", 10).numel() == 0
    with pytest.raises(ValueError):
        cat.top(10, "title")
    for (q, mode, extra_n, size), (want, scores) in cases.HAND_SIMILAR.items():
        lists, got = cat.similar_movies([q], size, mode=mode, extra_n=extra_n, return_scores=True)
        assert lists == [want], (q, mode)
        if scores is not None:
            assert got[0].tobytes() == np.array(scores, dtype=np.float64).tobytes(), (q, mode)
    twelve = CT.build({"movieId": [1] * 12, "rating": cases.TWELVE}, {"movieId": [1], "title": ["Toy Story (1995)"], "genres": ["Comedy"]}).to_host()
    assert float(twelve["avg"][1]).hex() == cases.TWELVE_AVG_HEX and twelve["rating_count"][1] == 12


def test_skipped_ratings_change_no_byte(synthetic):
    """Without the rows on ids that are negative, past the table, or of movies the table does not hold, every byte is the same."""
    ratings, movies, info, want = synthetic[False]
    table = CT.catalog_table(movies)
    m = ratings["movieId"]
    inside = (m >= 0) & (m < len(table.has))
    skipped = ~(inside & (table.has[np.where(inside, m, 0)] != 0))
    assert (m < 0).sum() == 100 and (m >= len(table.has)).sum() >= 100 and skipped.sum() == 300
    _assert_same(CT.build({k: v[~skipped] for k, v in ratings.items()}, movies).to_host(), want)
    import torch
    on_device = {k: torch.from_numpy(v).cuda() for k, v in ratings.items()}
    _assert_same(CT.build(on_device, movies).to_host(), want)                   # device columns are used where they lie


def _raw_build(ratings, movies, fill=None, guard_rows=0, guard_bytes=0, capacity=None):
    """sprk_catalog_build through ctypes on buffers of the test's making -> the outputs and the arena as numpy arrays, the error word."""
    import torch
    lib = L.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    table = CT.catalog_table(movies)
    cols = CT.table_to_device(table, dev)
    m, r = CT._rating_columns(ratings)
    m_d, r_d = torch.from_numpy(m.astype(np.int32)).to(dev), torch.from_numpy(r).to(dev)
    n, nm, G = len(m), len(table.has), len(table.dictionary)
    total = CT.list_total(table) if capacity is None else capacity
    def filled(count, dtype):
        n_bytes = count * torch.empty(0, dtype=dtype).element_size()
        return torch.full((max(n_bytes, 8),), 0 if fill is None else fill, dtype=torch.uint8, device=dev).view(dtype)
    avg, count = filled(nm + guard_rows, torch.float64), filled(nm + guard_rows, torch.int32)
    offsets, lists = filled(2 * (G + 1) + 1 + guard_rows, torch.int32), filled(total + guard_rows, torch.int32)
    word = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ws_bytes = lib.sprk_catalog_build_workspace_bytes(n, nm, total)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    arena = torch.full((guard_bytes + ws_bytes + guard_bytes,), 0 if fill is None else fill, dtype=torch.uint8, device=dev)
    assert arena.data_ptr() % 16 == 0 and guard_bytes % 16 == 0
    p = lambda x: C.c_void_p(x.data_ptr())
    L.check(lib.sprk_catalog_build(p(m_d), p(r_d), n, nm, p(cols["mask"]), p(cols["has"]), p(cols["year"]), p(cols["file_pos"]), p(cols["hash_pos"]), G, p(avg), p(count),
                                   p(offsets), p(lists), total, p(word), C.c_void_p(arena.data_ptr() + guard_bytes), ws_bytes,
                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    err = int(word.cpu()[0])
    out = {"avg": avg.cpu().numpy(), "rating_count": count.cpu().numpy(), "list_offsets": offsets.cpu().numpy(), "list_movies": lists.cpu().numpy()}
    return out, arena.cpu().numpy(), err, (nm, 2 * (G + 1) + 1, total, ws_bytes)


def test_a_rating_that_is_not_finite_sets_the_error_word_to_the_lowest_bad_row(synthetic):
    ratings, movies, info, want = synthetic[False]
    bad = {k: v.copy() for k, v in ratings.items()}
    rows = [4000, 123, 2500]
    bad["rating"][rows] = [np.nan, np.inf, -np.inf]
    out, _, err, (nm, n_off, total, _) = _raw_build(bad, movies)
    assert (err >> 32, err & 0xffffffff) == (CT.ERR_RATING, 123)
    keep = np.ones(len(bad["rating"]), dtype=bool)
    keep[rows] = False
    clean = CT.catalog_host({k: v[keep] for k, v in bad.items()}, movies)       # the bad rows took no part
    assert out["avg"][:nm].tobytes() == clean["avg"].tobytes() and out["rating_count"][:nm].tobytes() == clean["rating_count"].tobytes()
    with pytest.raises(ValueError) as device:
        CT.build(bad, movies)
    with pytest.raises(ValueError) as host:
        CT.catalog_host(bad, movies)
    assert str(device.value) == str(host.value) == "ratings row 123: the rating is not finite"
    out, _, err, _ = _raw_build(ratings, movies, capacity=total - 1)            # lists that do not fit: reported, every list empty
    assert (err >> 32) == CT.ERR_LISTS and not out["list_offsets"].any() and (out["list_movies"][:total - 1] == -1).all()


FILL = 0xA5
GUARD_ROWS, GUARD_BYTES = 64, 4096


def _is_fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


@pytest.mark.parametrize("grouped,sort_cap", [(False, cases.SORT_CAP), (False, None), (True, None)])
def test_nothing_is_written_outside_the_outputs_or_the_workspace(synthetic, monkeypatch, grouped, sort_cap):
    """Guard bands of a fill pattern after the four outputs and on both sides of a workspace of exactly the advertised length keep
    their fill; every output row is written."""
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    ratings, movies, info, want = synthetic[grouped]
    out, arena, err, (nm, n_off, total, ws_bytes) = _raw_build(ratings, movies, fill=FILL, guard_rows=GUARD_ROWS, guard_bytes=GUARD_BYTES)
    assert err == -1
    assert _is_fill(arena[:GUARD_BYTES]) and _is_fill(arena[GUARD_BYTES + ws_bytes:])
    for k, rows in (("avg", nm), ("rating_count", nm), ("list_offsets", n_off), ("list_movies", total)):
        assert _is_fill(out[k][rows:]) and len(out[k]) == rows + GUARD_ROWS, k
        assert out[k][:rows].tobytes() == want[k].tobytes(), k


def test_two_runs_give_the_same_bytes(synthetic):
    ratings, movies, info, want = synthetic[False]
    runs = [{k: v.tobytes() for k, v in _raw_build(ratings, movies)[0].items()} for _ in range(2)]
    assert runs[0] == runs[1]


def test_side_stream_and_no_synchronisation(synthetic):
    """Both calls are enqueued behind a spin of some milliseconds on a side stream and return while the stream is still busy; the event
    recorded after them orders the read."""
    import torch
    ratings, movies, info, want = synthetic[False]
    table = CT.catalog_table(movies)
    dev = torch.device("cuda", torch.cuda.current_device())
    cols = CT.table_to_device(table, dev)
    m_d = torch.from_numpy(ratings["movieId"].astype(np.int32)).to(dev)
    r_d = torch.from_numpy(ratings["rating"]).to(dev)
    queries = torch.from_numpy(info["ids"].astype(np.int32)).to(dev)
    want_similar = CT.similar_host(want, info["ids"], size=10)
    torch.cuda.synchronize()
    side, done = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(40_000_000)
        avg, count, offsets, lists, word = CT.catalog_device(m_d, r_d, cols, len(table.dictionary), CT.list_total(table))
        cat = CT.Catalog(table, cols, avg, count, offsets, lists, want["list_offsets"], dev)
        ids, scores, counts = cat.similar_device(queries, 0, 100, 100, 1, 10, 10)
        done.record(side)
        returned_early = not done.query()
    done.synchronize()
    assert returned_early
    assert int(word.cpu()[0]) == -1
    _assert_same(cat.to_host(), want)
    for g, w in zip((ids, scores, counts), want_similar):
        assert g.cpu().numpy().tobytes() == w.tobytes()


# ---- candidates and the default ranker ----

def _similar_equals_host(cat, host, queries, mode, size, top_n=None, extra_n=100):
    import torch
    top = CT._heads(top_n, mode)
    q = cat._queries(queries)
    want = CT.similar_host(host, queries, size=size, mode=mode, top_n=top_n, extra_n=extra_n)
    ids, scores, counts = cat.similar_device(q, mode, top, extra_n, 1, size, max(size, 1))
    ids, scores = ids[:, :size], scores[:, :size]
    for name, g, w in zip(("ids", "scores", "counts"), (ids, scores, counts), want):
        g = np.ascontiguousarray(g.cpu().numpy())
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, mode, size, np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))[:8])
    want = CT.similar_host(host, queries, mode=mode, top_n=top_n, extra_n=extra_n, model="candidates")
    cand, counts = cat.candidates(queries, mode, top_n, extra_n)
    cand, counts = cand.cpu().numpy(), counts.cpu().numpy()
    assert cand.dtype == np.int32 and cand.tobytes() == want[0].tobytes() and counts.tobytes() == want[2].tobytes(), (mode, "candidates")
    for row, n in zip(cand, counts):
        assert (np.diff(row[:n]) > 0).all() and (row[n:] == -1).all()            # ascending, padded with -1
    return want[2]


@pytest.fixture(scope="module")
def built(synthetic):
    ratings, movies, info, want = synthetic[False]
    return CT.build(ratings, movies), want, info


@pytest.mark.parametrize("mode", [0, 1])
def test_similar_movies_of_the_synthetic_set(built, mode):
    """Every movie of the set, ids the table does not hold and ids outside it: Q = 345, then Q = 257, 1 and 0; sizes 0, 1 and more than any
    count."""
    cat, host, info = built
    everyone = np.concatenate([np.arange(-2, cases.N_TABLE + 2), [2**31 - 2]])
    for size in (0, 1, 10, 4096):
        _similar_equals_host(cat, host, everyone, mode, size)
    _similar_equals_host(cat, host, everyone[:257], mode, 10)
    _similar_equals_host(cat, host, info["ids"][:1], mode, 10)
    _similar_equals_host(cat, host, info["ids"][:0], mode, 10)
    _similar_equals_host(cat, host, info["ids"], mode, 10, top_n=3, extra_n=7)
    _similar_equals_host(cat, host, info["ids"], mode, 10, top_n=0, extra_n=0)
    assert cat.similar_movies([int(info["ids"][0]), -5, cases.N_TABLE + 9], 10, mode=mode)[1:] == [[], []]


@pytest.mark.parametrize("mode", [0, 1])
def test_candidate_counts_around_the_powers_of_two(lib, mode):
    """Mode-0 candidate counts of 0, 1, 2, 63, 64, 65, 1 024 and 1 025 (tests/test_catalog.py asserts them); the 1 024 / 1 025 queries are
    outside the heads of ten of their genres and inside the head of the eleventh."""
    ratings, movies, queries = cases.counts_table()
    host = CT.catalog_host(ratings, movies)
    cat = CT.build(ratings, movies)
    _assert_same(cat.to_host(), host)
    counts = _similar_equals_host(cat, host, list(queries.values()), mode, 2000)
    if mode == 0:
        assert counts.tolist() == list(queries)
    _similar_equals_host(cat, host, np.flatnonzero(host["has"])[::7], mode, 20)


@pytest.mark.parametrize("mode", [0, 1])
def test_a_query_with_all_32_genres(lib, mode):
    """32 lists' heads of 100: 3 200 gathered entries in mode 0; 32 x 20 + 200 by default in mode 1, and 32 x 100 + 200 = 3 400 with
    top_n = 100; the most the call takes: 32 x 125 + 2 x 48 = 4 096."""
    ratings, movies, query = cases.all_genres_table()
    host = CT.catalog_host(ratings, movies)
    cat = CT.build(ratings, movies)
    _assert_same(cat.to_host(), host)
    some = [query] + np.flatnonzero(host["has"])[:40].tolist()
    _similar_equals_host(cat, host, some, mode, 1000)
    _similar_equals_host(cat, host, some, mode, 1000, top_n=100, extra_n=100)
    _similar_equals_host(cat, host, some, mode, 1000, top_n=125, extra_n=48)
    with pytest.raises(ValueError):
        cat.candidates(some, mode, top_n=125, extra_n=49)


def test_emb_model_equals_the_ranker_over_the_hosts_candidates(built):
    """Two movies in three have an embedding: a candidate without one scores -1 and keeps candidate order, and so does every candidate of
    a query without one."""
    cat, host, info = built
    rng = np.random.RandomState(9)
    with_emb = [int(m) for k, m in enumerate(info["ids"]) if k % 3]
    ranker = R.EmbRanker({m: rng.standard_normal(10).astype(np.float32) for m in with_emb})
    table = ranker.table.cpu().numpy()
    queries = info["ids"][:24].tolist() + [-1, cases.N_TABLE + 5]
    for mode in (0, 1):
        cand, _, counts = CT.similar_host(host, queries, mode=mode, model="candidates")
        got = cat.similar_movies(queries, 15, model="emb", mode=mode, ranker=ranker)
        for j, q in enumerate(queries):
            mine = cand[j, :counts[j]].tolist()
            vec = table[ranker.row_of[q]] if q in ranker.row_of else None
            assert got[j] == (ranker.rank(vec, mine)[:15] if mine else []), (mode, q)
    assert any(q not in ranker.row_of for q in queries[:24]) and cat.similar_movies([], 5, model="emb", ranker=ranker) == []
    with pytest.raises(ValueError):
        cat.similar_movies(queries, 5, model="emb")


def test_rec_for_you_equals_the_existing_calls_on_the_hosts_top_800(built):
    import torch
    cat, host, info = built
    G, off = len(host["dictionary"]), host["list_offsets"]
    top = host["list_movies"][off[G]:off[G + 1]][:800]
    assert len(top) == cases.N_HELD and cat.top(800).cpu().numpy().tobytes() == top.tobytes()
    assert cat.rec_for_you([3, 4], 10, "default") == [top[:10].tolist()] * 2 and cat.rec_for_you([3], 1000, "default") == [top.tolist()]
    assert cat.rec_for_you([3], 10, "default", candidate_size=4) == [top[:4].tolist()] and cat.rec_for_you([], 10, "default") == []
    # "emb": users 0 .. 19 rate the set's movies; user 20 rates nothing
    rng = np.random.RandomState(3)
    ranker = R.EmbRanker({int(m): rng.standard_normal(10).astype(np.float32) for k, m in enumerate(info["ids"]) if k % 3})
    ratings = {"userId": rng.randint(0, 20, 600), "movieId": info["ids"][rng.randint(0, cases.N_HELD, 600)], "rating": np.full(600, 4.0), "timestamp": np.arange(600)}
    user_emb = UE.build(ratings, ranker, n_users=21)
    users = [0, 7, 20, -1, 21, 19]
    got = cat.rec_for_you(users, 12, "emb", ranker=ranker, user_emb=user_emb)
    for u, mine in zip(users, got):
        vec = user_emb.vector(u)
        assert mine == ([] if vec is None else ranker.rank(vec, top.tolist())[:12]), u
    # a CTRModel: the store of the feature-store cases (movie ids below the set's 340 are in its range)
    store = FeatureStore.from_samples(FC.samples())
    try:
        model = M.NeuralCF(seed=7)
        users = FC.pairs(8, seed=3)[0][:5].copy()
        users[3] = FC.pairs(8, seed=2)[0][-3]                                   # no row in the store: an empty list
        assert cat.rec_for_you(users, 10, model, store=store) == model.recommend(store, users, top, 10)
        assert cat.rec_for_you(users, 10, model, store=store, candidate_size=50) == model.recommend(store, users, top[:50], 10)
    finally:
        store.close()
