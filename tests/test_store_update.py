"""New ratings applied to a feature store on the host (featureeng.update_host behind FeatureStore.empty / update with device="cpu")
against the REBUILD from all ratings so far, the four tables byte for byte after every update."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import featureeng as FE
from sparrowrecsys_amd import featurestore as FS
from tests import store_update_cases as SU


def _table_bytes(store):
    return tuple(a.tobytes() for a in store.images[:4])


def _all_bytes(store):
    return {k: v.tobytes() for k, v in store._state.to_host().items()}


@pytest.mark.parametrize("name,hist_len", SU.RUNS)
def test_every_update_equals_the_rebuild(name, hist_len):
    """The synthetic set in 1, 3 and 6 batches (hist_len 5, 1, 100), the hand-built edges (an empty batch among them) and
    featureeng_cases.all_genres_ratings' ties split in two."""
    c, want = SU.case(name), SU.expected(name, hist_len)
    store = FS.FeatureStore.empty(c.movies, c.n_users, c.n_movies, hist_len, device="cpu")
    assert store.updatable and store.n_ratings == 0 and not store.images.user_has.any() and not store.images.movie_has.any()
    applied = 0
    for k, batch in enumerate(c.batches):
        assert store.update(batch) == len(batch["userId"])
        applied += len(batch["userId"])
        assert store.n_ratings == applied
        for name_, got, w in zip(FE.TABLE_NAMES, _table_bytes(store), want[k]):
            assert got == w, (k, name_)


@pytest.mark.parametrize("hist_len", [5, 100])
def test_from_ratings_updatable_equals_from_ratings(hist_len):
    """empty + update(all), from_ratings(updatable=True) and plain from_ratings: the same bytes, the default table sizes included;
    the updatable one then takes a further batch."""
    c = SU.case("synthetic-3")
    first, rest = SU.concatenation(c.batches[:2]), c.batches[2]
    plain = FS.FeatureStore.from_ratings(first, c.movies, hist_len, device="cpu")
    kept = FS.FeatureStore.from_ratings(first, c.movies, hist_len, device="cpu", updatable=True)
    assert not plain.updatable and kept.updatable and kept.n_ratings == len(first["userId"])
    assert (kept.n_users, kept.n_movies) == (plain.n_users, plain.n_movies)
    assert _table_bytes(kept) == _table_bytes(plain)
    sized = FS.FeatureStore.from_ratings(first, c.movies, hist_len, device="cpu", n_users=c.n_users, n_movies=c.n_movies, updatable=True)
    empty = FS.FeatureStore.empty(c.movies, c.n_users, c.n_movies, hist_len, device="cpu")
    empty.update(first)
    assert _table_bytes(sized) == _table_bytes(empty) == SU.expected("synthetic-3", hist_len)[1]
    sized.update(rest)
    assert _table_bytes(sized) == SU.expected("synthetic-3", hist_len)[2]


def test_edges_do_what_their_names_say():
    """What tests/store_update_cases.py edges_batches promises, so that test_every_update_equals_the_rebuild covers it: user_has
    flips at 3 ratings and not at 2, the ring user's counts, a movie first flagged by an update, a movie counted at dropped positions
    only that keeps its NA row until it is flagged, a movie outside the movie table."""
    states, at = SU.host_states("edges", 5), SU.EDGES_AFTER
    b = [states[at[k]] for k in ("b1", "b2", "b3", "b4")]
    assert [int(s["user_count"][SU.RING_USER]) for s in b] == SU.RING_COUNTS
    assert [int(s["user_count"][SU.LONG_BATCH_USER]) for s in b] == [5, 5, 5, 135]
    assert [int(s["user_has"][SU.FLIP_USER]) for s in b[:2]] == [0, 1] and [int(s["user_count"][SU.FLIP_USER]) for s in b[:2]] == [2, 3]
    assert [int(s["user_has"][SU.NO_FLIP_USER]) for s in b[:2]] == [0, 0] and [int(s["user_count"][SU.NO_FLIP_USER]) for s in b[:2]] == [1, 2]
    assert [int(s["movie_has"][SU.FLAGGED_LATER]) for s in b[:2]] == [0, 1] and [int(s["movie_count"][SU.FLAGGED_LATER]) for s in b[:2]] == [1, 2]
    assert [int(s["movie_count"][SU.DROPPED_ONLY]) for s in b] == SU.DROPPED_ONLY_COUNTS
    assert [int(s["movie_has"][SU.DROPPED_ONLY]) for s in b] == [0, 0, 0, 1] == [int(s["movie_flag"][SU.DROPPED_ONLY]) for s in b]
    na = np.array([-1, -1, -1, 0, 0, 0, 0, 0], dtype=np.int32)
    assert all(np.array_equal(s["movie_rows"][SU.DROPPED_ONLY], na) for s in b[:3])
    assert b[3]["movie_rows"][SU.DROPPED_ONLY, 4:5].view(np.float32)[0] == 4.0                   # the grown count, once flagged
    table = SU.case("edges").movies
    assert SU.OUTSIDE_TABLE >= len(table.has) and b[3]["movie_has"][SU.OUTSIDE_TABLE] == 1
    assert b[3]["movie_rows"][SU.OUTSIDE_TABLE, 3:4].view(np.float32)[0] == FE.DEFAULT_YEAR
    one = SU.concatenation(SU.case("edges").batches)
    assert set(one["timestamp"][one["userId"] == SU.ONE_STAMP_USER]) == {777}
    assert states[at["empty"]].keys() == states[at["b2"]].keys() and all(np.array_equal(states[at["empty"]][k], states[at["b2"]][k]) for k in states[0])


@pytest.fixture()
def edges_store():
    c = SU.case("edges")
    store = FS.FeatureStore.empty(c.movies, c.n_users, c.n_movies, 5, device="cpu")
    store.update(c.batches[0])
    return store


@pytest.mark.parametrize("kind", [FE.ERR_USER, FE.ERR_MOVIE, FE.ERR_RATING, FE.ERR_OLDER])
def test_a_failed_update_changes_nothing(edges_store, kind):
    """Each error kind names the first of its two wrong rows; state and tables keep their bytes, and the store still takes the next batch."""
    latest = int(edges_store._state.user_last_ts[SU.LONG_BATCH_USER])
    batch, message = SU.bad_batches(SU.LONG_BATCH_USER, latest)[kind]
    before = _all_bytes(edges_store)
    with pytest.raises(ValueError) as e:
        edges_store.update(batch)
    assert str(e.value) == message
    assert _all_bytes(edges_store) == before and edges_store.n_ratings == len(SU.case("edges").batches[0]["userId"])
    edges_store.update(SU.case("edges").batches[1])
    assert _table_bytes(edges_store) == SU.expected("edges", 5)[1]


def test_the_least_kind_wins_over_the_least_row(edges_store):
    latest = int(edges_store._state.user_last_ts[SU.LONG_BATCH_USER])
    batch = SU.bad_batches(SU.LONG_BATCH_USER, latest)[FE.ERR_OLDER][0]
    batch = dict(batch, movieId=np.array([1, 3, 5, -2]))                      # row 1 is older (kind 4), row 3 names no movie (kind 2)
    with pytest.raises(ValueError, match="ratings row 3: movieId outside the movie table"):
        edges_store.update(batch)
    same = dict(batch, movieId=np.array([1, 3, 5, 7]), timestamp=np.array([latest + 10**6, latest, latest + 10**6, latest]))
    assert edges_store.update(same) == 4                                      # (a timestamp EQUAL to the latest is in order)


def test_update_takes_a_csv_path(tmp_path):
    c = SU.case("synthetic-3")
    store = FS.FeatureStore.empty(c.movies, c.n_users, c.n_movies, 5, device="cpu")
    for k, batch in enumerate(c.batches):
        path = tmp_path / ("batch%d.csv" % k)
        with open(path, "w") as f:
            f.write("userId,movieId,rating,timestamp\n")
            for row in zip(*(batch[key].tolist() for key in FE.RATING_KEYS)):
                f.write("%d,%d,%s,%d\n" % row)
        store.update(str(path))
    assert _table_bytes(store) == SU.expected("synthetic-3", 5)[-1]


def test_only_updatable_stores_update():
    c = SU.case("synthetic-1")
    samples = FE.samples_host(c.batches[0], c.movies)
    for store in (FS.FeatureStore.from_ratings(c.batches[0], c.movies, device="cpu"), FS.FeatureStore.from_samples(samples, device="cpu"),
                  FS.FeatureStore.from_feature_maps({1: {"userGenre1": 2}}, {3: {"releaseYear": 1999}}, device="cpu")):
        assert not store.updatable
        with pytest.raises(RuntimeError, match="not updatable"):
            store.update(c.batches[0])
        with pytest.raises(RuntimeError, match="not updatable"):
            store.n_ratings


def test_the_total_stays_below_builds_limit(edges_store):
    edges_store._state.n_ratings = 2**31 - 1 - 4
    batch = SU.bad_batches(SU.LONG_BATCH_USER, 10**7)[FE.ERR_USER][0]         # (four rows; the limit is checked first)
    before = _all_bytes(edges_store)
    with pytest.raises(ValueError, match=r"at most 2\^31 - 2 ratings"):
        edges_store.update(batch)
    assert _all_bytes(edges_store) == before


def test_state_bytes_and_capacities():
    c = SU.case("edges")
    store = FS.FeatureStore.empty(c.movies, c.n_users, c.n_movies, 5, device="cpu")
    per_user, per_movie = 4 + 8 + 100 * 4 + 100, 4 + 8 + 8 + 1                # count, latest timestamp, ring; n, S, Q, flag
    assert store._state.state_bytes() == c.n_users * per_user + c.n_movies * per_movie == sum(v.nbytes for k, v in store._state.arrays.items())
    with pytest.raises(ValueError, match="does not fit a table of 100 rows"):
        FS.FeatureStore.empty(c.movies, c.n_users, 100, 5, device="cpu")     # (the movie table's greatest id is 119)
    with pytest.raises(ValueError, match="hist_len"):
        FS.FeatureStore.empty(c.movies, c.n_users, c.n_movies, 101, device="cpu")


def test_new_symbols_in_header_map_list_and_library(lib):
    names = ["sprk_store_update_workspace_bytes", "sprk_store_update"]
    header = open(os.path.join(L.INCLUDE_DIR, "sparrow_hip.h")).read()
    assert re.search(r"\bsize_t\s+sprk_store_update_workspace_bytes\(int64_t n_new, int32_t n_users, int32_t n_movies\);", header)
    assert re.search(r"\bint\s+sprk_store_update\(const int32_t\* user_id,", header)
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    patterns = re.findall(r"global:\s*([^;]+);", open(os.path.join(os.path.dirname(L.SRC_PATH), "exports.map")).read())
    for name in names:
        assert name in exported and name in L.EXPORTED_SYMBOLS
        assert any(fnmatch.fnmatch(name, p.strip()) for p in patterns)
    # no device call: sizes the call rejects give 0, and the workspace grows with each of the three sizes
    ws = lib.sprk_store_update_workspace_bytes
    assert ws(-1, 10, 10) == 0 and ws(10, -1, 10) == 0 and ws(2**31 - 1, 10, 10) == 0
    assert 0 < ws(0, 0, 0) and ws(0, 0, 0) % 16 == 0
    assert ws(1000, 40, 150) < ws(2000, 40, 150) and ws(1000, 40, 150) < ws(1000, 4000, 150) and ws(1000, 40, 150) < ws(1000, 40, 15000)
