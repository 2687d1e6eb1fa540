"""New ratings applied to a feature store on the device (sprk_store_update, csrc/k_store_update.h) against the REBUILD from all
ratings so far on the host -- featurestore.row_images_from_samples(featureeng.samples_host(...)) -- the four tables byte for byte after
every update, and the device state against featureeng.update_host's (``-m gpu``).  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import featureeng as FE
from sparrowrecsys_amd import featurestore as FS
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import schema as S
from tests import store_update_cases as SU

pytestmark = pytest.mark.gpu


def _tables(store):
    """The four tables as bytes, the spare last row (which stays zero) cut off."""
    out = []
    for t in store.tensors():
        a = t.cpu().numpy()
        assert not a[-1].any()
        out.append(a[:-1].tobytes())
    return tuple(out)


def _same_state(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))[:8])


def _run(name, hist_len, lib, as_tensors=False):
    """Every batch of the case applied to an empty store: after each update the tables equal the rebuild and state and tables equal
    update_host's.  -> the store."""
    import torch
    c, want, states = SU.case(name), SU.expected(name, hist_len), SU.host_states(name, hist_len)
    store = FS.FeatureStore.empty(c.movies, c.n_users, c.n_movies, hist_len)
    assert store.updatable and store.n_ratings == 0 and (store.n_users, store.n_movies) == (c.n_users, c.n_movies)
    for k, batch in enumerate(c.batches):
        given = {key: torch.from_numpy(v).cuda() for key, v in batch.items()} if as_tensors else batch
        assert store.update(given) == len(batch["userId"])
        for name_, got, w in zip(FE.TABLE_NAMES, _tables(store), want[k]):
            assert got == w, (k, name_)
        _same_state(store._state.to_host(), states[k])
    assert store.n_ratings == sum(len(b["userId"]) for b in c.batches)
    return store


@pytest.mark.parametrize("name,hist_len", SU.RUNS)
def test_every_update_equals_the_rebuild(lib, name, hist_len):
    """tests/test_store_update.py's cases: the synthetic set in 1, 3 and 6 batches (hist_len 5, 1, 100), the hand-built edges -- has flips,
    the ring wrapping twice, 130 new ratings of one user, ties inside a batch and across a boundary, movies flagged late, an empty batch
    -- the genre counters' ties split in two, and ids past 768."""
    _run(name, hist_len, lib)


def test_long_sort_path(lib, monkeypatch):
    """SPRK_FE_SORT_CAP=64: the batches of 99, 129 and 130 new ratings of one user take the chunked sort and a merge pass."""
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    _run("edges", 5, lib)


@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride_loops_past_their_first_round(lib, monkeypatch, cap):
    """SPRK_FE_MAX_GRID: every loop over the batch, over the users and over the movies has more items than cap x 256, and the users
    and movies with work sit past the first round (ids >= 800)."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", str(cap))
    c = SU.case("wide-2")
    for items in [c.n_users, c.n_movies] + [len(b["userId"]) for b in c.batches]:
        assert lib.sprk_segments_grid(items) == cap and items > cap * 256
    assert min(b["userId"].min() for b in c.batches) >= cap * 256 and min(b["movieId"].min() for b in c.batches) >= cap * 256
    _run("wide-2", 5, lib)


def test_two_runs_give_the_same_bytes(lib):
    runs = []
    for _ in range(2):
        store = _run("synthetic-3", 5, lib)
        runs.append([v.tobytes() for v in store._state.to_host().values()])
    assert runs[0] == runs[1]


def test_device_tensors_on_a_side_stream(lib):
    """The batches as device tensors, the update enqueued on a stream that is not the default one."""
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        store = _run("synthetic-3", 5, lib, as_tensors=True)
    side.synchronize()
    assert _tables(store) == SU.expected("synthetic-3", 5)[-1]


def test_from_ratings_updatable_equals_from_ratings(lib):
    c = SU.case("synthetic-3")
    first = SU.concatenation(c.batches[:2])
    plain = FS.FeatureStore.from_ratings(first, c.movies)
    kept = FS.FeatureStore.from_ratings(first, c.movies, updatable=True)
    assert not plain.updatable and kept.updatable and (kept.n_users, kept.n_movies) == (plain.n_users, plain.n_movies)
    assert _tables(kept) == _tables(plain)
    with pytest.raises(RuntimeError, match="not updatable"):
        plain.update(c.batches[2])
    sized = FS.FeatureStore.from_ratings(first, c.movies, n_users=c.n_users, n_movies=c.n_movies, updatable=True)
    assert _tables(sized) == SU.expected("synthetic-3", 5)[1]
    sized.update(c.batches[2])
    assert _tables(sized) == SU.expected("synthetic-3", 5)[2]


@pytest.mark.parametrize("kind", [FE.ERR_USER, FE.ERR_MOVIE, FE.ERR_RATING, FE.ERR_OLDER])
def test_a_failed_update_leaves_every_byte(lib, kind):
    """The error of the host definition, by kind; state and tables as they were; the next batch applies."""
    c = SU.case("edges")
    store = FS.FeatureStore.empty(c.movies, c.n_users, c.n_movies, 5)
    store.update(c.batches[0])
    before = store._state.to_host()
    batch, message = SU.bad_batches(SU.LONG_BATCH_USER, int(before["user_last_ts"][SU.LONG_BATCH_USER]))[kind]
    with pytest.raises(ValueError) as e:
        store.update(batch)
    assert str(e.value) == message
    _same_state(store._state.to_host(), before)
    assert store.n_ratings == len(c.batches[0]["userId"])
    store.update(c.batches[1])
    assert _tables(store) == SU.expected("edges", 5)[1]


def test_tensors_stay_and_has_user_follows(lib):
    c = SU.case("edges")
    store = FS.FeatureStore.empty(c.movies, c.n_users, c.n_movies, 5)
    tensors = store.tensors()
    places = [t.data_ptr() for t in tensors]
    users = [SU.FLIP_USER, SU.NO_FLIP_USER, SU.RING_USER, c.n_users + 3]
    assert store.has_user(users).tolist() == [False, False, False, False]
    store.update(c.batches[0])
    assert store.has_user(users).tolist() == [False, False, True, False]
    store.update(c.batches[1])
    assert store.has_user(users).tolist() == [True, False, True, False]
    assert store.tensors() is tensors and [t.data_ptr() for t in store.tensors()] == places
    assert tuple(a.tobytes() for a in store.images[:4]) == SU.expected("edges", 5)[1]


@pytest.mark.parametrize("cls", [M.DeepFMv2, M.DIN])
def test_predict_pairs_after_an_update_equals_a_rebuilt_store(lib, cls):
    """The join plan is made before the update (the first predict_pairs caches it): the tables it points to are updated in place."""
    c = SU.case("synthetic-3")
    rng = np.random.RandomState(3)
    users, movies = rng.randint(0, c.n_users, 500), rng.randint(0, c.n_movies, 500)
    model, fresh = cls(seed=5), cls(seed=5)
    store = FS.FeatureStore.from_ratings(c.batches[0], c.movies, n_users=c.n_users, n_movies=c.n_movies, updatable=True)
    early = model.predict_pairs(store, users, movies)
    plan = model._join_plan_cache[1]
    for batch in c.batches[1:]:
        store.update(batch)
    rebuilt = FS.FeatureStore.from_ratings(SU.concatenation(c.batches), c.movies, n_users=c.n_users, n_movies=c.n_movies)
    got, want = model.predict_pairs(store, users, movies), fresh.predict_pairs(rebuilt, users, movies)
    assert model._join_plan_cache[1] is plan
    assert got.tobytes() == want.tobytes() and got.tobytes() != early.tobytes()


FILL = 0xA5
GUARD_BYTES = 4096


def _guarded(t, rows):
    """The first `rows` rows of tensor t copied into the middle of an arena of FILL bytes: -> (the arena, the view of the middle)."""
    import torch
    src = t[:rows].contiguous()
    n_bytes = src.numel() * src.element_size()
    arena = torch.full((GUARD_BYTES + n_bytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device=t.device)
    view = arena[GUARD_BYTES:GUARD_BYTES + n_bytes].view(src.dtype).reshape(src.shape)
    view.copy_(src)
    return arena, view


def _is_fill(a):
    return bool((a.cpu().numpy() == FILL).all())


@pytest.mark.parametrize("name,sort_cap", [("edges", 64), ("edges", None), ("wide-2", None)])
def test_nothing_is_written_outside_the_workspace_the_state_or_the_tables(lib, monkeypatch, name, sort_cap):
    """sprk_store_update through ctypes: the workspace is a slice of exactly the advertised length, every state array and every table
    holds exactly n_users / n_movies rows, each between two guard bands that keep their fill; the result is the rebuild all the same."""
    import torch
    if sort_cap is not None:
        monkeypatch.setenv("SPRK_FE_SORT_CAP", str(sort_cap))
    c = SU.case(name)
    state = FE.empty_state(c.movies, c.n_users, c.n_movies, 5, torch.device("cuda", torch.cuda.current_device()))
    rows = [c.n_users] * 4 + [c.n_movies] * 4 + [c.n_users] * 2 + [c.n_movies] * 2
    held = [_guarded(t, n) for t, n in zip(list(state.arrays.values()) + list(state.tables), rows)]
    views = [v for _, v in held]
    p = lambda x: C.c_void_p(x.data_ptr())
    for k, batch in enumerate(c.batches):
        u_d, m_d, r_d, t_d, n, _ = FE._device_rating_columns(batch, state.device)
        ws_bytes = lib.sprk_store_update_workspace_bytes(n, c.n_users, c.n_movies)
        assert ws_bytes > 0 and ws_bytes % 16 == 0
        arena = torch.full((GUARD_BYTES + ws_bytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device=state.device)
        word = torch.tensor([-1], dtype=torch.int64, device=state.device)
        L.check(lib.sprk_store_update(p(u_d), p(m_d), p(r_d), p(t_d), n, c.n_users, c.n_movies, *(p(x) for x in state.movie_dev), S.N_GENRES, 5,
                                      *(p(v) for v in views[:8]), p(views[8]), p(views[9]), FS.user_pitch(5), p(views[10]), p(views[11]),
                                      p(word), C.c_void_p(arena.data_ptr() + GUARD_BYTES), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert int(word.cpu()[0]) == -1
        assert _is_fill(arena[:GUARD_BYTES]) and _is_fill(arena[GUARD_BYTES + ws_bytes:]), k
        for (a, v), (key, _, _) in zip(held, FE.STATE_ARRAYS + [(t, None, None) for t in FE.TABLE_NAMES]):
            n_bytes = v.numel() * v.element_size()
            assert _is_fill(a[:GUARD_BYTES]) and _is_fill(a[GUARD_BYTES + n_bytes:]), (k, key)
        assert tuple(v.cpu().numpy().tobytes() for v in views[8:]) == SU.expected(name, 5)[k]
    want = SU.host_states(name, 5)[-1]
    for v, (key, dt, _) in zip(views[:8], FE.STATE_ARRAYS):
        assert v.cpu().numpy().view(dt).tobytes() == want[key].tobytes(), key
