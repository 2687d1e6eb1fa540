"""``trainer_tower.train_device`` (``sprk_train_tower_fit``, csrc/k_train_tower.h) against its definition ``trainer_tower.train_host``: every
weight, every ``m``, every ``v``, every ``p`` of the last epoch, accuracy and both AUCs of every epoch byte for byte, the loss within
``metrics_cases.loss_bound``; ``tower_rows_device`` (``sprk_tower_rows``) against ``tower_rows_host`` byte for byte; and the chain samples ->
trained towers -> ``towers`` -> ``predict`` / ``recommend_for_users`` / ``evaluate_ranking`` (``-m gpu``).  Vocabularies of 1 to 60 rows and 1 to a
few hundred samples, except the three larger cases named in their docstrings."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import als as A
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_tower as TT
from tests import metrics_cases as MC
from tests import train_tower_cases as TWC

pytestmark = pytest.mark.gpu
F = np.float32
same = TWC.same_bits
ROUND = 2048 * 256                                                     # FE_MAX_GRID workgroups of 256 threads: what one trip of a strided loop covers


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


def host_of(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def both(fam, w, ids, dense, y, **kw):
    """Host and device fits of one input: asserts the equalities of the module docstring, -> the host's result."""
    want = TT.train_host(fam, w, ids, dense, y, **kw)
    got = TT.train_device(fam, w, ids, dense, y, **kw)
    assert got.step == want.step and len(got.history) == len(want.history)
    for name, g, h in (("weight", got.weights, want.weights), ("m", got.m, want.m), ("v", got.v, want.v)):
        g = host_of(g)
        for k in TT.param_names(fam):
            assert same(g[k], h[k]), (name, k, np.flatnonzero(g[k].reshape(-1).view(np.uint32) != h[k].reshape(-1).view(np.uint32))[:8])
    p = got.p.cpu().numpy()
    assert same(p, want.p), np.flatnonzero(p.view(np.uint32) != want.p.view(np.uint32))[:8]
    for e, (a, b) in enumerate(zip(got.history, want.history)):
        assert a[1:] == b[1:] or (np.isnan(a[2:]).all() and np.isnan(b[2:]).all() and a[1] == b[1]), (e, a, b)
        assert abs(a[0] - b[0]) <= MC.loss_bound(len(y)) * abs(b[0]) or (np.isnan(a[0]) and np.isnan(b[0])), (e, a[0], b[0])
    return want


def moved(got, w, keys):
    return all(not same(got.weights[k], w[k]) for k in keys)


EVERY = ["emb/movieId", "emb/userId", "item0/kernel", "item0/bias", "user0/kernel", "user0/bias", "head/kernel", "head/bias"]


# ---------------------------------------------------------------- rows and batches

@pytest.mark.parametrize("n,batch,tile", [(1, 4, 8), (7, 16, 8), (8, 16, 8), (9, 16, 8), (50, 12, 8), (23, 1, 8), (40, 12, 32), (33, 32, 32)])
def test_row_counts_and_batching(torch, n, batch, tile):
    """N = 1, tile - 1, tile, tile + 1; B no multiple of the tile; a short last batch; B = 1; one batch only; three epochs."""
    fam, w, ids, dense, y = TWC.small(n, seed=n)
    want = both(fam, w, ids, dense, y, batch_size=batch, epochs=3, tile=tile)
    assert want.step == 3 * ((n + batch - 1) // batch) and moved(want, w, ["head/bias", "head/kernel"])


@pytest.mark.parametrize("as_tensor", [False, True])
def test_order(torch, as_tensor):
    fam, w, ids, dense, y = TWC.small(50, seed=4)
    order = np.random.default_rng(1).permutation(50)
    want = TT.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8, order=order)
    plain = TT.train_host(fam, w, ids, dense, y, batch_size=12, epochs=3, tile=8)
    assert not same(want.weights["head/kernel"], plain.weights["head/kernel"])
    dev = lambda a: torch.from_numpy(a).cuda()
    got = TT.train_device(fam, w, dev(ids), dev(dense), dev(y), batch_size=12, epochs=3, tile=8, order=dev(order) if as_tensor else order)
    assert all(same(host_of(got.weights)[k], want.weights[k]) for k in want.weights)
    assert same(got.p.cpu().numpy(), want.p) and [h[1:] for h in got.history] == [h[1:] for h in want.history]
    with pytest.raises(ValueError, match="permutation"):
        TT.train_device(fam, w, ids, dense, y, order=dev(np.zeros(50, dtype=np.int64)) if as_tensor else np.zeros(50, dtype=np.int64))


# ---------------------------------------------------------------- the graph's shapes

@pytest.mark.parametrize("emb_dim", [1, 3, 4, 10, 16, 17, 64, 128])
def test_row_widths(torch, emb_dim):
    fam, w, ids, dense, y = TWC.small(40, seed=20 + emb_dim, emb_dim=emb_dim)
    assert 2 * emb_dim <= T.MAX_X
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert moved(got, w, EVERY)


@pytest.mark.parametrize("hidden", [(1,), (10,), (10, 10), (16,), (17, 5), (3, 256), (256, 3), (6, 5, 4, 3, 4, 5, 6, 7)])
def test_hidden_widths(torch, hidden):
    fam, w, ids, dense, y = TWC.small(40, seed=35 + len(hidden), hidden=hidden)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


def test_a_tile_wider_than_the_workgroup(torch):
    """Tile 300 > 256 threads: every per-sample loop of k_tw_step goes round; N = batch = 300 is one tile."""
    fam, w, ids, dense, y = TWC.small(300, seed=24)
    assert TT.lds_bytes(fam, 300) <= TT.LDS_BYTES
    both(fam, w, ids, dense, y, batch_size=300, epochs=2, tile=300)


def test_a_step_of_more_than_48_kb_of_lds(torch):
    """``emb_dim`` 64 under hidden (256, 256) at tile 8: above the 48 KB a kernel gets without asking; the first tile beyond 160 KB is refused in
    words, with no device call."""
    fam, w, ids, dense, y = TWC.small(40, seed=14, emb_dim=64, hidden=(256, 256))
    assert 48 * 1024 < TT.lds_bytes(fam, 8) <= TT.LDS_BYTES
    both(fam, w, ids, dense, y, batch_size=40, epochs=2, tile=8)
    top = max(t for t in range(1, 200) if TT.lds_bytes(fam, t) <= TT.LDS_BYTES)
    with pytest.raises(ValueError, match="tile = %d needs %d bytes of LDS" % (top + 1, TT.lds_bytes(fam, top + 1))):
        TT.train_device(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=top + 1)


def test_tile_one(torch):
    """Tile 1 on 23 rows in batches of 7: every tile's partial sum is one sample's term."""
    fam, w, ids, dense, y = TWC.small(23, seed=23)
    both(fam, w, ids, dense, y, batch_size=7, epochs=2, tile=1)


def test_every_maximum_at_once(torch):
    """``emb_dim`` 128 (``2 D = MAX_X``) under eight layers of 256 units per tower at the largest tile that fits the LDS, 7: 987 138 Dense
    parameters, so the Dense Adam's loop also goes past one real round of its grid.  20 rows in batches of 12."""
    fam, w, ids, dense, y = TWC.small(20, seed=38, emb_dim=TT.MAX_DIM, hidden=(TT.MAX_WIDTH,) * TT.MAX_LAYERS)
    top = max(t for t in range(1, 64) if TT.lds_bytes(fam, t) <= TT.LDS_BYTES)
    assert top == 7 == TT.default_tile(fam) + 3 and TWC.dense_floats(fam) > ROUND
    both(fam, w, ids, dense, y, batch_size=12, epochs=2, tile=top)


def test_one_more_than_each_maximum_is_refused_in_words(torch):
    fam, w, ids, dense, y = TWC.small(8, seed=1)
    words = "trainer_tower takes 1 to 8 hidden layers of up to 256 units per tower, 2 x emb_dim up to 256"
    for change in (dict(emb_dim=TT.MAX_DIM + 1), dict(hidden=[TT.MAX_WIDTH + 1]), dict(hidden=[2] * (TT.MAX_LAYERS + 1))):
        with pytest.raises(ValueError, match=words):
            TT.train_device(fam._replace(**change), w, ids, dense, y)
        with pytest.raises(ValueError, match=words):
            TT.tower_rows_device(fam._replace(**change), w, "item")


# ---------------------------------------------------------------- ids and values

def test_one_movie_and_one_user_in_every_sample(torch):
    """Every sample carries movie 2 and user 2: one run per column, as long as the batch; every other row keeps its bits."""
    fam, w, ids, dense, y = TWC.small(48, seed=2)
    ids[:] = 2
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    for k, _, vocab in fam.columns:
        keep = np.arange(vocab) != 2
        assert same(got.weights["emb/" + k][keep], w["emb/" + k][keep]) and not same(got.weights["emb/" + k][2], w["emb/" + k][2])


@pytest.mark.parametrize("movies,users", [(1, 5), (7, 1), (1, 1)])
def test_a_vocabulary_of_one(torch, movies, users):
    fam, w, ids, dense, y = TWC.small(40, seed=5, movies=movies, users=users)
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


@pytest.mark.parametrize("side", ["item", "user"])
def test_a_dead_tower(torch, side):
    from tests.test_train_tower import dead
    fam, w, ids, dense, y = TWC.small(40, seed=4)
    w = dead(w, side, 2)
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert all(same(got.weights[k], w[k]) for k in w if k != "head/bias") and not same(got.weights["head/bias"], w["head/bias"])


def test_a_relu_at_exactly_zero(torch):
    fam, w, ids, dense, y = TWC.small(20, seed=5, hidden=(4,))
    w["item0/kernel"][:, 1] = 0
    w["item0/bias"][1] = 0
    got = both(fam, w, ids, dense, y, batch_size=20, epochs=1, tile=8)
    assert same(got.weights["item0/kernel"][:, 1], w["item0/kernel"][:, 1]) and not got.m["user0/kernel"][:, 1].any()


@pytest.mark.parametrize("bias", [100.0, -100.0])
def test_a_saturated_head(torch, bias):
    fam, w, ids, dense, y = TWC.small(40, seed=7)
    w["head/bias"][0] = bias
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert set(np.unique(got.p).tolist()) == ({1.0} if bias > 0 else {0.0}) and set(y.tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("scale", [1e-20, 1e-39])
def test_tiny_and_subnormal_rows(torch, scale):
    fam, w, ids, dense, y = TWC.small(40, seed=8, hidden=(6, 4))
    w = {k: (v.astype(np.float64) * (1.0 if k.startswith("head/") else scale)).astype(F) for k, v in w.items()}
    tiny = np.finfo(F).tiny
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    sub = lambda d: any(((np.abs(a) > 0) & (np.abs(a) < tiny)).any() for a in d.values())
    assert sub(got.m) or sub(got.v) if scale == 1e-20 else sub(w)


def test_a_dot_that_overflows(torch):
    """Identity towers over rows of 1e20: every dot is ``+inf``, ``p`` is 1, a sample of label 1 adds ``inf * 0`` to the head's kernel gradient; from
    the second step on everything is NaN, stored as ``0x7fc00000`` on both sides."""
    from tests.test_train_tower import overflowing
    fam, w, ids, dense, y = overflowing()
    got = both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert (got.p.view(np.uint32) == 0x7fc00000).all()
    for d in (got.weights, got.m, got.v):
        for a in d.values():
            assert (a.view(np.uint32)[np.isnan(a)] == 0x7fc00000).all()
    assert np.isnan(got.weights["head/kernel"]).all() and np.isnan(got.weights["emb/movieId"]).any()


# ---------------------------------------------------------------- grids and the sort

@pytest.mark.parametrize("grid", ["3", "1"])
def test_grids_capped(torch, monkeypatch, grid):
    """SPRK_FE_MAX_GRID 3 and 1 at 500 rows, 60 + 40 rows x 16, hidden (32, 16): every grid-stride loop of the schedule (1 000 entries) and of
    the two Adam kernels goes round (more than 3 x 256 Dense parameters and table elements)."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", grid)
    fam, w, ids, dense, y = TWC.small(500, seed=10, movies=60, users=40, emb_dim=16, hidden=(32, 16))
    assert ids.size > 3 * 256 and TWC.table_floats(fam) > 3 * 256 and TWC.dense_floats(fam) > 3 * 256
    both(fam, w, ids, dense, y, batch_size=200, epochs=1, tile=8)


def test_batches_beyond_the_lds_sort_capacity(torch, monkeypatch):
    """SPRK_FE_SORT_CAP=64: a batch's 40 x 2 entries take the chunked sort and the merge passes."""
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    fam, w, ids, dense, y = TWC.small(100, seed=9)
    both(fam, w, ids, dense, y, batch_size=40, epochs=2, tile=8)


@pytest.mark.parametrize("batch", [56, 64, 72, 136])
def test_tile_counts_around_the_unrolled_partial_sum(torch, batch):
    """Tile 8: 7, 8, 9 and 17 tiles -- the Dense Adam adds eight partials at a time, then the rest -- and a last batch of 5 rows."""
    fam, w, ids, dense, y = TWC.small(batch + 5, seed=batch)
    both(fam, w, ids, dense, y, batch_size=batch, epochs=1, tile=8)


def test_dense_parameters_beyond_one_round_of_a_capped_grid(torch, monkeypatch):
    """Hidden (256, 256): 2 x 66 820 Dense parameters + 2 under a grid capped at 64 workgroups of 256 threads: nine trips of the Dense Adam's loop
    (test_every_maximum_at_once passes one real round)."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", "64")
    fam, w, ids, dense, y = TWC.small(28, seed=39, hidden=(256, 256))
    assert TWC.dense_floats(fam) == 2 * (3 * 256 + 256 + 256 * 256 + 256) + 2 > 8 * 64 * 256
    both(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)


def test_a_user_table_beyond_one_real_round_of_the_grid(torch):
    """60 000 users x 10 behind 7 movies x 10: 600 070 table floats, more than the 524 288 one round of k_tw_table_adam's grid covers.  Step 1
    hits users 0, 52 421, 52 422 and 59 999: elements 524 280 .. 524 299 lie on both sides of the round's end.  Those rows move (the weights are positive, so no unit is off); rows never hit
    keep their bits and zero moments; a row hit in step 1 only still moves in step 3."""
    fam, w, ids, dense, y = TWC.small(40, seed=26, users=60000, emb_dim=10)
    w = {k: np.abs(v) for k, v in w.items()}                                # every unit of both towers is live: every row that is hit moves
    assert TWC.table_floats(fam) > ROUND and 70 + 52421 * 10 < ROUND <= 70 + 52422 * 10
    first = np.array([0, 52421, 52422, 59999])
    ids[:16, 1] = first[np.arange(16) % 4]
    ids[16:, 1] = np.random.default_rng(26).integers(100, 50000, 24)
    one = both(fam, w, ids[:16], dense[:16], y[:16], batch_size=16, epochs=1, tile=8)
    two = both(fam, w, ids[:32], dense[:32], y[:32], batch_size=16, epochs=1, tile=8)
    three = both(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert three.step == 3
    never = np.ones(60000, dtype=bool)
    never[ids[:, 1]] = False
    assert never.sum() > 59900
    for row in first:
        assert not same(one.weights["emb/userId"][row], w["emb/userId"][row]) and not same(three.weights["emb/userId"][row], two.weights["emb/userId"][row])
    assert same(three.weights["emb/userId"][never], w["emb/userId"][never]) and not three.m["emb/userId"][never].any() and not three.v["emb/userId"][never].any()
    assert same(one.weights["emb/userId"][np.setdiff1d(np.arange(60000), first)], w["emb/userId"][np.setdiff1d(np.arange(60000), first)])


def test_batch_4096_at_the_default_tile(torch):
    """The reference shape (1 001 movies, 30 001 users, ``emb_dim`` 10, hidden (10, 10)), N = 4096 + 77, one epoch: one full batch of
    ``DEFAULT_BATCH`` rows at the default tile and a short one."""
    model = M.NeuralCF(seed=3, arch=2)
    fam = TT.family_of(model)
    w = TWC.weights(fam, 21)
    ids, dense, y = TWC.data(fam, TT.DEFAULT_BATCH + 77, 21)
    assert TT.default_tile(fam) == TT.DEFAULT_TILE
    want = both(fam, w, ids, dense, y, epochs=1)
    assert want.step == 2


# ---------------------------------------------------------------- the C ABI: errors, memory, streams

GUARD = 64


def raw_fit(torch, fam, w, ids, y, batch, tile, epochs, stream=None):
    """``sprk_train_tower_fit`` itself: parameters, moments, p and the workspace each inside guard bands of a fixed pattern, the workspace
    exactly as large as ``sprk_train_tower_workspace_bytes`` reports.  -> (rc, params, m, v, p, error word, guards intact)."""
    lib = L.load_library()
    dev = torch.device("cuda")
    n = len(y)
    flat = TT._flatten(fam, w, dev)
    ms = TT._model_struct(fam)
    need = int(lib.sprk_train_tower_workspace_bytes(C.byref(ms), n, batch, tile))
    assert need > 0 and need % 16 == 0

    def banded(count, dtype, fill=None):
        buf = torch.full((count + 2 * GUARD,), 0x5A if dtype == torch.uint8 else -7, dtype=dtype, device=dev)
        if fill is not None:
            buf[GUARD:GUARD + count] = fill
        return buf
    params, m, v = banded(flat.numel(), torch.float32, flat), banded(flat.numel(), torch.float32, 0.0), banded(flat.numel(), torch.float32, 0.0)
    p = banded(max(epochs, 1) * n, torch.float32, 0.0)
    ws = banded(need, torch.uint8)
    steps = (n + batch - 1) // batch
    alphas = torch.from_numpy(np.array([T.adam_alpha(0.001, t + 1) for t in range(epochs * steps)] + [0.0], dtype=F)).to(dev)
    word = torch.full((1,), -1, dtype=torch.int64, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_ids, t_y = up(ids), up(y)
    c1, c2, eps = T.adam_constants()
    at = lambda b, size: C.c_void_p(b.data_ptr() + GUARD * size)
    rc = lib.sprk_train_tower_fit(C.byref(ms), C.c_void_p(t_ids.data_ptr()), C.c_void_p(t_y.data_ptr()), None, n, batch, tile, epochs, C.c_void_p(alphas.data_ptr()),
                                  float(c1), float(c2), float(eps), at(params, 4), at(m, 4), at(v, 4), at(p, 4), C.c_void_p(word.data_ptr()), at(ws, 1), need,
                                  C.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream))
    (stream or torch.cuda.current_stream()).synchronize()
    intact = all(bool((b[:GUARD] == b[0]).all()) and bool((b[-GUARD:] == b[0]).all()) and (float(b[0]) in (-7.0, 90.0)) for b in (params, m, v, p, ws))
    cut = lambda b: b[GUARD:-GUARD].cpu().numpy()
    return rc, cut(params), cut(m), cut(v), cut(p), int(word.cpu()[0]), intact


def test_guard_bands_side_stream_exact_workspace(torch):
    fam, w, ids, dense, y = TWC.small(50, seed=10)
    want = TT.train_host(fam, w, ids, dense, y, batch_size=12, epochs=2, tile=8)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, y, 12, 8, 2, stream=side)
    assert rc == 0 and word == -1 and intact
    assert same(params, TWC.flat(fam, want.weights)) and same(m, TWC.flat(fam, want.m)) and same(v, TWC.flat(fam, want.v))
    assert same(p[50:], want.p)
    lib = L.load_library()
    ms = TT._model_struct(fam)
    need = int(lib.sprk_train_tower_workspace_bytes(C.byref(ms), 50, 12, 8))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    word_t = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    f = torch.zeros(TT.n_params(fam), device="cuda")
    z = C.c_void_p(f.data_ptr())
    rc = lib.sprk_train_tower_fit(C.byref(ms), z, z, None, 50, 12, 8, 1, z, 0.1, 0.001, 1e-7, z, z, z, z, C.c_void_p(word_t.data_ptr()), C.c_void_p(ws.data_ptr()), need - 1, None)
    assert rc == L.EINVAL and b"sprk_train_tower_workspace_bytes" in lib.sprk_last_error()


def test_each_error_word_and_no_parameter_moves(torch):
    fam, w, ids, dense, y = TWC.small(40, seed=11)
    flat0 = TWC.flat(fam, w)

    def check(kind, row, message, ids=ids, y=y):
        rc, params, m, v, p, word, intact = raw_fit(torch, fam, w, ids, y, 16, 8, 2)
        assert rc == 0 and intact and word == (kind << 32 | row), (word >> 32, word & 0xffffffff)
        assert same(params, flat0) and not m.any() and not v.any() and not p.any()
        for fit in (TT.train_device, TT.train_host):
            with pytest.raises(ValueError, match=message):
                fit(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    bad = ids.copy(); bad[30, 0] = 7; bad[12, 1] = -1                       # an id column takes no -1
    check(T.ERR_ID, 12, "samples row 12: an id outside", ids=bad)
    bad = ids.copy(); bad[25, 1] = 5                                        # == the user vocabulary
    check(T.ERR_ID, 25, "samples row 25: an id outside", ids=bad)
    bad = y.copy(); bad[7] = np.nan; bad[39] = -np.inf
    check(T.ERR_LABEL, 7, "samples row 7: the label", y=bad)
    bad_y = y.copy(); bad_y[5] = np.inf
    bad = ids.copy(); bad[30, 0] = 7
    check(T.ERR_ID, 30, "samples row 30: an id outside", ids=bad, y=bad_y)  # the least key: kind 1 at row 30 before kind 3 at row 5


def test_two_fits_give_the_same_bytes_and_a_fit_continues(torch):
    fam, w, ids, dense, y = TWC.small(200, seed=12, hidden=(65, 7))
    a = TT.train_device(fam, w, ids, dense, y, batch_size=48, epochs=2, tile=8)
    b = TT.train_device(fam, w, ids, None, y, batch_size=48, epochs=2, tile=8)
    for x, z in ((a.weights, b.weights), (a.m, b.m), (a.v, b.v)):
        assert all(same(x[k].cpu().numpy(), z[k].cpu().numpy()) for k in x)
    assert same(a.p.cpu().numpy(), b.p.cpu().numpy()) and a.history == b.history
    one = TT.train_device(fam, w, ids, dense, y, batch_size=48, epochs=1, tile=8)
    two = TT.train_device(fam, one.weights, ids, dense, y, batch_size=48, epochs=1, tile=8, state=(one.m, one.v, one.step))
    assert two.step == a.step and all(same(two.weights[k].cpu().numpy(), a.weights[k].cpu().numpy()) and same(two.v[k].cpu().numpy(), a.v[k].cpu().numpy()) for k in w)
    none = TT.train_device(fam, w, ids, dense, y, epochs=0)
    assert none.step == 0 and none.history == [] and all(same(none.weights[k].cpu().numpy(), w[k]) for k in w)


# ---------------------------------------------------------------- tower_rows_device

@pytest.mark.parametrize("grid", [None, "1", "3"])
@pytest.mark.parametrize("rows", [1, 7, 8, 9, 1000])
def test_tower_rows_are_the_definitions_bytes(torch, monkeypatch, rows, grid):
    """Vocabularies of 1, tile - 1, tile, tile + 1 and 1 000 rows at tile 8, both sides, the grid free and capped at 1 and 3 workgroups: 125 tiles
    under a grid of 1 or 3 are many trips of the loop over the tiles."""
    if grid:
        monkeypatch.setenv("SPRK_FE_MAX_GRID", grid)
    fam = TWC.family(movies=rows, users=rows + 2, emb_dim=5, hidden=(9, 6))
    w = TWC.weights(fam, rows)
    for side in ("item", "user"):
        want = TT.tower_rows_host(fam, w, side)
        got = TT.tower_rows_device(fam, w, side, tile=8)
        assert tuple(got.shape) == want.shape == (rows + 2 * (side == "user"), 6) and same(got.cpu().numpy(), want) and want.any()
        assert same(TT.tower_rows_device(fam, w, side).cpu().numpy(), want)          # the default tile


@pytest.mark.parametrize("hidden", [(1,), (17, 5), (3, 256), (256, 3), (6, 5, 4, 3, 4, 5, 6, 7)])
def test_tower_rows_widths(torch, hidden):
    fam = TWC.family(movies=40, users=30, emb_dim=17, hidden=hidden)
    w = TWC.weights(fam, len(hidden))
    for side in ("item", "user"):
        assert same(TT.tower_rows_device(fam, w, side).cpu().numpy(), TT.tower_rows_host(fam, w, side))
    top = max(t for t in range(1, 20000) if TT.rows_lds_bytes(fam, t) <= TT.LDS_BYTES)
    assert same(TT.tower_rows_device(fam, w, "item", tile=top).cpu().numpy(), TT.tower_rows_host(fam, w, "item"))     # above 48 KB of LDS
    with pytest.raises(ValueError, match="tile = %d needs %d bytes of LDS" % (top + 1, TT.rows_lds_bytes(fam, top + 1))):
        TT.tower_rows_device(fam, w, "item", tile=top + 1)


def test_tower_rows_leave_a_wider_stride_and_the_guard_bands_alone(torch):
    fam = TWC.family(movies=21, users=9, emb_dim=4, hidden=(6, 3))
    w = TWC.weights(fam, 3)
    for side, rows in (("item", 21), ("user", 9)):
        buf = torch.full((GUARD + rows * 8 + GUARD,), -7.0, dtype=torch.float32, device="cuda")
        out = buf[GUARD:GUARD + rows * 8].reshape(rows, 8)
        got = TT.tower_rows_device(fam, w, side, out=out, tile=4)
        assert got.data_ptr() == out.data_ptr()
        host = buf.cpu().numpy()
        body = host[GUARD:-GUARD].reshape(rows, 8)
        assert same(body[:, :3], TT.tower_rows_host(fam, w, side)) and (body[:, 3:] == -7).all() and (host[:GUARD] == -7).all() and (host[-GUARD:] == -7).all()
    with pytest.raises(ValueError, match="out must be a float32"):
        TT.tower_rows_device(fam, w, "item", out=torch.zeros((21, 2), device="cuda"))
    with pytest.raises(ValueError, match="neither 'item' nor 'user'"):
        TT.tower_rows_device(fam, w, "movie")


def test_tower_rows_from_a_device_fits_flat_vector(torch):
    """A device fit's ``TrainResult.weights`` are views of one flat vector: ``tower_rows_device`` reads that memory (no copy), and the flat vector
    itself is taken too."""
    fam, w, ids, dense, y = TWC.small(60, seed=13, emb_dim=5, hidden=(9, 6))
    got = TT.train_device(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    flat = TT._flat_view(fam, got.weights, got.weights["emb/movieId"].device)
    assert flat.data_ptr() == got.weights["emb/movieId"].data_ptr() and int(flat.numel()) == TT.n_params(fam)
    host = host_of(got.weights)
    assert same(flat.cpu().numpy(), TWC.flat(fam, host))
    for side in ("item", "user"):
        want = TT.tower_rows_host(fam, host, side)
        assert same(TT.tower_rows_device(fam, got.weights, side).cpu().numpy(), want) and same(TT.tower_rows_device(fam, flat, side).cpu().numpy(), want)
        assert not same(want, TT.tower_rows_host(fam, w, side))
    with pytest.raises(ValueError, match="flat parameter vector"):
        TT.tower_rows_device(fam, flat[:-1], "item")


# ---------------------------------------------------------------- the chain

@pytest.mark.parametrize("seed", [14, 15])
def test_fit_towers_predict_recommend(torch, seed):
    """After a device fit, ``towers(result, seen)``: ``predict(users, movies)`` is the host definition's kept dot bit for bit (seed 14, a positive
    head) or its exact negation (seed 15, a negative head: ``sign = -1``; a dot of +0 stays +0); ``sigmoid_def`` of ``_dense(dot, head)`` is the
    fit's ``p`` on the same weights; ``recommend_for_users(k)`` is ``als.topk_host`` on the host vectors, rows and scores; rows with ``has == 0``
    never appear."""
    fam, w, ids, dense, y = TWC.small(120, seed=seed, movies=30, users=20, emb_dim=6, hidden=(8, 5))
    ids[:, 0] = np.where(ids[:, 0] % 7 == 3, 0, ids[:, 0])                  # movies 3, 10, 17, 24: never seen
    ids[:, 1] = np.where(ids[:, 1] == 11, 12, ids[:, 1])                    # user 11: never seen
    got = TT.train_device(fam, w, ids, dense, y, batch_size=32, epochs=3, tile=8, learning_rate=0.01)
    seen = {"movieId": torch.from_numpy(ids[:, 0]).cuda(), "userId": ids[:, 1]}
    tm = TT.towers(got, seen)
    trained = host_of(got.weights)
    sign = 1 if seed % 2 == 0 else -1
    assert isinstance(tm, A.ALSModel) and tm.sign == sign == TT.head_sign(trained["head/kernel"]) and (tm.n_users, tm.n_items, tm.rank) == (20, 30, 5)
    uf, itf, uh, ih, uc, ic, s = TT.towers_host(fam, trained, {"movieId": ids[:, 0], "userId": ids[:, 1]})
    for a, b in zip(tm.to_host(), (uf, itf, uh, ih, uc, ic)):
        assert a.dtype == b.dtype and same(a, b) if a.dtype == F else np.array_equal(a, b)
    assert not ih[[3, 10, 17, 24]].any() and not uh[11] and ih.sum() == 26 and uh.sum() == 19
    keep = {}
    p = TT.forward_host(fam, trained, ids, dense, keep)
    score = tm.predict(ids[:, 1], ids[:, 0]).cpu().numpy()
    nz = keep["dot"] != 0
    assert np.array_equal(score, sign * keep["dot"]) and same(score[nz], (sign * keep["dot"])[nz]) and nz.sum() > 60
    after = TT.train_device(fam, got.weights, ids, dense, y, batch_size=120, epochs=1, tile=8, learning_rate=0.01)
    assert same(after.p.cpu().numpy(), p) and same(p, T.sigmoid_def(T._dense(keep["dot"][:, None], trained["head/kernel"], trained["head/bias"])[:, 0]))
    assert np.isnan(tm.predict(np.array([11, 0]), np.array([0, 3])).cpu().numpy()).all()
    rec = tm.recommend_for_users(k=4)
    rows, scores = A.topk_host(uf[uh != 0], uh[uh != 0], itf, ih, 4)
    assert np.array_equal(rec.query.cpu().numpy(), np.flatnonzero(uh)) and np.array_equal(rec.ids.cpu().numpy(), rows) and same(rec.scores.cpu().numpy(), scores)
    assert not np.isin(rec.ids.cpu().numpy(), [3, 10, 17, 24]).any() and 11 not in rec.query.cpu().numpy()
    items = tm.recommend_for_items(np.array([0, 3, 5]), k=3)
    rows, scores = A.topk_host(itf[[0, 3, 5]], ih[[0, 3, 5]], uf, uh, 3)
    assert np.array_equal(items.ids.cpu().numpy(), rows) and (rows[1] == -1).all() and 11 not in rows
    free = TT.towers(trained)                                               # a host dict, no seen: every row is a candidate
    assert free.sign == sign and bool(free.user_has.all()) and bool(free.item_has.all()) and not bool(free.item_count.any())
    with pytest.raises(ValueError, match="every pair scores the same"):
        TT.towers(dict(trained, **{"head/kernel": np.zeros((1, 1), dtype=F)}))
    wide = TWC.family(hidden=(5, 17))
    with pytest.raises(ValueError, match="hidden\\[-1\\] = 17"):
        TT.towers(TWC.weights(wide, 0))
    assert tuple(TT.tower_rows_device(wide, TWC.weights(wide, 0), "user").shape) == (5, 17)


def test_the_fitted_model_serves_what_the_towers_score(torch):
    """``model.predict`` of the fitted model (the forward engine) against the definition's ``p`` under the same weights, within 1e-4 absolute -- the
    bound tests/test_gpu_parity.py holds the arch-2 forward to -- and in the order of the towers' dots."""
    model = M.NeuralCF(seed=5, arch=2, emb_dim=6, movie_buckets=30, user_buckets=20, hidden=(8, 5))
    fam = TT.family_of(model)
    ids, dense, y = TWC.data(fam, 150, 5)
    feats = {"movieId": ids[:, 0], "userId": ids[:, 1], "label": y}
    start = {k: v.copy() for k, v in model.weights.items()}
    history = TT.fit(model, feats, batch_size=32, epochs=3, learning_rate=0.01)
    want = TT.train_host(fam, start, ids, dense, y, batch_size=32, epochs=3, learning_rate=0.01)
    assert len(history) == 3 and all(same(model.weights[k], want.weights[k]) for k in want.weights) and [h[1:] for h in history] == [h[1:] for h in want.history]
    p = TT.forward_host(fam, model.weights, ids, dense)
    served = model.predict({"movieId": ids[:, 0], "userId": ids[:, 1]})[:, 0]
    assert float(np.abs(served.astype(np.float64) - p).max()) <= 1e-4 and p.max() - p.min() > 1e-3
    tm = TT.towers(model, {"movieId": ids[:, 0], "userId": ids[:, 1]})
    score = tm.predict(ids[:, 1], ids[:, 0]).cpu().numpy().astype(np.float64)
    order = np.argsort(score, kind="stable")
    assert (np.diff(p[order].astype(np.float64)) >= 0).all()
    again = TT.fit(model, feats, batch_size=32, epochs=1, learning_rate=0.01)                  # continues through model._fit_state
    cont = TT.train_host(fam, want.weights, ids, dense, y, batch_size=32, epochs=1, learning_rate=0.01, state=(want.m, want.v, want.step))
    assert all(same(model.weights[k], cont.weights[k]) for k in cont.weights) and again[0][1:] == cont.history[0][1:]
    with pytest.raises(NotImplementedError, match=r"NeuralCF\(arch=1\) and EmbeddingMLP"):
        model.fit(feats)


def test_ratings_to_ranking_metrics(torch):
    """3 000 structured ratings (tests/train_wide_cases.py): featureeng.build -> split(mode="time") -> trainer_tower.fit(train.columns) ->
    evaluate_device(test.columns), the held-out AUC above its value before the fit -> towers(model, train.columns) -> recommend_for_users ->
    evaluate_ranking(test.columns, train.columns): finite metrics, every list a device tensor."""
    from sparrowrecsys_amd import featureeng as FE
    from sparrowrecsys_amd import rankeval as RE
    from tests import featureeng_cases as cases
    built = FE.build(TWC.structured_ratings(), cases.synthetic_movies(), 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    train, test = built.split(mode="time", sample=1.0)
    model = M.NeuralCF(seed=3, arch=2, movie_buckets=cases.N_MOVIES, user_buckets=cases.N_USERS, hidden=(16, 8))
    auc_before = model.evaluate_device(test.columns)[2]
    history = TT.fit(model, train.columns, batch_size=128, epochs=5, learning_rate=0.01)
    after = model.evaluate_device(test.columns)
    print("held-out AUC %.4f -> %.4f over %d training rows; last epoch %s" % (auc_before, after[2], int(train.columns["label"].numel()), history[-1]))
    assert len(history) == 5 and int(train.columns["label"].numel()) > 2000 and after[2] > auc_before
    tm = TT.towers(model, train.columns)
    assert tm.item_factors.is_cuda and int(tm.user_has.sum()) == 30 and int(tm.item_count.sum()) == int(train.columns["label"].numel())
    rec = tm.recommend_for_users(k=10)
    assert rec.ids.is_cuda and tuple(rec.ids.shape) == (30, 10) and bool((rec.ids >= 0).all()) and bool(tm.item_has[rec.ids.to(torch.int64)].all())
    ev = tm.evaluate_ranking(test.columns, train.columns, ks=(5, 10))
    mean = ev.mean()
    assert ev.per_query.is_cuda and np.isfinite(np.asarray(mean)).all() and 0.0 <= float(mean[1, RE.NDCG]) <= 1.0
