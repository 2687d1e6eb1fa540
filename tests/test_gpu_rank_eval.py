"""Ranking metrics on the device (sprk_rank_eval, csrc/k_rank_eval.h) against the definition, rankeval.rank_eval_host: per_query,
n_relevant, n_ranked, sums and counts BYTE FOR BYTE -- no tolerance anywhere, both routes add the same float64 values in the same
order -- at the list lengths where the rank and the hit count are carried into the next round of a wave, at cut-offs on either side of
the list's and the truth's length, with truth and seen segments on either side of the LDS sort's capacity, at the binary search's
edges, at the chunk edges of the sums, under small grids; strided lists, guard bands, a side stream, the error word; and ALS end to end."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import rankeval as RE
from tests import rank_eval_cases as K

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 4096


def _run(c, ks):
    want = RE.rank_eval_host(ks=ks, **c)
    got = RE.rank_eval_device(ks=ks, **c)
    assert got.per_query.is_cuda and got.sums.is_cuda
    K.same(got.to_host(), want)
    return want


@pytest.mark.parametrize("Lp", [1, 63, 64, 65, 129, 1025])
def test_list_lengths_around_a_round_of_64(lib, Lp):
    """Half the catalogue is truth and a quarter seen, so hits and dropped entries fall in every round: the rank and the hit count are
    carried across one, two and sixteen round edges.  Cut-offs: 1, 64, Lp, Lp + 1 and 1024."""
    n_items = max(2 * Lp, 8)
    c = K.case(Q=24, Lp=Lp, n_users=10, n_items=n_items, per_truth=n_items // 2, per_seen=n_items // 4, seed=Lp)
    ks = sorted({1, min(Lp, 64), min(Lp, 1024), min(Lp + 1, 1024), 1024})
    want = _run(c, ks)
    assert want.n_ranked.max() > min(Lp, 64) // 2
    if Lp > 65:                                                                          # hits past the first round, and dropped entries before them
        assert (want.per_query[:, -1, RE.RECALL] > want.per_query[:, ks.index(64), RE.RECALL]).any() and (want.n_ranked < Lp).any()


@pytest.mark.parametrize("ks", [(6,), (1, 20, 21, 6, 7, 1024, 2, 19)])
def test_cut_offs_on_either_side_of_the_list_and_of_the_truth(lib, ks):
    """Lists of 20 entries, 6 truth items a user: k = 1, Lp, Lp + 1, R, R + 1, 1024; one cut-off and eight."""
    want = _run(K.case(Q=60, Lp=20, per_truth=6, duplicates=False, seed=11), ks)
    assert set(want.n_relevant.tolist()) == {0, 6}


def _segments(sizes_truth, sizes_seen, n_items=400, Lp=130, seed=0):
    """User u has sizes_truth[u] truth items and sizes_seen[u] seen items, rows shuffled, every user queried once and user 2 twice."""
    rng = np.random.default_rng(seed)
    n = len(sizes_truth)
    cols = []
    for sizes in (sizes_truth, sizes_seen):
        u = np.concatenate([np.full(s, i, np.int32) for i, s in enumerate(sizes)] + [np.zeros(0, np.int32)])
        it = np.concatenate([rng.choice(n_items, size=s, replace=False).astype(np.int32) for s in sizes] + [np.zeros(0, np.int32)])
        order = rng.permutation(len(u))
        cols += [u[order], it[order]]
    pred = np.stack([rng.permutation(n_items)[:Lp] for _ in range(n + 1)]).astype(np.int32)
    return dict(pred=pred, query_user=np.array(list(range(n)) + [2], np.int32), truth_user=cols[0], truth_item=cols[1], seen_user=cols[2], seen_item=cols[3], n_users=n)


def test_segments_on_either_side_of_the_lds_sort(lib, monkeypatch):
    """SPRK_FE_SORT_CAP = 64: users with 0, 1, 64, 65 and 200 truth items, and with 200, 65, 64, 1 and 0 seen items, and the reverse --
    segments of 65 and 200 rows take the chunked sort and the merge passes."""
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    sizes = [0, 1, 64, 65, 200]
    for a, b, seed in ((sizes, sizes[::-1], 1), (sizes, sizes, 2), (sizes[::-1], [200] * 5, 3)):
        want = _run(_segments(a, b, seed=seed), (1, 10, 64, 65, 130, 200, 201, 1024))
        assert want.n_relevant.tolist() == a + [a[2]]
    monkeypatch.delenv("SPRK_FE_SORT_CAP")
    _run(_segments(sizes, sizes[::-1], seed=1), (10, 200))


def test_lists_that_are_wholly_seen(lib):
    c = K.case(Q=20, Lp=70, n_users=6, n_items=90, per_truth=30, per_seen=20, seed=21)
    su, si = [c["seen_user"]], [c["seen_item"]]
    for q in (0, 7, 19):                                                     # everything these lists hold is seen by their users
        keep = c["pred"][q][c["pred"][q] >= 0]
        su.append(np.full(len(keep), c["query_user"][q], np.int32)); si.append(keep)
    c = dict(c, seen_user=np.concatenate(su), seen_item=np.concatenate(si))
    want = _run(c, (1, 5, 70))
    assert (want.n_ranked[[0, 7, 19]] == 0).all() and (want.per_query[[0, 7, 19]] == 0.0).all() and want.n_ranked.max() > 0


def test_binary_search_edges_and_the_greatest_item_ids(lib):
    """Entries equal to a segment's first and last key, below and above every key, next to a key on either side; ids up to 2^31 - 1."""
    top = K.TOP_ITEM
    truth = [10, 20, 30, top]
    seen = [5, 15, top - 1]
    pred = np.array([[10, top, 9, 31, 0, top - 1, 5, 15, 4, 16, top + 1, 20, 30, 11, 29, top - 2],
                     [top + 1, top, top - 1, top - 2, 0, 1, 5, 10, 15, 20, 25, 30, 35, 4, 6, 14],
                     [5, 15, top - 1, 5, 15, top - 1, 10, 10, 20, 20, 30, 30, top, top, 9, 9]], dtype=np.int32)
    c = dict(pred=pred, query_user=np.array([1, 1, 1], np.int32), truth_user=np.full(4, 1, np.int32), truth_item=np.array(truth, np.int32),
             seen_user=np.full(3, 1, np.int32), seen_item=np.array(seen, np.int32), n_users=3)
    want = _run(c, (1, 4, 16))
    assert want.n_ranked.tolist() == [13, 13, 10] and want.n_relevant.tolist() == [4, 4, 4]
    assert want.per_query[:, 2, RE.RECALL].tolist() == [1.0, 1.0, 2.0] and want.per_query[2, 2, RE.PRECISION] == 0.5
    one = dict(c, truth_user=np.array([1], np.int32), truth_item=np.array([top + 1], np.int32), seen_user=np.array([1], np.int32), seen_item=np.array([0], np.int32))
    want = _run(one, (16,))
    assert want.per_query[:, 0, RE.HIT].tolist() == [1.0, 1.0, 0.0] and want.n_ranked.tolist() == [15, 15, 16]


@pytest.mark.parametrize("users", ["identity", "random", "beyond"])
def test_query_users(lib, users):
    """query_user NULL and given; one user queried twice; users beyond every rated user."""
    c = K.case(Q=70, users=users, seed=31)
    want = _run(c, (3, 10))
    if users != "identity":
        assert c["query_user"][0] == c["query_user"][-1] and want.n_relevant[0] == want.n_relevant[-1]
    if users == "beyond":
        assert (c["query_user"] > c["truth_user"].max()).any()


@pytest.mark.parametrize("Q", [0, 1, 255, 256, 257, 513])
def test_query_counts_at_the_chunk_edges_of_the_sums(lib, Q):
    want = _run(K.case(Q=Q, Lp=12, seed=Q), (1, 5, 12))
    assert want.counts[0] == Q and want.per_query.shape == (Q, 3, 6)
    if Q > 1:
        assert 0 < want.counts[1] < Q and (want.sums[:, RE.HIT] > 0).all()


def test_empty_truth_and_empty_seen(lib):
    c = K.case(Q=50, seed=41)
    e = np.zeros(0, np.int32)
    want = _run(dict(c, truth_user=e, truth_item=e), (5,))
    assert want.counts.tolist() == [50, 0] and (want.sums == 0.0).all()
    _run(dict(c, seen_user=e, seen_item=e), (5,))
    _run(dict(c, seen_user=None, seen_item=None), (5,))
    _run(dict(c, truth_user=e, truth_item=e, seen_user=None, seen_item=None), (5,))


@pytest.mark.parametrize("grid", [1, 3])
def test_small_grids(lib, monkeypatch, grid):
    """513 queries and a few thousand pairs with one workgroup and with three: every grid-stride loop goes past its first round."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", str(grid))
    _run(K.case(Q=513, Lp=70, n_users=300, n_items=120, per_truth=10, per_seen=20, seed=51), (1, 10, 70))


# ---------------------------------------------------------------- the raw call: layout, guard bands, errors

def _is_fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def _raw(lib, torch, c, ks, stride, stream=None, word=-1):
    """sprk_rank_eval on arenas of fill: GUARD bytes on both sides of every output and of a workspace of exactly the reported length; the
    lists at a row stride of `stride` with item 7 in the gap.  -> the arenas on the host, the sizes."""
    Q, Lp = c["pred"].shape
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    wide = np.full((Q, stride), 7, dtype=np.int32)                            # item 7 in the gap: a hit or a miss if it were read
    wide[:, :Lp] = c["pred"]
    pred, qu, tu, ti, su, si = (dev(a) for a in (wide, c["query_user"], c["truth_user"], c["truth_item"], c["seen_user"], c["seen_item"]))
    gain, gain_sum = (dev(a) for a in RE.gain_table())
    n_truth, n_seen = len(c["truth_user"]), (0 if c["seen_user"] is None else len(c["seen_user"]))
    ws_bytes = lib.sprk_rank_eval_workspace_bytes(n_truth, n_seen, c["n_users"], Q)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    sizes = {"per_query": Q * len(ks) * 48, "n_relevant": Q * 4, "n_ranked": Q * 4, "sums": len(ks) * 48, "counts": 16, "word": 8, "ws": ws_bytes}
    mem = {name: torch.full((GUARD + b + GUARD,), FILL, dtype=torch.uint8, device="cuda") for name, b in sizes.items()}
    mem["word"][GUARD:GUARD + 8] = torch.from_numpy(np.array([word], np.int64).view(np.uint8).copy()).cuda()
    at = lambda name: C.c_void_p(mem[name].data_ptr() + GUARD)
    p = lambda t: C.c_void_p(None if t is None or not t.numel() else t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    L.check(lib.sprk_rank_eval(p(pred), Q, Lp, stride, p(qu), p(tu), p(ti), n_truth, p(su), p(si), n_seen, c["n_users"], (C.c_int32 * len(ks))(*ks), len(ks), p(gain), p(gain_sum),
                               at("per_query"), at("n_relevant"), at("n_ranked"), at("sums"), at("counts"), at("word"), at("ws"), ws_bytes, s))
    torch.cuda.synchronize()
    return {name: a.cpu().numpy() for name, a in mem.items()}, sizes


def _body(host, sizes, name, dtype):
    return host[name][GUARD:GUARD + sizes[name]].view(dtype)


@pytest.mark.parametrize("Lp,stride", [(65, 66), (20, 64), (129, 1000)])
def test_strided_lists_and_nothing_written_outside(lib, monkeypatch, Lp, stride):
    import torch
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    c = K.case(Q=300, Lp=Lp, n_users=40, n_items=150, per_truth=20, per_seen=80, seed=61)
    ks = (1, 7, Lp)
    host, sizes = _raw(lib, torch, c, ks, stride)
    for name, b in sizes.items():
        assert _is_fill(host[name][:GUARD]) and _is_fill(host[name][GUARD + b:]), name
    want = RE.rank_eval_host(ks=ks, **c)
    assert _body(host, sizes, "word", np.int64).tolist() == [-1]
    for name, dtype in (("per_query", np.float64), ("n_relevant", np.int32), ("n_ranked", np.int32), ("sums", np.float64), ("counts", np.int64)):
        assert _body(host, sizes, name, dtype).tobytes() == getattr(want, name).tobytes(), name
    ws_bytes = sizes["ws"]
    buf = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert lib.sprk_rank_eval(p, 300, Lp, stride, None, p, p, len(c["truth_user"]), p, p, len(c["seen_user"]), c["n_users"], (C.c_int32 * 1)(5), 1, p, p, p, p, p, p, p, p, p,
                              ws_bytes - 1, None) == L.EINVAL
    assert str(ws_bytes).encode() in lib.sprk_last_error()


def test_every_error_kind_leaves_the_outputs_untouched(lib):
    """The error word names the smallest (kind, row); per_query, n_relevant, n_ranked, sums and counts keep their fill.  An error word
    that is already set when the call starts stays as it is, with nothing written either."""
    import torch
    c = K.case(Q=300, Lp=12, seed=71)
    n = c["n_users"]
    def broken(name, rows, value):
        a = c[name].copy()
        a[rows] = value
        return dict(c, **{name: a})
    for case, word, want in ((broken("truth_user", [150, 31], n), -1, 1 << 32 | 31), (broken("truth_item", [77], -1), -1, 1 << 32 | 77),
                             (broken("seen_user", [9, 200], -1), -1, 2 << 32 | 9), (broken("seen_item", [123], -4), -1, 2 << 32 | 123),
                             (broken("query_user", [299, 258], n), -1, 3 << 32 | 258), (dict(broken("query_user", [4], -1), seen_item=broken("seen_item", [60], -1)["seen_item"]), -1, 2 << 32 | 60),
                             (c, 0, 0), (c, 5 << 32 | 1, 5 << 32 | 1)):
        host, sizes = _raw(lib, torch, case, (3, 10), 12, word=word)
        assert _body(host, sizes, "word", np.int64).tolist() == [want]
        for name in ("per_query", "n_relevant", "n_ranked", "sums", "counts"):
            assert _is_fill(host[name]), name
        assert _is_fill(host["ws"][:GUARD]) and _is_fill(host["ws"][GUARD + sizes["ws"]:])
    with pytest.raises(ValueError, match="error kind 3, query 258:"):
        RE.rank_eval_device(ks=(3,), **broken("query_user", [299, 258], n))
    with pytest.raises(ValueError, match="error kind 1, truth row 31:"):
        RE.rank_eval_device(ks=(3,), **broken("truth_user", [150, 31], n))


def test_side_stream(lib):
    """The call is enqueued behind a spin of some milliseconds on a side stream; its own synchronisation (the error word) waits for it."""
    import torch
    c = K.case(Q=513, Lp=70, n_users=300, n_items=120, per_truth=10, per_seen=20, seed=51)
    dev = {k: (v if v is None or isinstance(v, int) else torch.from_numpy(v).cuda()) for k, v in c.items()}
    torch.cuda.synchronize()
    side, done = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(40_000_000)
        got = RE.rank_eval_device(ks=(1, 10, 70), **dev)
        done.record(side)
    done.synchronize()
    K.same(got.to_host(), RE.rank_eval_host(ks=(1, 10, 70), **c))


def test_twenty_calls_give_the_same_bytes(lib):
    c = K.case(Q=513, Lp=70, n_users=300, n_items=120, per_truth=10, per_seen=20, seed=51)
    runs = set()
    for _ in range(20):
        got = RE.rank_eval_device(ks=(1, 10, 70), **c).to_host()
        runs.add(got.per_query.tobytes() + got.sums.tobytes() + got.n_ranked.tobytes())
    assert len(runs) == 1


# ---------------------------------------------------------------- end to end

def test_als_fit_then_evaluate_ranking(lib):
    """A few hundred users: als.fit(train) -> evaluate_ranking(test, train) equals the definition on the copied lists; device tensors
    and a strided view as columns; lists_as_truth gives recall 1.0 of lists against themselves."""
    import torch

    from sparrowrecsys_amd import als
    rng = np.random.default_rng(5)
    n_users, n_items, n = 300, 80, 6000
    ratings = {"userId": rng.integers(0, n_users, n).astype(np.int32), "movieId": rng.integers(0, n_items, n).astype(np.int32),
               "rating": (rng.integers(1, 11, n) / 2).astype(np.float32)}
    train, test = als.split(ratings, (0.8, 0.2), seed=1)
    model = als.fit(train, rank=4, iters=2, n_users=n_users, n_items=n_items)
    got = model.evaluate_ranking(test, train, ks=(1, 10, 80))
    users = np.unique(test["userId"][test["rating"] >= 3.5])
    lists = model.recommend_for_users(users, n_items).ids.cpu().numpy()
    keep = test["rating"] >= 3.5
    want = RE.rank_eval_host(lists, users, test["userId"][keep], test["movieId"][keep], train["userId"], train["movieId"], ks=(1, 10, 80))
    K.same(got.to_host(), want)
    assert want.counts.tolist() == [len(users), len(users)] and (want.n_ranked < n_items).all() and 0.0 < got.mean()[1, RE.NDCG] <= 1.0
    short = model.evaluate_ranking({k: torch.from_numpy(v).cuda() for k, v in test.items()}, None, ks=(5,), list_len=20)
    K.same(short.to_host(), RE.rank_eval_host(lists[:, :20], users, test["userId"][keep], test["movieId"][keep], ks=(5,)))
    tu, ti = RE.lists_as_truth(torch.from_numpy(lists[:, :10]).cuda())
    again = RE.rank_eval_device(torch.from_numpy(lists).cuda()[:, :10], None, tu, ti, ks=(10,))
    assert again.mean("truth")[0, RE.RECALL] == 1.0 and again.mean("truth")[0, RE.NDCG] == 1.0
