"""The held-out split on the device (sprk_split_plan / sprk_take_rows, csrc/k_split.h) against its definition, featureeng.split_host:
every column of both parts, the three counts and split_timestamp BYTE FOR BYTE -- no tolerance anywhere -- at the edges of a tile and
of a workgroup's rows, past one round of every grid-stride loop, at every fraction's ends, on the timestamp patterns a radix select
can go wrong on, with every kind of key; sprk_take_rows on its own; guard bands, the workspace exactly as reported, a side stream, the
error word; and build -> split -> fit -> evaluate_device end to end."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import featureeng as FE
from tests import split_cases as K

pytestmark = pytest.mark.gpu

_columns = {}


def _cols(n, seed=0, ts="random", key="shuffled"):
    """The columns of a shape, made once and left unchanged."""
    k = (n, seed, ts, key)
    if k not in _columns:
        _columns[k] = K.columns(n, seed, ts, key)
    return _columns[k]


def _host(res):
    return FE.SplitResult({k: v.cpu().numpy() for k, v in res.train.items()}, {k: v.cpu().numpy() for k, v in res.test.items()}, res.n_sampled, res.split_timestamp)


def _run(cols, **kw):
    want = FE.split_host(cols, **kw)
    got = _host(FE.split_device(cols, **kw))
    K.same_split(got, want)
    return want


@pytest.mark.parametrize("mode", ["random", "time"])
@pytest.mark.parametrize("n", K.SIZES)
def test_sizes_at_the_edges_of_a_tile_and_of_a_workgroup(lib, mode, n):
    """n = 0 and 1; one less than, exactly and one more than the 256 rows a workgroup takes a round and the 1024 rows of a tile.  At the
    reference's fractions and with every row sampled (the lists are then as long as they can be)."""
    _run(_cols(n), mode=mode)
    want = _run(_cols(n), mode=mode, sample=1.0, seed=5)
    assert want.n_sampled == n


@pytest.mark.parametrize("mode", ["random", "time"])
@pytest.mark.parametrize("grid", [1, 3])
def test_three_tiles_and_a_row_under_a_small_grid(lib, monkeypatch, mode, grid):
    """3 * 1024 + 1 rows with one workgroup and with three: every grid-stride loop goes past its first round, the tile loops too."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", str(grid))
    want = _run(_cols(3 * K.TILE + 1), mode=mode, sample=0.5)
    assert len(want.train["label"]) > K.TILE and len(want.test["label"]) > 0
    _run(_cols(3 * K.TILE + 1, ts="ties"), mode=mode, sample=1.0)


@pytest.mark.parametrize("mode", ["random", "time"])
@pytest.mark.parametrize("n", [65_537, 512 * K.TILE + 1])
def test_past_65536_rows_and_past_one_tile_of_the_scan(lib, mode, n):
    """65 537 rows; 512 tiles and a row: 1027 tile counts, more than the 1024 that one tile of the scan over them holds."""
    want = _run(_cols(n), mode=mode)
    assert abs(want.n_sampled - 0.1 * n) <= 4 * (n * 0.09) ** 0.5


@pytest.mark.parametrize("mode", ["random", "time"])
@pytest.mark.parametrize("sample,train", [(0.0, 0.8), (1.0, 0.0), (1.0, 1.0), (0.1, 0.0), (0.1, 1.0), (0.0, 0.0), (0.1, 0.8)])
def test_fractions_at_their_ends(lib, mode, sample, train):
    """Nothing sampled; everything in one part; an empty part.  (Time mode with train = 0: the earliest timestamp and its ties are training.)"""
    want = _run(_cols(3 * K.TILE + 1, ts="ties"), mode=mode, sample=sample, train=train, seed=2)
    n_train, n_test = len(want.train["label"]), len(want.test["label"])
    if sample == 0.0:
        assert want.n_sampled == 0 and want.split_timestamp is None
    elif train == 1.0:
        assert n_train == want.n_sampled > 0 and n_test == 0
    elif train == 0.0:
        assert (n_train == 0) == (mode == "random") and n_test > 0


@pytest.mark.parametrize("ts", ["equal", "bit63", "top_byte", "low_byte", "extremes", "ties"])
@pytest.mark.parametrize("sample", [0.1, 1.0])
def test_timestamps_for_the_select(lib, ts, sample):
    """All equal; values that differ only in bit 63, only in the top byte, only in the lowest byte; INT64_MIN and INT64_MAX present; ties."""
    cols = _cols(5000, seed=3, ts=ts)
    want = _run(cols, mode="time", sample=sample)
    _run(cols, mode="time", sample=sample, train=0.5, seed=11)
    if ts == "extremes":
        assert cols["timestamp"].min() == K.INT64_MIN and cols["timestamp"].max() == K.INT64_MAX
        low, high = _run(cols, mode="time", sample=1.0, train=0.0), _run(cols, mode="time", sample=1.0, train=1.0)
        assert low.split_timestamp == K.INT64_MIN and high.split_timestamp == K.INT64_MAX
    if ts == "bit63":
        assert want.split_timestamp in (5, 5 + K.INT64_MIN)


def test_two_values_with_the_rank_on_either_side_and_one_sampled_row(lib):
    """1000 rows, all sampled, train 0.8: the rank is position 799 -- the last 100 of 800, the first 200 after 799."""
    for n_low, stamp in ((800, 100), (799, 200)):
        cols = dict(_cols(1000, seed=7))
        cols["timestamp"] = K.two_values(1000, n_low)
        assert _run(cols, mode="time", sample=1.0).split_timestamp == stamp
    cols = _cols(40, seed=8)
    seed = next(s for s in range(200) if FE.split_host(cols, mode="time", sample=0.03, seed=s).n_sampled == 1)
    want = _run(cols, mode="time", sample=0.03, seed=seed)
    assert len(want.train["label"]) == 1 and want.split_timestamp == int(want.train["timestamp"][0])


@pytest.mark.parametrize("mode", ["random", "time"])
def test_keys(lib, mode):
    """source_row shuffled (the other tests), the position, an int64 key column beyond 2^32, an int32 key of 2^31 - 2, another column as the key."""
    import torch
    cols = _cols(3000, seed=4)
    _run(cols, mode=mode, sample=0.3, key=None)
    wide = _cols(3000, seed=4, key="wide")
    assert wide["source_row"].dtype == np.int64 and wide["source_row"].min() > 1 << 32
    _run(wide, mode=mode, sample=0.3)
    top = dict(cols, source_row=cols["source_row"].copy())
    top["source_row"][[0, 1500, 2999]] = (1 << 31) - 2
    _run(top, mode=mode, sample=0.3, seed=(1 << 63) + 7)
    _run(cols, mode=mode, sample=0.3, key="userId", seed=(1 << 64) - 1)
    # device tensors are used where they are, strided views too
    dev = {k: torch.from_numpy(v).cuda() for k, v in cols.items()}
    matrix = torch.stack([dev["userId"], dev["movieId"], dev["label"]], dim=1)
    dev["userId"], dev["movieId"], dev["label"] = matrix[:, 0], matrix[:, 1], matrix[:, 2]
    K.same_split(_host(FE.split_device(dev, mode=mode, sample=0.3)), FE.split_host(cols, mode=mode, sample=0.3))


def test_a_negative_key_in_a_device_column_is_reported(lib):
    import torch
    cols = _cols(3000, seed=4)
    dev = {k: torch.from_numpy(v).cuda() for k, v in cols.items()}
    dev["source_row"] = dev["source_row"].clone()
    dev["source_row"][[2100, 777]] = -5
    with pytest.raises(ValueError, match="row 777: negative key"):
        FE.split_device(dev)


def test_twenty_calls_give_the_same_lists(lib):
    cols = _cols(65_537)
    runs = set()
    for _ in range(20):
        res = FE.split_device(cols, mode="time", sample=0.5)
        runs.add(res.train["source_row"].cpu().numpy().tobytes() + res.test["source_row"].cpu().numpy().tobytes())
    assert len(runs) == 1


# ---------------------------------------------------------------- sprk_take_rows on its own

FILL = 0xA5
GUARD = 4096


def _is_fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def _arena(torch, n_bytes, shift=0):
    """A device buffer of fill with GUARD bytes on both sides of n_bytes that start `shift` bytes past a 16-byte boundary."""
    a = torch.full((GUARD + shift + n_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert a.data_ptr() % 16 == 0
    return a


@pytest.mark.parametrize("words,pitch", [(1, 1), (2, 2), (7, 7), (8, 8), (1, 8), (2, 5), (7, 10), (8, 12), (4, 4), (4, 6)])
@pytest.mark.parametrize("shift", [0, 4, 8])
def test_take_rows_widths_strides_and_alignment(lib, words, pitch, shift):
    """Rows of 4, 8, 28 and 32 bytes (and 16), dense and as columns of a wider matrix (a stride of 16 bytes' multiple and not), into
    destinations on a 16-byte boundary and 4 and 8 bytes past one; an index with repeats, 1001 long (the last unit of 16 bytes is short)."""
    import torch
    n_rows, n_index = 700, 1001
    rng = np.random.default_rng(words * 100 + pitch)
    src = rng.integers(-2**31, 2**31 - 1, (n_rows, pitch), dtype=np.int64).astype(np.int32)
    index = rng.integers(0, n_rows, n_index).astype(np.int32)
    index[:6] = [5, 5, 5, 0, n_rows - 1, 5]
    src_d, index_d = torch.from_numpy(src).cuda(), torch.from_numpy(index).cuda()
    first = pitch - words                                                     # the column's first word within the matrix row
    dst = _arena(torch, n_index * words * 4, shift)
    desc = (L.SplitCol * 1)(L.SplitCol(src_d.data_ptr() + first * 4, pitch * 4, words * 4, 0, dst.data_ptr() + GUARD + shift))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.sprk_take_rows(desc, 1, C.c_void_p(index_d.data_ptr()), n_index, n_rows, stream))
    got = dst.cpu().numpy()
    body = got[GUARD + shift:GUARD + shift + n_index * words * 4]
    assert body.tobytes() == np.ascontiguousarray(src[index][:, first:]).tobytes()
    assert _is_fill(got[:GUARD + shift]) and _is_fill(got[GUARD + shift + n_index * words * 4:])


def test_take_rows_many_columns_an_empty_index_and_an_index_outside_the_source(lib):
    """40 columns in one call (more than one launch holds), of 4 and 8 bytes; no index at all; an index outside [0, n_rows) leaves its row unwritten."""
    import torch
    n_rows, n_index = 300, 257
    rng = np.random.default_rng(5)
    index = rng.integers(0, n_rows, n_index).astype(np.int32)
    srcs = [rng.integers(0, 1 << 30, n_rows).astype(np.int32 if c % 3 else np.int64) for c in range(40)]
    src_d, index_d = [torch.from_numpy(s).cuda() for s in srcs], torch.from_numpy(index).cuda()
    dst = [_arena(torch, n_index * s.itemsize) for s in srcs]
    desc = (L.SplitCol * 40)(*(L.SplitCol(s.data_ptr(), s.element_size(), s.element_size(), 0, d.data_ptr() + GUARD) for s, d in zip(src_d, dst)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.sprk_take_rows(desc, 40, C.c_void_p(index_d.data_ptr()), n_index, n_rows, stream))
    for s, d in zip(srcs, dst):
        got = d.cpu().numpy()
        assert got[GUARD:GUARD + n_index * s.itemsize].tobytes() == s[index].tobytes() and _is_fill(got[:GUARD]) and _is_fill(got[GUARD + n_index * s.itemsize:])
    fresh = _arena(torch, 64)
    one = (L.SplitCol * 1)(L.SplitCol(src_d[1].data_ptr(), 4, 4, 0, fresh.data_ptr() + GUARD))
    L.check(lib.sprk_take_rows(one, 1, C.c_void_p(index_d.data_ptr()), 0, n_rows, stream))
    assert _is_fill(fresh.cpu().numpy())
    bad = torch.tensor([3, -1, 4, n_rows, 5, 2**31 - 1, 6, 7, 8], dtype=torch.int32, device="cuda")
    L.check(lib.sprk_take_rows(one, 1, C.c_void_p(bad.data_ptr()), 9, n_rows, stream))
    got = fresh.cpu().numpy()[GUARD:GUARD + 36].view(np.int32)
    fill = np.frombuffer(bytes([FILL] * 4), dtype=np.int32)[0]
    assert got.tolist() == [srcs[1][3], fill, srcs[1][4], fill, srcs[1][5], fill, srcs[1][6], srcs[1][7], srcs[1][8]]
    assert _is_fill(fresh.cpu().numpy()[GUARD + 36:])


# ---------------------------------------------------------------- robustness

def _plan(lib, torch, cols, mode, sample, train, seed, mem, ws_bytes, stream, key="source_row"):
    at = lambda name: C.c_void_p(mem[name].data_ptr() + GUARD)
    key_d = torch.from_numpy(cols[key]).cuda()
    ts_d = torch.from_numpy(cols["timestamp"]).cuda()
    n = len(cols[key])
    L.check(lib.sprk_split_plan(C.c_void_p(key_d.data_ptr()), 1 if cols[key].dtype == np.int32 else 2, C.c_void_p(ts_d.data_ptr()), n, seed, FE.split_threshold(sample),
                                FE.split_threshold(train), float(train), FE.SPLIT_MODES[mode], at("index_train"), at("index_test"), at("words"), at("ws"), ws_bytes, stream))
    torch.cuda.synchronize()
    return {name: a.cpu().numpy() for name, a in mem.items()}


@pytest.mark.parametrize("mode", ["random", "time"])
@pytest.mark.parametrize("n", [1025, 3 * K.TILE + 1, 512 * K.TILE + 1])
def test_nothing_is_written_outside_the_outputs_or_the_workspace(lib, mode, n):
    """Guard bands of a fill pattern on both sides of the two lists, the five words and a workspace of exactly the reported length keep
    their fill; the lists hold the parts' positions and nothing past n_train / n_test."""
    import torch
    cols = _cols(n, ts="ties")
    ws_bytes = lib.sprk_split_plan_workspace_bytes(n)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    sizes = {"index_train": n * 4, "index_test": n * 4, "words": 40, "ws": ws_bytes}
    mem = {name: _arena(torch, b) for name, b in sizes.items()}
    mem["words"][GUARD:GUARD + 8] = 0xFF                                      # the error word: ~0
    host = _plan(lib, torch, cols, mode, 0.5, 0.8, 3, mem, ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for name, b in sizes.items():
        assert _is_fill(host[name][:GUARD]) and _is_fill(host[name][GUARD + b:]), name
    want = FE.split_host(cols, mode=mode, sample=0.5, train=0.8, seed=3)
    words = host["words"][GUARD:GUARD + 40].view(np.int64)
    n_train, n_test = len(want.train["label"]), len(want.test["label"])
    assert words.tolist() == [-1, want.n_sampled, n_train, n_test, want.split_timestamp or 0]
    position = np.empty(n, dtype=np.int64)
    position[cols["source_row"]] = np.arange(n)
    for name, part, count in (("index_train", want.train, n_train), ("index_test", want.test, n_test)):
        body = host[name][GUARD:GUARD + n * 4]
        assert body[:count * 4].view(np.int32).tolist() == position[part["source_row"]].tolist() and _is_fill(body[count * 4:]), name
    # a workspace one byte short is refused before any device call
    assert lib.sprk_split_plan(None, 0, None, n, 0, 0, 0, 0.8, 0, C.c_void_p(mem["index_train"].data_ptr()), C.c_void_p(mem["index_test"].data_ptr()),
                               C.c_void_p(mem["words"].data_ptr()), C.c_void_p(mem["ws"].data_ptr()), ws_bytes - 1, None) == L.EINVAL
    assert str(ws_bytes).encode() in lib.sprk_last_error()


@pytest.mark.parametrize("mode", ["random", "time"])
def test_the_error_word_stays_set_and_nothing_is_written(lib, mode):
    """A negative key: the error word names the first such row, and the lists and the other four words keep their fill.  An error word
    that is already set when the call starts stays as it is, with nothing written either."""
    import torch
    n = 3 * K.TILE + 1
    cols = dict(_cols(n))
    cols["source_row"] = cols["source_row"].copy()
    cols["source_row"][[3000, 1234]] = -1
    ws_bytes = lib.sprk_split_plan_workspace_bytes(n)
    sizes = {"index_train": n * 4, "index_test": n * 4, "words": 40, "ws": ws_bytes}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for first, source in ((0xFF, cols), (0x00, _cols(n))):                     # ~0 and a negative key; an error word of 0 and good keys
        mem = {name: _arena(torch, b) for name, b in sizes.items()}
        mem["words"][GUARD:GUARD + 8] = first
        host = _plan(lib, torch, source, mode, 0.5, 0.8, 3, mem, ws_bytes, stream)
        words = host["words"][GUARD:GUARD + 40]
        assert int(words[:8].view(np.int64)[0]) == ((1 << 32 | 1234) if first else 0)
        assert _is_fill(words[8:]) and _is_fill(host["index_train"]) and _is_fill(host["index_test"])
        assert _is_fill(host["ws"][:GUARD]) and _is_fill(host["ws"][GUARD + ws_bytes:])


def test_side_stream(lib):
    """The plan and the takes are enqueued behind a spin of some milliseconds on a side stream; the split's own synchronisation (the five
    words) waits for that stream, and the event recorded after it orders the read of the columns."""
    import torch
    cols = _cols(65_537, ts="ties")
    dev = {k: torch.from_numpy(v).cuda() for k, v in cols.items()}
    torch.cuda.synchronize()
    side, done = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(40_000_000)
        got = FE.split_device(dev, mode="time", sample=0.5)
        done.record(side)
    done.synchronize()
    K.same_split(_host(got), FE.split_host(cols, mode="time", sample=0.5))


# ---------------------------------------------------------------- end to end

def test_build_split_fit_evaluate(lib):
    """A few thousand ratings: featureeng.build -> split(mode="time") -> NeuralCF.fit(train.columns) -> evaluate_device(test.columns): four
    finite numbers; DeviceSamples.split(...).to_host() is split_host(samples_host(...)), in both modes; the parts share the store."""
    import math

    from sparrowrecsys_amd import models as M
    from tests import featureeng_cases as cases
    ratings, movies = cases.synthetic_ratings(), cases.synthetic_movies()
    built = FE.build(ratings, movies, 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    host = FE.samples_host(ratings, movies, 5, n_users=cases.N_USERS, n_movies=cases.N_MOVIES)
    for kw in ({"mode": "time", "sample": 0.5}, {"mode": "random", "sample": 0.5, "seed": 4}, {"mode": "time"}, {}):
        train, test = built.split(**kw)
        want = FE.split_host(host, **kw)
        got = FE.SplitResult(train.to_host(), test.to_host(), train.n_sampled, train.split_timestamp)
        K.same_split(got, want)
        assert (test.n_sampled, test.split_timestamp) == (want.n_sampled, want.split_timestamp)
        assert train.n_samples == len(want.train["label"]) and test.n_samples == len(want.test["label"]) and train.hist_len == 5
        assert all(v.shape[0] == train.n_samples for v in train.columns.values())
    # the genre, history and numeric columns are taken as three row-wide columns and come back as views of three matrices; taken singly
    # they hold the same values
    assert FE._matrix_groups(built.columns) == [[k] for k in FE.sample_keys(5)[:5]] + [FE.sample_keys(5)[5:13], FE.sample_keys(5)[13:18], FE.DENSE_KEYS, ["source_row"]]
    grouped, single = FE.split_device(built.columns, mode="time", sample=0.5), FE.split_device(built.columns, mode="time", sample=0.5, group_matrices=False)
    assert grouped.train["userGenre5"].stride(0) == 8 and grouped.test["userRatingStddev"].stride(0) == 7 and single.train["userGenre5"].stride(0) == 1
    K.same_split(_host(grouped), _host(single))
    train, test = built.split(mode="time", sample=0.5)
    assert train.n_samples > 200 and test.n_samples > 50
    assert train._store_tensors is built._store_tensors and test._store_tensors is built._store_tensors
    model = M.NeuralCF(seed=3, movie_buckets=cases.N_MOVIES, user_buckets=cases.N_USERS)
    model.set_weights(model.init_weights(3, trained_like=False))
    history = model.fit(train.columns, batch_size=64, epochs=2, learning_rate=0.01)
    assert len(history) == 2
    result = model.evaluate_device(test.columns)
    assert len(result) == 4 and all(math.isfinite(float(v)) for v in result)
