"""The device route of the exact ROC and PR areas (``sprk_exact_auc``, csrc/k_exact_auc.h, ``metrics.exact_auc_device``) against its
definition, ``metrics.exact_auc_host``: every word of the result and every element of the curve, bit for bit (``-m gpu``).

The shapes are the smallest at which a stage can go wrong: the workgroup (256) and the scan tile (FE_SCAN_TILE) edges, one bin at the
LDS sort's capacity and one key past it (also at the smallest capacity, SPRK_FE_SORT_CAP=64, where chunks and merge passes run at a
few hundred rows), ties across a bin boundary, a scan tile and a PR run, the first and the last bin, a capped grid's later rounds."""
import ctypes as C
import os

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import metrics as MT
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import schema as S
from tests import exact_auc_cases as EC
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
EXCERPT = os.path.join(GOLDEN, "test_samples_512.csv")
K = EC.kernel_constants()
GUARD = 64                                                                     # 8-byte words on each side of every buffer
FILL = 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for name in ("SPRK_EXACT_AUC_BIN_BITS", "SPRK_FE_SORT_CAP", "SPRK_FE_MAX_GRID"):
        monkeypatch.delenv(name, raising=False)


def _same(got, want):
    assert got.words() == want.words(), (got, want)
    assert got.thresholds.dtype == np.float32 and got.tp.dtype == np.uint32 and got.fp.dtype == np.uint32
    assert np.array_equal(got.thresholds.view(np.uint32), want.thresholds.view(np.uint32))
    assert np.array_equal(got.tp, want.tp) and np.array_equal(got.fp, want.fp)


def _check(torch, y, p, labels=None):
    """The device result over (y, p) -- labels: the device tensor to hand over instead of y -- equals the definition's."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    want = MT.exact_auc_host(y, p, return_curve=True)
    got = MT.exact_auc_device(torch.from_numpy(p.copy()).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda() if labels is None else labels, return_curve=True)
    _same(got, want)
    plain = MT.exact_auc_device(torch.from_numpy(p.copy()).cuda().reshape(-1, 1), np.asarray(y))      # host labels, [n, 1] scores, no curve
    assert plain.words() == want.words() and plain.thresholds is None
    return want


def _bins(p):
    bits = L.load_library().sprk_exact_auc_bin_bits(len(p))
    return MT.exact_score_keys(np.asarray(p, dtype=np.float32)) >> np.uint32(32 - bits), bits


def _rows_in_the_bin_of(p, value):
    bins, bits = _bins(p)
    return int((bins == (MT.exact_score_keys(np.array([value], dtype=np.float32))[0] >> np.uint32(32 - bits))).sum())


class _Guarded:
    """A device buffer of exactly `nbytes` (a multiple of 8) between two guard bands."""

    def __init__(self, torch, nbytes, fill=FILL):
        assert nbytes % 8 == 0
        self.words = nbytes // 8
        self.t = torch.full((self.words + 2 * GUARD,), fill, dtype=torch.int64, device="cuda")
        self.ptr = self.t.data_ptr() + 8 * GUARD
        assert self.ptr % 16 == 0

    def guards_intact(self):
        h = self.t.cpu().numpy()
        return bool((h[:GUARD] == FILL).all() and (h[GUARD + self.words:] == FILL).all())

    def body(self):
        return self.t[GUARD:GUARD + self.words].cpu().numpy()


def _raw(torch, p, y, stream=None, word=-1):
    """sprk_exact_auc through ctypes with guard bands round the workspace (exactly as large as reported), the result, the error word and
    the three curve arrays -> (ExactAuc or None, error word, the buffers)."""
    lib = L.load_library()
    n = len(p)
    pd, yd = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda()
    need = lib.sprk_exact_auc_workspace_bytes(n)
    assert need % 16 == 0
    curve_bytes = (4 * n + 7) // 8 * 8
    bufs = {"ws": _Guarded(torch, need), "result": _Guarded(torch, 56), "word": _Guarded(torch, 8, word), "thr": _Guarded(torch, curve_bytes),
            "tp": _Guarded(torch, curve_bytes), "fp": _Guarded(torch, curve_bytes)}
    if word != FILL:
        bufs["word"].t[:GUARD] = FILL
        bufs["word"].t[GUARD + 1:] = FILL
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    rc = lib.sprk_exact_auc(pd.data_ptr(), yd.data_ptr(), L.COL_F32, 4, n, bufs["result"].ptr, bufs["thr"].ptr, bufs["tp"].ptr, bufs["fp"].ptr, bufs["word"].ptr,
                            bufs["ws"].ptr, need, C.c_void_p(st))
    assert rc == 0, lib.sprk_last_error()
    (torch.cuda.current_stream() if stream is None else stream).synchronize()
    for name, b in bufs.items():
        assert b.guards_intact(), name
    err = int(bufs["word"].body()[0])
    if err != -1:
        return None, err, bufs
    w = bufs["result"].body()
    f = w[4:7].view(np.float64)
    res = MT.ExactAuc(int(w[0]), int(w[1]), int(w[2]), int(w[3:4].view(np.uint64)[0]), f[0], f[1], f[2])
    G = res.n_thresholds
    res.thresholds = bufs["thr"].body().view(np.float32)[:G].copy()
    res.tp, res.fp = bufs["tp"].body().view(np.uint32)[:G].copy(), bufs["fp"].body().view(np.uint32)[:G].copy()
    # past the G rows the curve arrays keep what they held
    for name in ("thr", "tp", "fp"):
        assert (bufs[name].body().view(np.uint32)[G:] == 0x5a5a5a5a).all(), name
    return res, err, bufs


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_small_sizes(torch, n):
    for grid in (None, 7):
        y, p = EC.random_rows(n, 40 + n, grid)
        _check(torch, y, p)


def _one_bin(m, extra, seed):
    """m distinct scores in [0.75, 0.75 + m ulp) -- one bin at every width up to 2^21 keys -- and `extra` rows spread over (0, 0.5)."""
    p = np.concatenate([EC.floats_from_bits(0x3f400000, m), (np.random.RandomState(seed).random_sample(extra) * 0.5).astype(np.float32)])
    np.random.RandomState(seed + 1).shuffle(p)
    return EC.labels_for(p, seed + 2), p


@pytest.mark.parametrize("m", [K["FE_SORT_CAP"] - 1, K["FE_SORT_CAP"], K["FE_SORT_CAP"] + 1])
def test_one_bin_at_the_sort_capacity(torch, m):
    y, p = _one_bin(m, 300, m)
    bins, bits = _bins(p)
    assert 32 - bits <= 21 and _rows_in_the_bin_of(p, 0.75) == m
    _check(torch, y, p)


@pytest.mark.parametrize("m", [63, 64, 65, 129, 1000])
def test_sort_capacity_edges_at_the_smallest_capacity(torch, monkeypatch, m):
    """SPRK_FE_SORT_CAP=64: 65 keys are two chunks, 129 three, 1000 sixteen; the merge passes double the runs from 64 keys up to the
    number of rows, so an even and an odd number of passes (a copy back) both occur."""
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    y, p = _one_bin(m, 90, m)
    assert _rows_in_the_bin_of(p, 0.75) == m
    _check(torch, y, p)


def test_one_tie_group_longer_than_the_sort_capacity(torch):
    rng = np.random.RandomState(8)
    p = np.concatenate([np.full(5000, 0.625, dtype=np.float32), rng.random_sample(700).astype(np.float32)])
    rng.shuffle(p)
    want = _check(torch, EC.labels_for(p, 9), p)
    assert want.n_thresholds <= 701
    _check(torch, np.ones(5000, dtype=np.float32), np.full(5000, 0.625, dtype=np.float32))      # all rows one group, one class


@pytest.mark.parametrize("m", [2, 255, 256, 257, 513, K["FE_SORT_CAP"] + 1])
def test_bins_of_one_score_are_left_unsorted_and_one_other_key_is_found(torch, m):
    """k_ea_sort_short reads a bin 256 keys at a time and skips it when all are one score: bins of one score at the edges of that read,
    and the same bins with one row of the neighbouring score, which lands wherever the scatter puts it."""
    rng = np.random.RandomState(m)
    others = (rng.random_sample(200) * 0.5).astype(np.float32)
    for odd in (0, 1):
        p = np.concatenate([np.full(m - odd, 0.75, dtype=np.float32), EC.floats_from_bits(0x3f400001, odd), others])
        rng.shuffle(p)
        assert _rows_in_the_bin_of(p, 0.75) == m
        want = _check(torch, EC.labels_for(p, m + odd), p)
        assert want.n_thresholds == len(np.unique(others)) + 1 + odd


@pytest.mark.parametrize("extra", [0, 1])
def test_a_bin_of_one_score_at_the_longest_the_check_reads(torch, extra):
    m = K["EA_TIE_SCAN_MAX"] + extra                                           # one more: to the long list unread, sorted by row
    p = np.concatenate([np.full(m, 0.75, dtype=np.float32), np.linspace(0.1, 0.4, 77).astype(np.float32)])
    np.random.RandomState(extra).shuffle(p)
    y = EC.labels_for(p, 2 + extra)
    got = MT.exact_auc_device(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda(), return_curve=True)
    _same(got, MT.exact_auc_host(y, p, return_curve=True))


def test_first_and_last_bin_subnormals_and_zeros(torch):
    big = np.finfo(np.float32).max
    p = np.array([big, -big, big, -big, 0.0, -0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.0, -1.0, 3.5, np.nextafter(np.float32(big), np.float32(0)), 1e-45, -0.0],
                 dtype=np.float32)
    y = np.array([1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0, 1], dtype=np.float32)
    bins, bits = _bins(p)
    assert bins.min() == 0x00800000 >> (32 - bits) and bins.max() == 0xff7fffff >> (32 - bits)       # the first and the last bin there is
    want = _check(torch, y, p)
    assert want.n_thresholds == 11 and want.thresholds[0] == big and want.thresholds[-1] == -big
    for bits in (1, 24):
        os.environ["SPRK_EXACT_AUC_BIN_BITS"] = str(bits)
        try:
            _check(torch, y, p)
        finally:
            del os.environ["SPRK_EXACT_AUC_BIN_BITS"]


def test_tie_groups_across_a_bin_boundary_a_scan_tile_and_a_pr_run(torch, monkeypatch):
    tile, run = K["FE_SCAN_TILE"], K["EA_PR_RUN"]
    # the two sides of a bin boundary (0.75: a boundary at every width up to 2^22 keys), each several times, and their neighbours
    monkeypatch.setenv("SPRK_EXACT_AUC_BIN_BITS", "12")
    edge = np.array([0x3f3ffffe, 0x3f3fffff, 0x3f400000, 0x3f400001], dtype=np.uint32).view(np.float32)
    p = np.repeat(edge, [3, 5, 4, 2])
    bins, _ = _bins(p)
    assert bins[3] != bins[8] and len(np.unique(bins)) == 2
    _check(torch, EC.labels_for(p, 1), p)
    monkeypatch.delenv("SPRK_EXACT_AUC_BIN_BITS")
    # sorted places tile - 4 .. tile + 5 are one group: `tile - 4` distinct scores above it
    p = np.concatenate([EC.floats_from_bits(0x3f400000, tile - 4, 3), np.full(10, 0.5, dtype=np.float32), EC.floats_from_bits(0x3e000000, 50, 7)])
    np.random.RandomState(2).shuffle(p)
    want = _check(torch, EC.labels_for(p, 3), p)
    assert int(want.tp[tile - 5]) + int(want.fp[tile - 5]) == tile - 4 and int(want.tp[tile - 4]) + int(want.fp[tile - 4]) == tile + 6
    # groups run - 1 and run (0-based: the last of the first PR run, the first of the second) are tie groups
    p = np.concatenate([EC.floats_from_bits(0x3f400000, run + 40, 5), np.repeat(EC.floats_from_bits(0x3f400000 + 5 * 39, 2, 5), 6)])
    np.random.RandomState(4).shuffle(p)
    want = _check(torch, EC.labels_for(p, 5), p)
    counts = np.diff(np.concatenate([[0], want.tp.astype(np.int64) + want.fp.astype(np.int64)]))
    assert want.n_thresholds == run + 40 and counts[run - 1] == 7 and counts[run] == 7


@pytest.mark.parametrize("G", [K["EA_PR_RUN"] - 1, K["EA_PR_RUN"], K["EA_PR_RUN"] + 1, 3 * K["EA_PR_RUN"] + 1])
def test_group_counts_round_the_pr_run(torch, G):
    y, p = EC.distinct_groups(G, G)
    assert _check(torch, y, p).n_thresholds == G


@pytest.mark.parametrize("grid", ["1", "3"])
def test_capped_grids(torch, monkeypatch, grid):
    """SPRK_FE_MAX_GRID: every grid-stride loop goes round several times, the sort's workgroups take several bins each."""
    monkeypatch.setenv("SPRK_FE_MAX_GRID", grid)
    y, p = EC.random_rows(5000, 12, 1000)
    _check(torch, y, p)
    y, p = EC.distinct_groups(2 * K["EA_PR_RUN"] + 300, 13)                    # three PR runs on one or three workgroups
    _check(torch, y, p)
    monkeypatch.setenv("SPRK_FE_SORT_CAP", "64")
    y, p = _one_bin(700, 500, 14)
    _check(torch, y, p)


@pytest.mark.parametrize("rounded", [True, False], ids=["rounded_to_1e-3", "continuous"])
def test_300000_rows(torch, rounded):
    rng = np.random.RandomState(21)
    z = rng.standard_normal(300000) * 1.5
    p = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    if rounded:
        p = (np.round(p.astype(np.float64) * 1000.0) / 1000.0).astype(np.float32)
    y = (rng.random_sample(300000) < p).astype(np.float32)
    want = MT.exact_auc_host(y, p, return_curve=True)
    got = MT.exact_auc_device(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda(), return_curve=True)
    _same(got, want)
    assert (want.n_thresholds <= 1001) == rounded


def test_empty_classes(torch):
    _, p = EC.random_rows(700, 31, 50)
    none = _check(torch, np.zeros(700, dtype=np.float32), p)
    assert (none.area_under_roc, none.area_under_pr) == (0.0, 0.0)
    every = _check(torch, np.ones(700, dtype=np.float32), p)
    assert (every.area_under_roc, every.area_under_pr) == (1.0, 1.0)


@pytest.mark.parametrize("dtype", ["float32", "int32", "int64", "uint8", "bool"])
def test_every_label_storage(torch, dtype):
    y, p = EC.random_rows(1500, 33, 100)
    _check(torch, y, p, torch.from_numpy(y.copy()).cuda().to(getattr(torch, dtype)))
    if dtype == "float32":                                                      # label > 0.5, not label != 0
        y = np.where(np.arange(1500) % 3 == 0, np.float32(0.5), np.where(np.arange(1500) % 3 == 1, np.nextafter(np.float32(0.5), np.float32(1)), y)).astype(np.float32)
        _check(torch, y, p)
    elif dtype in ("int32", "int64"):
        y = np.where(np.arange(1500) % 3 == 0, -5, np.where(np.arange(1500) % 3 == 1, 9, y)).astype(dtype)
        _check(torch, y, p)


def test_a_strided_label_column(torch):
    y, p = EC.random_rows(4097, 35)
    wide = torch.zeros((4097, 7), dtype=torch.float32, device="cuda")
    wide[:, 3] = torch.from_numpy(y).cuda()
    wide[:, 2] = 7.0                                                            # (neighbours that must not be read)
    wide[:, 4] = float("nan")
    _check(torch, y, p, wide[:, 3])


def test_errors_leave_every_output_untouched(torch):
    y, p = EC.random_rows(3000, 37, 100)
    bad = p.copy(); bad[2000] = np.nan; bad[123] = -np.inf
    ybad = y.copy(); ybad[77] = np.nan; ybad[1500] = np.inf
    for scores, labels, kind, row in ((bad, y, 1, 123), (p, ybad, 2, 77), (bad, ybad, 1, 123)):
        res, err, bufs = _raw(torch, scores, labels)
        assert res is None and err == (kind << 32 | row)
        for name in ("result", "thr", "tp", "fp"):
            assert (bufs[name].body() == FILL).all(), name
        with pytest.raises(ValueError) as dev:
            MT.exact_auc_device(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda())
        with pytest.raises(ValueError) as host:
            MT.exact_auc_host(labels, scores)
        assert str(dev.value) == str(host.value) and "row %d " % row in str(dev.value)
    # a word that is already set: nothing runs
    res, err, bufs = _raw(torch, p, y, word=5)
    assert res is None and err == 5 and (bufs["result"].body() == FILL).all()
    with pytest.raises(ValueError, match="no sample"):
        MT.exact_auc_device(torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda"))


def test_workspace_guards_a_side_stream_and_repeatability(torch):
    for y, p in (EC.random_rows(9000, 39), EC.random_rows(9000, 41, 200), _one_bin(K["FE_SORT_CAP"] + 500, 100, 43)):
        want = MT.exact_auc_host(y, p, return_curve=True)
        first, err, _ = _raw(torch, p, y)
        assert err == -1
        _same(first, want)
        side = torch.cuda.Stream()
        second, err, _ = _raw(torch, p, y, stream=side)
        assert err == -1
        _same(second, want)


def test_end_to_end_on_neuralcf_and_the_csv_route(torch, samples):
    model = M.NeuralCF(seed=1)
    labels = np.asarray(samples["label"]).astype(np.float32)
    want = MT.exact_auc_host(labels, model.predict(samples), return_curve=True)
    got = model.evaluate_exact(samples, return_curve=True)
    _same(got, want)
    x = {k: v for k, v in samples.items() if k != "label"}
    assert model.evaluate_exact(x, labels).words() == want.words()
    assert model.evaluate_exact(samples, batch_size=100).words() == want.words()                 # three batches, two sizes

    def halves():
        yield {k: v[:128] for k, v in x.items()}, labels[:128]
        yield {k: v[128:] for k, v in x.items()}, torch.from_numpy(labels[128:]).cuda()
    assert model.evaluate_exact(halves()).words() == want.words()
    with pytest.raises(ValueError):
        model.evaluate_exact(iter([]))
    rows = S.read_samples_csv(EXCERPT)
    parsed = model.evaluate_exact(rows, return_curve=True)
    _same(parsed, MT.exact_auc_host(np.asarray(rows["label"]).astype(np.float32), model.predict(rows), return_curve=True))
    for got in (model.evaluate_exact_csv(EXCERPT, return_curve=True), model.evaluate_exact_csv(open(EXCERPT, "rb").read(), batch_size=200, return_curve=True)):
        _same(got, parsed)
    assert model.evaluate_exact_csv(EXCERPT, max_rows=100).words() == model.evaluate_exact(S.read_samples_csv(EXCERPT, limit=100)).words()
