"""The definition of the exact ROC and PR areas (``metrics.exact_auc_host``) against Spark 2.4's curves in exact
rationals, against ``exact_roc_auc`` and a hand-worked case; its special inputs, its summation order and its errors; and the C ABI of
the device route (``sprk_exact_auc``) as far as it needs no GPU.

Bounds.  ROC: two integer -> double conversions and one division, each within 2^-53 relative: below 2^-51.  PR: a term takes four
roundings (two divisions, a sum, a product) and is non-negative, so a run of PR_RUN terms added one by one, the run sums added one by
one and the last division stay within (PR_RUN + runs + 6) 2^-53 relative of the exact area."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import metrics as MT
from tests import exact_auc_cases as EC
from tests.conftest import ROOT

SIZES = [1, 2, 4, 50, 2000]
GRIDS = [None, 7, 100]


def _rel(got, exact):
    if exact == 0:
        return 0.0 if got == 0.0 else float("inf")
    return float(abs(Fraction(got) - exact) / exact)


@pytest.mark.parametrize("grid", GRIDS, ids=["continuous", "grid7", "grid100"])
@pytest.mark.parametrize("n", SIZES)
def test_definition_against_sparks_trapezoids_in_rationals(n, grid):
    for seed in range(4):
        y, p = EC.random_rows(n, 100 * n + seed, grid)
        got = MT.exact_auc_host(y, p)
        roc, pr = EC.spark_areas_exact(y, p)
        runs = (got.n_thresholds + MT.PR_RUN - 1) // MT.PR_RUN
        r_roc, r_pr = _rel(got.area_under_roc, roc), _rel(got.area_under_pr, pr)
        print("n %d grid %s seed %d: G %d, ROC rel %.3g x 2^-53, PR rel %.3g x 2^-53" % (n, grid, seed, got.n_thresholds, r_roc * 2.0 ** 53, r_pr * 2.0 ** 53))
        assert r_roc < 2.0 ** -51
        assert r_pr < (MT.PR_RUN + runs + 6) * 2.0 ** -53
        assert got.n == n and got.n_pos == int((y > 0.5).sum())


@pytest.mark.parametrize("grid", GRIDS, ids=["continuous", "grid7", "grid100"])
@pytest.mark.parametrize("n", SIZES)
def test_roc_area_is_exact_roc_auc(n, grid):
    for seed in range(4):
        y, p = EC.random_rows(n, 7 * n + seed, grid)
        want = MT.exact_roc_auc(y, p)
        if np.isnan(want):                                               # an empty class: exact_roc_auc is not defined there
            continue
        assert abs(MT.exact_auc_host(y, p).area_under_roc - want) <= 1e-12


def test_hand_case():
    got = MT.exact_auc_host([1, 0, 1, 0], np.array([.9, .8, .8, .1], dtype=np.float32), return_curve=True)
    assert (got.roc_numerator, got.n, got.n_pos, got.n_thresholds) == (7, 4, 2, 3)
    assert got.area_under_roc == 0.875
    # terms: 1 (1 + 1), 1 (2/3 + 1), 0 (..) = 11/3
    assert abs(Fraction(got.pr_sum) - Fraction(11, 3)) <= Fraction(11, 3) * Fraction(4, 2 ** 53)
    assert got.area_under_pr == got.pr_sum / 4.0 and abs(got.area_under_pr - 11.0 / 12.0) < 1e-15
    assert got.thresholds.dtype == np.float32 and got.thresholds.tolist() == [np.float32(.9), np.float32(.8), np.float32(.1)]
    assert got.tp.dtype == np.uint32 and got.tp.tolist() == [1, 2, 2] and got.fp.dtype == np.uint32 and got.fp.tolist() == [0, 1, 2]
    assert got.roc_points().tolist() == [[0, 0], [0, .5], [.5, 1], [1, 1], [1, 1]]
    assert got.pr_points().tolist() == [[0, 1], [.5, 1], [1, 2 / 3], [1, .5]]
    with pytest.raises(ValueError, match="return_curve"):
        MT.exact_auc_host([1, 0], np.array([.3, .2], dtype=np.float32)).roc_points()


def test_special_inputs():
    p = np.array([.3, .9, .3, -2.5, 7.0], dtype=np.float32)                # (any finite float32: negatives and values above 1)
    none = MT.exact_auc_host(np.zeros(5), p)
    assert (none.area_under_roc, none.area_under_pr, none.n_pos, none.roc_numerator, none.pr_sum) == (0.0, 0.0, 0, 0, 0.0)
    every = MT.exact_auc_host(np.ones(5), p)
    assert (every.area_under_roc, every.area_under_pr, every.n_pos, every.n_thresholds) == (1.0, 1.0, 5, 4)
    same = MT.exact_auc_host([1, 0, 0, 1], np.full(4, .25, dtype=np.float32), return_curve=True)
    assert (same.n_thresholds, same.roc_numerator, same.area_under_roc, same.area_under_pr) == (1, 4, 0.5, 0.5)
    zeros = MT.exact_auc_host([1, 0, 1], np.array([0.0, -0.0, -1.0], dtype=np.float32), return_curve=True)
    assert zeros.n_thresholds == 2 and zeros.tp.tolist() == [1, 2] and zeros.fp.tolist() == [1, 1]
    assert zeros.thresholds.view(np.uint32).tolist() == [0, 0xbf800000]        # the group of both zeros is +0.0
    tiny = np.array([1e-45, -1e-45, 0.0], dtype=np.float32)                     # subnormals are scores like any other
    assert MT.exact_auc_host([1, 0, 0], tiny).area_under_roc == 1.0 and MT.exact_auc_host([1, 0, 0], tiny).n_thresholds == 3
    half = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1))], dtype=np.float32)
    got = MT.exact_auc_host(half, np.array([.2, .7], dtype=np.float32))
    assert got.n_pos == 1 and got.area_under_roc == 1.0                         # 0.5 is negative, the next float32 positive
    for dtype in (np.float32, np.int32, np.int64, np.uint8, np.bool_, np.float64, np.int16):
        assert MT.exact_auc_host(np.array([1, 0, 1, 0]).astype(dtype), np.array([.9, .8, .8, .1], dtype=np.float32)).roc_numerator == 7


def test_the_pr_sum_takes_the_stated_order():
    y, p = EC.distinct_groups(5000, 3)
    got = MT.exact_auc_host(y, p)
    assert got.n_thresholds == 5000
    terms = EC.pr_terms(y, p)
    assert got.pr_sum == EC.pr_sum_defined(terms)
    plain = 0.0
    for t in terms:
        plain = plain + t
    assert got.pr_sum != plain                                                  # runs of PR_RUN, not one chain
    assert got.pr_sum != EC.pr_sum_defined(terms, 512)


def test_the_result_does_not_depend_on_the_order_of_the_rows():
    for grid in (None, 100):
        y, p = EC.random_rows(3000, 17, grid)
        want = MT.exact_auc_host(y, p, return_curve=True)
        perm = np.random.RandomState(5).permutation(len(p))
        got = MT.exact_auc_host(y[perm], p[perm], return_curve=True)
        assert got.words() == want.words()
        assert np.array_equal(got.thresholds, want.thresholds) and np.array_equal(got.tp, want.tp) and np.array_equal(got.fp, want.fp)


def test_errors_the_least_word_wins():
    y, p = EC.random_rows(100, 1)
    bad = p.copy(); bad[70] = np.nan; bad[30] = np.inf
    with pytest.raises(ValueError, match="score of row 30 "):
        MT.exact_auc_host(y, bad)
    ybad = y.copy(); ybad[60] = np.nan; ybad[20] = -np.inf
    with pytest.raises(ValueError, match="label of row 20 "):
        MT.exact_auc_host(ybad, p)
    with pytest.raises(ValueError, match="score of row 30 "):             # kind 1 is less than kind 2, whatever the rows
        MT.exact_auc_host(ybad, bad)
    with pytest.raises(ValueError, match="label of row 60 "):
        MT.exact_auc_host(np.where(np.arange(100) == 60, np.nan, y).astype(np.float64), p)
    with pytest.raises(ValueError, match="no sample"):
        MT.exact_auc_host([], np.zeros(0, dtype=np.float32))
    with pytest.raises(ValueError, match="3 scores, 2 labels"):
        MT.exact_auc_host([1, 0], np.zeros(3, dtype=np.float32))


# ---- the C ABI, without a device ------------------------------------------------------------------------------------------------------

def test_prototypes_and_ctypes_signatures(lib):
    header = open(os.path.join(ROOT, "include", "sparrow_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "size_t sprk_exact_auc_workspace_bytes(int64_t n);" in flat
    assert "int32_t sprk_exact_auc_bin_bits(int64_t n);" in flat
    assert ("int sprk_exact_auc(const float* scores, const void* labels, int32_t label_storage, int64_t label_stride , int64_t n, "
            "sprk_exact_auc_result* result, float* thresholds, uint32_t* tp, uint32_t* fp, uint64_t* error_key, void* workspace, "
            "size_t workspace_bytes, void* stream);") in flat
    assert re.search(r"typedef struct \{ int64_t n, n_pos, n_groups; uint64_t roc_numerator; double pr_sum, area_under_roc, area_under_pr; \} sprk_exact_auc_result;", flat)
    vp = C.c_void_p
    assert lib.sprk_exact_auc.argtypes == [vp, vp, C.c_int32, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    assert lib.sprk_exact_auc.restype == C.c_int
    assert lib.sprk_exact_auc_workspace_bytes.argtypes == [C.c_int64] and lib.sprk_exact_auc_workspace_bytes.restype == C.c_size_t
    assert lib.sprk_exact_auc_bin_bits.argtypes == [C.c_int64] and lib.sprk_exact_auc_bin_bits.restype == C.c_int32
    assert C.sizeof(L.ExactAucResult) == 56 and [f[0] for f in L.ExactAucResult._fields_] == ["n", "n_pos", "n_groups", "roc_numerator", "pr_sum", "area_under_roc",
                                                                                             "area_under_pr"]
    src = open(os.path.join(ROOT, "sparrowrecsys_amd", "csrc", "k_exact_auc.h")).read()
    assert int(re.search(r"EA_PR_RUN = (\d+);", src).group(1)) == MT.PR_RUN


def test_arguments_are_refused_before_any_device_call(lib, monkeypatch):
    monkeypatch.delenv("SPRK_EXACT_AUC_BIN_BITS", raising=False)
    err = lambda: lib.sprk_last_error().decode()
    need = lib.sprk_exact_auc_workspace_bytes(1000)
    assert need > 0 and need % 16 == 0
    assert lib.sprk_exact_auc_workspace_bytes(0) == 0 and lib.sprk_exact_auc_workspace_bytes(-1) == 0
    assert lib.sprk_exact_auc_workspace_bytes((1 << 31) - 1) == 0 and lib.sprk_exact_auc_workspace_bytes((1 << 31) - 2) > 32 * ((1 << 31) - 2)
    assert lib.sprk_exact_auc_bin_bits(0) == 0 and 1 <= lib.sprk_exact_auc_bin_bits(1) <= 24 and 1 <= lib.sprk_exact_auc_bin_bits((1 << 31) - 2) <= 24
    # (addresses that are never read: every check comes before the first device call)
    scores, labels, result, word, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000

    def call(n=1000, scores=scores, labels=labels, storage=L.COL_F32, stride=4, result=result, thr=None, tp=None, fp=None, word=word, ws=ws, ws_bytes=need):
        return lib.sprk_exact_auc(scores, labels, storage, stride, n, result, thr, tp, fp, word, ws, ws_bytes, None)
    assert call(n=-1) == L.EINVAL and "negative n" in err()
    assert call(n=0) == L.EINVAL and "n = 0" in err()
    assert call(n=(1 << 31) - 1) == L.EINVAL and "2^31 - 1" in err()
    assert call(n=1 << 40) == L.EINVAL
    assert call(ws_bytes=need - 1) == L.EINVAL and "sprk_exact_auc_workspace_bytes" in err() and str(need) in err()
    assert call(ws=None) == L.EINVAL and "sprk_exact_auc_workspace_bytes" in err()
    assert call(ws=ws + 8) == L.EINVAL and "sprk_exact_auc_workspace_bytes" in err() and "16-byte" in err()
    assert call(storage=L.COL_F64) == L.EINVAL and "label_storage" in err()
    assert call(stride=0) == L.EINVAL and call(stride=6) == L.EINVAL and call(storage=L.COL_I64, stride=4) == L.EINVAL
    assert call(scores=None) == L.EINVAL and call(labels=None) == L.EINVAL and call(result=None) == L.EINVAL and call(word=None) == L.EINVAL
    assert call(scores=scores + 2) == L.EINVAL and call(labels=labels + 2) == L.EINVAL and call(result=result + 4) == L.EINVAL and call(word=word + 4) == L.EINVAL
    assert call(thr=0x50002) == L.EINVAL and call(tp=0x50002) == L.EINVAL and call(fp=0x50002) == L.EINVAL
    # the bin width may be set from outside, and sizes the workspace
    monkeypatch.setenv("SPRK_EXACT_AUC_BIN_BITS", "20")
    assert lib.sprk_exact_auc_bin_bits(1000) == 20 and lib.sprk_exact_auc_workspace_bytes(1000) > need + 8 * (1 << 20) - 8 * 256
    monkeypatch.setenv("SPRK_EXACT_AUC_BIN_BITS", "25")
    assert lib.sprk_exact_auc_workspace_bytes(1000) == need


def test_device_entry_points_fail_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        MT.exact_auc_device(torch.zeros(4), torch.zeros(4))
