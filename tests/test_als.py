"""ALS collaborative filtering, the definition (sparrowrecsys_amd/als.py als_host), on the host: hand-worked
systems, the mathematics (residual, numpy.linalg.solve), the order of a row's ratings, convergence, rows without ratings, and the C
ABI's argument checks, which need no GPU.  tests/test_gpu_als.py holds the device to this definition byte for byte."""
import ctypes as C
import math

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import als as A
from tests import als_cases as cases


def _word(x):
    return int(np.float32(x).view(np.uint32))


def test_hand_worked_rank_1():
    differs = 0
    for reg, want, plain in cases.HAND_RANK1:
        a = (1.0 * 1.0 + 2.0 * 2.0) + 3.0 * 3.0 + 3.0 * reg
        b = (0.0 + 4.0 * 1.0) + 5.0 * 3.0                      # the rating 0 of user 1 skipped the daxpy
        if reg == 0.5:
            assert a == 14 + 1.5 and b == 19
        s = math.sqrt(a)
        assert _word((b / s) / s) == want and _word(b / a) == plain
        f, count, failed = A.half_sweep_host(np.zeros(3, int), np.arange(3), np.array([4, 0, 5], np.float32), 1,
                                             np.array([[1], [2], [3]], np.float32), reg)
        assert _word(f[0, 0]) == want and count.tolist() == [3] and len(failed) == 0
        differs += want != plain
    assert cases.HAND_RANK1[0][1] == 0x3f9ce73a
    assert differs >= 1                                        # the Cholesky's two divisions are not b / A


def test_hand_worked_rank_2():
    H = {k: float.fromhex(v) for k, v in cases.HAND2.items()}
    x, r = cases.HAND2_FACTORS.astype(np.float64), cases.HAND2_RATINGS.astype(np.float64)
    lam = 3.0 * cases.HAND2_REG
    assert ((x[0, 0] * x[0, 0] + x[1, 0] * x[1, 0]) + x[2, 0] * x[2, 0]) + lam == H["a00"]
    assert (x[0, 0] * x[0, 1] + x[1, 0] * x[1, 1]) + x[2, 0] * x[2, 1] == H["a01"]
    assert ((x[0, 1] * x[0, 1] + x[1, 1] * x[1, 1]) + x[2, 1] * x[2, 1]) + lam == H["a11"]
    assert (r[0] * x[0, 0] + r[1] * x[1, 0]) + r[2] * x[2, 0] == H["b0"]
    assert (r[0] * x[0, 1] + r[1] * x[1, 1]) + r[2] * x[2, 1] == H["b1"]
    assert math.sqrt(H["a00"]) == H["u00"] and H["a01"] / H["u00"] == H["u01"]
    assert H["u01"] * H["u01"] == H["t"] and H["a11"] - H["t"] == H["d"] and math.sqrt(H["d"]) == H["u11"]
    assert H["b0"] / H["u00"] == H["z0"] and (H["b1"] - H["u01"] * H["z0"]) / H["u11"] == H["z1"]
    assert H["z1"] / H["u11"] == H["y1"] and (H["z0"] - H["y1"] * H["u01"]) / H["u00"] == H["y0"]
    ata, atb, count = A.normal_equations_host(np.zeros(3, int), np.arange(3), cases.HAND2_RATINGS, 1, cases.HAND2_FACTORS, cases.HAND2_REG)
    assert ata[0].tolist() == [H["a00"], H["a01"], H["a11"]] and atb[0].tolist() == [H["b0"], H["b1"]] and count.tolist() == [3]
    y, ok = A.cholesky_solve_host(ata, atb)
    assert ok.all() and y[0].tolist() == [H["y0"], H["y1"]]
    f, _, _ = A.half_sweep_host(np.zeros(3, int), np.arange(3), cases.HAND2_RATINGS, 1, cases.HAND2_FACTORS, cases.HAND2_REG)
    assert f.view(np.uint32)[0].tolist() == cases.HAND2_WORDS
    # the same movie through als_host: iters = 1, init_user = the factors; the user half-sweep that follows does not touch the movie's row
    out = A.als_host([0, 1, 2], [0, 0, 0], cases.HAND2_RATINGS, 3, 1, rank=2, reg=cases.HAND2_REG, iters=1, init_user=cases.HAND2_FACTORS)
    assert out[1].view(np.uint32)[0].tolist() == cases.HAND2_WORDS


def _dense(ata, rank):
    I, J = A.tri_index(rank)
    M = np.zeros((len(ata), rank, rank))
    M[:, I, J] = ata
    M[:, J, I] = ata
    return M


@pytest.fixture(scope="module")
def systems():
    """The movies' and the users' normal equations of the low-rank set at rank 8 after one full iteration."""
    case = cases.low_rank()
    rank = 8
    uf = A.als_host(case["user"], case["movie"], case["rating"], case["n_users"], case["n_items"], rank=rank, iters=1)[0]
    itf = A.half_sweep_host(case["movie"], case["user"], case["rating"], case["n_items"], uf, 0.01)[0]
    out = []
    for dst, other, n_dst, src in ((case["movie"], case["user"], case["n_items"], uf), (case["user"], case["movie"], case["n_users"], itf)):
        ata, atb, _ = A.normal_equations_host(dst, other, case["rating"], n_dst, src, 0.01)
        y, ok = A.cholesky_solve_host(ata, atb)
        assert ok.all()
        out.append((_dense(ata, rank), atb, y))
    return out


def test_residual_of_every_row(systems):
    """Cholesky's backward error at rank <= 16 is a few units of 2^-53 and the matrices' condition is at most about 1 + 1 / reg."""
    for M, b, y in systems:
        res = np.abs(np.einsum("nij,nj->ni", M, y) - b).max(axis=1)
        bound = 1e-12 * (np.abs(M).sum(axis=2).max(axis=1) * np.abs(y).max(axis=1) + np.abs(b).max(axis=1))
        assert (res <= bound).all(), float((res / bound).max())


def test_against_numpy_linalg_solve(systems):
    for M, b, y in systems:
        want = np.linalg.solve(M, b[:, :, None])[:, :, 0]
        assert (np.abs(y - want).max(axis=1) <= 1e-9 * np.abs(want).max(axis=1)).all()


def test_the_order_of_a_rows_ratings_is_part_of_the_definition():
    """User factors of mixed magnitudes 1e-3, 1, 1e3 along one direction plus noise of 1e-3, and reg = 1e-6: the sums round, and the
    systems' condition carries the last bits of a double sum into the float32 result.  Walking every row's ratings backwards then
    changes output words (products of two float32 values are exact in a double, so well-conditioned sets show nothing)."""
    rng = np.random.default_rng(3)
    n_users, n_items = 40, 6
    mask = rng.random((n_users, n_items)) < 0.7
    u, m = np.nonzero(mask)
    r = cases.half_stars(rng.integers(1, 11, len(u)) / 2.0)
    scale = np.array([1e-3, 1.0, 1e3])[rng.integers(0, 3, n_users)]
    init = (scale[:, None] * np.array([1.0, 0.7, -1.3]) + 1e-3 * rng.standard_normal((n_users, 3))).astype(np.float32)
    fwd = A.als_host(u, m, r, n_users, n_items, rank=3, reg=1e-6, iters=1, init_user=init)
    bwd = A.als_host(u, m, r, n_users, n_items, rank=3, reg=1e-6, iters=1, init_user=init, descending=True)
    assert (fwd[1].view(np.uint32) != bwd[1].view(np.uint32)).sum() >= 3
    # shuffling the INPUT rows changes nothing (no pair repeats here)
    perm = rng.permutation(len(u))
    again = A.als_host(u[perm], m[perm], r[perm], n_users, n_items, rank=3, reg=1e-6, iters=1, init_user=init)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fwd, again))


def test_a_repeated_pair_counts_twice_in_input_order():
    init = np.array([[1.0, 1e-3], [3.0, 2.0]], dtype=np.float32)
    once = A.als_host([0, 1], [0, 0], [4.0, 3.0], 2, 1, rank=2, iters=1, init_user=init)
    twice = A.als_host([0, 1, 0], [0, 0, 0], [4.0, 3.0, 2.5], 2, 1, rank=2, iters=1, init_user=init)
    assert twice[4].tolist() == [2, 1] and twice[5].tolist() == [3] and once[1].tobytes() != twice[1].tobytes()
    f, _, _ = A.half_sweep_host([0, 0, 0], [0, 0, 1], np.array([4.0, 2.5, 3.0], np.float32), 1, init, 0.01)   # user 0's two rows, then user 1's
    assert twice[1].tobytes() == f.tobytes()


def _rmse(out, case):
    p = A.predict_host(case["user"], case["movie"], out[0], out[2], out[1], out[3])
    return float(np.sqrt(np.mean((p - case["rating"]).astype(np.float64) ** 2)))


def test_training_rmse_falls_and_ends_below_a_half():
    case = cases.low_rank()
    one, five = (_rmse(cases.host(case, rank=4, reg=0.01, iters=it), case) for it in (1, 5))
    assert five < one and five < 0.5, (one, five)


def test_a_row_without_ratings_has_no_factor_and_predicts_nan():
    out = A.als_host([0, 2, 2], [1, 1, 3], [4.0, 3.0, 5.0], 4, 5, rank=2, iters=2)
    assert out[2].tolist() == [1, 0, 1, 0] and out[3].tolist() == [0, 1, 0, 1, 0]
    assert out[4].tolist() == [1, 0, 2, 0] and out[5].tolist() == [0, 2, 0, 1, 0]
    assert not out[0][[1, 3]].any() and not out[1][[0, 2, 4]].any() and out[0][[0, 2]].all() and out[1][[1, 3]].all()
    p = A.predict_host([0, 1, 0, 4, 0, -1], [1, 1, 0, 1, 5, 1], out[0], out[2], out[1], out[3])
    assert np.isnan(p).tolist() == [False, True, True, True, True, True]
    assert all(o.dtype == t for o, t in zip(out, (np.float32, np.float32, np.uint8, np.uint8, np.int32, np.int32)))
    zero = A.als_host([0, 2, 2], [1, 1, 3], [4.0, 3.0, 5.0], 4, 5, rank=2, iters=0, seed=3)
    assert zero[0].tobytes() == A.init_factors(4, 2, 3).tobytes() and not zero[1].any() and zero[2].tolist() == [1, 0, 1, 0]


def test_errors_name_kind_and_row_or_id():
    ok = ([0, 1], [0, 1], [4.0, 3.0], 2, 2)
    for change, message in (((0, [0, 2]), "ratings row 1: userId outside the user table"), ((1, [-1, 1]), "ratings row 0: movieId outside the movie table"),
                            ((2, [4.0, np.nan]), "ratings row 1: rating is not finite")):
        args = list(ok)
        args[change[0]] = change[1]
        with pytest.raises(ValueError) as e:
            A.als_host(*args, rank=2)
        assert str(e.value) == message
    with pytest.raises(ValueError, match="init_user row 1: a value is not finite"):
        A.als_host(*ok, rank=2, init_user=np.array([[1, 2], [np.inf, 1]], np.float32))
    # reg = 0 at rank 4 on a movie of 2 ratings: the normal equations are singular (unit vectors: d = 0 - 0 exactly at j = 2)
    with pytest.raises(ValueError, match="movieId 1: the normal equations are not positive definite"):
        A.als_host(cases.SINGULAR["user"], cases.SINGULAR["movie"], cases.SINGULAR["rating"], 6, 2, rank=4, reg=0.0, iters=1, init_user=cases.SINGULAR["init"])
    for bad in (dict(rank=0), dict(rank=17), dict(iters=-1), dict(reg=float("nan")), dict(reg=-1.0)):
        with pytest.raises(ValueError):
            A.als_host(*ok, **bad)


def test_split_is_a_partition_in_input_order():
    ratings = {"userId": np.arange(100), "movieId": np.arange(100) * 2, "rating": np.arange(100) / 20.0}
    train, test = A.split(ratings, (0.8, 0.2), seed=4)
    assert len(train["userId"]) == 80 and len(test["userId"]) == 20
    assert sorted(train["userId"].tolist() + test["userId"].tolist()) == list(range(100))
    assert (np.diff(train["userId"]) > 0).all() and (train["movieId"] == 2 * train["userId"]).all()
    again, _ = A.split(ratings, (0.8, 0.2), seed=4)
    assert again["userId"].tolist() == train["userId"].tolist()


def test_topk_host_ties_padding_and_rows_without_factors():
    table = np.array([[1, 0], [2, 0], [1, 0], [5, 5], [0.5, 0]], dtype=np.float32)
    has = np.array([1, 1, 1, 0, 1], dtype=np.uint8)
    rows, scores = A.topk_host(np.array([[1, 1], [1, 1]], np.float32), [1, 0], table, has, 6)
    assert rows[0].tolist() == [1, 0, 2, 4, -1, -1] and scores[0, :4].tolist() == [2, 1, 1, 0.5] and np.isnan(scores[0, 4:]).all()
    assert rows[1].tolist() == [-1] * 6 and np.isnan(scores[1]).all()


# ---------------------------------------------------------------- the C ABI's checks, before any device call

def _fit_args(**over):
    n, nu, ni, rank = 4, 3, 2, 2
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    base += -base % 16
    a = dict(user=base, movie=base + 64, rating=base + 128, n=n, nu=nu, ni=ni, rank=rank, reg=0.01, iters=1, init=base + 192, init_stride=rank,
             uf=base + 256, us=rank, itf=base + 320, is_=rank, uh=base + 384, ih=base + 400, uc=base + 416, ic=base + 448, err=base + 480,
             ws=base + 512, ws_bytes=3072, stream=None)
    a.update(over)
    return buf, [a[k] for k in ("user", "movie", "rating", "n", "nu", "ni", "rank", "reg", "iters", "init", "init_stride", "uf", "us", "itf", "is_", "uh", "ih",
                                "uc", "ic", "err", "ws", "ws_bytes", "stream")], base


def test_fit_arguments_are_checked_before_any_device_call(lib):
    need = lib.sprk_als_workspace_bytes(4, 3, 2, 2)
    assert 0 < need <= 3072 and need % 16 == 0
    _, _, base = _fit_args()
    bad = [dict(rank=0), dict(rank=17), dict(iters=-1), dict(reg=float("nan")), dict(reg=float("inf")), dict(reg=-0.5), dict(n=-1), dict(nu=-1), dict(ni=-1),
           dict(user=None), dict(rating=None), dict(init=None), dict(uf=None), dict(itf=None), dict(uh=None), dict(ic=None), dict(err=None), dict(ws=None),
           dict(us=1), dict(is_=1), dict(init_stride=1), dict(ws_bytes=need - 1), dict(n=1 << 31)]
    for over in bad:
        keep, args, _ = _fit_args(**over)
        assert lib.sprk_als_fit(*args) == L.EINVAL, over
        assert lib.sprk_last_error()
    for key, off in (("user", 2), ("movie", 1), ("rating", 2), ("init", 2), ("uf", 1), ("itf", 2), ("uc", 2), ("ic", 1), ("err", 4), ("ws", 8)):
        keep, args, b = _fit_args()
        names = ("user", "movie", "rating", "n", "nu", "ni", "rank", "reg", "iters", "init", "init_stride", "uf", "us", "itf", "is_", "uh", "ih", "uc", "ic", "err", "ws")
        args[names.index(key)] += off
        assert lib.sprk_als_fit(*args) == L.EINVAL, key
    keep, args, _ = _fit_args(ws_bytes=16)
    assert lib.sprk_als_fit(*args) == L.EINVAL and (b"%d bytes" % need) in lib.sprk_last_error()
    for sizes in ((-1, 3, 2, 2), (4, -1, 2, 2), (4, 3, -1, 2), (4, 3, 2, 0), (4, 3, 2, 17), (1 << 31, 3, 2, 2)):
        assert lib.sprk_als_workspace_bytes(*sizes) == 0, sizes


def test_predict_and_topk_arguments_are_checked_before_any_device_call(lib):
    buf = (C.c_char * 1024)()
    b = C.addressof(buf)
    b += -b % 16
    good = [b, b + 64, 4, b + 128, 2, b + 192, b + 256, 2, b + 320, 3, 2, 2, b + 384, None]
    for at, value in ((2, -1), (4, 1), (7, 1), (9, -1), (10, -1), (11, 0), (11, 17), (0, None), (12, None), (3, None), (5, None), (6, None), (8, None), (0, b + 2), (12, b + 386)):
        args = list(good)
        args[at] = value
        assert lib.sprk_als_predict(*args) == L.EINVAL, (at, value)
    good = [b, b + 64, 5, 2, 2, b + 128, b + 192, 3, 2, 4, b + 256, b + 320, None, 0, None]
    for at, value in ((2, -1), (3, 0), (3, 17), (4, 1), (7, -1), (8, 1), (9, 0), (9, 1025), (0, None), (1, None), (5, None), (6, None), (10, None), (11, None), (0, b + 1)):
        args = list(good)
        args[at] = value
        assert lib.sprk_als_topk(*args) == L.EINVAL, (at, value)
    assert lib.sprk_als_topk_workspace_bytes(5, 3, 0) == 0 and lib.sprk_als_topk_workspace_bytes(5, 3, 1025) == 0 and lib.sprk_als_topk_workspace_bytes(-1, 3, 4) == 0
    assert lib.sprk_als_topk_workspace_bytes(4096, 3, 10) == 0                    # one chunk: no workspace
    big = lib.sprk_als_topk_workspace_bytes(10000, 3, 10)
    assert big > 0
    args = [b, b + 64, 10000, 2, 2, b + 128, b + 192, 3, 2, 10, b + 256, b + 320, b + 512, 64, None]
    assert lib.sprk_als_topk(*args) == L.EINVAL and (b"%d bytes" % big) in lib.sprk_last_error()
