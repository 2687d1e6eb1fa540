"""User embeddings from ratings (sparrowrecsys_amd/userembedding.py): the host definition against its row-by-row restatement and the
hand-worked user, the properties of the cases the device tests rely on, sprk_user_emb's argument checks (no GPU) and the text form."""
import ctypes as C

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import ranker as R
from sparrowrecsys_amd import userembedding as UE
from tests import userembedding_cases as cases


def _host(case, mode, D=None):
    D = case["emb"].shape[1] if D is None else D
    return UE.user_emb_host(case["user"], case["row"], case["emb"][:, :D], case["has"], case["n_users"], mode)


def _same(got, want):
    for g, w, name in zip(got, want, ("emb", "has", "count")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))[:8])


@pytest.mark.parametrize("mode", ["mean", "sum"])
def test_hand_worked_user(mode):
    case = cases.hand_worked()
    emb, has, count = _host(case, mode)
    assert emb.view(np.uint32).tolist() == (cases.HAND_MEAN_WORDS if mode == "mean" else cases.HAND_SUM_WORDS).tolist()
    assert has.tolist() == [1] and count.tolist() == [cases.HAND_COUNT[mode]]
    _same((emb, has, count), cases.loop_reference(case["user"], case["row"], case["emb"], case["has"], 1, mode))
    forward = cases.loop_reference(case["user"], case["row"], case["emb"], case["has"], 1, "sum", forward=True)[0]
    assert forward.view(np.uint32).tolist() == cases.HAND_FORWARD_SUM_WORDS.tolist()


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("mode", ["mean", "sum"])
def test_host_definition_equals_the_plain_loop(mode, grouped):
    case = cases.synthetic(grouped=grouped)
    D = case["D"]
    _same(_host(case, mode, D), cases.loop_reference(case["user"], case["row"], case["emb"][:, :D], case["has"], case["n_users"], mode))


def test_grouped_copy_has_the_same_result():
    a, b = cases.synthetic(), cases.synthetic(grouped=True)
    assert (np.diff(b["user"]) >= 0).all() and (np.diff(a["user"]) < 0).any()
    _same(_host(a, "mean", 10), _host(b, "mean", 10))


def test_synthetic_set_holds_the_cases_it_names():
    case = cases.synthetic()
    user, row, has, emb = case["user"], case["row"], case["has"], case["emb"]
    assert (len(user), case["n_users"], len(has), emb.shape) == (5000, 97, 211, (211, 12))
    lens = np.bincount(user, minlength=97)
    assert [lens[u] for u in cases.NO_RATING_USERS] == [0, 0, 0] and (lens > 0).sum() == 94
    assert lens[cases.LONG_USER] == 300 and lens[cases.COUNT_3_USER] == 3 and lens[cases.COUNT_7_USER] == 7
    assert (has == 0).sum() == 42 and np.isnan(emb[has == 0, :10]).all() and not np.isnan(emb[has == 1, :10]).any()
    assert (row == -1).any() and (row == 211).any() and (row > 211).any()
    assert (emb[:, 10:] == cases.PAD).all()
    mags = np.abs(emb[has == 1, :10]).max(axis=1)
    assert (mags < 1e-2).any() and (mags > 1e2).any()
    got, g_has, count = _host(case, "mean", 10)
    assert g_has[cases.NO_EMBEDDING_USER] == 1 and count[cases.NO_EMBEDDING_USER] == 9 and not got[cases.NO_EMBEDDING_USER].any()
    assert not g_has[list(cases.NO_RATING_USERS)].any() and not got[list(cases.NO_RATING_USERS)].any()
    s_emb, s_has, s_count = _host(case, "sum", 10)
    assert s_has[cases.NO_EMBEDDING_USER] == 0 and s_count[cases.NO_EMBEDDING_USER] == 0
    assert not np.isnan(got).any()                             # no has = 0 row was added
    # the division rounds: for the users of 3 and 7 ratings the quotient times the count is not the sum
    for u in (cases.COUNT_3_USER, cases.COUNT_7_USER):
        assert (got[u] * np.float32(count[u]) != s_emb[u]).any()


def test_forward_sum_differs_from_the_definition():
    """The cases' power to detect a wrong order: summing first row to last changes most of the output words."""
    case = cases.synthetic()
    want = _host(case, "sum", 10)[0]
    forward = cases.loop_reference(case["user"], case["row"], case["emb"][:, :10], case["has"], case["n_users"], "sum", forward=True)[0]
    differ = (want.view(np.uint32) != forward.view(np.uint32))
    assert differ.mean() > 0.5, differ.mean()


def test_bad_user_id_names_the_first_bad_row():
    case = cases.synthetic()
    user = case["user"].astype(np.int64)
    user[[900, 31]] = [97, -1]
    with pytest.raises(ValueError) as e:
        UE.user_emb_host(user, case["row"], case["emb"][:, :10], case["has"], 97)
    assert str(e.value) == "ratings row 31: userId outside the user table"
    with pytest.raises(ValueError):
        UE.user_emb_host(case["user"], case["row"], case["emb"][:, :10], case["has"], 97, mode="median")


def test_user_emb_abi_rejects_bad_arguments_before_any_device_call(lib):
    n, nu, ni, D = 8, 4, 5, 10
    need = lib.sprk_user_emb_workspace_bytes(n, nu)
    assert need > 0 and need % 16 == 0
    assert lib.sprk_user_emb_workspace_bytes(-1, nu) == 0 and lib.sprk_user_emb_workspace_bytes(n, -1) == 0
    assert lib.sprk_user_emb_workspace_bytes(2**31 - 1, nu) == 0 and lib.sprk_user_emb_workspace_bytes(n, 2**31 - 1) == 0
    # host memory stands in for device memory: every call below must return before it touches any of it
    buf = (C.c_uint64 * (need // 8 + 64))()
    p = C.c_void_p(C.addressof(buf))
    off = lambda k: C.c_void_p(C.addressof(buf) + k)
    def call(**kw):
        a = dict(user=p, row=p, n=n, nu=nu, emb=p, has=p, ni=ni, D=D, istride=D, mode=0, out=p, ostride=D, ohas=p, ocount=p, err=p, ws=p, ws_bytes=need)
        a.update(kw)
        return lib.sprk_user_emb(a["user"], a["row"], a["n"], a["nu"], a["emb"], a["has"], a["ni"], a["D"], a["istride"], a["mode"], a["out"], a["ostride"],
                                 a["ohas"], a["ocount"], a["err"], a["ws"], a["ws_bytes"], None)
    bad = [dict(user=None), dict(row=None), dict(emb=None), dict(has=None), dict(out=None), dict(ohas=None), dict(ocount=None), dict(err=None), dict(ws=None),
           dict(user=off(2)), dict(row=off(2)), dict(emb=off(1)), dict(out=off(2)), dict(ocount=off(2)), dict(err=off(4)), dict(ws=off(8)),
           dict(n=-1), dict(nu=-1), dict(ni=-1), dict(n=2**31 - 1), dict(D=0), dict(D=1025), dict(istride=D - 1), dict(ostride=D - 1), dict(mode=2), dict(mode=-1),
           dict(ws_bytes=need - 16), dict(ws_bytes=0)]
    for kw in bad:
        assert call(**kw) == L.EINVAL, kw
        assert b"user_emb" in lib.sprk_last_error()
    assert call(ws_bytes=need - 16) == L.EINVAL
    assert ("needs a workspace of %d bytes" % need).encode() in lib.sprk_last_error()
    import torch
    if not torch.cuda.is_available():
        assert call() == L.EHIP                                 # a good call reaches the device, and there is none


def test_save_and_load_emb_file_round_trip_the_bits(tmp_path):
    case = cases.synthetic()
    emb, has, count = _host(case, "mean", 10)
    emb = emb.copy()
    emb[0, :4] = [1e-40, -0.0, np.float32(1) / np.float32(3), 3.4028235e38]      # a subnormal, a signed zero, a rounded quotient, the largest
    ue = UE.UserEmbeddings(emb, has, count)
    path = str(tmp_path / "userEmb.csv")
    assert ue.save(path) == int(has.sum()) == 94
    back = R.load_emb_file(path)
    assert sorted(back) == np.flatnonzero(has).tolist()
    for u, v in back.items():
        assert v.dtype == np.float32 and v.tobytes() == emb[u].tobytes(), u
    assert ue.vector(cases.NO_RATING_USERS[0]) is None and ue.vector(-1) is None and ue.vector(97) is None
    assert ue.vector(3).tobytes() == emb[3].tobytes()
    got = ue.to_host()
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, (emb, has, count)))
