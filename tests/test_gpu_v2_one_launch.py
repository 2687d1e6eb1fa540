"""DeepFM_v2 ``forward_many`` beyond one kernel-argument table (``-m gpu``): a call of more batches than ``many_batches`` is ONE launch
of k_deepfm_v2_joint_many_tab, its per-batch pointers in an engine-owned device table.  Every case compares with a ``forward`` per batch,
bit for bit (``torch.equal``): samples are independent, the chains are the same.  Small vocabularies, small batches: seconds in all."""
import os

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import synthetic as SY

pytestmark = pytest.mark.gpu

FIELDS = [(k, kind, min(v, 1000) if kind == "id" else v) for k, kind, v in SY.CONFIG2_FIELDS]
N_MAX = 130


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    assert os.path.exists(L.LIB_PATH), "libsparrow_hip.so must be built in-tree"
    return t


@pytest.fixture(scope="module")
def model(torch):
    m = M.DeepFMv2(seed=71, emb_dim=16, fields=FIELDS, proj_dim=16)
    assert m.engine.kernel_name() == "k_deepfm_v2_joint"
    return m


def _batches(torch, model, B, n, seed):
    """n packed batches of B rows on the device, and their scores from one ``forward`` each (the reference, computed once)."""
    ids, dense, ref = [], [], []
    for i in range(n):
        f = SY.synth_fields(B, FIELDS, seed=seed + i, dist="zipf" if i % 2 else "uniform")
        pi, pd = model.pack(f)
        ids.append(torch.from_numpy(np.ascontiguousarray(pi)).cuda())
        dense.append(torch.from_numpy(np.ascontiguousarray(pd)).cuda())
        o = torch.full((B,), -1.0, dtype=torch.float32, device="cuda")
        model.engine.forward(ids[-1], dense[-1], o)
        ref.append(o)
    torch.cuda.synchronize()
    model.engine.check_ids()
    return ids, dense, ref


@pytest.fixture(scope="module")
def b48(torch, model):
    return _batches(torch, model, 48, N_MAX, 300)


def _many(torch, eng, ids, dense, per_launch=64):
    B = ids[0].shape[0]
    outs = [torch.full((B,), -1.0, dtype=torch.float32, device="cuda") for _ in ids]
    eng.set_many_batches(per_launch)
    try:
        eng.forward_many(ids, dense, outs)
        torch.cuda.synchronize()
    finally:
        eng.set_many_batches(1)
    return outs


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_batch_counts_across_the_table_cap(torch, model, b48, n):
    """B = 48 (three tasks per batch): below, at and above the 64 batches one kernel-argument table holds; both parities of tasks per
    wave; fewer tasks than waves (idle waves leave after the barrier)."""
    ids, dense, ref = b48
    outs = _many(torch, model.engine, ids[:n], dense[:n])
    model.engine.check_ids()
    for i in range(n):
        assert torch.equal(outs[i], ref[i]), "batch %d of %d" % (i, n)


@pytest.mark.parametrize("B", [17, 1])
def test_partial_last_task(torch, model, B):
    ids, dense, ref = _batches(torch, model, B, 66, 500 + B)
    outs = _many(torch, model.engine, ids, dense)
    model.engine.check_ids()
    for i in range(len(ids)):
        assert torch.equal(outs[i], ref[i]), "batch %d" % i


@pytest.mark.parametrize("per_launch", [64, 2])
def test_more_than_two_tasks_per_wave_odd_tail(torch, model, per_launch):
    """B = 16 x 2 048 x 2 + 16, three batches: every wave of a full chip loops, and the last task of the launch stands alone.
    per_launch = 64: the kernel-argument table; 2: three batches exceed it, the device table."""
    B = 16 * 2048 * 2 + 16
    ids, dense, ref = _batches(torch, model, B, 3, 700)
    outs = _many(torch, model.engine, ids, dense, per_launch)
    model.engine.check_ids()
    for i in range(3):
        assert torch.equal(outs[i], ref[i]), "batch %d" % i


def test_unaligned_ids_fall_back(torch, model, b48):
    ids, dense, ref = b48
    n, B, F = 70, 48, ids[0].shape[1]
    big = torch.empty(B * F + 3, dtype=torch.int32, device="cuda")
    off = big[1:1 + B * F].view(B, F).copy_(ids[5])
    assert off.data_ptr() % 16 != 0
    use = ids[:5] + [off] + ids[6:n]
    outs = _many(torch, model.engine, use, dense[:n])
    model.engine.check_ids()
    for i in range(n):
        assert torch.equal(outs[i], ref[i]), "batch %d" % i


def test_prepared_run_replayed_and_slots_alternate(torch, model, b48):
    """The same prepared run twice (the second call finds its table uploaded), another pointer set (the other slot), the first again
    (uploaded anew over the slot the first two calls read), and once more on another stream (never taken for the table uploaded last)."""
    ids, dense, ref = b48
    eng = model.engine
    n1, n2 = 100, 90
    out1 = [torch.full((48,), -1.0, dtype=torch.float32, device="cuda") for _ in range(n1)]
    out2 = [torch.full((48,), -1.0, dtype=torch.float32, device="cuda") for _ in range(n2)]
    eng.set_many_batches(64)
    try:
        run1 = eng.prepare_many(ids[:n1], dense[:n1], out1)
        run2 = eng.prepare_many(ids[N_MAX - n2:], dense[N_MAX - n2:], out2)   # other inputs, other outputs, another count
    finally:
        eng.set_many_batches(1)

    def check(outs, first):
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert torch.equal(o, ref[first + i]), "batch %d" % i
            o.fill_(-1.0)
        torch.cuda.synchronize()

    run1()
    check(out1, 0)
    run1()
    check(out1, 0)
    run2()
    check(out2, N_MAX - n2)
    run1()
    run2()                                   # back to back, nothing waited for in between
    torch.cuda.synchronize()
    for i, o in enumerate(out2):
        assert torch.equal(o, ref[N_MAX - n2 + i])
    check(out1, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    run1(stream=side.cuda_stream)
    side.synchronize()
    check(out1, 0)
    eng.check_ids()


def test_missing_and_out_of_range_ids(torch, model, b48):
    ids, dense, ref = b48
    n, k = 80, 77
    bad = ids[k].clone()
    bad[3, 0] = -1                           # the "missing" marker: the zero row, not an error
    bad[40, 1] = 10 ** 6                     # no such row: flagged, scored as the zero row
    use = ids[:k] + [bad] + ids[k + 1:n]
    outs = _many(torch, model.engine, use, dense[:n])
    with pytest.raises(ValueError):
        model.engine.check_ids()
    model.engine.check_ids()                 # (the flag was cleared)
    keep = torch.ones(48, dtype=torch.bool, device="cuda")
    keep[3] = False
    keep[40] = False
    for i in range(n):
        if i == k:
            assert torch.equal(outs[i][keep], ref[i][keep])
            assert not torch.equal(outs[i][~keep], ref[i][~keep])
        else:
            assert torch.equal(outs[i], ref[i]), "batch %d" % i
    # the same batch through a launch of its own: the same scores in the two changed rows as well
    one = torch.full((48,), -1.0, dtype=torch.float32, device="cuda")
    model.engine.forward(bad, dense[k], one)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        model.engine.check_ids()
    assert torch.equal(outs[k], one)
