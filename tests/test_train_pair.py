"""The pair-dot DeepFM trainer's definition (sparrowrecsys_amd/trainer_pair.py, ``train_host``) against independent implementations; no GPU.
The measured figures are in docs/train_pair_results.md."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import synthetic as S
from sparrowrecsys_amd import trainer as T
from sparrowrecsys_amd import trainer_fm as TF
from sparrowrecsys_amd import trainer_pair as TP
from tests import train_pair_cases as TPC
from tests.conftest import ROOT

F = np.float32
same = TPC.same_bits
SHARED = [False, True]
SIX_REFERENCE = [("movieId", "id", 1001), ("userId", "id", 30001), ("userRatedMovie1", "id", 1001), ("userGenre1", "genre", 19), ("userGenre2", "genre", 19),
                 ("movieGenre1", "genre", 19)]


# ---------------------------------------------------------------- the family

def test_family_of_the_reference_model():
    model = M.DeepFM(seed=1)
    fam = TP.family_of(model)
    keys = [k for k, _, _ in fam.fields]
    assert fam.fields == [("movieId", "id", 1001), ("userId", "id", 30001), ("userGenre1", "genre", 19), ("movieGenre1", "genre", 19)] == fam.columns
    assert dict(zip(keys, fam.fo_off)) == {"movieGenre1": 0, "movieId": 19, "userGenre1": 1020, "userId": 1039} and fam.fo_total == 31040
    assert [(keys[a], keys[b]) for a, b in fam.pairs] == M.DeepFM.DEFAULT_PAIRS and fam.pairs == [(0, 1), (3, 2), (3, 1), (0, 2)]
    assert fam.deep_cols == [0, 1] and fam.shared is False and (fam.emb_dim, fam.n_dense, fam.hidden) == (10, 7, [64, 64])
    rows, n_x = model._deep_rows()
    assert n_x == len(fam.xsrc) == len(fam.xsub) == 27
    for j, k in enumerate(model.deep_emb):
        r = rows[k + "_embedding"]
        assert fam.xsrc[r:r + 10] == [j] * 10 and fam.xsub[r:r + 10] == list(range(10))
    assert [fam.xsrc[rows[k]] for k in model.numeric_keys] == [-1] * 7 and [fam.xsub[rows[k]] for k in model.numeric_keys] == list(range(7))
    assert TP.default_tile(fam) == TF.DEFAULT_TILE == 8 and TP.lds_bytes(fam, 8) == 4 * 8 * (4 * 10 + 27 + 128 + 8 + 2 * 64)


@pytest.mark.parametrize("kw", [dict(), dict(share_deep_tables=True), dict(emb_dim=16, fields=SIX_REFERENCE, pairs=S.CONFIG2_PAIRS, deep_emb=("movieId", "userGenre2"))])
def test_param_shapes_are_weight_shapes(kw):
    model = M.DeepFM(seed=1, **kw)
    fam = TP.family_of(model)
    names, shapes = TP.param_names(fam), TP.param_shapes(fam)
    assert sorted(names) == sorted(model.weight_shapes()) == sorted(shapes) and all(shapes[k] == tuple(s) for k, s in model.weight_shapes().items())
    assert names[:len(fam.fields)] == ["emb/" + k for k, _, _ in fam.fields] and names[-2:] == ["head/bias", "head/kernel"]
    deep = [n for n in names if n.startswith("deep_emb/")]
    assert deep == ([] if fam.shared else ["deep_emb/" + k for k in model.deep_emb]) and names.index("deep0/kernel") == len(fam.fields) + len(deep)
    assert fam.shared == bool(kw.get("share_deep_tables"))


def test_family_of_takes_deepfm_itself_only(samples):
    class Sub(M.DeepFM):
        pass
    for make in (lambda: Sub(seed=1), lambda: M.DeepFMv2(seed=1), lambda: M.WideNDeep(seed=1), lambda: M.EmbeddingMLP(seed=1), lambda: M.DIN(seed=1),
                 lambda: M.NeuralCF(seed=1)):
        with pytest.raises(NotImplementedError, match="trainer_pair trains DeepFM, not"):
            TP.family_of(make())
    with pytest.raises(NotImplementedError, match="trainer_pair trains DeepFM"):
        TP.fit(M.DeepFMv2(seed=1), samples)
    with pytest.raises(NotImplementedError, match=r"NeuralCF\(arch=1\) and EmbeddingMLP, and DeepFMv2 through trainer_fm, not for DeepFM"):
        M.DeepFM(seed=1).fit({"label": np.zeros(1)})


def test_one_over_each_limit_raises_in_words():
    words = "trainer_pair takes up to 8 fields, 1 to 32 pairs"
    with pytest.raises(ValueError, match=words):
        TPC.family(emb_dim=TP.MAX_DIM + 1, deep_emb=())
    assert TPC.family(emb_dim=TP.MAX_DIM, deep_emb=()).emb_dim == TP.MAX_DIM
    for kw in (dict(hidden=(TP.MAX_WIDTH + 1,)), dict(hidden=(2,) * (TP.MAX_LAYERS + 1)), dict(pairs=[]), dict(pairs=[("movieId", "userId")] * (TP.MAX_PAIRS + 1)),
               dict(fields=TPC.EIGHT + [("f8", "id", 2)], pairs=TPC.EIGHT_PAIRS, deep_emb=()), dict(emb_dim=63, deep_emb=("movieId", "userId", "userGenre1", "movieGenre1")),
               dict(deep_emb=(), n_dense=0)):
        with pytest.raises(ValueError, match=words):
            TPC.family(**kw)
    assert len(TPC.family(pairs=[("movieId", "userId")] * TP.MAX_PAIRS).pairs) == TP.MAX_PAIRS
    assert TPC.family(pairs=[("movieId", "movieId")]).pairs == [(0, 0)]    # a pair (a, a) is legal
    fam = TPC.family()
    with pytest.raises(ValueError, match="a pair names two fields"):
        TP._check_family(fam._replace(pairs=[(0, 4)]))
    with pytest.raises(ValueError, match="the deep keys are distinct fields"):
        TP._check_family(fam._replace(deep_cols=[0, 0]))
    with pytest.raises(ValueError, match="every numeric, once each"):
        TP._check_family(fam._replace(xsub=fam.xsub[:-1] + [fam.xsub[-2]]))
    with pytest.raises(ValueError, match="must be distinct and every pair and deep key must name a field"):
        TPC.family(pairs=[("movieId", "nobody")])
    with pytest.raises(ValueError, match="the schedule's key holds fewer than 2\\^31 - 1 rows"):
        TPC.family(fields=[("movieId", "id", TP.MAX_ROWS - 5), ("userId", "id", 5)], pairs=[("movieId", "userId")], deep_emb=())


# ---------------------------------------------------------------- forward

def _oracle_case(samples, shape, shared):
    if shape == "reference":
        return M.DeepFM(seed=11, share_deep_tables=shared), samples
    model = M.DeepFM(seed=12, emb_dim=16, fields=SIX_REFERENCE, pairs=S.CONFIG2_PAIRS, deep_emb=("movieId", "userId"), share_deep_tables=shared)
    return model, samples


@pytest.mark.parametrize("shared", SHARED)
@pytest.mark.parametrize("shape", ["reference", "six fields, eight pairs"])
def test_forward_matches_the_float64_oracle(samples, shape, shared):
    """The definition's float32 forward against oracle.ctr_oracle.deepfm_forward in float64 on the golden rows, random trained-like weights: the
    reference shape and config 2's six fields and eight pairs at emb_dim 16, tables shared and not; within 1e-4 absolute, the bound
    tests/test_train_wide.py holds the same comparison to."""
    from oracle import ctr_oracle as O
    model, feats = _oracle_case(samples, shape, shared)
    fam = TP.family_of(model)
    ids, dense = model._pack_python(feats)
    got = TP.forward_host(fam, model.weights, ids, dense)
    want = O.deepfm_forward(feats, model.weights, dtype=np.float64, fields=model.fields, pairs=model.pairs, deep_emb=model.deep_emb, share_deep_tables=shared).reshape(-1)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("pair-dot DeepFM %s shared %s: max |p - oracle| = %.3e over %d rows" % (shape, shared, err, len(got)))
    assert got.dtype == F and len(got) == 256 and err <= 1e-4 and (ids[:, [c for c, f in enumerate(fam.fields) if f[1] == "genre"]] == -1).any()


# ---------------------------------------------------------------- gradients

PINNED = dict(pairs=[("movieId", "userId"), ("movieGenre1", "movieId"), ("movieId", "userGenre1"), ("movieId", "movieId"), ("userGenre1", "movieGenre1")],
              deep_emb=("movieGenre1", "userId"))                         # movieId in three pairs and in (a, a); genre ids of -1 in pairs and in the deep part


@pytest.mark.parametrize("shared", SHARED)
@pytest.mark.parametrize("tile", [1, 8, 200])
def test_step_gradients_match_float64_and_torch_autograd(shared, tile):
    """One step's gradients against a float64 restatement in plain numpy (which must agree with torch CPU autograd in float64 to 1e-12) on 200
    rows (tile 200 = n), five fixed draws, every parameter, tables shared and not, over the pinned family: one table in three pairs, the pair
    ``(a, a)``, a quarter of the genre ids -1 in pairs and in the deep part.  tests/test_train_wide.py's bound for the same comparison: per
    tensor, the definition's largest error relative to the tensor's largest magnitude is at most 4 x the same error of torch's own float32
    autograd; a small tensor whose gradient is a cancelling sum over the samples may exceed the ratio and is then held to the sequential-sum
    bound (terms - 1) 2^-24 sum |term|, the terms from the float64 run."""
    import torch
    fam = TPC.family(shared=shared, **PINNED)
    mine, theirs, runs = {}, {}, []
    for seed in range(5):
        w = TPC.weights(fam, 3 + seed)
        ids, dense, y = TPC.data(fam, 200, 5 + seed)
        assert (ids[:, 2] == -1).any() and (ids[:, 3] == -1).any()
        g, p = TP.step_gradients(fam, w, ids, dense, y, tile)
        g64, p64 = TPC.torch_gradients(fam, w, ids, dense, y, torch.float64)
        gnp, pnp = TPC.float64_gradients(fam, w, ids, dense, y)
        g32, _ = TPC.torch_gradients(fam, w, ids, dense, y, torch.float32)
        runs.append((w, ids, dense, y, g, g64))
        assert float(np.abs(p - p64).max()) <= 1e-6 and float(np.abs(pnp - p64).max()) <= 1e-12
        assert set(g) == set(TP.param_names(fam)) == set(w) == set(gnp)
        for k in TP.param_names(fam):
            assert g[k].dtype == F and g[k].shape == w[k].shape
            big = float(np.abs(g64[k]).max())
            assert big > 0.0, k
            assert float(np.abs(gnp[k].reshape(g64[k].shape) - g64[k]).max()) <= 1e-12 * max(big, 1.0), k
            mine[k] = max(mine.get(k, 0.0), float(np.abs(g[k] - g64[k]).max()) / big)
            theirs[k] = max(theirs.get(k, 0.0), float(np.abs(g32[k] - g64[k]).max()) / big)
    for k in sorted(mine):
        print("shared %s tile %d %-18s definition %.3e torch float32 %.3e ratio %.2f" % (shared, tile, k, mine[k], theirs[k], mine[k] / max(theirs[k], 1e-300)))
    for k in sorted(mine):
        if mine[k] <= 4.0 * theirs[k]:
            continue
        assert w[k].size <= 64, k                                          # a small tensor whose gradient is a cancelling sum over the samples
        for w_, ids, dense, y, g, g64 in runs:
            terms = TPC.torch_sample_terms(fam, w_, ids, dense, y, k)
            bound = (len(y) - 1) * 2.0 ** -24 * np.abs(terms).sum(axis=0)
            worst = float((np.abs(g[k] - g64[k]) / np.maximum(bound, 1e-300)).max())
            print("shared %s tile %d %-18s cancelling sum: error / sequential-sum bound = %.3f" % (shared, tile, k, worst))
            assert worst <= 1.0, k


def test_a_row_gradient_walks_the_pairs_in_order():
    """One sample, one tile: ``emb/movieId``'s row gradient is the explicit chain -- from +0, per pair in pair order, as ``a`` then as ``b`` --
    over the pinned family (movieId: pair 0 as a, pair 1 as b, pair 2 as a, pair 3 as a and as b).  With pairs 0 and 2 swapped the same terms
    are added in another order and the bits differ (seed 0: checked here, not assumed), while the dots' kernel rows swap exactly."""
    fam, w, ids, dense, y = TPC.small(1, seed=0, emb_dim=8, **PINNED)
    ids[0] = [3, 2, 1, 2]
    T_, P = fam.fo_total, len(fam.pairs)
    g, p = TP.step_gradients(fam, w, ids, dense, y, 8)
    dl = ((p - y) / F(1)).astype(F)[0]
    t = [(F(0) + w["head/kernel"][T_ + q, 0] * dl).astype(F) for q in range(P)]
    e = {k: w["emb/" + k][ids[0, f]] for f, (k, _, _) in enumerate(fam.fields)}

    def chain(order):
        s = np.zeros(8, dtype=F)
        for q in order:
            a, b = (fam.fields[c][0] for c in fam.pairs[q])
            if a == "movieId":
                s = s + t[q] * e[b]
            if b == "movieId":
                s = s + t[q] * e[a]
        return (np.zeros(8, dtype=F) + s).astype(F)                        # one tile, then the tiles: + 0 changes no bit
    assert same(g["emb/movieId"][3], chain(range(P))) and not g["emb/movieId"][[0, 1, 2, 4, 5, 6]].any()
    assert not same(chain(range(P)), chain([2, 1, 0, 3, 4]))
    swapped = fam._replace(pairs=[fam.pairs[q] for q in (2, 1, 0, 3, 4)])
    ws = dict(w, **{"head/kernel": w["head/kernel"].copy()})
    ws["head/kernel"][[T_, T_ + 2]] = w["head/kernel"][[T_ + 2, T_]]
    gs, ps = TP.step_gradients(swapped, ws, ids, dense, y, 8)
    assert same(gs["emb/movieId"][3], chain([2, 1, 0, 3, 4])) and not same(gs["emb/movieId"][3], g["emb/movieId"][3])
    assert same(gs["head/kernel"][[T_ + 2, T_]], g["head/kernel"][[T_, T_ + 2]])
    twice = TPC.family(pairs=[("movieId", "movieId")], emb_dim=8, deep_emb=PINNED["deep_emb"])     # (a, a): the same vector twice
    g2, p2 = TP.step_gradients(twice, dict(w, **{"head/kernel": w["head/kernel"][:twice.fo_total + 1 + 5]}), ids, dense, y, 8)
    t0 = (F(0) + w["head/kernel"][twice.fo_total, 0] * ((p2 - y) / F(1)).astype(F)[0]).astype(F)
    assert same(g2["emb/movieId"][3], ((np.zeros(8, dtype=F) + t0 * e["movieId"]) + t0 * e["movieId"]).astype(F))


@pytest.mark.parametrize("shared", SHARED)
def test_the_deep_gradient_goes_to_the_right_table(shared):
    """Shared: ``emb/userId`` receives the pairs' terms and then the deep input's gradient; not shared: the latter is ``deep_emb/userId``'s."""
    fam, w, ids, dense, y = TPC.small(1, seed=2, shared=shared, pairs=[("movieId", "userId")])
    g, p = TP.step_gradients(fam, w, ids, dense, y, 8)
    dl = ((p - y) / F(1)).astype(F)[0]
    t = (F(0) + w["head/kernel"][fam.fo_total, 0] * dl).astype(F)
    pair_term = (np.zeros(3, dtype=F) + t * w["emb/movieId"][ids[0, 0]]).astype(F)
    if shared:
        apart = TPC.family(pairs=[("movieId", "userId")])
        wa = dict(w, **{"deep_emb/movieId": w["emb/movieId"], "deep_emb/userId": w["emb/userId"]})
        ga, pa = TP.step_gradients(apart, wa, ids, dense, y, 8)
        assert same(pa, p) and same(ga["emb/userId"][ids[0, 1]], pair_term)
        assert same(g["emb/userId"][ids[0, 1]], (pair_term + ga["deep_emb/userId"][ids[0, 1]]).astype(F))
    else:
        assert same(g["emb/userId"][ids[0, 1]], pair_term) and g["deep_emb/userId"][ids[0, 1]].any()


def test_gradients_are_summed_tile_by_tile():
    """Every sample carries the same ids: a row's gradient is the explicit two-level float32 sum -- a tile's samples from +0, then the tiles
    from +0 -- and differs in bits from the flat sum (seed 0: checked here, not assumed); the first-order row likewise."""
    fam, w, ids, dense, y = TPC.small(50, seed=0)
    ids[:] = 1
    tile = 8
    g, p = TP.step_gradients(fam, w, ids, dense, y, tile)
    dl = ((p - y) / F(50)).astype(F)

    def sums(terms):
        two = np.zeros(terms.shape[1:], dtype=F)
        for t0 in range(0, 50, tile):
            s = np.zeros(terms.shape[1:], dtype=F)
            for i in range(t0, min(50, t0 + tile)):
                s = s + terms[i]
            two = two + s
        flat = np.zeros(terms.shape[1:], dtype=F)
        for i in range(50):
            flat = flat + terms[i]
        return two, flat
    two, flat = sums(dl)
    assert same(g["head/kernel"][fam.fo_off[0] + 1, 0], two) and not same(two, flat)
    whole, _ = TP.step_gradients(fam, w, ids, dense, y, 50)
    assert same(whole["head/kernel"][fam.fo_off[0] + 1, 0], flat)
    other = TP.train_host(fam, w, ids, dense, y, batch_size=50, epochs=1, tile=5)
    one = TP.train_host(fam, w, ids, dense, y, batch_size=50, epochs=1, tile=8)
    again = TP.train_host(fam, w, ids, dense, y, batch_size=50, epochs=1, tile=8)
    assert not same(other.m["head/kernel"], one.m["head/kernel"])           # the tile is part of the definition
    assert all(same(one.weights[k], again.weights[k]) and same(one.m[k], again.m[k]) for k in w) and same(one.p, again.p)


# ---------------------------------------------------------------- Adam

@pytest.mark.parametrize("shared", SHARED)
def test_one_step_is_step_gradients_and_adam_step(shared):
    fam, w, ids, dense, y = TPC.small(40, seed=1, shared=shared)
    got = TP.train_host(fam, w, ids, dense, y, batch_size=40, epochs=1, tile=8)
    g, p = TP.step_gradients(fam, w, ids, dense, y, 8)
    assert got.step == 1 and same(got.p, p)
    for k in TP.param_names(fam):
        wk, m, v = w[k].copy(), np.zeros_like(w[k]), np.zeros_like(w[k])
        T.adam_step(wk, m, v, g[k], T.adam_alpha(0.001, 1))
        assert same(got.weights[k], wk) and same(got.m[k], m) and same(got.v[k], v), k
        assert not same(wk, w[k]), k


def test_untouched_rows_and_a_field_in_no_pair():
    """A row no sample carries keeps its bits after step 1 (g = +0, m = v = 0) in ``emb/``, ``deep_emb/`` and ``head/kernel``; a row hit in step
    1 only keeps moving in step 3; the table of a field that is in no pair and no deep key never moves, while its first-order rows do."""
    fam, w, ids, dense, y = TPC.small(48, seed=5, pairs=[("movieId", "userId")])
    ids[:, 0] = np.where(ids[:, 0] >= 5, 0, ids[:, 0])                      # movies 5 and 6: never
    ids[5, 0] = 4
    ids[np.arange(48) != 5, 0] %= 4                                         # movie 4: row 5 (step 1) only
    off = fam.fo_off[0]
    one = TP.train_host(fam, w, ids[:16], dense[:16], y[:16], batch_size=16, epochs=1, tile=8)
    two = TP.train_host(fam, w, ids[:32], dense[:32], y[:32], batch_size=16, epochs=1, tile=8)
    three = TP.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    for name, rows in (("emb/movieId", [5, 6]), ("deep_emb/movieId", [5, 6]), ("head/kernel", [off + 5, off + 6])):
        assert same(three.weights[name][rows], w[name][rows]) and not three.m[name][rows].any() and not np.signbit(three.m[name][rows]).any()
    for name, row in (("emb/movieId", 4), ("deep_emb/movieId", 4), ("head/kernel", off + 4)):
        assert not same(one.weights[name][row], w[name][row]) and not same(three.weights[name][row], two.weights[name][row])
    for k in ("emb/userGenre1", "emb/movieGenre1"):
        assert same(three.weights[k], w[k]) and not three.v[k].any()
    assert not same(three.weights["head/kernel"][fam.fo_off[3]:fam.fo_off[3] + 3], w["head/kernel"][fam.fo_off[3]:fam.fo_off[3] + 3])


@pytest.mark.parametrize("bias", [100.0, -100.0])
def test_a_saturated_head(bias):
    fam, w, ids, dense, y = TPC.small(40, seed=7)
    w["head/bias"][0] = bias
    got = TP.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=8)
    assert set(np.unique(got.p).tolist()) == ({1.0} if bias > 0 else {0.0}) and set(y.tolist()) == {0.0, 1.0}
    assert all(np.isfinite(a).all() for a in got.weights.values())


def test_nans_are_stored_as_the_quiet_nan():
    """A dot of ``+inf`` and ``-inf``: ``p`` is NaN, stored as ``0x7fc00000``, and so is every NaN the weights, ``m`` and ``v`` then hold --
    also where the arithmetic produced the NaN with the sign bit set (``inf - inf`` on x86)."""
    fam, w, ids, dense, y = TPC.small(16, seed=6, emb_dim=4)
    w["emb/movieId"][:] = F(1e20)
    w["emb/userId"][:] = np.array([1e20, -1e20, 1e20, -1e20], dtype=F)
    with np.errstate(all="ignore"):
        raw = (F(np.inf) - F(np.inf))
    assert np.isnan(raw) and TP.QNAN.view(np.uint32) == 0x7fc00000
    got = TP.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert (got.p.view(np.uint32) == 0x7fc00000).all() and (TP.forward_host(fam, w, ids, dense).view(np.uint32) == 0x7fc00000).all()
    seen = 0
    for d in (got.weights, got.m, got.v):
        for a in d.values():
            seen += int(np.isnan(a).sum())
            assert (a.view(np.uint32)[np.isnan(a)] == 0x7fc00000).all()
    assert seen > 0 and np.isnan(got.weights["head/bias"]).all()


# ---------------------------------------------------------------- it learns

LEARN_AUC = 1.0


def test_it_learns_what_only_the_dots_carry(monkeypatch):
    """``label = (movieId + userId) mod 2`` over 8 x 8 ids, constant numerics, ``deep_emb`` on a third field the label ignores
    (tests/train_pair_cases.py learning()): the first order is additive in the two ids and the deep part never sees them, so only the dot can
    carry the label.  256 rows, batch 64, 40 epochs, lr 0.02.  The training AUC (exact, of all rows under the final weights) beats the same fit
    with the two FM tables' gradients zeroed, and it is at least the worst of ``torch.optim.Adam(eps=1e-7)`` on the same graph and arrays over
    five initialisation seeds minus their spread, measured on the CPU: 1.0000 1.0000 1.0000 1.0000 1.0000 -> worst 1.0000 - spread 0.0000 =
    1.0000 (the definition: 1.0000 at each of the five seeds; with the tables' gradients zeroed it stays near a coin's 0.5)."""
    fam, w, ids, dense, y = TPC.learning(seed=0)
    assert 0.4 < y.mean() < 0.6
    got = TP.train_host(fam, w, ids, dense, y, batch_size=64, epochs=40, learning_rate=0.02)
    full = TP.step_gradients

    def without_the_dots_gradient(*a, **k):
        g, p = full(*a, **k)
        g["emb/movieId"][:] = 0
        g["emb/userId"][:] = 0
        return g, p
    monkeypatch.setattr(TP, "step_gradients", without_the_dots_gradient)
    blind = TP.train_host(fam, w, ids, dense, y, batch_size=64, epochs=40, learning_rate=0.02)
    monkeypatch.setattr(TP, "step_gradients", full)
    assert same(blind.weights["emb/movieId"], w["emb/movieId"]) and same(blind.weights["emb/userId"], w["emb/userId"])
    auc, auc_blind = TPC.auc(y, TP.forward_host(fam, got.weights, ids, dense)), TPC.auc(y, TP.forward_host(fam, blind.weights, ids, dense))
    print("training AUC %.4f, without the dots' gradient %.4f, before %.4f" % (auc, auc_blind, TPC.auc(y, TP.forward_host(fam, w, ids, dense))))
    assert auc >= LEARN_AUC and auc_blind < 0.75 < auc


def test_the_torch_twin_of_the_learning_test():
    """The twin the threshold above was measured with, at one seed: it still gives the figure in the docstring."""
    fam, w, ids, dense, y = TPC.learning(seed=0)
    assert TPC.torch_adam_fit(fam, w, ids, dense, y, 64, 40, 0.02) == 1.0


# ---------------------------------------------------------------- errors, order, continuation

@pytest.mark.parametrize("shared", SHARED)
def test_errors_name_the_smallest_failing_row_and_change_nothing(shared):
    fam, w, ids, dense, y = TPC.small(40, seed=0, shared=shared)
    keep = {k: v.copy() for k, v in w.items()}

    def raises(match, ids=ids, dense=dense, y=y):
        with pytest.raises(ValueError, match=match):
            TP.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1)
        assert all(same(w[k], keep[k]) for k in w)
    bad = ids.copy(); bad[30, 0] = 7; bad[12, 0] = -1; bad[20, 2] = -2
    raises("samples row 12: an id outside", ids=bad)
    bad = ids.copy(); bad[35, 3] = 3                                        # == the genre field's vocabulary
    raises("samples row 35: an id outside", ids=bad)
    bad = dense.copy(); bad[9, 1] = np.inf; bad[3, 0] = np.nan
    raises("samples row 3: a numeric feature is not finite", dense=bad)
    bad = y.copy(); bad[7] = np.nan
    raises("samples row 7: the label is not finite", y=bad)
    with pytest.raises(ValueError, match="permutation"):
        TP.train_host(fam, w, ids, dense, y, order=np.zeros(40, dtype=np.int64))
    for kw in ({"batch_size": 0}, {"epochs": -1}, {"learning_rate": 0.0}, {"learning_rate": np.nan}, {"tile": 0}):
        with pytest.raises(ValueError):
            TP.train_host(fam, w, ids, dense, y, **kw)
    with pytest.raises(ValueError, match=r"ids must be \[N, 4\]"):
        TP.train_host(fam, w, ids[:, :3], dense, y)
    with pytest.raises(ValueError, match="weight 'head/kernel' has shape"):
        TP.train_host(fam, dict(w, **{"head/kernel": w["head/kernel"][:5]}), ids, dense, y)


@pytest.mark.parametrize("shared", SHARED)
def test_batches_order_and_continuation(shared):
    fam, w, ids, dense, y = TPC.small(40, seed=5, shared=shared)
    one = TP.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5)
    assert one.step == 6 and len(one.history) == 2 and one.p.shape == (40,)
    a = TP.train_host(fam, w, ids, dense, y, batch_size=16, epochs=1, tile=5)
    b = TP.train_host(fam, a.weights, ids, dense, y, batch_size=16, epochs=1, tile=5, state=(a.m, a.v, a.step))
    assert b.step == 6 and all(same(b.weights[k], one.weights[k]) and same(b.m[k], one.m[k]) and same(b.v[k], one.v[k]) for k in w)
    order = np.random.default_rng(3).permutation(40)
    c = TP.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=5, order=order)
    d = TP.train_host(fam, w, ids[order], dense[order], y[order], batch_size=16, epochs=2, tile=5)
    assert all(same(c.weights[k], d.weights[k]) for k in w) and same(c.p, d.p) and c.history == d.history
    assert not same(c.weights["head/kernel"], one.weights["head/kernel"])
    other = TP.train_host(fam, w, ids, dense, y, batch_size=16, epochs=2, tile=8)
    assert not same(other.weights["deep0/kernel"], one.weights["deep0/kernel"])    # the tile is part of the definition
    none = TP.train_host(fam, w, ids, dense, y, epochs=0)
    assert none.step == 0 and none.history == [] and all(same(none.weights[k], w[k]) for k in w)


def test_fit_without_a_device_points_to_the_host_definition(samples):
    import torch
    model = M.DeepFM(seed=1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device.*trainer_pair.train_host"):
            TP.fit(model, samples)
        with pytest.raises(RuntimeError, match="no HIP device.*train_host"):
            TP.train_device(TP.family_of(model), model.weights, np.zeros((1, 4), np.int32), np.zeros((1, 7), F), np.zeros(1, F))


# ---------------------------------------------------------------- the C side, without a device

def _fit_null(lib, ms, n=100, batch=50, tile=8):
    return lib.sprk_train_pair_fit(C.byref(ms) if ms is not None else None, None, None, None, None, n, batch, tile, 1, None, 0.1, 0.001, 1e-7, None, None, None, None, None,
                                   None, 0, None)


def test_lds_bytes_is_what_the_library_reports(lib):
    """``sprk_train_pair_fit`` checks its arguments before any device call: a tile beyond the LDS is refused with the bytes it would take,
    and ``sprk_train_pair_workspace_bytes`` is 0 from the first tile that does not fit."""
    for kw in (dict(), dict(shared=True), dict(fields=TPC.SIX, pairs=TPC.SIX_PAIRS, emb_dim=16, hidden=(64, 64)), dict(fields=TPC.EIGHT, pairs=TPC.EIGHT_PAIRS, deep_emb=("f1",)),
               dict(hidden=(7, 200, 3), emb_dim=TP.MAX_DIM), dict(hidden=(1,), emb_dim=1, deep_emb=(), n_dense=1)):
        fam = TPC.family(**kw)
        ms = TP._model_struct(fam)
        fits = TP.LDS_BYTES // TP.lds_bytes(fam, 1)
        assert TP.lds_bytes(fam, fits) <= TP.LDS_BYTES < TP.lds_bytes(fam, fits + 1)
        assert lib.sprk_train_pair_workspace_bytes(C.byref(ms), 100, 50, fits) > 0 and lib.sprk_train_pair_workspace_bytes(C.byref(ms), 100, 50, fits + 1) == 0
        assert _fit_null(lib, ms, tile=fits + 3) == L.EINVAL
        told = re.search(rb"tile = (\d+) needs (\d+) bytes of LDS", lib.sprk_last_error())
        assert told and int(told.group(1)) == fits + 3 and int(told.group(2)) == TP.lds_bytes(fam, fits + 3)


def test_the_library_refuses_what_the_family_check_refuses(lib):
    fam = TPC.family()

    def bad(change):
        ms = TP._model_struct(fam)
        assert lib.sprk_train_pair_workspace_bytes(C.byref(ms), 40, 16, 8) > 0
        change(ms)
        assert lib.sprk_train_pair_workspace_bytes(C.byref(ms), 40, 16, 8) == 0 and _fit_null(lib, ms, 40, 16) == L.EINVAL
        assert b"train_pair_fit: bad model (need 1..8 fields" in lib.sprk_last_error() and b"1..32 pairs" in lib.sprk_last_error()
    bad(lambda ms: setattr(ms, "n_fields", TP.MAX_FIELDS + 1))
    bad(lambda ms: setattr(ms, "n_fields", 0))
    bad(lambda ms: setattr(ms, "n_pairs", TP.MAX_PAIRS + 1))
    bad(lambda ms: setattr(ms, "n_pairs", 0))
    bad(lambda ms: setattr(ms, "n_layers", TP.MAX_LAYERS + 1))
    bad(lambda ms: setattr(ms, "emb_dim", TP.MAX_DIM + 1))
    bad(lambda ms: setattr(ms, "n_x", TP.MAX_X + 1))
    bad(lambda ms: setattr(ms, "n_x", 12))                                 # not n_deep x emb_dim + n_dense
    bad(lambda ms: setattr(ms, "n_deep", 5))
    bad(lambda ms: ms.width.__setitem__(0, TP.MAX_WIDTH + 1))
    bad(lambda ms: ms.vocab.__setitem__(1, 0))
    bad(lambda ms: ms.fo_off.__setitem__(0, 2))                            # the first-order blocks no longer tile the rows
    bad(lambda ms: ms.pair_a.__setitem__(3, 4))
    bad(lambda ms: ms.pair_b.__setitem__(0, -1))
    bad(lambda ms: ms.deep_col.__setitem__(1, 0))                          # a deep field twice
    bad(lambda ms: ms.xsrc.__setitem__(0, 2))
    rows = [k for k, j in enumerate(fam.xsrc) if j == 0]
    bad(lambda ms: ms.xsub.__setitem__(rows[1], fam.xsub[rows[0]]))        # an element twice
    assert lib.sprk_train_pair_workspace_bytes(None, 40, 16, 8) == 0 and _fit_null(lib, None, 40, 16) == L.EINVAL and b"bad model" in lib.sprk_last_error()
    ms = TP._model_struct(TPC.family(pairs=[("movieId", "movieId")]))      # (a, a) is legal
    assert lib.sprk_train_pair_workspace_bytes(C.byref(ms), 40, 16, 8) > 0
    ms = TP._model_struct(fam)
    assert _fit_null(lib, ms, 40, 0) == L.EINVAL and b"batch = 0" in lib.sprk_last_error()
    assert _fit_null(lib, ms, 40, 16) == L.EINVAL and b"NULL error word" in lib.sprk_last_error()
    word = (C.c_uint64 * 1)(2 ** 64 - 1)
    buf = (C.c_float * 64)()
    need = int(lib.sprk_train_pair_workspace_bytes(C.byref(ms), 40, 16, 8))
    z = C.cast(buf, C.c_void_p)
    for given in (need - 1, 0):                                             # a workspace that is too small: refused before any device call
        rc = lib.sprk_train_pair_fit(C.byref(ms), z, z, z, None, 40, 16, 8, 1, z, 0.1, 0.001, 1e-7, z, z, z, z, C.cast(word, C.c_void_p), z, given, None)
        assert rc == L.EINVAL and b"sprk_train_pair_workspace_bytes" in lib.sprk_last_error() and word[0] == 2 ** 64 - 1


def test_header_exports_and_prototypes_agree(lib):
    import subprocess
    header = open(os.path.join(ROOT, "include", "sparrow_hip.h")).read()
    names = ["sprk_train_pair_workspace_bytes", "sprk_train_pair_fit"]
    declared = set(re.findall(r"\b(sprk_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in names:
        assert name in declared and name in L.EXPORTED_SYMBOLS and name in exported and hasattr(lib, name)
    assert re.search(r"\}\s*sprk_train_pair_model;", header)
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(SPRK_TRAIN_PAIR_[A-Z_]+)\s+(\d+)", header)}
    assert consts == {"SPRK_TRAIN_PAIR_MAX_FIELDS": L.TRAIN_PAIR_MAX_FIELDS, "SPRK_TRAIN_PAIR_MAX_PAIRS": L.TRAIN_PAIR_MAX_PAIRS, "SPRK_TRAIN_PAIR_MAX_LAYERS": L.TRAIN_PAIR_MAX_LAYERS,
                      "SPRK_TRAIN_PAIR_MAX_WIDTH": L.TRAIN_PAIR_MAX_WIDTH, "SPRK_TRAIN_PAIR_MAX_X": L.TRAIN_PAIR_MAX_X, "SPRK_TRAIN_PAIR_MAX_DIM": L.TRAIN_PAIR_MAX_DIM}
    assert (TP.MAX_FIELDS, TP.MAX_PAIRS, TP.MAX_LAYERS, TP.MAX_WIDTH, TP.MAX_X, TP.MAX_DIM) == (8, 32, 8, 256, 256, 64) == \
        (L.TRAIN_PAIR_MAX_FIELDS, L.TRAIN_PAIR_MAX_PAIRS, L.TRAIN_PAIR_MAX_LAYERS, L.TRAIN_PAIR_MAX_WIDTH, L.TRAIN_PAIR_MAX_X, L.TRAIN_PAIR_MAX_DIM)
    body = re.sub(r"\s+", " ", re.search(r"typedef struct \{([^}]*)\}\s*sprk_train_pair_model;", header).group(1))
    fields = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.replace("int32_t", "").strip())]
    assert fields == [f[0] for f in L.TrainPairModel._fields_]
    assert C.sizeof(L.TrainPairModel) == 4 * (8 + 3 * 8 + 2 * 32 + 8 + 8 + 2 * 256)
    assert lib.sprk_train_pair_fit.argtypes[1:] == lib.sprk_train_fit.argtypes[1:] and lib.sprk_train_pair_fit.restype == C.c_int
    assert lib.sprk_train_pair_workspace_bytes.restype == C.c_size_t
    proto = lambda name: re.sub(r"\s+", " ", re.search(name + r"\(const sprk_train\w*_model\* model,(.*?)\);", header, re.S).group(1))
    assert proto("sprk_train_pair_fit") == proto("sprk_train_fit") and proto("sprk_train_pair_workspace_bytes") == proto("sprk_train_workspace_bytes")
