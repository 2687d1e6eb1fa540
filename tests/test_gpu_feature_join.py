"""The join kernel (sprk_join_features, k_feature_join.h behind model.pack_pairs_device / predict_pairs) against the oracle of
tests/featurestore_cases.py: the packed arrays of (userId, movieId) pairs are, byte for byte, what schema.pack_ids / pack_dense make of
the feature dict assembled from each entity's latest sample; scores are those of model.predict on that dict; a value outside its
range raises pack_ids' error (``-m gpu``).  No tolerance anywhere."""
import numpy as np
import pytest

from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import schema as S
from sparrowrecsys_amd import synthetic as SY
from sparrowrecsys_amd.featurestore import FeatureStore
from tests import featurestore_cases as FC

pytestmark = pytest.mark.gpu
CLASSES = [M.NeuralCF, M.EmbeddingMLP, M.WideNDeep, M.DeepFM, M.DeepFMv2, M.DIN, M.DIEN]
_models = {}


@pytest.fixture(scope="module")
def store():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    st = FeatureStore.from_samples(FC.samples())
    yield st
    st.close()


def model_of(cls):
    if cls not in _models:
        _models[cls] = cls(seed=5)
    return _models[cls]


def same(got, want):
    ids, dense = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert ids.dtype == np.int32 and dense.dtype == np.float32
    assert ids.shape == want[0].shape and dense.shape == want[1].shape
    assert ids.tobytes() == want[0].tobytes()
    assert dense.tobytes() == want[1].tobytes()


@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("cls", CLASSES)
def test_pair_form_equals_the_packed_assembled_rows(store, cls, B):
    model = model_of(cls)
    u, m = FC.pairs(B, seed=B)
    same(model.pack_pairs_device(store, u, m), FC.expected(model, u, m))


def test_pair_form_takes_lists_int32_and_device_tensors(store):
    import torch
    model = model_of(M.DIN)
    u, m = FC.pairs(300, seed=9)
    want = FC.expected(model, u, m)
    same(model.pack_pairs_device(store, u.tolist(), m.tolist()), want)
    same(model.pack_pairs_device(store, u.astype(np.int32), torch.from_numpy(m)), want)
    same(model.pack_pairs_device(store, torch.from_numpy(u).cuda(), torch.from_numpy(m.astype(np.int32)).cuda()), want)


@pytest.mark.parametrize("C", [1, 800, 1025])
@pytest.mark.parametrize("cls", [M.DeepFMv2, M.DIN, M.WideNDeep])
def test_cross_form_equals_the_pair_form_on_the_expanded_arrays(store, cls, C):
    model = model_of(cls)
    users, _ = FC.pairs(3, seed=1)
    users[1] = FC.pairs(8, seed=2)[0][-3]                          # the middle query: a user the store does not hold
    _, cand = FC.pairs(3 * C + 4, seed=C)
    shared, per_query = cand[:C], cand[:3 * C].reshape(3, C)
    eu = np.repeat(users, C)
    want_shared = FC.expected(model, eu, np.tile(shared, 3))
    want_per_query = FC.expected(model, eu, per_query.reshape(-1))
    same(model.pack_pairs_device(store, users, shared, shared_candidates=True), want_shared)
    same(model.pack_pairs_device(store, users, per_query), want_per_query)
    same(model.pack_pairs_device(store, eu, np.tile(shared, 3)), want_shared)
    same(model.pack_pairs_device(store, eu, per_query.reshape(-1)), want_per_query)


def test_wide_user_row(store):
    """hist_len 50: a user row of 240 bytes (15 granules), 57 id columns (two groups of the output tile), ids beyond 2^15."""
    H = 50
    cols = SY.synth_din(300, H, 5000, 7000, seed=11)
    cols["userId"][150:] = cols["userId"][:150]                    # every user twice: the later timestamp's row must be the one stored
    cols["timestamp"] = np.random.default_rng(3).permutation(300).astype(np.int64)
    st = FeatureStore.from_samples(cols, hist_len=H)
    assert st.user_pitch == 60 and st.n_users <= 7000
    model = M.DIN(seed=4, emb_dim=32, hist_len=H, movie_buckets=5000, user_buckets=7000)
    rows = (FC.latest_rows(cols, "userId"), FC.latest_rows(cols, "movieId"))
    rng = np.random.default_rng(5)
    u = cols["userId"][rng.integers(0, 300, 700)].astype(np.int64)
    m = cols["movieId"][rng.integers(0, 300, 700)].astype(np.int64)
    u[-1], m[-2] = 6999, 4999                                      # inside the vocabularies, beyond (or absent from) the tables
    want = FC.expected(model, u, m, cols, rows)
    same(model.pack_pairs_device(st, u, m), want)
    d = FC.assembled(u, m, cols, rows)
    assert np.array_equal(model.predict_pairs(st, u, m), model.predict(d))
    st.close()


@pytest.mark.parametrize("cls", [M.DeepFMv2, M.DIN, M.WideNDeep])
def test_scores_equal_predict_on_the_assembled_dict(store, cls):
    model = model_of(cls)
    u, m = FC.pairs(1000, seed=21)
    got = model.predict_pairs(store, u, m)
    want = model.predict(FC.assembled(u, m))
    assert got.shape == (1000, 1) and got.dtype == np.float32
    assert np.array_equal(got, want)
    assert model.predict_pairs(store, u[:0], m[:0]).shape == (0, 1)


def _pack_ids_error(model, u, m):
    with pytest.raises(ValueError) as e:
        S.pack_ids(model._columns(FC.assembled(u, m)), model.id_columns)
    return str(e.value)


def test_range_errors_are_pack_ids_errors(store):
    u, m = FC.pairs(600, seed=31)
    # a model with fewer movie buckets than the fixture's ids: candidate ids AND stored history ids are out of range; the first id
    # column (movieId) decides, then its first bad row
    small = M.DIN(seed=1, movie_buckets=500)
    want = _pack_ids_error(small, u, m)
    assert want.startswith("movieId id ")
    for call in (small.pack_pairs_device, small.predict_pairs):
        with pytest.raises(ValueError) as e:
            call(store, u, m)
        assert str(e.value) == want
    # candidates in range: the error comes from a history id read from the store
    m_ok = np.where(m < 500, m, 1)
    want = _pack_ids_error(small, u, m_ok)
    assert want.startswith("userRatedMovie")
    with pytest.raises(ValueError) as e:
        small.predict_pairs(store, u, m_ok)
    assert str(e.value) == want
    # the model still answers afterwards (the forward's own id flag was cleared with the error)
    ok_u = np.array([0, 0], dtype=np.int64)
    assert np.array_equal(small.predict_pairs(store, ok_u, m_ok[:2]), small.predict(FC.assembled(ok_u, m_ok[:2])))
    # a request user id >= user_buckets (also one that does not fit int32)
    model = model_of(M.DeepFMv2)
    for bad in (30001, 1 << 40, -7):
        u2 = u.copy()
        u2[417] = bad
        u2[555] = bad + 1
        want = _pack_ids_error(model, u2, m)
        assert want.startswith("userId id %d " % bad)
        with pytest.raises(ValueError) as e:
            model.predict_pairs(store, u2, m)
        assert str(e.value) == want
