"""sprk_rank_scores (k_rank_scores.h) against a numpy oracle, ``model.recommend`` against predict_pairs' scores put through the same
oracle, and the Jetty request answered by PredictServer in front of a StoreBackedModel (``-m gpu``)."""
import ctypes as C
import json
import urllib.error
import urllib.request

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd.featurestore import FeatureStore
from sparrowrecsys_amd.serving import PredictServer, StoreBackedModel
from tests import featurestore_cases as FC

pytestmark = pytest.mark.gpu
_models = {}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def store(torch):
    st = FeatureStore.from_samples(FC.samples())
    yield st
    st.close()


def model_of(cls):
    if cls not in _models:
        _models[cls] = cls(seed=7)
    return _models[cls]


def rank(torch, scores):
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).cuda()
    order = torch.full(s.shape, -1, dtype=torch.int32, device="cuda")
    L.check(L.load_library().sprk_rank_scores(C.c_void_p(s.data_ptr()), s.shape[0], s.shape[1], C.c_void_p(order.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return order.cpu().numpy()


@pytest.mark.parametrize("Cn", [1, 2, 63, 64, 65, 800, 1024, 1025, 4096])
def test_rank_scores_with_many_ties(torch, Cn):
    rng = np.random.default_rng(Cn)
    scores = (rng.integers(0, 8, size=(3, Cn)) / 8.0).astype(np.float32)          # 8 levels: ties everywhere
    got = rank(torch, scores)
    assert np.array_equal(got, FC.rank_oracle(scores))


def test_rank_scores_special_values(torch):
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0, 1e-45, -1e-45], dtype=np.float32)
    other_nan = np.array([0x7FC00001, 0xFFFFFFFF, 0x7F800001], dtype=np.uint32).view(np.float32)   # NaNs of other bits: all one value
    rng = np.random.default_rng(2)
    scores = np.concatenate([special, other_nan])[rng.integers(0, 13, size=(3, 100))]
    scores[0, :13] = np.concatenate([special, other_nan])
    got = rank(torch, scores)
    assert np.array_equal(got, FC.rank_oracle(scores))
    first = got[0][:5].tolist()
    assert np.isnan(scores[0][first]).all() and sorted(first) == first and not np.isnan(scores[0][got[0][-1]])


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("cls", [M.DeepFMv2, M.DIN])
def test_recommend_is_predict_pairs_then_the_oracle(torch, store, cls, shared):
    model = model_of(cls)
    users, movies = FC.pairs(64, seed=3)
    users = users[:5].copy()
    absent = FC.pairs(8, seed=2)[0][-3]
    users[3] = absent                                              # no row in the store: an empty list
    Cn = 800
    rng = np.random.default_rng(4)
    pool = np.array(sorted(FC.latest()[1]))[:200]                  # 800 candidates from 200 movies: every id about four times
    cand = pool[rng.integers(0, pool.size, size=(Cn,) if shared else (5, Cn))]
    per_user = np.tile(cand, (5, 1)) if shared else cand
    scores = model.predict_pairs(store, np.repeat(users, Cn), per_user.reshape(-1)).reshape(5, Cn)
    order = FC.rank_oracle(scores)
    # (a movie id that comes twice is scored twice: whatever scores are equal must come out in candidate order)
    for size in (1, 10, 800, 900):
        got = model.recommend(store, users, cand, size)
        assert len(got) == 5 and got[3] == []
        for q in (0, 1, 2, 4):
            assert got[q] == per_user[q][order[q][:min(size, Cn)]].tolist(), (q, size)
    # candidates (and users) that live on the device already: the same lists, the ids picked on the device
    assert model.recommend(store, users, torch.from_numpy(cand).cuda(), 10) == model.recommend(store, users, cand, 10)
    assert model.recommend(store, torch.from_numpy(users).cuda(), torch.from_numpy(cand.astype(np.int32)).cuda(), 10) == model.recommend(store, users, cand, 10)
    assert model.recommend(store, users[:0], cand if shared else cand[:0], 10) == []


def _post(port, body):
    req = urllib.request.Request("http://127.0.0.1:%d/v1/models/recmodel:predict" % port, data=body, headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=30) as r:
        return r.status, json.loads(r.read())


def test_server_answers_the_jetty_request_from_the_store(store):
    model = model_of(M.DeepFMv2)
    _, movies = FC.pairs(800, seed=5)
    user = int(FC.pairs(1, seed=6)[0][0])
    want = model.predict_pairs(store, np.full(800, user), movies)
    srv = PredictServer(StoreBackedModel(model, store), port=0).start()
    plain = PredictServer(model, port=0).start()
    try:
        # the Jetty ranker's bytes (org.json writes no spaces): RecForYouProcess.java:113-127
        body = ('{"instances":[' + ",".join('{"userId":%d,"movieId":%d}' % (user, m) for m in movies) + "]}").encode()
        status, got = _post(srv.port, body)
        assert status == 200
        assert np.array_equal(np.array(got["predictions"], dtype=np.float32), want)
        status, got = _post(srv.port, json.dumps({"inputs": {"userId": [user] * 3, "movieId": movies[:3].tolist()}}).encode())
        assert status == 200 and np.array_equal(np.array(got["outputs"], dtype=np.float32), model.predict_pairs(store, [user] * 3, movies[:3]))
        # a request that sends the full feature columns is the plain model's business
        d = FC.assembled(np.full(16, user), movies[:16])
        full = json.dumps({"instances": [{k: (v[i].item() if hasattr(v[i], "item") else v[i]) for k, v in d.items()} for i in range(16)]}).encode()
        a, b = _post(srv.port, full), _post(plain.port, full)
        assert a[0] == b[0] == 200 and a[1] == b[1]
        assert np.array_equal(np.array(a[1]["predictions"], dtype=np.float32), model.predict_pairs(store, [user] * 16, movies[:16]))
        # an id outside the model's range is the 400 TF Serving would answer with
        req = urllib.request.Request("http://127.0.0.1:%d/v1/models/recmodel:predict" % srv.port, data=b'{"instances":[{"userId":30001,"movieId":1}]}')
        with pytest.raises(urllib.error.HTTPError) as e:
            urllib.request.urlopen(req, timeout=30)
        assert e.value.code == 400 and b"userId id 30001 outside [0, 30001)" in e.value.read()
    finally:
        srv.close()
        plain.close()
