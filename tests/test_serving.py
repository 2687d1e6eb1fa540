"""TF-Serving-compatible REST shim (sparrowrecsys_amd/serving.py): the wire contract of
RecForYouProcess.java:113-138 against a stub model on CPU, and end to end over the HIP path with the
reference-trained NeuralCF weights on a GPU."""
import json
import os
import threading
import urllib.error
import urllib.request

import numpy as np
import pytest

from sparrowrecsys_amd.serving import PredictServer
from tests.conftest import GOLDEN


class _StubModel:
    """score = sigmoid-free closed form of (userId, movieId); ids >= 1000 are 'out of vocabulary'."""

    def __init__(self):
        self.calls = []

    def predict(self, feats):
        u = np.asarray(feats["userId"], dtype=np.int64)
        m = np.asarray(feats["movieId"], dtype=np.int64)
        self.calls.append(len(u))
        if getattr(self, "delay", 0):
            import time
            time.sleep(self.delay)
        if (m >= 1000).any() or (m < 0).any():
            raise ValueError("an id was outside its table")
        return ((u % 7) * 0.1 + (m % 5) * 0.01).astype(np.float32).reshape(-1, 1)


def _post(port, body, path="/v1/models/recmodel:predict"):
    req = urllib.request.Request("http://127.0.0.1:%d%s" % (port, path), data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    try:
        with urllib.request.urlopen(req, timeout=30) as r:
            return r.status, json.loads(r.read())
    except urllib.error.HTTPError as e:
        return e.code, json.loads(e.read())


@pytest.fixture()
def stub_server():
    model = _StubModel()
    srv = PredictServer(model, port=0).start()
    yield srv, model
    srv.close()


def test_row_format_matches_jetty_client(stub_server):
    srv, model = stub_server
    inst = [{"userId": 10 + i, "movieId": (3 * i) % 1000} for i in range(800)]   # RecForYouProcess.java:118-127
    code, resp = _post(srv.port, {"instances": inst})
    assert code == 200 and list(resp) == ["predictions"]
    p = resp["predictions"]
    assert len(p) == 800 and all(isinstance(x, list) and len(x) == 1 for x in p)    # getJSONArray(i).getDouble(0)
    want = [((10 + i) % 7) * 0.1 + (((3 * i) % 1000) % 5) * 0.01 for i in range(800)]
    np.testing.assert_allclose([x[0] for x in p], want, atol=1e-6)


def test_columnar_format_status_and_errors(stub_server):
    srv, _ = stub_server
    code, resp = _post(srv.port, {"inputs": {"userId": [1, 2, 3], "movieId": [4, 5, 6]}})
    assert code == 200 and len(resp["outputs"]) == 3
    code, resp = _post(srv.port, {"instances": [{"userId": 1, "movieId": 5000}]})       # out-of-range id -> 400 + error
    assert code == 400 and "error" in resp
    code, resp = _post(srv.port, {"foo": 1})
    assert code == 400 and "error" in resp
    code, resp = _post(srv.port, {"instances": []})
    assert code == 200 and resp == {"predictions": []}
    code, resp = _post(srv.port, {"instances": [{"userId": 1, "movieId": 2}]}, path="/v1/models/other:predict")
    assert code == 404
    with urllib.request.urlopen("http://127.0.0.1:%d/v1/models/recmodel" % srv.port, timeout=30) as r:
        assert json.loads(r.read())["model_version_status"][0]["state"] == "AVAILABLE"


def test_concurrent_requests_are_batched_and_isolated(stub_server):
    srv, model = stub_server
    srv.batcher.max_wait_s = 0.05                       # give the 16 client threads time to pile up
    model.delay = 0.02                                  # ... behind a forward that takes long enough for the others to arrive
    results = {}

    def client(i):
        bad = i == 5
        inst = [{"userId": 100 * i + j, "movieId": (5000 if bad else j)} for j in range(50)]
        results[i] = _post(srv.port, {"instances": inst})

    ts = [threading.Thread(target=client, args=(i,)) for i in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i in range(16):
        code, resp = results[i]
        if i == 5:
            assert code == 400                          # its neighbours in the merged batch are not affected
        else:
            assert code == 200
            want = [((100 * i + j) % 7) * 0.1 + (j % 5) * 0.01 for j in range(50)]
            np.testing.assert_allclose([x[0] for x in resp["predictions"]], want, atol=1e-6)
    # at least one merged forward ([r5] inline forwards count as batches now, so this inequality really says "merged": before, every
    # inline request satisfied it by itself)
    assert srv.batcher.batches < srv.batcher.requests == 16


class _GenreStub:
    """score encodes which genre strings arrived: index of the genre in a 3-entry list, -1 (-> 0.5) if unknown."""
    VOC = {"Action": 0.1, "Drama": 0.2, "": 0.3}

    def predict(self, feats):
        g = feats["userGenre1"]
        out = np.array([self.VOC.get(str(x), 0.5) for x in g], dtype=np.float32)
        if "nan_please" in feats:
            out[0] = np.nan
        return out.reshape(-1, 1)


def test_bracketed_string_features_are_unwrapped_not_stringified():
    """TF Serving accepts [x] for a scalar feature; on the fast path str(['Action']) used to reach the model."""
    srv = PredictServer(_GenreStub(), port=0).start()
    try:
        code, resp = _post(srv.port, {"instances": [{"userId": [1], "movieId": [2], "userGenre1": ["Action"]},
                                                    {"userId": [3], "movieId": [4], "userGenre1": ["Drama"]}]})
        assert code == 200
        np.testing.assert_allclose([x[0] for x in resp["predictions"]], [0.1, 0.2], atol=1e-7)
        code, resp = _post(srv.port, {"instances": [{"userId": 1, "movieId": 2, "userGenre1": "Action"},
                                                    {"userId": 3, "movieId": 4, "userGenre1": None}]})
        assert code == 200
        np.testing.assert_allclose([x[0] for x in resp["predictions"]], [0.1, 0.3], atol=1e-7)
        # a genuinely non-scalar string feature is a client error, not an out-of-vocabulary genre
        code, resp = _post(srv.port, {"instances": [{"userId": 1, "movieId": 2, "userGenre1": ["Action", "Drama"]}]})
        assert code == 400 and "error" in resp
    finally:
        srv.close()


def test_threads_do_not_pile_up_and_raw_http_variants(stub_server):
    """(1) One batcher thread for the server's life: round 4's first inline-forward commit started a NEW batcher thread in every
    request's withdraw() -- 300 threads after 300 requests, and eight concurrent clients got HALF the throughput of one.
    (2) The handler's own header parser: keep-alive, HTTP/1.0, `Connection: close`, odd header spellings, and the requests it hands
    to the stock parser (`Expect`, a folded header) all answer like the stock handler."""
    import http.client
    import socket
    srv, model = stub_server
    body = json.dumps({"instances": [{"userId": 8, "movieId": 3}, {"userId": 9, "movieId": 4}]}).encode()
    want = [[0.13], [0.24]]
    c = http.client.HTTPConnection("127.0.0.1", srv.port, timeout=30)
    before = None
    for i in range(60):                                           # one keep-alive connection
        c.request("POST", "/v1/models/recmodel:predict", body=body, headers={"Content-Type": "application/json"})
        r = c.getresponse()
        got = json.loads(r.read())
        assert r.status == 200
        np.testing.assert_allclose(got["predictions"], want, atol=1e-6)
        if i == 9:
            before = threading.active_count()
    assert threading.active_count() <= before
    c.close()

    def raw(req: bytes):
        with socket.create_connection(("127.0.0.1", srv.port), timeout=10) as sk:
            sk.sendall(req)
            sk.shutdown(socket.SHUT_WR)
            data = b""
            while True:
                b = sk.recv(65536)
                if not b:
                    break
                data += b
        head, _, payload = data.partition(b"\r\n\r\n")
        return int(head.split()[1]), payload
    path = b"/v1/models/recmodel:predict"
    cl = b"Content-Length: %d\r\n" % len(body)
    for req in (b"POST " + path + b" HTTP/1.1\r\nHost: x\r\nConnection: close\r\n" + cl + b"\r\n" + body,
                b"POST " + path + b" HTTP/1.0\r\n" + cl + b"\r\n" + body,
                b"POST " + path + b" HTTP/1.1\r\nhost:x\r\nCONTENT-LENGTH:   %d  \r\nConnection: close\r\n\r\n" % len(body) + body,
                b"POST " + path + b" HTTP/1.1\r\nHost: x\r\nX-Folded: a\r\n  b\r\nConnection: close\r\n" + cl + b"\r\n" + body):
        code, payload = raw(req)
        assert code == 200, req[:80]
        np.testing.assert_allclose(json.loads(payload)["predictions"], want, atol=1e-6)
    code, payload = raw(b"GET /v1/models/recmodel HTTP/1.1\r\nHost: x\r\nConnection: close\r\n\r\n")
    assert code == 200 and b"AVAILABLE" in payload
    code, payload = raw(b"POST /nope HTTP/1.1\r\nConnection: close\r\n" + cl + b"\r\n" + body)
    assert code == 404


def test_non_finite_scores_still_parse():
    """'%.9g' of NaN is not JSON; such a response falls back to json.dumps' NaN spelling."""
    srv = PredictServer(_GenreStub(), port=0).start()
    try:
        code, resp = _post(srv.port, {"instances": [{"userId": 1, "movieId": 2, "userGenre1": "Action", "nan_please": 1},
                                                    {"userId": 1, "movieId": 2, "userGenre1": "Drama", "nan_please": 1}]})
        assert code == 200
        p = [x[0] for x in resp["predictions"]]
        assert np.isnan(p[0]) and abs(p[1] - 0.2) < 1e-7
    finally:
        srv.close()


@pytest.mark.gpu
def test_neuralcf_served_end_to_end_with_reference_trained_weights():
    """The reference's own trained NeuralCF (modeldata/neuralcf/001) behind the shim: the scores the Jetty
    ranker would receive equal the oracle's on the same (userId, movieId) pairs."""
    from oracle import ctr_oracle as O
    from sparrowrecsys_amd import models as M
    g = np.load(os.path.join(GOLDEN, "neuralcf_ckpt.npz"))
    w = {k[4:]: g[k] for k in g.files if k.startswith("001/")}
    table = np.zeros((30001, 10), np.float32)
    table[g["users"]] = g["user_rows_001"]
    w["emb/userId"] = table
    model = M.NeuralCF(weights=w)
    srv = PredictServer(model, port=0).start()
    try:
        n = 800
        inst = [{"userId": int(u), "movieId": int(m)} for u, m in zip(g["userId"][:n], g["movieId"][:n])]
        code, resp = _post(srv.port, {"instances": inst})
        assert code == 200
        got = np.array([x[0] for x in resp["predictions"]], dtype=np.float32)
        ref = O.neural_cf_forward({"userId": g["userId"][:n], "movieId": g["movieId"][:n]}, w, dtype=np.float64)[:, 0]
        assert np.abs(got - ref).max() <= 1e-4
        code, resp = _post(srv.port, {"instances": [{"userId": 1, "movieId": 1001}]})     # movie table has 1001 rows
        assert code == 400 and "error" in resp
    finally:
        srv.close()


def test_fast_and_general_instance_paths_agree_and_scores_round_trip(stub_server):
    """Uniform scalar instances take the fast conversion; ragged ones (a missing key, the [x] spelling of a scalar) the general
    one -- same scores; the hand-written response body reproduces every float32 score exactly; keep-alive requests on one
    connection each get their own complete response (headers and body leave in one write)."""
    import http.client
    srv, model = stub_server
    uniform = [{"userId": 3 + i, "movieId": 10 + i} for i in range(50)]
    ragged = [dict(d) for d in uniform]
    ragged[7]["movieId"] = [ragged[7]["movieId"]]                  # TF Serving's [x] form
    st1, r1 = _post(srv.port, {"instances": uniform})
    st2, r2 = _post(srv.port, {"instances": ragged})
    assert st1 == 200 and st2 == 200 and r1 == r2
    want = ((np.arange(3, 53) % 7) * 0.1 + (np.arange(10, 60) % 5) * 0.01).astype(np.float32)
    got = np.array(r1["predictions"], dtype=np.float64)[:, 0].astype(np.float32)
    np.testing.assert_array_equal(got, want)
    st3, r3 = _post(srv.port, {"instances": uniform + [17]})
    assert st3 == 400 and "error" in r3
    c = http.client.HTTPConnection("127.0.0.1", srv.port, timeout=10)
    for k in range(5):
        c.request("POST", "/v1/models/recmodel:predict", body=json.dumps({"instances": uniform[:k + 1]}), headers={"Content-Type": "application/json"})
        resp = c.getresponse()
        body = json.loads(resp.read())
        assert resp.status == 200 and len(body["predictions"]) == k + 1
    c.close()


def test_byte_level_parser_of_the_jetty_request_equals_the_json_path():
    """serving._fast_uniform_int_instances reads the ranker's request (RecForYouProcess.java:113-127: flat objects, the same integer
    keys in the same order) without json.loads; it must give the columns the general path gives -- for org.json's compact spelling
    and Python's spaced one -- and step aside (None) for everything else, so that those requests keep the general path's behaviour,
    errors included."""
    import json as J
    from sparrowrecsys_amd import serving as S
    rng = np.random.default_rng(3)
    inst = [{"userId": int(u), "movieId": int(m)} for u, m in zip(rng.integers(-3, 30000, 800), rng.integers(0, 1000, 800))]
    for seps in ((", ", ": "), (",", ":")):
        body = J.dumps({"instances": inst}, separators=seps).encode()
        got = S._fast_uniform_int_instances(body)
        assert got is not None and list(got) == ["userId", "movieId"]
        want = S._to_feature_arrays(S._columns_from_instances(J.loads(body)["instances"], fast=True), 800)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k])
            assert got[k].dtype == want[k].dtype
    one = J.dumps({"instances": [{"movieId": 5}]}).encode()
    np.testing.assert_array_equal(S._fast_uniform_int_instances(one)["movieId"], [5])
    # everything that is not exactly that shape: the general path's business
    for other in (
            {"instances": [{"userId": 1, "movieId": 2}, {"movieId": 3, "userId": 4}]},          # another key order
            {"instances": [{"userId": 1, "movieId": 2}, {"userId": 3}]},                        # a missing key
            {"instances": [{"userId": 1, "movieId": 2.5}]},                                     # a float
            {"instances": [{"userId": 1, "movieId": 1e3}]},
            {"instances": [{"userId": 1, "movieId": [2]}]},                                     # the [x] spelling
            {"instances": [{"userId": 1, "movieId": "2"}]},                                     # a string
            {"instances": [{"userId": 1, "movieId": True}]},
            {"instances": [{"userId": 1, "movieId": None}]},
            {"instances": [{"userId": 1, "userRatedMovie1": 2}]},                               # a digit inside a key
            {"instances": []},
            {"inputs": {"userId": [1, 2], "movieId": [3, 4]}},
            {"instances": [{"userId": 1, "movieId": 2}], "signature_name": "serving_default"}):
        assert S._fast_uniform_int_instances(J.dumps(other).encode()) is None, other
    assert S._fast_uniform_int_instances(J.dumps({"instances": inst[:3]}, indent=2).encode()) is None          # pretty-printed
    assert S._fast_uniform_int_instances(b'{"instances": [{"userId": 1, "movieId": 99999999999999999999999}]}') is None
    assert S._fast_uniform_int_instances(b'{"instances": [{"userId": 1, "movieId": --2}]}') is None
    assert S._fast_uniform_int_instances(b'not json') is None


def test_fast_and_json_parse_paths_answer_alike(stub_server, monkeypatch):
    """The same request through both parsers of the running server: same status, same predictions; a bad id is a 400 on both."""
    import http.client
    import json as J
    from sparrowrecsys_amd import serving as S
    srv, model = stub_server
    inst = [{"userId": 7, "movieId": m} for m in range(1, 41)]
    out = {}
    for fast in (True, False):
        srv.fast_parse = fast
        c = http.client.HTTPConnection("127.0.0.1", srv.port, timeout=30)
        c.request("POST", "/v1/models/recmodel:predict", body=J.dumps({"instances": inst}, separators=(",", ":")).encode(), headers={"Content-Type": "application/json"})
        r = c.getresponse()
        out[fast] = (r.status, J.loads(r.read()))
        c.close()
    assert out[True] == out[False] and out[True][0] == 200 and len(out[True][1]["predictions"]) == 40


def test_content_length_is_validated_before_the_body_is_read():
    """`int(Content-Length)` went straight into rfile.read() -- a negative value meant "read until EOF" (a handler
    thread parked for as long as the client holds the connection), and nothing bounded the buffer.  Negative, non-numeric, missing and
    oversize lengths are answered (400 / 400 / 411 / 413) WITHOUT waiting for a body, the connection is closed, and the server keeps
    serving; a body shorter than its announced length is a 400 as well."""
    import socket
    import time
    model = _StubModel()
    srv = PredictServer(model, port=0, max_body_bytes=4096).start()
    try:
        def raw(req: bytes, half_close=False):
            t0 = time.monotonic()
            with socket.create_connection(("127.0.0.1", srv.port), timeout=10) as sk:
                sk.sendall(req)
                if half_close:
                    sk.shutdown(socket.SHUT_WR)
                data = b""
                while True:                                       # the SERVER must end the exchange: the client never closes first
                    b = sk.recv(65536)
                    if not b:
                        break
                    data += b
            head, _, payload = data.partition(b"\r\n\r\n")
            return int(head.split()[1]), payload, time.monotonic() - t0
        path = b"POST /v1/models/recmodel:predict HTTP/1.1\r\nHost: x\r\n"
        for hdr, want in ((b"Content-Length: -1\r\n", 400), (b"Content-Length: 12abc\r\n", 400), (b"Content-Length: 1e3\r\n", 400),
                          (b"", 411), (b"Content-Length: 5000\r\n", 413), (b"Content-Length: 99999999999999999999\r\n", 413)):
            code, payload, dt = raw(path + hdr + b"\r\n")         # no body is ever sent, and the socket stays open on the client's side
            assert code == want, (hdr, code, payload)
            assert "error" in json.loads(payload) and dt < 5.0
        body = json.dumps({"instances": [{"userId": 8, "movieId": 3}]}).encode()
        code, payload, _ = raw(path + b"Content-Length: %d\r\n\r\n" % (len(body) + 10) + body, half_close=True)   # announced more than sent
        assert code == 400 and b"ended after" in payload
        code, payload, _ = raw(path + b"Connection: close\r\nContent-Length: %d\r\n\r\n" % len(body) + body)
        assert code == 200
        np.testing.assert_allclose(json.loads(payload)["predictions"], [[0.13]], atol=1e-6)
        # the batch counters: an inline forward counts as a batch (requests / batches was skewed by the inline path)
        assert srv.batcher.requests == srv.batcher.batches >= 1
    finally:
        srv.close()


def _stub_factory():
    return _StubModel()


def test_worker_processes_share_one_port():
    """serving.serve_workers: N front processes on one port (SO_REUSEPORT) in front of ONE engine process that owns the model.  Every
    front answers the Jetty request with the same scores; the status route says which process served, and over a few dozen fresh
    connections more than one did; a model-side ValueError crosses the process boundary as HTTP 400; concurrent requests from
    different fronts come back right (the engine merges them into one forward)."""
    import http.client
    from sparrowrecsys_amd.serving import serve_workers
    pool = serve_workers(_stub_factory, (), n_workers=3, port=0, start_method="fork")
    try:
        assert len(set(pool.pids)) == 3 and pool.engine_pid not in pool.pids
        seen = set()
        for i in range(60):
            c = http.client.HTTPConnection("127.0.0.1", pool.port, timeout=30)   # a fresh connection each: the kernel picks the front
            c.request("GET", "/v1/models/recmodel")
            seen.add(json.loads(c.getresponse().read())["worker_pid"])
            c.request("POST", "/v1/models/recmodel:predict", body=json.dumps({"instances": [{"userId": 8, "movieId": 3}, {"userId": 9, "movieId": 4}]}),
                      headers={"Content-Type": "application/json"})
            r = c.getresponse()
            got = json.loads(r.read())
            assert r.status == 200
            np.testing.assert_allclose(got["predictions"], [[0.13], [0.24]], atol=1e-6)
            c.close()
        assert seen <= set(pool.pids) and len(seen) >= 2, (seen, pool.pids)
        code, resp = _post(pool.port, {"instances": [{"userId": 1, "movieId": 5000}]})      # the stub's "outside its table"
        assert code == 400 and "outside" in resp["error"]
        results = {}

        def client(i):
            inst = [{"userId": 100 * i + j, "movieId": (5000 if i == 5 else j)} for j in range(40)]
            results[i] = _post(pool.port, {"instances": inst})
        ts = [threading.Thread(target=client, args=(i,)) for i in range(12)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for i in range(12):
            code, resp = results[i]
            if i == 5:
                assert code == 400                              # its neighbours in a merged forward are not affected
            else:
                assert code == 200
                want = [((100 * i + j) % 7) * 0.1 + (j % 5) * 0.01 for j in range(40)]
                np.testing.assert_allclose([x[0] for x in resp["predictions"]], want, atol=1e-6)
    finally:
        pool.close()


def _slow_stub_factory():
    m = _StubModel()
    m.delay = 0.3
    return m


def test_engine_survives_a_front_that_dies_with_a_request_in_flight():
    """[r6, ADVICE r05] The engine process against raw connections (no HTTP): three fronts send requests that merge into one forward; one of them
    closes its connection before the answer.  Round 5's blanket handler then answered every member a SECOND time -- live fronts were one reply out
    of step for ever (same candidate counts: nothing to notice it by) -- and the dead connection's second failure killed the engine loop.  Now: each
    live front gets exactly ONE reply carrying ITS request id, and the engine keeps serving."""
    import multiprocessing as mp
    import time
    from multiprocessing.connection import Client
    from sparrowrecsys_amd.serving import _engine_main
    ctx = mp.get_context("fork")
    ready, stop = ctx.Queue(), ctx.Event()
    # an abstract-namespace socket: no file, so no limit from how deep the temporary directory lies (AF_UNIX paths stop at 107 bytes)
    address = "\0sprk_engine_test_%d_%d" % (os.getpid(), time.monotonic_ns())
    eng = ctx.Process(target=_engine_main, args=(_slow_stub_factory, (), address, ready, stop), daemon=True)
    eng.start()
    try:
        assert ready.get(timeout=60)[2] is None
        a, b, dead = (Client(address, family="AF_UNIX") for _ in range(3))
        feats = lambda u: {"userId": np.arange(u, u + 4, dtype=np.int64), "movieId": np.arange(4, dtype=np.int64)}
        want = lambda u: ((np.arange(u, u + 4) % 7) * 0.1 + (np.arange(4) % 5) * 0.01).astype(np.float32)
        a.send(((1, 1), feats(10)))                               # warm: the first pass may take it alone
        assert a.recv()[0] == (1, 1)
        a.send(((1, 2), feats(20))); b.send(((2, 1), feats(30))); dead.send(((3, 1), feats(40)))
        dead.close()                                              # gone while the (slow) forward runs
        for conn, rid, u in ((a, (1, 2), 20), (b, (2, 1), 30)):
            got, kind, payload = conn.recv()
            assert got == rid and kind == "ok"
            np.testing.assert_allclose(payload, want(u), atol=1e-6)
        time.sleep(0.5)
        assert not a.poll(0) and not b.poll(0)                    # no second reply waiting
        a.send(((1, 3), feats(50)))
        got, kind, payload = a.recv()
        assert got == (1, 3) and kind == "ok"
        np.testing.assert_allclose(payload, want(50), atol=1e-6)
        assert eng.is_alive()
        # same keys, different dtype kinds: not merged into one upcast batch (each answered on its own, both right)
        fa = {"userId": np.array([8, 9], dtype=np.int64), "movieId": np.array([3, 4], dtype=np.int64)}
        fb = {"userId": np.array([8.0, 9.0], dtype=np.float64), "movieId": np.array([3, 4], dtype=np.int64)}
        from sparrowrecsys_amd.serving import _merge_key
        assert _merge_key(fa) != _merge_key(fb) and _merge_key(fa) == _merge_key(feats(1))
        a.send(((1, 4), fa)); b.send(((2, 2), fb))
        assert a.recv()[:2] == ((1, 4), "ok") and b.recv()[:2] == ((2, 2), "ok")
    finally:
        stop.set()
        eng.join(timeout=10)
        if eng.is_alive():
            eng.terminate()


def test_fronts_leave_the_port_when_the_engine_dies():
    """[r6, ADVICE r05] WorkerPool.alive() turns False and the fronts exit (a request after the engine's death is a 5xx, then the port closes)
    instead of answering 500 for ever."""
    import os
    import signal
    import time
    from sparrowrecsys_amd.serving import serve_workers
    pool = serve_workers(_stub_factory, (), n_workers=2, port=0, start_method="fork")
    try:
        assert pool.alive()
        code, resp = _post(pool.port, {"instances": [{"userId": 8, "movieId": 3}]})
        assert code == 200
        os.kill(pool.engine_pid, signal.SIGKILL)
        deadline = time.time() + 20
        while pool.alive() and time.time() < deadline:
            time.sleep(0.2)
        assert not pool.alive()
        for _ in range(4):                                        # every front notices at its next request at the latest
            try:
                _post(pool.port, {"instances": [{"userId": 8, "movieId": 3}]})
            except Exception:
                pass
        deadline = time.time() + 20
        while any(p.is_alive() for p in pool.procs[1:]) and time.time() < deadline:
            time.sleep(0.2)
        assert not any(p.is_alive() for p in pool.procs[1:])
    finally:
        pool.close()
