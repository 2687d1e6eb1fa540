"""The device column packer (sprk_pack_columns_device, k_pack_columns.h behind ingest.pack_columns_device / model.pack_device / model.predict)
against its host twin (sprk_pack_columns, itself pinned on the Python packer by tests/test_pack_columns.py): identical bits, with the route
asserted for every case -- the device converted the batch, no decline -- and model.predict(dict) identical to the Python-packer route (``-m gpu``)."""
import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import ingest
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import schema as S
from sparrowrecsys_amd import synthetic as SY
from tests import pack_cases as PC

pytestmark = pytest.mark.gpu
SIZES = [1, 255, 256, 257, 65536, 200003]
TORCH_OK = "bif"                                                    # numpy kinds torch takes as they are (uint16 / uint32 stay numpy: "mixed")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


def to_cuda(torch, features, strided=False):
    """Numeric columns as CUDA tensors (strided: each one a column view of its own [B, 3] device matrix); the rest stay numpy."""
    out = {}
    for k, v in features.items():
        a = np.asarray(v) if not isinstance(v, np.ndarray) else v
        if a.dtype.kind in TORCH_OK or a.dtype == np.uint8:
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            if strided and t.dim() == 1:
                m = torch.zeros((t.shape[0], 3), dtype=t.dtype, device="cuda")
                m[:, 1] = t
                t = m[:, 1]
            out[k] = t
        else:
            out[k] = v
    return out


def device_equals_host(features, id_columns, numeric_keys, host_features=None):
    """The route cap on both sides: the device packed it (route 2), the host twin packed it (route 1), same bits."""
    lib = L.load_library()
    got = ingest.pack_columns_device(features, id_columns, list(numeric_keys))
    assert got is not None, "the device declined: %s" % lib.sprk_last_error().decode()
    assert ingest.last_pack_route() == "device" and lib.sprk_pack_last_route() == 2
    assert got[0].is_cuda and got[1].is_cuda
    ref = ingest.pack_columns(features if host_features is None else host_features, id_columns, list(numeric_keys))
    assert ref is not None and ingest.last_pack_route() == "host"
    PC.assert_same(got, ref)
    return ref


def to_host(features):
    return {k: (v.cpu() if hasattr(v, "cpu") else v) for k, v in features.items()}


# ---- 1. device == host native ----
@pytest.mark.parametrize("model_cls", PC.MODELS)
def test_sample_columns_every_model(torch, samples, model_cls):
    model = model_cls(seed=1)
    typed = PC.typed_from_strings(samples)
    for feats in (samples, PC.as_unicode(samples), PC.as_bytes(samples), S.read_samples_csv(PC.EXCERPT), typed, to_cuda(torch, typed),
                  to_cuda(torch, typed, strided=True)):
        cols = model._columns(feats, keep_device=True)
        ref = device_equals_host(cols, model.id_columns, model.numeric_keys, to_host(cols))
        PC.assert_same(ref, PC.python_pack(to_host(cols), model.id_columns, list(model.numeric_keys)))


@pytest.mark.parametrize("B", SIZES)
def test_typed_columns_every_storage_kind_under_every_rule(torch, B):
    feats, idc, dense = PC.typed_case(B, seed=100 + B)
    ref = device_equals_host(feats, idc, dense)                      # numpy, strided and reversed views: staged by the library
    PC.assert_same(ref, PC.python_pack(feats, idc, dense))
    for strided in (False, True):                                    # CUDA tensors read in place; uint16 / uint32 columns stay numpy: mixed
        cu = to_cuda(torch, feats, strided)
        assert any(hasattr(v, "is_cuda") for v in cu.values()) and any(isinstance(v, np.ndarray) for v in cu.values())
        PC.assert_same(device_equals_host(cu, idc, dense, feats), ref)


def test_int64_to_float_is_one_rounding(torch):
    feats = {"x": np.array([2 ** 53 + 2 ** 29 + 1], np.int64)}
    for f in (feats, to_cuda(torch, feats)):
        got = ingest.pack_columns_device(f, [], ["x"])
        assert ingest.last_pack_route() == "device"
        assert got[1].cpu().numpy().view(np.uint32)[0, 0] == 0x5A000001


@pytest.mark.parametrize("B", [300, 65536])
def test_synthetic_config_columns_and_the_history_matrix_on_the_device(torch, B):
    for feats, model in PC.config_cases(B):
        cols = model._columns(feats, keep_device=True)
        ref = device_equals_host(cols, model.id_columns, model.numeric_keys)
        PC.assert_same(ref, PC.python_pack(cols, model.id_columns, list(model.numeric_keys)))
        cu = to_cuda(torch, feats)                                   # DIN: userRatedMovies [B, 50] on the device, 50 strided views of it
        if "userRatedMovies" in cu:
            assert cu["userRatedMovies"].is_cuda and cu["userRatedMovies"].dim() == 2
        cols = model._columns(cu, keep_device=True)
        assert all(v.is_cuda for v in cols.values() if hasattr(v, "is_cuda"))
        PC.assert_same(device_equals_host(cols, model.id_columns, model.numeric_keys, model._columns(feats)), ref)
        mixed = dict(feats)
        for k in list(mixed)[::2]:
            mixed[k] = cu[k]
        cols = model._columns(mixed, keep_device=True)
        PC.assert_same(device_equals_host(cols, model.id_columns, model.numeric_keys, model._columns(feats)), ref)


@pytest.mark.parametrize("width", [None, 40, 80])
def test_string_columns_every_form(torch, width):
    f, idc, dense = PC.string_case()
    for form, feats in PC.string_forms(f, width).items():
        ref = device_equals_host(feats, idc, dense)
        PC.assert_same(ref, PC.python_pack(feats, idc, dense))


def test_nul_padding_and_embedded_nul(torch):
    idc = [S.IdColumn("g", "genre", S.N_GENRES), S.IdColumn("i", "id", 100)]
    feats = {"g": np.array([b"War", b"War\x00\x00", b"Wa\x00r", b"\x00War", b"IMAX", b""], dtype="S7"),
             "i": np.array([b"7", b"07\x00", b"", b"1.5", b"99", b"0"], dtype="S3")}
    ref = device_equals_host(feats, idc, [])
    assert ref[0][:, 0].tolist() == [5, 5, -1, -1, 15, -1]
    device_equals_host({k: v.astype("U") for k, v in feats.items()}, idc, [])


@pytest.mark.parametrize("form", ["object", "S", "U"])
def test_short_decimal_spellings(torch, form):
    vals = PC.short_decimal_spellings()
    pos = [v for v in vals if not v.startswith("-") or float(v) == 0.0]
    device_equals_host(PC.string_forms({"x": vals}, None)[form], [], ["x"])
    device_equals_host(PC.string_forms({"x": pos}, None)[form], [S.IdColumn("x", "id", 2 ** 31 - 1)], [])


@pytest.mark.parametrize("B", SIZES)
def test_sample_columns_tiled(torch, samples, B):
    model = M.EmbeddingMLP(seed=1)
    for feats in (PC.tiled(samples, B), PC.typed_from_strings(PC.tiled(samples, B))):
        device_equals_host(feats, model.id_columns, model.numeric_keys)


# ---- 2. beyond the exact path: the device declines, the host twin converts ----
def test_long_numbers_decline_on_the_device_and_convert_on_the_host(torch):
    lib = L.load_library()
    with np.errstate(over="ignore"):                           # (1.79e308 narrows to inf, on every route)
        want = np.array([np.float32(float(s)) for s in PC.LONG_NUMBERS], np.float32)
    for form, feats in PC.string_forms({"x": PC.LONG_NUMBERS}, None).items():
        assert ingest.pack_columns_device(feats, [], ["x"]) is None
        assert lib.sprk_pack_last_route() == 0 and ingest.last_pack_route() is None
    for s in PC.LONG_NUMBERS:                                           # each of them alone is beyond 15 digits or +-22
        assert ingest.pack_columns_device({"x": np.array([s, "1.5"], dtype="S")}, [], ["x"]) is None, s

    class Dense(M.CTRModel):                                         # the routes of pack_device on one dense column
        numeric_keys = ["x"]
        PACK_DEVICE_MIN_ROWS = 1

        def __init__(self):
            self.id_columns = []
    feats = PC.string_forms({"x": PC.LONG_NUMBERS}, None)["S"]
    ids, dense = Dense().pack_device(feats)
    assert ingest.last_pack_route() == "host" and lib.sprk_pack_last_route() == 1
    np.testing.assert_array_equal(dense.cpu().numpy()[:, 0].view(np.uint32), want.view(np.uint32))


# ---- 3. model.predict(dict) == the same call on the Python packer ----
def _forced(monkeypatch, fn):
    monkeypatch.setenv("SPRK_PACK_NATIVE", "0")
    try:
        out = fn()
        assert ingest.last_pack_route() == "python"
        return out
    finally:
        monkeypatch.delenv("SPRK_PACK_NATIVE")


@pytest.mark.parametrize("model_cls", PC.MODELS)
def test_predict_equals_the_python_route(torch, samples, monkeypatch, model_cls):
    model = model_cls(seed=3)
    typed = PC.typed_from_strings(samples)
    forms = {"typed": typed, "S": PC.as_bytes(samples), "object": samples, "cuda": to_cuda(torch, typed)}
    for name, feats in forms.items():
        for bs in (None, 7, 100):
            want = _forced(monkeypatch, lambda: model.predict(feats, batch_size=bs))
            got = model.predict(feats, batch_size=bs)
            assert ingest.last_pack_route() in ("device", "host"), name
            np.testing.assert_array_equal(got, want)
    big = PC.typed_from_strings(PC.tiled(samples, 65536))             # case b: typed + S genre columns, one batch
    want = _forced(monkeypatch, lambda: model.predict(big))
    got = model.predict(big)
    assert ingest.last_pack_route() == "device"
    np.testing.assert_array_equal(got, want)


def test_predict_one_large_batch_config_shapes(torch, monkeypatch):
    B = 65536
    f2 = SY.synth_fields(B, SY.CONFIG2_FIELDS, seed=1)
    m2 = M.DeepFMv2(seed=2, emb_dim=16, fields=SY.CONFIG2_FIELDS, proj_dim=16)
    f3 = SY.synth_din(B, 50, 5000, 7000, seed=3)
    m3 = M.DIN(seed=4, emb_dim=32, hist_len=50, movie_buckets=5000, user_buckets=7000)
    for feats, model in ((f2, m2), (f3, m3)):
        want = _forced(monkeypatch, lambda: model.predict(feats))
        for f in (feats, to_cuda(torch, feats)):
            got = model.predict(f)
            assert ingest.last_pack_route() == "device"
            np.testing.assert_array_equal(got, want)


# ---- 4. a bad id ----
def test_bad_id_raises_from_predict_and_the_engine_stays_intact(torch, samples):
    model = M.DeepFM(seed=5)
    clean = PC.typed_from_strings(PC.tiled(samples, 8192))
    before = model.predict(clean)
    assert ingest.last_pack_route() == "device"
    for make in (lambda f: f, lambda f: to_cuda(torch, f)):
        bad = dict(clean)
        u = bad["userId"].copy(); u[17] = 30001; u[5000] = -4; bad["userId"] = u
        m = bad["movieId"].copy(); m[8000] = 2000; bad["movieId"] = m
        with pytest.raises(ValueError) as want:
            S.pack_ids(bad, model.id_columns)
        with pytest.raises(ValueError) as got:
            model.predict(make(bad))
        assert str(got.value) == str(want.value) and ingest.last_pack_route() == "device"
        np.testing.assert_array_equal(model.predict(make(clean)), before)      # no stale flag, same scores
    s = dict(samples)
    col = s["movieId"].copy(); col[100] = "1001"; s["movieId"] = col
    with pytest.raises(ValueError, match=r"movieId id 1001 outside \[0, 1001\) \(reference: assert_less_than_num_buckets\)"):
        ingest.pack_columns_device(s, model.id_columns, list(model.numeric_keys))
    assert ingest.last_pack_route() == "device"


# ---- 5. the staging buffer over calls of different shapes ----
def test_a_large_pack_then_a_small_one_reuse_the_staging_buffer(torch, samples):
    model = M.EmbeddingMLP(seed=1)
    big = PC.tiled(samples, 100000)
    small = {k: v[5:42] for k, v in samples.items()}
    typed_small = PC.typed_from_strings(small)
    for feats in (big, small, typed_small, big, typed_small, PC.as_bytes(small)):
        device_equals_host(feats, model.id_columns, model.numeric_keys)
