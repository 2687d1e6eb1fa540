"""The native column packer on the host (sprk_pack_columns behind ingest.pack_columns / model.pack), no GPU needed: it converts the storage
kinds it lists with the bits of the Python packer (schema.pack_ids / pack_dense) -- and the route assertion proves the native code ran, with
ZERO declines -- or it declines, and model.pack returns / raises exactly what the Python packer returns / raises."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from sparrowrecsys_amd import _lib as L
from sparrowrecsys_amd import ingest
from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import schema as S
from tests import pack_cases as PC
from tests.conftest import REFERENCE, ROOT, needs_reference


def host_native(features, id_columns, numeric_keys, threads=None):
    """ingest.pack_columns with the route cap: the native packer ran and declined nothing."""
    got = ingest.pack_columns(features, id_columns, list(numeric_keys), threads=threads)
    assert got is not None, "declined: %s" % L.load_library().sprk_last_error().decode()
    assert ingest.last_pack_route() == "host" and L.load_library().sprk_pack_last_route() == 1
    return got


def check_model(model, features):
    cols = model._columns(features)
    PC.assert_same(host_native(cols, model.id_columns, model.numeric_keys), PC.python_pack(cols, model.id_columns, list(model.numeric_keys)))
    got = model.pack(features)                                     # the public call: same bits, and it did not fall back
    assert ingest.last_pack_route() == "host"
    PC.assert_same(got, PC.python_pack(cols, model.id_columns, list(model.numeric_keys)))


# ---- 1. every model class on the sample columns ----
@pytest.mark.parametrize("model_cls", PC.MODELS)
def test_sample_columns_every_model(lib, samples, model_cls):
    model = model_cls(seed=1)
    check_model(model, samples)                                    # object strings -> text block
    check_model(model, PC.as_unicode(samples))
    check_model(model, PC.as_bytes(samples))
    check_model(model, S.read_samples_csv(PC.EXCERPT))
    check_model(model, PC.typed_from_strings(samples))


@needs_reference
@pytest.mark.parametrize("model_cls", PC.MODELS)
def test_all_reference_rows_every_model(lib, model_cls):
    feats = S.read_samples_csv(os.path.join(REFERENCE, "src", "main", "resources", "webroot", "sampledata", "testSamples.csv"))
    assert len(feats["movieId"]) == 22440
    check_model(model_cls(seed=1), feats)


# ---- 2. typed columns ----
@pytest.mark.parametrize("B", PC.TYPED_SIZES)
def test_typed_columns_every_storage_kind_under_every_rule(lib, B):
    feats, idc, dense = PC.typed_case(B, seed=100 + B)
    ref = PC.python_pack(feats, idc, dense)
    for threads in (1, 8):
        PC.assert_same(host_native(feats, idc, dense, threads=threads), ref)


def test_int64_to_float_is_one_rounding(lib):
    """2^53 + 2^29 + 1 -> 0x5A000001 (numpy's astype(float32)); by way of double it would be 0x5A000000."""
    feats = {"x": np.array([2 ** 53 + 2 ** 29 + 1], np.int64)}
    _, dense = host_native(feats, [], ["x"])
    assert dense.view(np.uint32)[0, 0] == 0x5A000001 == S.pack_dense(feats, ["x"]).view(np.uint32)[0, 0]


def test_synthetic_config_columns(lib):
    for feats, model in PC.config_cases():
        check_model(model, feats)


def test_torch_cpu_tensors_are_read_in_place(lib):
    import torch
    feats, model = PC.config_cases(B=300)[1]                        # DIN with the [B, 50] history matrix
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in feats.items()}
    check_model(model, t)


# ---- 3. strings ----
@pytest.mark.parametrize("width", [None, 40])
def test_string_columns_every_form(lib, width):
    f, idc, dense = PC.string_case()
    for form, feats in PC.string_forms(f, width).items():
        PC.assert_same(host_native(feats, idc, dense), PC.python_pack(feats, idc, dense))


def test_nul_padding_and_embedded_nul(lib):
    idc = [S.IdColumn("g", "genre", S.N_GENRES), S.IdColumn("i", "id", 100)]
    feats = {"g": np.array([b"War", b"War\x00\x00", b"Wa\x00r", b"\x00War", b"IMAX", b""], dtype="S7"),
             "i": np.array([b"7", b"07\x00", b"", b"1.5", b"99", b"0"], dtype="S3")}
    ref = PC.python_pack(feats, idc, [])
    assert ref[0][:, 0].tolist() == [5, 5, -1, -1, 15, -1]
    PC.assert_same(host_native(feats, idc, []), ref)
    uni = {k: v.astype("U") for k, v in feats.items()}
    PC.assert_same(host_native(uni, idc, []), PC.python_pack(uni, idc, []))


def test_non_ascii_in_a_numeric_column_declines(lib):
    """float() reads fullwidth digits; strtod does not: the native packer declines and the Python packer decides."""
    model = M.NeuralCF(seed=1)
    for bad in ("１２", "1١"):
        feats = {"movieId": np.array(["3", bad], dtype=object), "userId": np.array(["4", "5"], dtype=object)}
        assert ingest.pack_columns(feats, model.id_columns, []) is None and L.load_library().sprk_pack_last_route() == 0
        assert ingest.pack_columns(PC.as_unicode(feats), model.id_columns, []) is None
        got = model.pack(feats)
        assert ingest.last_pack_route() == "python"
        PC.assert_same(got, PC.python_pack(feats, model.id_columns, []))


@pytest.mark.parametrize("form", ["object", "S", "U"])
def test_short_decimal_spellings(lib, form):
    vals = PC.short_decimal_spellings()
    pos = [v for v in vals if not v.startswith("-") or float(v) == 0.0]
    feats = PC.string_forms({"x": vals}, None)[form]
    PC.assert_same(host_native(feats, [], ["x"]), PC.python_pack(feats, [], ["x"]))
    feats = PC.string_forms({"x": pos}, None)[form]
    idc = [S.IdColumn("x", "id", 2 ** 31 - 1)]
    PC.assert_same(host_native(feats, idc, []), PC.python_pack(feats, idc, []))


def test_long_numbers_convert_on_the_host(lib):
    """16+ digits and large exponents: strtod takes any digit count; bits equal np.float32(float(s))."""
    for form, feats in PC.string_forms({"x": PC.LONG_NUMBERS}, None).items():
        _, dense = host_native(feats, [], ["x"])
        with np.errstate(over="ignore"):                           # (1.79e308 narrows to inf, on every route)
            want = np.array([np.float32(float(s)) for s in PC.LONG_NUMBERS], np.float32)
        np.testing.assert_array_equal(dense[:, 0].view(np.uint32), want.view(np.uint32))


# ---- 4. declines: the outcome is the Python packer's ----
def _outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:                                         # noqa: BLE001 (the exception IS the result under comparison)
        return ("raise", type(e), str(e))


def _same_outcome(model, feats):
    cols = dict(feats)
    want = _outcome(lambda: PC.python_pack(model._columns(cols), model.id_columns, list(model.numeric_keys)))
    got = _outcome(lambda: model.pack(feats))
    assert got[0] == want[0], (got, want)
    if want[0] == "ok":
        assert ingest.last_pack_route() == "python"
        PC.assert_same(got[1], want[1])
    else:
        assert got[1:] == want[1:]
    return want


@pytest.mark.parametrize("bad", [" 5", "1_0", "inf", "nan", "0x10", "1e400", "abc", "5\n", "\n"])
@pytest.mark.parametrize("where", ["movieId", "movieAvgRating", "movieGenre1"])
def test_declined_spellings_end_as_in_python(lib, samples, bad, where):
    model = M.EmbeddingMLP(seed=1)
    feats = dict(samples)
    col = feats[where].copy()
    col[3] = bad
    feats[where] = col
    if where == "movieGenre1" and "\n" not in bad:
        check_model(model, feats)                                  # a genre column takes any string: -1, natively
        return
    assert ingest.pack_columns(feats, model.id_columns, list(model.numeric_keys)) is None
    assert L.load_library().sprk_pack_last_route() == 0
    _same_outcome(model, feats)
    if "\n" not in bad:
        assert ingest.pack_columns(PC.as_unicode(feats), model.id_columns, list(model.numeric_keys)) is None
        _same_outcome(model, PC.as_unicode(feats))


def test_declined_storage_kinds_end_as_in_python(lib, samples):
    model = M.EmbeddingMLP(seed=1)
    typed = PC.typed_from_strings(samples)
    check_model(model, typed)
    cases = {
        "None in an object array": ("movieId", np.array([None if i == 2 else v for i, v in enumerate(samples["movieId"])], dtype=object)),
        "NaN in an object array": ("movieAvgRating", np.array([float("nan") if i == 2 else v for i, v in enumerate(samples["movieAvgRating"])], dtype=object)),
        "float16": ("movieAvgRating", typed["movieAvgRating"].astype(np.float16)),
        "uint64": ("movieId", typed["movieId"].astype(np.uint64)),
        "big-endian": ("userId", typed["userId"].astype(">i4")),
        "float genre column": ("movieGenre1", np.where(np.arange(256) % 3 == 0, np.nan, 2.0)),
        "bool genre column": ("movieGenre1", np.arange(256) % 2 == 0),
        "mixed list": ("movieId", [None] + list(typed["movieId"][1:])),
        "2-d column": ("movieId", np.zeros((256, 2), np.int32)),
        "short column": ("movieId", typed["movieId"][:100]),
    }
    for name, (key, col) in cases.items():
        feats = dict(typed)
        feats[key] = col
        assert ingest.pack_columns(feats, model.id_columns, list(model.numeric_keys)) is None, name
        _same_outcome(model, feats)


def test_missing_key_is_the_python_keyerror(lib, samples):
    model = M.EmbeddingMLP(seed=1)
    feats = {k: v for k, v in samples.items() if k != "userGenre3"}
    want = _same_outcome(model, feats)
    assert want[1] is KeyError


def test_force_python_switch(lib, samples, monkeypatch):
    model = M.DeepFM(seed=1)
    monkeypatch.setenv("SPRK_PACK_NATIVE", "0")
    got = model.pack(samples)
    assert ingest.last_pack_route() == "python"
    PC.assert_same(got, PC.python_pack(samples, model.id_columns, list(model.numeric_keys)))


# ---- 5. range errors ----
def test_range_error_message_and_precedence(lib):
    B = 70001
    feats, idc, dense = PC.typed_case(B, seed=9)
    order = [c.key for c in idc]
    assert order.index("id_int32") < order.index("id_int64") < order.index("id_float64")
    # a bad value in a LATER row of an EARLIER column beats an earlier row of a later column
    feats = dict(feats)
    a = np.array(feats["id_int32"]); a[60000] = -7; a[65000] = -8; feats["id_int32"] = a
    b = np.array(feats["id_float64"]); b[5] = 1e6; feats["id_float64"] = b
    c = np.array(feats["id_int64"]); c[69999] = 2 ** 40 + 3; feats["id_int64"] = c
    with pytest.raises(ValueError) as want:
        S.pack_ids(feats, idc)
    assert "id_int32 id -7 outside" in str(want.value)
    for threads in (1, 3, 8):
        with pytest.raises(ValueError) as got:
            ingest.pack_columns(feats, idc, dense, threads=threads)
        assert str(got.value) == str(want.value)
        assert ingest.last_pack_route() == "host"                  # the native packer raised it itself
    feats["id_int32"] = np.where(np.array(feats["id_int32"]) < 0, 0, feats["id_int32"]).astype(np.int32)
    with pytest.raises(ValueError) as want:
        S.pack_ids(feats, idc)
    assert "id_int64 id %d outside" % (2 ** 40 + 3) in str(want.value)
    for threads in (1, 3, 8):
        with pytest.raises(ValueError) as got:
            ingest.pack_columns(feats, idc, dense, threads=threads)
        assert str(got.value) == str(want.value)


def test_range_error_from_strings_and_through_model_pack(lib, samples):
    model = M.EmbeddingMLP(seed=1)
    for form in (dict, PC.as_unicode, PC.as_bytes, PC.typed_from_strings):
        feats = dict(samples)
        col = feats["userId"].copy(); col[200] = "30001"; col[7] = "-2.5"; feats["userId"] = col
        col = feats["movieId"].copy(); col[255] = "1001"; feats["movieId"] = col
        feats = form(feats)
        want = _outcome(lambda: PC.python_pack(feats, model.id_columns, list(model.numeric_keys)))
        assert want[1] is ValueError and "movieId id 1001 outside [0, 1001) (reference: assert_less_than_num_buckets)" == want[2]
        assert _outcome(lambda: model.pack(feats))[1:] == want[1:]
        assert ingest.last_pack_route() == "host"


def test_range_error_next_to_a_declined_value_is_pythons(lib, samples):
    model = M.EmbeddingMLP(seed=1)
    feats = dict(samples)
    col = feats["movieId"].copy(); col[9] = "5000"; feats["movieId"] = col
    col = feats["userRatingCount"].copy(); col[1] = "abc"; feats["userRatingCount"] = col
    assert ingest.pack_columns(feats, model.id_columns, list(model.numeric_keys)) is None      # declined, not raised
    want = _same_outcome(model, feats)
    assert want[1] is ValueError and "movieId id 5000" in want[2]
    # the other order: Python meets the unparsable id before the range error of a later column
    feats = dict(samples)
    col = feats["movieId"].copy(); col[9] = "abc"; feats["movieId"] = col
    col = feats["userId"].copy(); col[1] = "999999"; feats["userId"] = col
    want = _same_outcome(model, feats)
    assert want[1] is ValueError and "could not convert" in want[2]


# ---- 6. ABI ----
def _col(data=None, stride=4, storage=L.COL_I32, width=0, rule=L.RULE_IDENTITY, vocab=10, name=b"c", on_device=0):
    c = L.PackCol()
    c.data, c.stride, c.storage, c.width, c.on_device, c.rule, c.vocab, c.name = data, stride, storage, width, on_device, rule, vocab, name
    return c


def test_bad_arguments_are_einval_without_a_gpu(lib):
    a = np.arange(4, dtype=np.int32)
    out = np.zeros((4, 1), np.int32)
    fout = np.zeros((4, 1), np.float32)
    ok = _col(a.ctypes.data)
    arr = lambda c: (L.PackCol * 1)(c)                              # noqa: E731
    for entry, extra in ((lib.sprk_pack_columns, ()), (lib.sprk_pack_columns_device, (None,))):
        def call(ids=arr(ok), n_id=1, dense=None, n_dense=0, text=None, rows=4, io=out.ctypes.data, do=None):
            return entry(ids, n_id, dense, n_dense, text, 0, rows, 1, io, do, *extra)
        assert call(ids=None) == L.EINVAL
        assert call(io=None) == L.EINVAL
        assert call(rows=-1) == L.EINVAL
        assert call(n_id=-1) == L.EINVAL
        assert call(ids=arr(_col(None))) == L.EINVAL and b"no data" in lib.sprk_last_error()
        assert call(ids=arr(_col(a.ctypes.data, storage=13))) == L.EINVAL and b"storage" in lib.sprk_last_error()
        assert call(ids=arr(_col(a.ctypes.data, storage=-1))) == L.EINVAL
        assert call(ids=arr(_col(a.ctypes.data, storage=L.COL_BYTES, width=0))) == L.EINVAL and b"width" in lib.sprk_last_error()
        assert call(ids=arr(_col(a.ctypes.data, storage=L.COL_UCS4, width=0))) == L.EINVAL
        assert call(ids=arr(_col(a.ctypes.data, rule=L.RULE_DENSE))) == L.EINVAL
        assert call(ids=arr(_col(a.ctypes.data, rule=7))) == L.EINVAL
        assert call(ids=arr(_col(None, storage=L.COL_TEXT))) == L.EINVAL and b"text block" in lib.sprk_last_error()
        assert call(ids=arr(_col(a.ctypes.data, name=None))) == L.EINVAL
        assert call(n_id=0, ids=None, dense=arr(_col(a.ctypes.data, rule=L.RULE_DENSE)), n_dense=1, do=None) == L.EINVAL
        assert call(n_id=0, ids=None, dense=arr(ok), n_dense=1, do=fout.ctypes.data) == L.EINVAL
        assert lib.sprk_pack_last_route() == -1
    assert lib.sprk_pack_columns(arr(_col(a.ctypes.data, on_device=1)), 1, None, 0, None, 0, 4, 1, out.ctypes.data, None) == L.EINVAL
    many = (L.PackCol * 129)(*[ok] * 129)
    assert lib.sprk_pack_columns_device(many, 129, None, 0, None, 0, 4, 1, out.ctypes.data, None, None) == L.EINVAL
    # and the valid call works here, with no GPU in the machine
    assert lib.sprk_pack_columns(arr(ok), 1, None, 0, None, 0, 4, 1, out.ctypes.data, None) == L.OK
    assert out[:, 0].tolist() == [0, 1, 2, 3] and lib.sprk_pack_last_route() == 1


def test_descriptor_matches_the_ctypes_mirror(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sparrow_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", '
                   "sizeof(sprk_pack_col), offsetof(sprk_pack_col, data), offsetof(sprk_pack_col, stride), offsetof(sprk_pack_col, storage), "
                   "offsetof(sprk_pack_col, width), offsetof(sprk_pack_col, on_device), offsetof(sprk_pack_col, rule), offsetof(sprk_pack_col, vocab), "
                   "offsetof(sprk_pack_col, name), SPRK_COL_F64, SPRK_COL_TEXT, SPRK_RULE_DENSE, SPRK_PACK_MAX_COLS); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = L.PackCol
    assert got == [C.sizeof(P), P.data.offset, P.stride.offset, P.storage.offset, P.width.offset, P.on_device.offset, P.rule.offset,
                   P.vocab.offset, P.name.offset, L.COL_F64, L.COL_TEXT, L.RULE_DENSE, L.PACK_MAX_COLS]
    assert C.sizeof(P) == 48 and sys.byteorder == "little"
