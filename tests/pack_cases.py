"""Inputs of the column-packer tests (tests/test_pack_columns.py on the CPU, tests/test_gpu_pack_columns.py on the GPU): every storage kind
the native packers list, under every output rule, with the values that separate a right conversion from a nearly right one.  The reference
of every comparison is the Python packer (schema.pack_ids / pack_dense), which defines the result."""
import os

import numpy as np

from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import schema as S
from sparrowrecsys_amd import synthetic as SY
from tests.conftest import GOLDEN

MODELS = [M.EmbeddingMLP, M.WideNDeep, M.NeuralCF, M.DeepFM, M.DeepFMv2, M.DIN, M.DIEN]
EXCERPT = os.path.join(GOLDEN, "test_samples_512.csv")
INT_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32]
FLOAT_DTYPES = [np.float32, np.float64]
TYPED_SIZES = [1, 255, 256, 257, 70001]


def python_pack(features, id_columns, numeric_keys):
    ids = S.pack_ids(features, id_columns)
    return ids, S.pack_dense(features, numeric_keys) if len(numeric_keys) else np.zeros((ids.shape[0], 0), np.float32)


def assert_same(got, ref):
    assert got is not None, "the native packer declined a batch it lists as native"
    ids, dense = [np.asarray(a.cpu()) if hasattr(a, "cpu") else a for a in got]
    assert ids.dtype == np.int32 and dense.dtype == np.float32
    np.testing.assert_array_equal(ids, ref[0])
    assert dense.shape == ref[1].shape
    np.testing.assert_array_equal(np.ascontiguousarray(dense).view(np.uint32), np.ascontiguousarray(ref[1]).view(np.uint32))


def as_unicode(features):
    return {k: np.asarray(v).astype(str) for k, v in features.items()}


def as_bytes(features):
    return {k: np.asarray(v).astype(str).astype("S") for k, v in features.items()}


def tiled(features, B):
    n = len(next(iter(features.values())))
    return {k: np.tile(v, (B + n - 1) // n)[:B] for k, v in features.items()}


def typed_from_strings(features):
    """The sample file's columns as a typed caller holds them: int32 ids and counts, float32 averages, S genre columns."""
    out = {}
    for k, v in features.items():
        if "Genre" in k:
            out[k] = np.asarray(v).astype(str).astype("S")
        elif k in S.FLOAT_KEYS or k == "rating":
            out[k] = S.to_float_column(v)
        else:
            out[k] = S.to_int_column(v).astype(np.int32)
    return out


def _views(rng, a, j):
    """The same values behind a contiguous array, an every-other-element view, a reversed view and a column of a matrix."""
    n = len(a)
    form = j % 4
    if form == 1:
        base = np.zeros(2 * n, a.dtype)
        base[::2] = a
        return base[::2]
    if form == 2:
        return np.ascontiguousarray(a[::-1])[::-1]
    if form == 3:
        m = np.zeros((n, 3), a.dtype)
        m[:, 1] = a
        return m[:, 1]
    return a


def typed_case(B, seed):
    """-> (features, id_columns, numeric_keys): every numeric storage kind as an identity id, as a genre index and as a dense value."""
    rng = np.random.default_rng(seed)
    feats, idc, dense = {}, [], []
    j = 0

    def put(key, a):
        nonlocal j
        feats[key] = _views(rng, a, j)
        j += 1
    special_i64 = np.array([2 ** 53 + 2 ** 29 + 1, 2 ** 24 + 1, 2 ** 63 - 1, -2 ** 63, 2 ** 63 - 2 ** 39 - 1, -(2 ** 24) - 1, 2 ** 31, -1, 0, 2 ** 40 + 3], np.int64)
    for dt in [np.bool_] + INT_DTYPES:
        name = np.dtype(dt).name
        hi = 2 if dt is np.bool_ else min(int(np.iinfo(dt).max), 2 ** 31 - 2)
        vocab = hi + 1
        a = rng.integers(0, hi + 1, size=B).astype(dt)                          # identity: [0, vocab), for int64 well above 2^24
        put("id_" + name, a)
        idc.append(S.IdColumn("id_" + name, "id", vocab))
        d = rng.integers(0, 2, size=B).astype(dt) if dt is np.bool_ else \
            rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, size=B, dtype=dt, endpoint=True)
        if dt is np.int64:
            d[:min(B, len(special_i64))] = special_i64[:B]
        put("dense_" + name, d)
        dense.append("dense_" + name)
        if dt is not np.bool_:
            lo = -3 if np.iinfo(dt).min < 0 else 0
            g = rng.integers(lo, 26, size=B).astype(dt)                         # out-of-range and negative genre indices -> -1
            if dt is np.int64:
                g[:min(B, len(special_i64))] = special_i64[:B]
            put("genre_" + name, g)
            idc.append(S.IdColumn("genre_" + name, "genre", S.N_GENRES))
    special_f = np.array([np.nan, 0.0, -0.0, 0.1, 1.0 / 3.0, 16777217.0, 1e-46, -1e-46, 3.0000000000000004, 123456789.987654321, 2.5, -2.5], np.float64)
    for dt in FLOAT_DTYPES:
        name = np.dtype(dt).name
        a = rng.uniform(0.0, 99.99, size=B).astype(dt)                          # identity: truncation toward zero, NaN / +-0.0 -> 0
        a[:min(B, 3)] = np.array([np.nan, 0.0, -0.0], dt)[:B]
        a[rng.random(B) < 0.05] = np.nan
        put("id_" + name, a)
        idc.append(S.IdColumn("id_" + name, "id", 100))
        d = (rng.standard_normal(B) * 10.0 ** rng.integers(-8, 9, size=B)).astype(dt)   # float64: values that round when narrowed
        d[:min(B, len(special_f))] = special_f[:B].astype(dt)
        d[rng.random(B) < 0.05] = np.nan
        put("dense_" + name, d)
        dense.append("dense_" + name)
    return feats, idc, dense


def config_cases(B=4096):
    """The synthetic columns of configs 2, 3 and 5 (typed), missing numerics injected as NaN."""
    rng = np.random.default_rng(5)
    out = []
    f2 = SY.synth_fields(B, SY.CONFIG2_FIELDS, seed=11)
    m2 = M.DeepFMv2(seed=2, emb_dim=16, fields=[(k, kind, min(v, 5000)) for k, kind, v in SY.CONFIG2_FIELDS], proj_dim=16)
    for k, kind, v in SY.CONFIG2_FIELDS:
        if kind == "id":
            f2[k] = f2[k] % 5000
    f3 = SY.synth_din(B, 50, 5000, 7000, seed=12)
    m3 = M.DIN(seed=4, emb_dim=32, hist_len=50, movie_buckets=5000, user_buckets=7000)
    f5 = SY.synth_embedding_mlp(B, 1001, 30001, seed=13, rated_vocab=1001)
    m5 = M.EmbeddingMLP(seed=1)
    for f, m in ((f2, m2), (f3, m3), (f5, m5)):
        for k in S.FLOAT_KEYS:
            f[k] = f[k].copy()
            f[k][rng.random(B) < 0.03] = np.nan
        out.append((f, m))
    return out


def short_decimal_spellings():
    """Every placement of the sign and the dot over 1 .. 8 characters (the generator of the CSV tokenizer's short-decimal test, restated)."""
    rng = np.random.default_rng(77)
    vals = [".5", "5.", "-0", "+0", "0", "00000000", "99999999", "-9999999", "+1234.56", "-1234.56", "1234.567", ".0000001", "0.000001",
            "1000000.", "-.5", "+.5", "7", "-7", "0012.300", "9.999999", "4.", "000.000"]
    for _ in range(20000):
        n = int(rng.integers(1, 9))
        sign = ["", "-", "+"][int(rng.integers(0, 3))] if n > 1 else ""
        body = n - len(sign)
        digits = "".join(rng.choice(list("0123456789"), size=body))
        if body >= 2 and rng.random() < 0.6:
            d = int(rng.integers(0, body))
            digits = digits[:d] + "." + digits[d + 1:]
        if digits == ".":
            digits = "1"
        vals.append(sign + digits)
    return vals


LONG_NUMBERS = ["1234567890123456", "0.12345678901234567890", "3.141592653589793238462643383279", "1e23", "1.5e-30", "9007199254740993",
                "123456789012345678901234567890", "2.2250738585072014e-308", "1e-400", "4.9e-324", "1.7976931348623157e308", "0.1e30",
                "12345678901234567e-10", "1E25", "5e-23"]


def string_case():
    """-> (features as lists of str, id_columns, numeric_keys): genre, identity and dense columns of strings -- empty fields, every
    vocabulary entry, near misses, an embedded NUL, non-ASCII in a genre column, the exponent forms."""
    genres = list(S.GENRE_VOCAB) + ["", "drama", "Drama ", "Dram", "Dramas", "Sci-Fi\x00x", "Dra\x00ma", "Comédie", "Documentaryy", "IMAX" * 5, "ドラマ"]
    ids = ["0", "", "17", "999", "3.9", "1e2", "+5", "007", "12.", ".9", "9.99e2", "0.0", "-0", "-0.5", "1E1"]
    nums = ["", "0", "-0", "3.5", "-2.25", "1e3", "1E-3", "+7.125", ".5", "5.", "0.1", "16777217", "1.0000001", "123456.789012345", "9e22", "-9e-22", "00.10"]
    n = 4 * len(genres)
    f = {"g": [genres[i % len(genres)] for i in range(n)], "gsmall": [genres[(3 * i) % len(genres)] for i in range(n)],
         "i": [ids[i % len(ids)] for i in range(n)], "x": [nums[i % len(nums)] for i in range(n)], "y": [nums[(5 * i + 1) % len(nums)] for i in range(n)]}
    return f, [S.IdColumn("g", "genre", S.N_GENRES), S.IdColumn("i", "id", 1000), S.IdColumn("gsmall", "genre", 7)], ["x", "y"]


def string_forms(f, width=None):
    """The same string columns as object arrays (-> text block), as U and as S arrays (utf-8 bytes; wider than needed when ``width``)."""
    obj = {k: np.asarray(v, dtype=object) for k, v in f.items()}
    uni = {k: np.asarray(v, dtype=("U%d" % width) if width else str) for k, v in f.items()}
    byt = {k: np.asarray([s.encode("utf-8") for s in v], dtype=("S%d" % width) if width else "S") for k, v in f.items()}
    lst = {k: list(v) for k, v in f.items()}
    return {"object": obj, "U": uni, "S": byt, "list": lst}
