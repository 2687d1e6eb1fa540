"""Inputs and a restatement shared by tests/test_split.py and tests/test_gpu_split.py: sample-like columns at any size, the timestamp
patterns the radix select can go wrong on, and the draw in Python integers."""
import numpy as np

INT64_MIN, INT64_MAX = int(np.iinfo(np.int64).min), int(np.iinfo(np.int64).max)
MASK = (1 << 64) - 1
# (seed, stream, key) -> u: DESIGN.md section 5.17's pins
PINS = {(0, 0, 0): 7956156453446585, (0, 1, 0): 3886858653415212, (1, 0, 5): 3640189043878601, ((1 << 63) + 7, 1, (1 << 31) - 2): 726993394987508,
        (12345, 0, 1000000): 5374023049858795}
THRESHOLDS = {0.0: 0, 0.1: 900719925474099, 0.5: 1 << 52, 0.8: 7205759403792794, 1.0: 1 << 53}
TILE = 1024                                 # rows of a tile of the split's kernels; a workgroup takes 256 a round
SIZES = [0, 1, 255, 256, 257, 1023, 1024, 1025]


def draw(seed: int, stream: int, key: int) -> int:
    """The definition's draw, restated in Python integers."""
    x = (seed + 0x9E3779B97F4A7C15 * (2 * key + stream + 1)) & MASK
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & MASK
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & MASK
    x ^= x >> 31
    return x >> 11


def timestamps(n, kind="random", seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "random":
        return rng.integers(1_000_000_000, 1_400_000_000, n, dtype=np.int64)
    if kind == "ties":                                                       # a range of 50 values: every rank sits in a run of equals
        return rng.integers(1_000_000, 1_000_050, n, dtype=np.int64)
    if kind == "equal":
        return np.full(n, 1_234_567_890, dtype=np.int64)
    if kind == "bit63":                                                      # two values that differ in the sign bit alone
        return np.where(rng.random(n) < 0.5, np.int64(5), np.int64(5 + INT64_MIN))
    if kind == "top_byte":                                                   # bits 56 .. 63 differ, the other 56 are one pattern
        return ((rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x00A5A5A5A5A5A5A5)).view(np.int64)
    if kind == "low_byte":
        return np.int64(0x0123456789ABCD00) + rng.integers(0, 256, n, dtype=np.int64)
    if kind == "extremes":                                                   # the whole range, both ends present (twice: ties at the ends)
        t = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
        t[rng.permutation(n)[:4]] = [INT64_MIN, INT64_MAX, INT64_MIN, INT64_MAX][:min(n, 4)]
        return t
    raise KeyError(kind)


def two_values(n, n_low, seed=0):
    """n timestamps, n_low of them 100 and the others 200, shuffled."""
    t = np.where(np.arange(n) < n_low, np.int64(100), np.int64(200))
    return t[np.random.default_rng(seed).permutation(n)]


def columns(n, seed=0, ts="random", key="shuffled"):
    """A dict shaped like a few columns of samples_host's: int32, float32 and int64 columns; source_row a permutation (shuffled), the
    positions (ordered), or int64 keys beyond 2^32 (wide)."""
    rng = np.random.default_rng(seed)
    if key == "shuffled":
        src = rng.permutation(n).astype(np.int32)
    elif key == "ordered":
        src = np.arange(n, dtype=np.int32)
    else:
        src = (rng.permutation(n).astype(np.int64) * 3 + (1 << 33))
    return {"userId": rng.integers(0, 1000, n).astype(np.int32), "movieId": rng.integers(0, 500, n).astype(np.int32),
            "rating": (rng.integers(1, 11, n) * 0.5).astype(np.float32), "timestamp": timestamps(n, ts, seed),
            "label": rng.integers(0, 2, n).astype(np.int32), "source_row": src}


def same_split(got, want):
    """Two SplitResults (host columns) byte for byte: every column of both parts, dtype and length, n_sampled, split_timestamp."""
    assert got.n_sampled == want.n_sampled and got.split_timestamp == want.split_timestamp, (got.n_sampled, want.n_sampled, got.split_timestamp, want.split_timestamp)
    for g, w, name in ((got.train, want.train, "train"), (got.test, want.test, "test")):
        assert list(g) == list(w), name
        for k in w:
            a, b = np.ascontiguousarray(g[k]), np.ascontiguousarray(w[k])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, k, a.shape, b.shape)
