"""Model shapes NO fused kernel was instantiated for (tests/test_offvariant_cpu.py, tests/test_gpu_offvariant_shapes.py).

Every constructor of sparrowrecsys_amd/models.py takes widths, depths and history lengths the fused kernels do not cover.  The engine does
not refuse them: the attention stage goes to the generic k_din_pool, the forward to the plan interpreter k_tile_forward, to a k_mlp_rows
instantiation whose column counts are run-time values, or to a fused kernel with zero-padded units.  The other suites run those generic
kernels at the FUSED kernels' shapes only (under SPRK_DIN_LEGACY / SPRK_DIN_COLS / SPRK_FORCE_INTERPRETER); this table holds the shapes a
user reaches by passing a non-default argument.  Without any GPU import:

* ``CASES``: model class, constructor keywords, a batch size ragged against the route's granule (16-sample tasks, 64-sample tiles, MS
  samples per k_din_pool pass), seeds, and the route the dispatch rules predict as describe()'s ``stage`` (exact) and ``kernel`` (prefix) --
  or the message the engine must refuse the shape with;
* ``features`` / ``refs``: the inputs (3 000 / 5 000-row tables, a fifth of the history slots 0) and the fp64 / fp32 references, computed
  once per case and shared;
* the bars of the GPU file, none of them new: TIGHT = 3e-5 (tests/test_gpu_parity.py) and twice the fp32 oracle's own error + 2e-6 (the
  second bar of tests/test_gpu_value_range.py), for the pooled vector scaled by its magnitude;
* the slips of the sensitivity check: the smallest plausible mistake on each axis (one attention unit, one 16-unit block, one history slot,
  one embedding dimension), applied to the oracle's inputs.

Routes are predicted from host_setup_din.h (kDinVariants: row stride <= 32, attention width 32 after padding, T <= 64; k_din_fused from
T = 12), host_setup_din_tail.h (kDinTailVariants: 128/64 and 64/32, row stride <= 32), host_setup_mlp.h (two ReLU layers of 128; a cross
embedding of 4 .. 32 floats, a multiple of 4) and api_engine.h (the interpreter's 64-sample tile has to fit 160 KiB of LDS whatever route
is chosen later: sprk_create checks it before any set-up runs)."""
import numpy as np

from oracle import ctr_oracle as O
from sparrowrecsys_amd import models as M, synthetic as SY
from sparrowrecsys_amd.schema import MOVIE_GENRE_KEYS, NUMERIC_KEYS, USER_GENRE_KEYS
from tests.plan_interp import din_pool, run_plan
from tests.value_range_cases import LIVE_MIN, ORACLE32_MAX, TIGHT, live_share

V_MOVIE, V_USER = 3000, 5000
STD_MIN = 0.02                     # the scores are spread out: a comparison of near-constant scores would be vacuous
HIST_ZERO = 0.2                    # share of history slots set to 0 (tests/test_gpu_shape_sweep.py)
LDS_REFUSAL = "bytes of LDS per tile"


# ---- EmbeddingMLP with column counts no model class has: the run-time-count forms of k_mlp_rows ------------------------------------------
class ThreeGenresOneId(M.EmbeddingMLP):
    EMB_KEYS = ["userGenre1", "userGenre2", "movieGenre1", "movieId"]


class FiveGenresTwoIds(M.EmbeddingMLP):
    EMB_KEYS = ["userGenre1", "userGenre2", "userGenre3", "movieGenre1", "movieGenre2", "movieId", "userId"]


class EightNumerics(M.EmbeddingMLP):
    """An eighth numeric column: the first layer's bias no longer rides in the numerics' eighth K slot (host_setup_mlp.h, flags & 2)."""
    numeric_keys = NUMERIC_KEYS + ["rating"]

    def _numeric_kernel_rows(self):
        rows = self._deep_blocks_order()
        return {"dense0/kernel": {k: rows[k] for k in NUMERIC_KEYS}}      # ("rating" is of order 1: its weights stay as drawn)


class Case:
    def __init__(self, name, cls, kw, B, kernel, stage="", seed=0, refused=None, note=""):
        self.name, self.cls, self.kw, self.B, self.kernel, self.stage, self.refused, self.note = name, cls, dict(kw), B, kernel, stage, refused, note
        self.seed, self.fseed = 100 + seed, 200 + seed
        self.kind = "din" if cls is M.DIN else "wnd" if cls is M.WideNDeep else "mlp"
        self.plan_ref = cls not in (M.DIN, M.EmbeddingMLP, M.WideNDeep)     # a column subset: the oracle has no entry, the model's plan is the reference
        self.kw.setdefault("movie_buckets", V_MOVIE)
        self.kw.setdefault("user_buckets", V_USER)

    def __repr__(self):
        return self.name

    def model(self, weights=None):
        return self.cls(seed=self.seed, **self.kw) if weights is None else self.cls(weights=weights, **self.kw)

    # the shape, with the constructors' defaults
    D = property(lambda s: s.kw.get("emb_dim", 10))
    T = property(lambda s: s.kw.get("hist_len", 5))
    H = property(lambda s: s.kw.get("att_hidden", 32))


def _stage(T):
    """kDinVariants shapes: k_din_attn_cols below SprkTuning::din_fused_min_t = 12, k_din_fused's attention half from there on."""
    return "k_din_fused" if T >= 12 else "k_din_attn_cols"


_DIN = [
    # attention widths: 16 = one block (k_din_pool's one-block trip), 20 = padded to 32 (twelve inert units on the fused kernel), 48 / 64 = three / four
    ("att16", dict(att_hidden=16), 131, "k_din_tail<8,4,1", "k_din_pool"),
    ("att20-D32-T50", dict(att_hidden=20, emb_dim=32, hist_len=50), 515, "k_din_fused<KC=2", "k_din_fused"),
    ("att48-D16-T20", dict(att_hidden=48, emb_dim=16, hist_len=20), 777, "k_din_tail<8,4,1", "k_din_pool"),
    ("att64-D32-T33", dict(att_hidden=64, emb_dim=32, hist_len=33), 300, "k_din_tail<8,4,2", "k_din_pool"),
    # histories beyond kDinVariants' 64: MS = 256 / T = 3, 2, 1 samples per workgroup pass (B = 100: the last pass of MS = 3 holds one sample)
    ("T65-D32", dict(hist_len=65, emb_dim=32), 100, "k_din_tail<8,4,2", "k_din_pool"),
    ("T100-D16", dict(hist_len=100, emb_dim=16), 777, "k_din_tail<8,4,1", "k_din_pool"),
    ("T256-D10", dict(hist_len=256, emb_dim=10), 65, "k_din_tail<8,4,1", "k_din_pool"),
    ("T256-D32", dict(hist_len=256, emb_dim=32), 33, "k_din_tail<8,4,2", "k_din_pool"),
    # rows wider than 32 floats: no attention variant, no tail variant; the interpreter with an AUX segment and the first-Dense fold
    ("D33-T7", dict(emb_dim=33, hist_len=7), 259, "k_tile_forward", "k_din_pool"),
    ("D40-T20", dict(emb_dim=40, hist_len=20), 1000, "k_tile_forward", "k_din_pool"),
    ("D64-T50", dict(emb_dim=64, hist_len=50), 515, "k_tile_forward", "k_din_pool"),
    # tails other than 128/64 and 64/32: the interpreter behind the fused attention stage
    ("tail256x128-D16-T12", dict(hidden=(256, 128), emb_dim=16, hist_len=12), 333, "k_tile_forward", _stage(12)),
    ("tail200x80", dict(hidden=(200, 80)), 131, "k_tile_forward", _stage(5)),
    ("tail64x256-D6", dict(hidden=(64, 256), emb_dim=6), 65, "k_tile_forward", _stage(5)),
    ("tail16x16-D6-T3", dict(hidden=(16, 16), emb_dim=6, hist_len=3), 1, "k_tile_forward", _stage(3)),
    ("tail100x50", dict(hidden=(100, 50)), 777, "k_tile_forward", _stage(5)),
    ("tail128", dict(hidden=(128,)), 131, "k_tile_forward", _stage(5)),
    ("tail128x64x32-D32-T20", dict(hidden=(128, 64, 32), emb_dim=32, hist_len=20), 259, "k_tile_forward", _stage(20)),
]
_ROWS_28 = "k_mlp_rows<8,8,NBIG=2,NSMALL=8>"
_MLP = [
    ("mlp64x32", M.EmbeddingMLP, dict(hidden=(64, 32)), 131, "k_tile_forward"),
    ("mlp100x50-D24", M.EmbeddingMLP, dict(hidden=(100, 50), emb_dim=24), 777, "k_tile_forward"),
    ("mlp128", M.EmbeddingMLP, dict(hidden=(128,)), 65, "k_tile_forward"),
    ("mlp256x128x64", M.EmbeddingMLP, dict(hidden=(256, 128, 64)), 259, "k_tile_forward"),
    ("mlp-D4", M.EmbeddingMLP, dict(emb_dim=4), 333, _ROWS_28),               # (the fold absorbs the width)
    ("mlp-D64", M.EmbeddingMLP, dict(emb_dim=64), 333, _ROWS_28),             # (k_mlp_rows would take it; see REFUSED below)
    ("mlp-V25-U1", M.EmbeddingMLP, dict(movie_buckets=25, user_buckets=1), 131, _ROWS_28),   # (the eight small slots are the genres': both ids stay big)
    ("wnd-cross8", M.WideNDeep, dict(cross_dim=8, cross_buckets=5000, emb_dim=32), 515, _ROWS_28),
    ("wnd-cross6", M.WideNDeep, dict(cross_dim=6, cross_buckets=5000, emb_dim=32), 515, "k_tile_forward"),
    ("wnd-cross64", M.WideNDeep, dict(cross_dim=64, cross_buckets=5000, emb_dim=32), 259, "k_tile_forward"),
    ("wnd128x64-indicator", M.WideNDeep, dict(hidden=(128, 64), cross_dim=0), 131, "k_tile_forward"),
    ("wnd32x16-cross32", M.WideNDeep, dict(hidden=(32, 16), cross_dim=32, cross_buckets=777, emb_dim=16), 1000, "k_tile_forward"),
    ("rows-3genres-1id", ThreeGenresOneId, {}, 259, "k_mlp_rows<8,8,NBIG=1,NSMALL=3>"),
    ("rows-5genres-2ids", FiveGenresTwoIds, {}, 259, "k_mlp_rows<8,8,NBIG=2,NSMALL=5>"),
    ("rows-8numerics", EightNumerics, {}, 259, _ROWS_28),
]
# Shapes the engine refuses, each with its own message.  mlp-D64: ten 64-float columns + the numerics are 648 floats per sample; the
# interpreter's tile of 64 samples (+ the 128-wide hidden buffer) is 203 264 bytes of LDS.  sprk_create sizes that tile for EVERY plan,
# before finalize looks for a fused route -- k_mlp_rows folds the columns and would not need the tile -- so the shape is refused up front
# with "plan needs ... bytes of LDS per tile (> 160 KiB)", as test_deepfm_pair_dot_random_shapes' wide pair-dot shapes are.
REFUSED = {"mlp-D64": LDS_REFUSAL}

# Seeds: the case's index, except where that draw misses the input conditions.  At T = 256 the pooled sum is tens of units large and most draws
# of the tail's weights saturate it or leave the scores flat (index seeds: live share 0.82 / std 0.002 at D = 10, std 0.017 at D = 32)
_SEED = {"T256-D10": 13, "T256-D32": 28}
CASES = [Case("din-" + n, M.DIN, kw, B, kern, stage, seed=_SEED.get(n, i)) for i, (n, kw, B, kern, stage) in enumerate(_DIN)]
CASES += [Case(n, cls, kw, B, kern, seed=50 + i, refused=REFUSED.get(n)) for i, (n, cls, kw, B, kern) in enumerate(_MLP)]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
DIN_NAMES = [c.name for c in CASES if c.kind == "din"]
T_TOO_LONG = 257                                                          # validate_plan: "DIN history length 257 outside [1,256]"
BATCHED = ["din-att48-D16-T20", "din-T100-D16", "din-D40-T20", "mlp100x50-D24"]   # batching and determinism


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def features(c, n):
    """``n`` rows of the case's input distribution."""
    V, U = c.kw["movie_buckets"], c.kw["user_buckets"]
    if c.kind == "din":
        f = SY.synth_din(n, c.T, V, U, seed=c.fseed)
        h = f["userRatedMovies"]
        h[np.random.default_rng(c.fseed + 1).random(h.shape) < HIST_ZERO] = 0
        return f
    f = SY.synth_embedding_mlp(n, max(V, 2), max(U, 2), seed=c.fseed, rated_vocab=V if c.kind == "wnd" else None)
    f["movieId"] %= V                                                      # (a one-row table: its only id is 0)
    f["userId"] %= U
    f["rating"] = np.round(np.random.default_rng(c.fseed + 2).uniform(0.5, 5.0, n), 1).astype(np.float32)
    return f


def subset_oracle(c, feats, w, dtype):
    """EmbeddingMLP.py:72-77 over the subclass' own columns, from the oracle's feature-column blocks (what _embedding_mlp_body does for
    the full column set)."""
    m = c.model(w)
    blocks = O._numeric_blocks(feats, dtype, m.numeric_keys)
    for k in m.EMB_KEYS:
        ids = O.vocab_ids(feats[k]) if k in USER_GENRE_KEYS + MOVIE_GENRE_KEYS else O.identity_ids(O.int_feature(feats, k), m._vocab(k), k)
        blocks[k + "_embedding"] = O.embedding_lookup(np.asarray(w["emb/" + k]).astype(dtype), ids)
    x, _ = O.dense_features(blocks)
    for i in range(len(m.hidden)):
        x = O.relu(O.dense(x, w["dense%d/kernel" % i], w["dense%d/bias" % i], dtype))
    return O.sigmoid(O.dense(x, w["head/kernel"], w["head/bias"], dtype)).astype(np.float32)


def oracle(c, feats, w, dtype):
    """-> (scores [B], parts or None) of the oracle in ``dtype``."""
    V, U = c.kw["movie_buckets"], c.kw["user_buckets"]
    if c.kind == "din":
        p, parts = O.din_forward(feats, w, dtype=dtype, hist_len=c.T, movie_buckets=V, user_buckets=U, return_parts=True)
        return p[:, 0], parts
    if c.plan_ref:
        return subset_oracle(c, feats, w, dtype)[:, 0], None
    if c.kind == "wnd":
        return O.wide_n_deep_forward(feats, w, dtype=dtype, movie_buckets=V, user_buckets=U, cross_buckets=c.kw.get("cross_buckets", 10000),
                                     rated_buckets=V)[:, 0], None
    return O.embedding_mlp_forward(feats, w, dtype=dtype, movie_buckets=V, user_buckets=U)[:, 0], None


class Refs:
    """One case's model, inputs and references; computed once (``refs``) and not modified by any test.

    The input conditions are properties of the model and of the distribution its inputs are drawn from, so they are taken over
    max(B, 256) rows of that draw (one row has no standard deviation); the case's batch is the first B of those rows, and every error
    figure and bar below is taken over these B rows alone."""
    POOL = 256

    def __init__(self, c):
        self.case, self.model = c, c.model()
        w, B = self.model.weights, c.B
        pool = features(c, max(B, self.POOL))
        p64, parts64 = oracle(c, pool, w, np.float64)
        p32, parts32 = oracle(c, pool, w, np.float32)
        self.live, self.std = live_share(p64), float(np.std(p64))
        self.e32_pool = float(np.abs(np.asarray(p32, np.float64) - p64).max())
        self.feats = {k: v[:B] for k, v in pool.items()}
        self.o64, self.o32 = p64[:B], p32[:B]
        self.parts64 = {k: v[:B] for k, v in parts64.items()} if parts64 else None
        self.parts32 = {k: v[:B] for k, v in parts32.items()} if parts32 else None
        self.plan, self.slots = self.model.build_plan()
        self.ids, self.dense = self.model._pack_python(self.feats)
        self.plan64 = run_plan(self.plan, self.slots, self.ids, self.dense, np.float64)
        # the GPU file's reference: the fp64 oracle; for a column subset the model's own plan in float64 (pinned to subset_oracle on the CPU)
        self.ref = self.plan64 if c.plan_ref else np.asarray(self.o64, np.float64)
        self.e32 = float(np.abs(np.asarray(self.o32, np.float64) - self.o64).max())
        if c.kind == "din":
            a64, p64 = self.parts64["att"], self.parts64["pooled"]
            self.e32_att = float(np.abs(self.parts32["att"].astype(np.float64) - a64).max())
            self.e32_pooled = float(np.abs(self.parts32["pooled"].astype(np.float64) - p64).max())
            self.pooled_mag = float(np.abs(p64).max())

    def conditions_met(self):
        return self.live >= LIVE_MIN and self.std >= STD_MIN and self.e32_pool <= ORACLE32_MAX

    # ---- the bars of the GPU file ----
    def score_bar(self):
        return min(TIGHT, 2 * self.e32 + 2e-6)

    def att_bar(self):
        return min(TIGHT, 2 * self.e32_att + 2e-6)

    def pooled_bar(self):
        """A sum over T slots grows with T (max |pooled| = 33 at T = 256, where the fp32 oracle itself is 1.6e-5 off): twice the fp32
        oracle's own error of the pooled vector + 2e-6 relative to its magnitude."""
        return 2 * self.e32_pooled + 2e-6 * max(1.0, self.pooled_mag)


_REFS = {}


def refs(name):
    if name not in _REFS:
        _REFS[name] = Refs(BY_NAME[name])
    return _REFS[name]


def plan_parts(r):
    """-> (pooled [B, Dp], att [B, T]) of the model's own plan in float64."""
    return din_pool(r.plan, r.slots, r.ids, np.float64)


# ---- the slips of the sensitivity check ----------------------------------------------------------------------------------------------------
def _moved(r, w=None, feats=None):
    """How far att / pooled of the fp64 oracle move under changed weights or features: (max |d att|, max |d pooled|)."""
    c = r.case
    _, parts = oracle(c, r.feats if feats is None else feats, r.model.weights if w is None else w, np.float64)
    return float(np.abs(parts["att"] - r.parts64["att"]).max()), float(np.abs(parts["pooled"] - r.parts64["pooled"]).max())


def slip_last_unit(r):
    """The last real attention unit dropped: what a kernel that mishandles the partial 16-block (or the padding) would lose."""
    w = dict(r.model.weights)
    w["att1/kernel"] = w["att1/kernel"].copy()
    w["att1/kernel"][-1] = 0
    return _moved(r, w=w)


def slip_last_block(r):
    """The last 16-unit block dropped whole: a block loop that ends one trip early (k_din_pool takes two blocks per trip)."""
    w = dict(r.model.weights)
    w["att1/kernel"] = w["att1/kernel"].copy()
    w["att1/kernel"][16 * ((r.case.H - 1) // 16):] = 0
    return _moved(r, w=w)


def slip_last_slot(r):
    """The last history slot replaced by another movie: a pass that reads the wrong sample's slot or stops one slot short."""
    f = dict(r.feats)
    h = f["userRatedMovies"].copy()
    h[:, -1] = (h[:, -1] + 1 + np.arange(len(h))) % (V_MOVIE - 1) + 1
    f["userRatedMovies"] = h
    return _moved(r, feats=f)


def slip_last_dim(r):
    """One input row of att0/kernel zeroed -- the last embedding dimension of the h * c block: a K loop that stops at 32 floats."""
    w = dict(r.model.weights)
    w["att0/kernel"] = w["att0/kernel"].copy()
    w["att0/kernel"][4 * r.case.D - 1] = 0
    return _moved(r, w=w)


SLIPS = ([("last unit", slip_last_unit, n) for n in DIN_NAMES[:4]]
         + [("last block", slip_last_block, n) for n in ("din-att20-D32-T50", "din-att48-D16-T20", "din-att64-D32-T33")]
         + [("last slot", slip_last_slot, n) for n in ("din-T65-D32", "din-T100-D16", "din-T256-D10", "din-T256-D32")]
         + [("last dim", slip_last_dim, n) for n in ("din-D40-T20", "din-D64-T50")])
