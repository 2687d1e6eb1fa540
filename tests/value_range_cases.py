"""Value-range cases for every kernel built on the split-f16 idiom (tests/test_value_range_cpu.py, tests/test_gpu_value_range.py).

An operand is multiplied by a power of two, split into hi + lo f16 halves and fed to the f16 matrix pipe.  Where the scale is STATIC (one
power of two per table or weight matrix, chosen at finalize from max |x|) this is fp32-class only while the operand's dynamic range stays
under about 2^20; a finalize-time guard (wide_dynamic_range, host_setup_common.h) has to notice the other case and keep the f32 variant.
``describe()["split_f16"]`` names the sites that run split (api_forward.h).  This module holds, without any GPU import:

* ``live_share`` and the two INPUT conditions every compared case has to meet on the oracle alone (``conditions``): at least 0.9 of the
  fp64 oracle's scores have |logit| < 8 (a saturated sigmoid hides any error), and the fp32 oracle is within 1e-5 of the fp64 oracle
  (a third of TIGHT: the other 2e-5 are left for summation order);
* the ROUTES: one entry per kernel, with the describe() it has to report and the switches that select its f32 twin;
* the CASES: functions of a route's weights / features.

Static-scale sites, the describe token of each, and the case that reaches it:

  site                                              token      guard        cases
  DeepFM_v2 folded rows p_scale, W0 w_scale          v2         yes / yes    outlier_row, small_table (*), outlier_weight, nonfinite_*
  DIN attention tables h_scale, a_scale              din_attn   yes (**)     outlier_row, nonfinite_row, scale_down
  pair-dot deep tables e_scale                       pairs_e    yes          outlier_row, small_table, nonfinite_row
  rows chain raw rows p_scale; projection w_scale    rows_unf   yes / yes    outlier_row, small_table, outlier_weight, nonfinite_*
  DIN / DIEN tail raw rows e_scale; fc0 w_scale      tail_unf   yes / yes    outlier_row, small_table, outlier_weight, nonfinite_*
  weight fragments of the dynamic chains             dyn_w1 ..  yes          outlier_weight (dead hidden unit), nonfinite_weight
  DIEN sequence stage s_xh, s_p, 12 block scales     dien_seq   yes / yes    outlier_row, outlier_weight, nonfinite_*

(*) DeepFM_v2 scales the FOLDED rows P = E Wp + bp: a whole table times 2^-24 leaves P at the projection's bias, which is not small, so the
guard need not act; ``guard_trips`` applies the rule to the operand the site really scales and the case expects what it says.
(**) and a range window of its own for W4 (din_attention_fits): tables x 2^-12 leave it, the stage falls back to k_din_pool by design.
The per-sample DYNAMIC scales (dyn_split.h: the hidden activations of every chain) have no finalize-time guard by construction -- the scale
follows each sample -- and are probed by scale_down / scale_up / numeric_spread / poisoned_sample instead.
NeuralCF's chain (k_rows_chain without UNF) has no split-f16 operand at all: it runs the compared cases against the interpreter as its twin."""
import numpy as np

from oracle import ctr_oracle as O
from sparrowrecsys_amd import models as M, synthetic as SY
from sparrowrecsys_amd.schema import NUMERIC_KEYS

TIGHT = 3e-5                       # tests/test_gpu_parity.py: fp32-class against the fp64 oracle
LIVE_MIN = 0.9                     # share of oracle scores with |logit| < 8
ORACLE32_MAX = 1e-5                # fp32 oracle against fp64 oracle
B = 4096
V_MOVIE, V_USER = 3000, 5000
FREE_ROW = 3                       # the table row no sample references (features(): id 3 -> 4 in every id column)
OUTLIER_FACTORS = (3.0e8, 2.0 ** 36)
POISONS = (("nan", np.float32("nan")), ("+inf", np.float32("inf")), ("-inf", np.float32("-inf")), ("3e38", np.float32(3e38)),
           ("subnormal", np.float32(1e-40)), ("-0.0", np.float32(-0.0)))
POISON_ASSERTED = ("subnormal", "-0.0")                    # the poisoned sample's own score is compared with the oracle for these only
POISON_COLUMN = "movieAvgRating"


def live_share(ref):
    """Share of fp64 oracle scores whose logit lies in (-8, 8)."""
    p = np.asarray(ref, np.float64).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        logit = np.log(p) - np.log1p(-p)
    return float((np.abs(logit) < 8).mean())


def conditions(ref64, ref32):
    """-> (live share, max |fp32 oracle - fp64 oracle|, both conditions met)."""
    live, e32 = live_share(ref64), float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    return live, e32, bool(live >= LIVE_MIN and e32 <= ORACLE32_MAX)


def guard_trips(tables):
    """wide_dynamic_range's rule on each of ``tables`` against one joint maximum: more than 1 in 1024 of the non-zero entries lie over 2^20
    below the maximum.  A non-finite maximum refuses the site as well (every set-up's `mx < 3.0e38f`)."""
    mx = max(float(np.abs(t).max()) for t in tables)
    if not mx < 3.0e38:
        return True
    for t in tables:
        a = np.abs(np.asarray(t, np.float32))
        if (a[a > 0] < np.float32(mx) * np.float32(2.0 ** -20)).sum() * 1024 > (a > 0).sum():
            return True
    return False


def pow2_scale(m):
    """host_setup_common.h: the power of two that puts m * scale in [2^14, 2^15), the exponent clamped to +-60; 1 for m <= 0."""
    return 2.0 ** min(60, max(-60, 15 - int(np.frexp(np.float32(m))[1]))) if m > 0 else 1.0


def din_attention_fits(w):
    """setup_din_attn's own range rule (host_setup_din.h, "a W4 whose range does not fit the split"): with h_scale from max |E| and a_scale
    from max |W12| + max |W4| max |E|, the h*c block's weights carry s4 = a_scale 2^15 / h_scale and max |W4| s4 has to lie in [16, 60000) --
    f16's normal range with headroom.  Outside it the attention tables are refused and the generic f32 k_din_pool runs the stage: a documented
    fall-back, so a case that leaves the window expects describe() without din_attn instead of pretending the split path stayed on."""
    K, E = np.asarray(w["att0/kernel"], np.float32), np.asarray(w["emb/movie"], np.float32)
    D = E.shape[1]
    mx0, mx1, mx2 = float(np.abs(E).max()), float(np.abs(K[:D] + K[D:2 * D]).max()), float(np.abs(K[3 * D:4 * D]).max())
    w4s = mx2 * pow2_scale(np.float32(mx1) + np.float32(mx2) * np.float32(mx0)) * 32768.0 / pow2_scale(mx0)
    return mx2 == 0 or 16.0 <= w4s < 60000.0


def static_split(x):
    """The UNGUARDED static split of one table: scale = the power of two that puts max |x| in [2^14, 2^15) (pow2_scale), hi = f16(x s),
    lo = f16(x s - hi); what the matrix pipe then multiplies is (hi + lo) / s.  numpy's float16 rounds to nearest even and goes subnormal
    as the hardware's conversion does."""
    x = np.asarray(x, np.float32)
    s = np.float32(pow2_scale(float(np.abs(x[np.isfinite(x)]).max())))
    with np.errstate(over="ignore"):
        xs = x * s
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return ((hi.astype(np.float32) + lo.astype(np.float32)) / s).astype(np.float32)


# ---- routes -----------------------------------------------------------------------------------------------------------------------------
GENRES3 = [("userGenre1", "genre", 19), ("userGenre2", "genre", 19), ("movieGenre1", "genre", 19)]
F6 = [("movieId", "id", V_MOVIE), ("userId", "id", V_USER), ("userRatedMovie1", "id", V_MOVIE)] + GENRES3
F4 = [("movieId", "id", V_MOVIE), ("userId", "id", V_USER), ("userGenre1", "genre", 19), ("movieGenre1", "genre", 19)]
F4_ORDER = list(M.DeepFMv2.DEFAULT_ORDER)


def _tame(feats):
    """Numerics in sigmoid's live range (the existing range tests' `% 7`), all as float32; id FREE_ROW referenced by nobody."""
    out = {}
    for k, v in feats.items():
        v = np.asarray(v)
        if k in NUMERIC_KEYS:
            if k in ("movieRatingCount", "userRatingCount", "releaseYear"):
                v = np.asarray(v, np.float64) % 7
            out[k] = np.ascontiguousarray(v, dtype=np.float32)
        else:
            out[k] = np.where(v == FREE_ROW, FREE_ROW + 1, v).astype(v.dtype)
    return out


class Model:
    """One model shape: constructor, inputs, oracle."""

    def __init__(self, name, cls, kw, seed, feats, oracle):
        self.name, self.cls, self.kw, self.seed, self._feats, self._oracle = name, cls, kw, seed, feats, oracle
        self._w = None

    def build(self, weights=None):
        return self.cls(weights=self.weights() if weights is None else weights, **self.kw)

    def weights(self):
        if self._w is None:
            self._w = dict(self.cls(seed=self.seed, **self.kw).weights)
        return dict(self._w)

    def features(self):
        return _tame(self._feats())

    def oracle(self, feats, w, dtype=np.float64):
        with np.errstate(all="ignore"):
            return np.asarray(self._oracle(feats, w, dtype), dtype)[:, 0]


def _din_like(name, cls, fwd, T, D, seed):
    kw = dict(emb_dim=D, hist_len=T, movie_buckets=V_MOVIE, user_buckets=V_USER)
    return Model(name, cls, kw, seed, lambda: SY.synth_din(B, T, V_MOVIE, V_USER, seed=seed + 1),
                 lambda f, w, dt: fwd(f, w, dtype=dt, hist_len=T, movie_buckets=V_MOVIE, user_buckets=V_USER))


def _mlp_like(name, cls, fwd, seed, **extra):
    kw = dict(emb_dim=10, movie_buckets=V_MOVIE, user_buckets=V_USER, **extra)
    okw = dict(movie_buckets=V_MOVIE, user_buckets=V_USER)
    if cls is M.WideNDeep:
        okw.update(cross_buckets=extra["cross_buckets"], rated_buckets=V_MOVIE)
    rated = V_MOVIE if cls is M.WideNDeep else None
    return Model(name, cls, kw, seed, lambda: SY.synth_embedding_mlp(B, V_MOVIE, V_USER, seed=seed + 1, rated_vocab=rated),
                 lambda f, w, dt: fwd(f, w, dtype=dt, **okw))


MODELS = {m.name: m for m in (
    Model("deepfm_v2_c2", M.DeepFMv2, dict(emb_dim=16, fields=F6, proj_dim=16), 201, lambda: SY.synth_fields(B, F6, seed=202),
          lambda f, w, dt: O.deepfm_v2_forward(f, w, dtype=dt, fields=F6, order=[k for k, _, _ in F6])),
    Model("deepfm_c2", M.DeepFM, dict(emb_dim=16, fields=F6, pairs=SY.CONFIG2_PAIRS), 203, lambda: SY.synth_fields(B, F6, seed=204),
          lambda f, w, dt: O.deepfm_forward(f, w, dtype=dt, fields=F6, pairs=SY.CONFIG2_PAIRS)),
    Model("deepfm_v2_ref", M.DeepFMv2, dict(emb_dim=10, fields=F4, order=F4_ORDER, proj_dim=64), 205, lambda: SY.synth_fields(B, F4, seed=206),
          lambda f, w, dt: O.deepfm_v2_forward(f, w, dtype=dt, fields=F4, order=F4_ORDER)),
    _mlp_like("embedding_mlp", M.EmbeddingMLP, O.embedding_mlp_forward, 207),
    _mlp_like("widedeep", M.WideNDeep, O.wide_n_deep_forward, 209, cross_buckets=10000, cross_dim=16),
    Model("neuralcf", M.NeuralCF, dict(emb_dim=10, movie_buckets=V_MOVIE, user_buckets=V_USER), 211,
          lambda: SY.synth_fields(B, F4[:2], seed=212),
          lambda f, w, dt: O.neural_cf_forward(f, w, dtype=dt, movie_buckets=V_MOVIE, user_buckets=V_USER)),
    _din_like("din_t50_d32", M.DIN, O.din_forward, 50, 32, 213),
    _din_like("din_t5_d10", M.DIN, O.din_forward, 5, 10, 215),
    _din_like("dien_t5_d10", M.DIEN, O.dien_forward, 5, 10, 217),
)}

TAIL = ("dyn_w1", "dyn_w0p", "tail_unf")
_F32_TAIL = {"SPRK_DYN_F16": "0"}


class Route:
    """A kernel route: the model, the switches that select it, what describe() has to say, the switches of its f32 twin, and per poisoned
    operand (a table or Dense kernel key) what describe() has to say once the guard has acted: (kernel prefix, UNF in kernel, stage, sites)."""

    def __init__(self, name, model, kernel, stage, split, twin_env, twin, env=None, unf=None, after=None, row_tables=(), joint_tables=(),
                 zero_col=(), dead_unit=(), nan_weights=()):
        self.name, self.model, self.kernel, self.stage, self.split = name, MODELS[model], kernel, stage, frozenset(split)
        self.env, self.twin_env, self.twin, self.unf = dict(env or {}), dict(twin_env), twin, unf
        self.after = after or {}
        self.row_tables = tuple(row_tables)          # tables a static scale is taken from (outlier_row, nonfinite_row)
        self.joint_tables = tuple(joint_tables)      # tables that share ONE scale (small_table takes the last of them)
        self.zero_col = tuple(zero_col)              # (table, column d, kernel, kernel row): the row multiplies an all-zero embedding column
        self.dead_unit = tuple(dead_unit)            # (first layer, second layer): the second layer's row of a dead hidden unit
        self.nan_weights = tuple(nan_weights)

    def expected(self, key=None):
        """-> dict(kernel, unf, stage, split) describe() must report; ``key``: the poisoned operand, None = the split path."""
        e = dict(kernel=self.kernel, unf=self.unf, stage=self.stage, split=self.split)
        if key is not None:
            e.update(self.after[key])
            e["split"] = frozenset(e["split"])
        return e


def _tail_after(kernel_full, stage_full, stage_site, fused_needs_raw, stage_f32):
    """describe() of a DIN / DIEN route after a poison in each operand of its tail and stage."""
    full = set(TAIL) | {stage_site}
    a = {}
    # the candidate / history table: the stage's own tables AND the tail's raw rows are refused
    a["emb/movie"] = dict(kernel="k_din_tail", unf=False, stage=stage_f32, split=set(TAIL[:2]))
    for t in ("emb/userId", "emb/userGenre1", "emb/movieGenre1"):            # the tail's raw rows only
        a[t] = dict(kernel="k_din_tail" if fused_needs_raw else kernel_full, unf=False if kernel_full == "k_din_tail" or fused_needs_raw else None,
                    stage=stage_full, split=full - {"tail_unf"})
    a["fc0/kernel"] = a["emb/userId"]                                          # fc0's columns of the raw rows
    # fc1's fragments refused: every f16 form of the tail goes with them (and the one-launch kernels, which need them)
    a["fc1/kernel"] = dict(kernel="k_din_tail", unf=False, stage=stage_full, split={stage_site})
    # DIN only: the attention weights leave setup_din_attn's W4 window (din_attention_fits): the stage alone falls back
    a["att_range"] = dict(kernel="k_din_tail", unf=True, stage=stage_f32, split=set(TAIL))
    return a


_DIN_TWIN = {"SPRK_DIN_COLS": "0", "SPRK_DYN_F16": "0"}
_DIEN_TWIN = {"SPRK_DIEN_MFMA": "0", "SPRK_DYN_F16": "0"}
_DIN_TABLES = ("emb/movie", "emb/userId", "emb/userGenre1", "emb/movieGenre1")


def _din_route(name, model, kernel, stage, env, unf):
    m = MODELS[model]
    D = m.kw["emb_dim"]
    urow = m.cls(seed=0, **m.kw)._fc_rows()[0]["userId_embedding"][0]
    return Route(name, model, kernel, stage, set(TAIL) | {"din_attn"}, _DIN_TWIN, dict(kernel="k_din_tail", unf=False, stage="k_din_pool", split=()),
                 env=env, unf=unf, after=_tail_after(kernel, stage, "din_attn", False, "k_din_pool"), row_tables=_DIN_TABLES,
                 joint_tables=("emb/movie", "emb/userId"), zero_col=(("emb/userId", D - 1, "fc0/kernel", urow + D - 1),),
                 dead_unit=(("fc0", "fc1"),), nan_weights=("fc1/kernel", "fc0/kernel"))


def _dien_route(name, kernel, env, unf, fused):
    m = MODELS["dien_t5_d10"]
    D = m.kw["emb_dim"]
    urow = m.cls(seed=0, **m.kw)._fc_rows()[0]["userId_embedding"][0]
    after = _tail_after(kernel, "k_dien_seq_mfma", "dien_seq", fused, "k_dien_seq")
    after["gru/kernel"] = dict(kernel="k_din_tail", unf=True, stage="k_dien_seq", split=set(TAIL))
    return Route(name, "dien_t5_d10", kernel, "k_dien_seq_mfma", set(TAIL) | {"dien_seq"}, _DIEN_TWIN,
                 dict(kernel="k_din_tail", unf=False, stage="k_dien_seq", split=()), env=env, unf=unf, after=after, row_tables=_DIN_TABLES,
                 joint_tables=("emb/movie", "emb/userId"),
                 zero_col=(("emb/userId", D - 1, "fc0/kernel", urow + D - 1), ("emb/movie", D - 1, "gru/kernel", D - 1)),
                 dead_unit=(("fc0", "fc1"),), nan_weights=("fc1/kernel", "fc0/kernel", "gru/kernel"))


def _mlp_route(name, model):
    return Route(name, model, "k_mlp_rows", "", {"dyn_w1"}, _F32_TAIL, dict(kernel="k_mlp_rows", unf=None, stage="", split=()),
                 after={"dense1/kernel": dict(split=())}, dead_unit=(("dense0", "dense1"),), nan_weights=("dense1/kernel",))


_V2_BIG = ("emb/movieId", "emb/userId", "emb/userRatedMovie1")
ROUTES = {r.name: r for r in (
    Route("k_deepfm_v2_joint", "deepfm_v2_c2", "k_deepfm_v2_joint", "", {"v2"}, {"SPRK_V2_HALF": "0"},
          dict(kernel="k_deepfm_v2_joint", unf=None, stage="", split=()),
          after={k: dict(split=()) for k in _V2_BIG + ("deep0/kernel",)}, row_tables=_V2_BIG, joint_tables=_V2_BIG, nan_weights=("deep0/kernel",)),
    Route("k_deepfm_pairs", "deepfm_c2", "k_deepfm_pairs", "", {"dyn_w1", "dyn_w0", "pairs_e"}, _F32_TAIL,
          dict(kernel="k_deepfm_pairs", unf=None, stage="", split=()),
          after={"deep_emb/movieId": dict(split=("dyn_w1", "dyn_w0")), "deep_emb/userId": dict(split=("dyn_w1", "dyn_w0")), "deep1/kernel": dict(split=())},
          row_tables=("deep_emb/movieId", "deep_emb/userId"), joint_tables=("deep_emb/movieId", "deep_emb/userId"),
          dead_unit=(("deep0", "deep1"),), nan_weights=("deep1/kernel",)),
    _din_route("k_din_fused", "din_t50_d32", "k_din_fused", "k_din_fused", {}, None),
    _mlp_route("k_mlp_rows-widedeep", "widedeep"),
    _mlp_route("k_mlp_rows-embedding_mlp", "embedding_mlp"),
    Route("k_rows_chain", "deepfm_v2_ref", "k_rows_chain", "", {"rows_unf"}, _F32_TAIL, dict(kernel="k_rows_chain", unf=False, stage="", split=()),
          unf=True, after={k: dict(unf=False, split=()) for k in ("emb/movieId", "emb/userId", "proj/movieId/kernel")},
          row_tables=("emb/movieId", "emb/userId"), joint_tables=("emb/movieId", "emb/userId"),
          zero_col=(("emb/movieId", 9, "proj/movieId/kernel", 9),), nan_weights=("proj/movieId/kernel",)),
    _din_route("k_din_tail", "din_t5_d10", "k_din_tail", "k_din_attn_cols", {}, True),
    _dien_route("k_dien_fused", "k_dien_fused", {}, None, True),
    _din_route("k_din_attn_cols", "din_t50_d32", "k_din_tail", "k_din_attn_cols", {"SPRK_DIN_FUSED": "0"}, True),
    _dien_route("k_dien_seq_mfma", "k_din_tail", {"SPRK_DIEN_FUSED": "0"}, True, False),
    Route("neuralcf-k_rows_chain", "neuralcf", "k_rows_chain", "", (), {"SPRK_NCF_CHAIN": "0"}, dict(kernel="k_tile_forward", unf=None, stage="", split=()),
          unf=False),
)}


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """kind: "split" (cases 1 - 3: the split path stays on), "guard" (4 - 6: the site named by ``key`` falls back), "nonfinite_row",
    "nonfinite_weight".  ``clean`` = (weights, feats) of the same model without the poison, where the oracle must not move (else None)."""

    def __init__(self, name, kind, weights, feats, key=None, clean=None, guard_off=False, note=""):
        self.name, self.kind, self.weights, self.feats, self.key, self.clean, self.guard_off, self.note = name, kind, weights, feats, key, clean, guard_off, note


def _tables(w):
    return [k for k in w if k.startswith("emb/") or k.startswith("deep_emb/")]


def scale_tables(w, s):
    out = dict(w)
    for k in _tables(w):
        out[k] = (np.asarray(w[k]) * np.float32(s)).astype(np.float32)
    return out


def spread_dense(feats, lo, hi, seed=5):
    """Each sample's dense columns times 10^U(lo, hi)."""
    out = dict(feats)
    n = len(next(iter(feats.values())))
    f = (10.0 ** np.random.default_rng(seed).uniform(lo, hi, size=n)).astype(np.float32)
    for k in NUMERIC_KEYS:
        if k in out:
            out[k] = (np.asarray(out[k], np.float32) * f).astype(np.float32)
    return out


def with_row(w, key, value=None, factor=None):
    out = dict(w)
    t = np.array(w[key], np.float32)
    with np.errstate(over="ignore"):
        t[FREE_ROW] = t[FREE_ROW] * np.float32(factor) if factor is not None else np.float32(value)
    out[key] = t
    return out


def with_zero_column(w, table, d):
    out = dict(w)
    t = np.array(w[table], np.float32)
    t[:, d] = 0
    out[table] = t
    return out


def with_dead_unit(w, first, j=0):
    """Hidden unit j of layer ``first`` made dead: bias -1e6 (ReLU / PReLU with alpha 0 then give exactly 0 for every sample)."""
    out = dict(w)
    b = np.array(w[first + "/bias"], np.float32)
    b[j] = -1e6
    out[first + "/bias"] = b
    if first + "_prelu/alpha" in w:
        a = np.array(w[first + "_prelu/alpha"], np.float32)
        a[j] = 0
        out[first + "_prelu/alpha"] = a
    return out


def with_entry(w, key, row, col, factor=None, value=None):
    out = dict(w)
    k = np.array(w[key], np.float32)
    k[row, col] = k[row, col] * np.float32(factor) if factor is not None else np.float32(value)
    out[key] = k
    return out


def v2_folded(w, key):
    """What DeepFM_v2's static p_scale is taken from: the projected rows P = E Wp + bp of one big field."""
    f = key.split("/", 1)[1]
    return np.asarray(w[key], np.float32) @ np.asarray(w["proj/%s/kernel" % f], np.float32) + np.asarray(w["proj/%s/bias" % f], np.float32)


def scaled_operand(route, w):
    """The arrays the route's ONE static scale spans (for guard_trips)."""
    if route.name == "k_deepfm_v2_joint":
        return [v2_folded(w, k) for k in route.joint_tables]
    return [np.asarray(w[k]) for k in route.joint_tables]


_ORACLE = {}


def oracle(model, w, feats, dtype, tag):
    """The oracle of (model, case), computed once per process (``tag`` names the case)."""
    key = (model.name, tag, np.dtype(dtype).name)
    if key not in _ORACLE:
        _ORACLE[key] = model.oracle(feats, w, dtype)
    return _ORACLE[key]


_SCALE_UP = {}


def scale_up_factor(model):
    """The largest power of two <= 16 by which every table can grow with both input conditions still met; 1 = no up-scaled case."""
    if model.name not in _SCALE_UP:
        feats, w = model.features(), model.weights()
        _SCALE_UP[model.name] = 1
        for s in (16, 8, 4, 2):
            ws, tag = scale_tables(w, s), "scale_up-x%d" % s
            if conditions(oracle(model, ws, feats, np.float64, tag), oracle(model, ws, feats, np.float32, tag))[2]:
                _SCALE_UP[model.name] = s
                break
    return _SCALE_UP[model.name]


def outlier_bite_factor(model, key):
    """The outlier factor of the guard-off comparison: 2^36, raised 4 binades at a time (below pow2_scale's clamp 2^60) until the emulated
    unguarded split of the poisoned table moves the oracle by more than TIGHT.  -> (factor, emulated error); factor None = never bites."""
    feats, w = model.features(), model.weights()
    ref = oracle(model, w, feats, np.float64, "base")
    e = 0.0
    for p in range(36, 60, 4):
        wp = with_row(w, key, factor=2.0 ** p)
        wq = dict(wp)
        wq[key] = static_split(wp[key])
        e = float(np.abs(model.oracle(feats, wq, np.float64) - ref).max())
        if e > TIGHT:
            return 2.0 ** p, e
    return None, e


def compared_cases(route):
    """Cases 1 - 3: the split path stays on."""
    m = route.model
    w, f = m.weights(), m.features()
    out = [Case("base", "split", w, f), Case("scale_down", "split", scale_tables(w, 2.0 ** -12), f)]
    s = scale_up_factor(m)
    if s > 1:
        out.append(Case("scale_up-x%d" % s, "split", scale_tables(w, s), f))
    if m.cls is M.DIN:
        # the attention site has a range window of its own: a case outside it expects the documented fall-back of that site, and the
        # smallest tables still inside it are compared as well, so that the split attention runs on scaled-down tables too
        k = next((k for k in range(12, 0, -1) if din_attention_fits(scale_tables(w, 2.0 ** -k))), None)
        if k is not None and k < 12:
            out.append(Case("scale_down-x2^-%d" % k, "split", scale_tables(w, 2.0 ** -k), f))
        for c in out:
            if not din_attention_fits(c.weights):
                c.key, c.note = "att_range", "max |W4| s4 leaves [16, 60000): the attention tables are refused by their own range rule"
    if any(k in f for k in NUMERIC_KEYS):
        out.append(Case("numeric_spread-3..0", "split", w, spread_dense(f, -3, 0)))
        if route.name != "k_deepfm_v2_joint" and m.name != "deepfm_v2_ref":
            out.append(Case("numeric_spread-3..1", "split", w, spread_dense(f, -3, 1)))
    return out


def guard_cases(route):
    """Cases 4 - 7: one operand poisoned at a time.  ``key`` is the operand; route.expected(key) what describe() must say."""
    m = route.model
    w, f = m.weights(), m.features()
    out = []
    for key in route.row_tables:
        for fac in OUTLIER_FACTORS:
            out.append(Case("outlier_row-%s-x%.3g" % (key, fac), "guard", with_row(w, key, factor=fac), f, key=key, clean=(w, f),
                            guard_off=fac == OUTLIER_FACTORS[1]))
        for tag, val in (("nan", np.nan), ("inf", np.inf)):
            out.append(Case("nonfinite_row-%s-%s" % (key, tag), "nonfinite_row", with_row(w, key, value=val), f, key=key, clean=(w, f)))
    if route.joint_tables:
        key = route.joint_tables[-1]
        ws = dict(w)
        ws[key] = (np.asarray(w[key]) * np.float32(2.0 ** -24)).astype(np.float32)
        trips = guard_trips(scaled_operand(route, ws))
        out.append(Case("small_table-%s" % key, "guard" if trips else "split", ws, f, key=key if trips else None,
                        note="" if trips else "the scaled operand (folded rows) is not small: the guard need not act"))
    for table, d, kern, row in route.zero_col:
        wz = with_zero_column(w, table, d)
        out.append(Case("outlier_weight-%s[%d]" % (kern, row), "guard", with_entry(wz, kern, row, 1, factor=2.0 ** 26), f, key=kern, clean=(wz, f)))
    for first, second in route.dead_unit:
        wd = with_dead_unit(w, first)
        out.append(Case("outlier_weight-%s/kernel[0]" % second, "guard", with_entry(wd, second + "/kernel", 0, 1, factor=2.0 ** 26), f,
                        key=second + "/kernel", clean=(wd, f)))
    if route.name == "k_deepfm_v2_joint":
        # W0's row of a projected numeric that is 0 for every sample (its projection column and bias zeroed)
        wz = dict(w)
        pk, pb = np.array(w["proj/num/kernel"]), np.array(w["proj/num/bias"])
        pk[:, 5] = 0
        pb[5] = 0
        wz["proj/num/kernel"], wz["proj/num/bias"] = pk, pb
        row = len(F6) * 16 + 5
        out.append(Case("outlier_weight-deep0/kernel[%d]" % row, "guard", with_entry(wz, "deep0/kernel", row, 1, factor=2.0 ** 26), f,
                        key="deep0/kernel", clean=(wz, f)))
    for kern in route.nan_weights:
        row = {t[2]: t[3] for t in route.zero_col}.get(kern, 1)              # (a row of the columns the static scale is taken from)
        out.append(Case("nonfinite_weight-%s[%d]" % (kern, row), "nonfinite_weight", with_entry(w, kern, row, 1, value=np.nan), f, key=kern))
    return out


def poisoned_batches(route):
    """Case 8: -> [(label, poison name, position, feats)]: one sample's POISON_COLUMN replaced, at the tile edges of the batch."""
    f = route.model.features()
    if POISON_COLUMN not in route.model.cls.numeric_keys:
        return []
    out = []
    for name, val in POISONS:
        for pos in (0, 15, 16, B - 1):
            g = dict(f)
            col = np.array(f[POISON_COLUMN], np.float32)
            col[pos] = val
            g[POISON_COLUMN] = col
            out.append(("poisoned_sample-%s@%d" % (name, pos), name, pos, g))
    return out
