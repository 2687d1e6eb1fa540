"""ctypes binding of ``libsparrow_hip.so`` (C ABI: include/sparrow_hip.h) and its in-tree build.

The product path has NO CPU fallback: if the shared library cannot be loaded, or no HIP device
is visible when a forward is requested, the callers raise ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "libsparrow_hip.so")
SRC_PATH = os.path.join(_HERE, "csrc", "sparrow_hip.hip")
INCLUDE_DIR = os.path.join(REPO_ROOT, "include")

ABI_VERSION = 2
TILE_M = 64
MAX_SEGS, MAX_OPS, MAX_TAPS, MAX_PAIRS, MAX_BUFS = 40, 24, 8, 32, 3

OK, EINVAL, EHIP, ESTATE, ERANGE, EKIND = 0, -1, -2, -3, -4, -5

MODEL_GENERIC, MODEL_EMBEDDING_MLP, MODEL_WIDE_DEEP, MODEL_NEURALCF, MODEL_DEEPFM, MODEL_DEEPFM_V2, MODEL_DIN, MODEL_DIEN = range(8)
SEG_ROWS, SEG_SCALAR, SEG_DENSE, SEG_ZERO, SEG_CROSS_SCALAR, SEG_CROSS_ROWS, SEG_AUX = range(7)
OP_DENSE, OP_FM_SUMSQ, OP_PAIR_DOT = range(3)
ACT_NONE, ACT_RELU, ACT_PRELU = range(3)

# every symbol include/sparrow_hip.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = [
    "sprk_runtime_info", "sprk_create", "sprk_upload", "sprk_finalize", "sprk_workspace_bytes",
    "sprk_forward", "sprk_forward_many", "sprk_forward_many_opts", "sprk_forward_embedding_mlp", "sprk_forward_widedeep", "sprk_forward_neuralcf",
    "sprk_forward_deepfm", "sprk_forward_deepfm_v2", "sprk_forward_din", "sprk_forward_dien", "sprk_din_pool",
    "sprk_check_ids", "sprk_destroy", "sprk_embedding_gather", "sprk_cross_hash", "sprk_last_error",
    "sprk_pack_csv", "sprk_pack_csv_mt", "sprk_pack_csv_device", "sprk_csv_last_path",
    "sprk_pack_columns", "sprk_pack_columns_device", "sprk_pack_last_route", "sprk_set_many_streams", "sprk_set_many_batches", "sprk_emb_rank",
    "sprk_emb_topk", "sprk_emb_topk_workspace_bytes", "sprk_join_features", "sprk_rank_scores",
    "sprk_metrics_state_bytes", "sprk_metrics_reset", "sprk_metrics_update",
    "sprk_exact_auc_workspace_bytes", "sprk_exact_auc_bin_bits", "sprk_exact_auc",
    "sprk_feature_eng_workspace_bytes", "sprk_feature_eng", "sprk_store_update_workspace_bytes", "sprk_store_update", "sprk_segments_grid",
    "sprk_user_emb_workspace_bytes", "sprk_user_emb",
    "sprk_lsh_hash", "sprk_lsh_build_workspace_bytes", "sprk_lsh_build", "sprk_lsh_query",
    "sprk_split_plan_workspace_bytes", "sprk_split_plan", "sprk_take_rows",
    "sprk_rank_eval_workspace_bytes", "sprk_rank_eval",
    "sprk_catalog_build_workspace_bytes", "sprk_catalog_build", "sprk_catalog_similar",
    "sprk_als_workspace_bytes", "sprk_als_fit", "sprk_als_predict", "sprk_als_topk_workspace_bytes", "sprk_als_topk",
    "sprk_item_sequences_workspace_bytes", "sprk_item_sequences", "sprk_item_walks_workspace_bytes", "sprk_item_walks",
    "sprk_skipgram_workspace_bytes", "sprk_skipgram_fit",
    "sprk_train_workspace_bytes", "sprk_train_fit", "sprk_train_fm_workspace_bytes", "sprk_train_fm_fit", "sprk_train_din_workspace_bytes", "sprk_train_din_fit",
    "sprk_train_wide_workspace_bytes", "sprk_train_wide_fit", "sprk_train_pair_workspace_bytes", "sprk_train_pair_fit",
    "sprk_train_dien_workspace_bytes", "sprk_train_dien_fit", "sprk_train_tower_workspace_bytes", "sprk_train_tower_fit", "sprk_tower_rows",
    "sprk_describe", "sprk_comm_unique_id", "sprk_comm_create", "sprk_comm_allgather_scores", "sprk_comm_destroy",
    "sprk_peer_create", "sprk_peer_connect", "sprk_peer_allgather_scores", "sprk_peer_check", "sprk_peer_memory_kind", "sprk_peer_destroy",
    "sprk_vtable_create", "sprk_vtable_export", "sprk_vtable_import", "sprk_vtable_info", "sprk_vtable_destroy", "sprk_upload_external",
]


class CsvCol(C.Structure):
    _fields_ = [("name", C.c_char_p), ("kind", C.c_int32), ("vocab", C.c_int32)]


# storage kinds / rules of a PackCol (include/sparrow_hip.h SPRK_COL_*, SPRK_RULE_*)
COL_BOOL, COL_I8, COL_I16, COL_I32, COL_I64, COL_U8, COL_U16, COL_U32, COL_F32, COL_F64, COL_BYTES, COL_UCS4, COL_TEXT = range(13)
RULE_IDENTITY, RULE_GENRE, RULE_DENSE = range(3)
PACK_MAX_COLS = 128


class PackCol(C.Structure):
    _fields_ = [("data", C.c_void_p), ("stride", C.c_int64), ("storage", C.c_int32), ("width", C.c_int32), ("on_device", C.c_int32),
                ("rule", C.c_int32), ("vocab", C.c_int32), ("reserved", C.c_int32), ("name", C.c_char_p)]


# sources of a JoinCol (include/sparrow_hip.h SPRK_JOIN_*)
JOIN_PAIR_USER, JOIN_PAIR_MOVIE, JOIN_USER_ROW, JOIN_MOVIE_ROW = range(4)
RANK_MAX_SORT = 4096
METRICS_MAX_THRESHOLDS = 1024


class JoinCol(C.Structure):
    _fields_ = [("source", C.c_int32), ("offset", C.c_int32), ("rule", C.c_int32), ("vocab", C.c_int32)]


class ExactAucResult(C.Structure):
    """sprk_exact_auc_result (include/sparrow_hip.h): seven 8-byte words."""
    _fields_ = [("n", C.c_int64), ("n_pos", C.c_int64), ("n_groups", C.c_int64), ("roc_numerator", C.c_uint64),
                ("pr_sum", C.c_double), ("area_under_roc", C.c_double), ("area_under_pr", C.c_double)]


class SplitCol(C.Structure):
    """sprk_split_col (include/sparrow_hip.h): a column of sprk_take_rows -- source, bytes between source rows, bytes of a row, 0, destination."""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_int64), ("row_bytes", C.c_int32), ("reserved", C.c_int32), ("dst", C.c_void_p)]


TRAIN_MAX_COLS, TRAIN_MAX_LAYERS, TRAIN_MAX_X, TRAIN_MAX_WIDTH = 16, 8, 256, 256


class TrainModel(C.Structure):
    """sprk_train_model (include/sparrow_hip.h): what trainer.family_of gives, as the library takes it."""
    _fields_ = [("n_cols", C.c_int32), ("n_dense", C.c_int32), ("emb_dim", C.c_int32), ("n_x", C.c_int32), ("n_layers", C.c_int32),
                ("vocab", C.c_int32 * TRAIN_MAX_COLS), ("genre", C.c_int32 * TRAIN_MAX_COLS), ("width", C.c_int32 * TRAIN_MAX_LAYERS),
                ("xcol", C.c_int32 * TRAIN_MAX_X), ("xsub", C.c_int32 * TRAIN_MAX_X)]


TRAIN_FM_MAX_FIELDS, TRAIN_FM_MAX_LAYERS, TRAIN_FM_MAX_PROJ, TRAIN_FM_MAX_FLAT, TRAIN_FM_MAX_WIDTH, TRAIN_FM_MAX_IN = 8, 8, 128, 1024, 256, 256


class TrainFmModel(C.Structure):
    """sprk_train_fm_model (include/sparrow_hip.h): what trainer_fm.family_of gives, as the library takes it."""
    _fields_ = [("n_fields", C.c_int32), ("n_dense", C.c_int32), ("emb_dim", C.c_int32), ("proj_dim", C.c_int32), ("n_order", C.c_int32), ("n_layers", C.c_int32),
                ("vocab", C.c_int32 * TRAIN_FM_MAX_FIELDS), ("genre", C.c_int32 * TRAIN_FM_MAX_FIELDS), ("fo_off", C.c_int32 * TRAIN_FM_MAX_FIELDS),
                ("order", C.c_int32 * TRAIN_FM_MAX_FIELDS), ("width", C.c_int32 * TRAIN_FM_MAX_LAYERS)]


TRAIN_DIN_MAX_COLS, TRAIN_DIN_MAX_LAYERS, TRAIN_DIN_MAX_X, TRAIN_DIN_MAX_WIDTH, TRAIN_DIN_MAX_EMB = 16, 8, 256, 256, 64


class TrainDinModel(C.Structure):
    """sprk_train_din_model (include/sparrow_hip.h): what trainer_din.family_of gives, as the library takes it."""
    _fields_ = [("n_cols", C.c_int32), ("n_dense", C.c_int32), ("emb_dim", C.c_int32), ("hist_len", C.c_int32), ("att_hidden", C.c_int32), ("n_x", C.c_int32),
                ("n_layers", C.c_int32),
                ("vocab", C.c_int32 * TRAIN_DIN_MAX_COLS), ("genre", C.c_int32 * TRAIN_DIN_MAX_COLS), ("table", C.c_int32 * TRAIN_DIN_MAX_COLS),
                ("width", C.c_int32 * TRAIN_DIN_MAX_LAYERS), ("xsrc", C.c_int32 * TRAIN_DIN_MAX_X), ("xsub", C.c_int32 * TRAIN_DIN_MAX_X)]


class TrainDienModel(C.Structure):
    """sprk_train_dien_model (include/sparrow_hip.h): what trainer_dien.family_of gives, as the library takes it."""
    _fields_ = list(TrainDinModel._fields_)


TRAIN_WIDE_MAX_CROSS_DIM = 64


class TrainWideModel(C.Structure):
    """sprk_train_wide_model (include/sparrow_hip.h): what trainer_wide.family_of gives, as the library takes it."""
    _fields_ = TrainModel._fields_ + [("cross_a", C.c_int32), ("cross_b", C.c_int32), ("cross_buckets", C.c_int32), ("cross_dim", C.c_int32)]


TRAIN_PAIR_MAX_FIELDS, TRAIN_PAIR_MAX_PAIRS, TRAIN_PAIR_MAX_LAYERS, TRAIN_PAIR_MAX_WIDTH, TRAIN_PAIR_MAX_X, TRAIN_PAIR_MAX_DIM = 8, 32, 8, 256, 256, 64


class TrainPairModel(C.Structure):
    """sprk_train_pair_model (include/sparrow_hip.h): what trainer_pair.family_of gives, as the library takes it."""
    _fields_ = [("n_fields", C.c_int32), ("n_dense", C.c_int32), ("emb_dim", C.c_int32), ("n_pairs", C.c_int32), ("n_deep", C.c_int32), ("shared", C.c_int32),
                ("n_x", C.c_int32), ("n_layers", C.c_int32),
                ("vocab", C.c_int32 * TRAIN_PAIR_MAX_FIELDS), ("genre", C.c_int32 * TRAIN_PAIR_MAX_FIELDS), ("fo_off", C.c_int32 * TRAIN_PAIR_MAX_FIELDS),
                ("pair_a", C.c_int32 * TRAIN_PAIR_MAX_PAIRS), ("pair_b", C.c_int32 * TRAIN_PAIR_MAX_PAIRS), ("deep_col", C.c_int32 * TRAIN_PAIR_MAX_FIELDS),
                ("width", C.c_int32 * TRAIN_PAIR_MAX_LAYERS), ("xsrc", C.c_int32 * TRAIN_PAIR_MAX_X), ("xsub", C.c_int32 * TRAIN_PAIR_MAX_X)]


TRAIN_TOWER_MAX_LAYERS, TRAIN_TOWER_MAX_WIDTH, TRAIN_TOWER_MAX_DIM = 8, 256, 128


class TrainTowerModel(C.Structure):
    """sprk_train_tower_model (include/sparrow_hip.h): what trainer_tower.family_of gives, as the library takes it."""
    _fields_ = [("emb_dim", C.c_int32), ("n_layers", C.c_int32), ("vocab", C.c_int32 * 2), ("width", C.c_int32 * TRAIN_TOWER_MAX_LAYERS)]


class Seg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("slot", C.c_int32), ("field", C.c_int32), ("field2", C.c_int32),
                ("row_stride", C.c_int32), ("count", C.c_int32), ("dst", C.c_int32), ("vocab", C.c_int32)]


class Op(C.Structure):
    _fields_ = [("kind", C.c_int32), ("src_buf", C.c_int32), ("src_off", C.c_int32), ("K", C.c_int32),
                ("dst_buf", C.c_int32), ("dst_off", C.c_int32), ("N", C.c_int32), ("w_slot", C.c_int32),
                ("ldw", C.c_int32), ("b_slot", C.c_int32), ("alpha_slot", C.c_int32), ("act", C.c_int32),
                ("groups", C.c_int32), ("group_stride", C.c_int32)]


class Tap(C.Structure):
    _fields_ = [("buf", C.c_int32), ("off", C.c_int32), ("len", C.c_int32), ("w_slot", C.c_int32),
                ("scale", C.c_float), ("bias", C.c_float)]


class Din(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("T", C.c_int32), ("hist_col", C.c_int32), ("cand_col", C.c_int32),
                ("table_slot", C.c_int32), ("row_stride", C.c_int32), ("vocab", C.c_int32),
                ("hidden", C.c_int32), ("w_slot", C.c_int32), ("b_slot", C.c_int32),
                ("alpha_slot", C.c_int32), ("w2_slot", C.c_int32), ("b2", C.c_float),
                ("emb_dim", C.c_int32), ("seq_slot", C.c_int32)]


class Plan(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("model_kind", C.c_int32), ("n_id_cols", C.c_int32),
                ("n_dense", C.c_int32), ("n_aux", C.c_int32), ("n_slots", C.c_int32),
                ("n_bufs", C.c_int32), ("buf_width", C.c_int32 * MAX_BUFS),
                ("n_segs", C.c_int32), ("segs", Seg * MAX_SEGS),
                ("n_ops", C.c_int32), ("ops", Op * MAX_OPS),
                ("n_pairs", C.c_int32), ("pair_a", C.c_int32 * MAX_PAIRS), ("pair_b", C.c_int32 * MAX_PAIRS),
                ("n_taps", C.c_int32), ("taps", Tap * MAX_TAPS),
                ("head_bias", C.c_float), ("din", Din)]


_lock = threading.Lock()
_lib = None


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/sparrow_hip.hip + csrc/tu_*.hip + csrc/sparrow_metrics.hip + csrc/sparrow_feature_eng.hip + csrc/sparrow_train.hip for gfx950 into the in-tree libsparrow_hip.so
    (hipcc cross-compiles without a GPU)."""
    csrc = os.path.dirname(SRC_PATH)
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(INCLUDE_DIR, "sparrow_hip.h")]
    # [r5, ADVICE r04] the experiment defines are part of what "fresh" means: a library built once with SPRK_BUILD_DEFINES must not be
    # reused as the product after the variable is unset, nor the product when it is set.  The string the library was built with sits
    # next to it.
    defines = " ".join(os.environ.get("SPRK_BUILD_DEFINES", "").split())
    stamp = LIB_PATH + ".defines"
    def fresh():
        if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(d) for d in deps):
            return False
        try:
            built_with = open(stamp).read().strip()
        except OSError:
            built_with = ""                                       # (no stamp: a product build of an earlier tree)
        return built_with == defines
    if not force and fresh():
        return LIB_PATH
    # several processes (one rank per GPU, pytest-xdist workers) may get here at once: one builds, the others wait
    import fcntl
    with open(LIB_PATH + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and fresh():
                return LIB_PATH
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            if not os.path.exists(hipcc):
                hipcc = "hipcc"
            tmp = "%s.tmp.%d" % (LIB_PATH, os.getpid())
            # [r5] seven translation units, compiled in parallel and linked: sparrow_hip.hip (host side, light kernels) and the kernel-family
            # units tu_1.hip .. tu_6.hip (csrc/tu_kernels.h; the heavy templates' instantiations, csrc/tu_instances.h).  One unit of
            # 57-70 s until round 4.  sparrow_metrics.hip (model.evaluate's accumulators, csrc/k_metrics.h) is an eighth, independent of the engine.
            import shutil
            import tempfile
            from concurrent.futures import ThreadPoolExecutor
            units = [SRC_PATH] + sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.startswith("tu_") and f.endswith(".hip"))
            if "SPRK_SINGLE_TU" in defines:                       # one unit: sparrow_hip.hip includes every kernel header itself
                units = [SRC_PATH]
            units.append(os.path.join(csrc, "sparrow_metrics.hip"))   # the evaluation metrics: a unit of their own, no part of the engine's
            units.append(os.path.join(csrc, "sparrow_feature_eng.hip"))   # ratings -> samples and store rows (featureeng.py): likewise
            units.append(os.path.join(csrc, "sparrow_train.hip"))         # model.fit (trainer.py): likewise
            flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-fvisibility=hidden", "-fvisibility-inlines-hidden",
                     "-I", INCLUDE_DIR, "-I", csrc]               # [r6] hidden by default: include/sparrow_hip.h's declarations are the only exports
            if defines:                                           # experiment builds
                flags = defines.split() + ["-DSPRK_BUILD_DEFINES_STR=\"%s\"" % defines.replace('"', "'")] + flags
            objdir = tempfile.mkdtemp(prefix="sprk_obj_")
            try:
                def compile_unit(src):
                    obj = os.path.join(objdir, os.path.basename(src) + ".o")
                    cmd = [hipcc] + flags + ["-c", src, "-o", obj]
                    if verbose:
                        print(" ".join(cmd))
                    res = subprocess.run(cmd, capture_output=True, text=True)
                    if res.returncode != 0:
                        raise RuntimeError("hipcc failed on %s:\n%s\n%s" % (os.path.basename(src), res.stdout, res.stderr))
                    return obj
                with ThreadPoolExecutor(max_workers=min(len(units), os.cpu_count() or 1)) as pool:
                    objs = list(pool.map(compile_unit, units))
                cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-Wl,--version-script=" + os.path.join(csrc, "exports.map")] + objs + ["-o", tmp]
                if verbose:
                    print(" ".join(cmd))
                res = subprocess.run(cmd, capture_output=True, text=True)
                if res.returncode != 0:
                    raise RuntimeError("hipcc (link) failed:\n%s\n%s" % (res.stdout, res.stderr))
            finally:
                shutil.rmtree(objdir, ignore_errors=True)
            os.replace(tmp, LIB_PATH)
            with open(stamp, "w") as f:
                f.write(defines + "\n")
            return LIB_PATH
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def load_library():
    """Load libsparrow_hip.so (never builds implicitly; never falls back)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libsparrow_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; "
                               "g.build()'` or sparrowrecsys_amd._lib.build_library(); there is no CPU fallback" % LIB_PATH)
        # torch ships its own libamdhip64.so: it must be in the process BEFORE libsparrow_hip.so resolves its HIP symbols, or the
        # library binds /opt/rocm's copy, the process ends up with two HIP runtimes and device pointers made by torch are
        # unknown to ours ("no ROCm-capable device is detected" from the first call that takes one)
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        lib = C.CDLL(LIB_PATH)
        vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
        lib.sprk_last_error.restype = C.c_char_p
        lib.sprk_last_error.argtypes = []
        lib.sprk_runtime_info.argtypes = [C.POINTER(i32 * 4)]
        lib.sprk_create.argtypes = [C.POINTER(Plan), C.POINTER(vp)]
        lib.sprk_upload.argtypes = [vp, i32, vp, sz]
        lib.sprk_finalize.argtypes = [vp]
        lib.sprk_workspace_bytes.argtypes = [vp, i32]
        lib.sprk_workspace_bytes.restype = sz
        fwd = [vp, vp, vp, vp, i32, vp, sz, vp]
        for name in ("sprk_forward", "sprk_forward_embedding_mlp", "sprk_forward_widedeep", "sprk_forward_neuralcf",
                     "sprk_forward_deepfm", "sprk_forward_deepfm_v2", "sprk_forward_din", "sprk_forward_dien"):
            getattr(lib, name).argtypes = fwd
        lib.sprk_forward_many.argtypes = [vp, i32, vp, vp, vp, i32, vp, sz, vp]
        lib.sprk_forward_many_opts.argtypes = [vp, i32, vp, vp, vp, i32, vp, sz, vp, i32, i32]
        lib.sprk_din_pool.argtypes = [vp, vp, vp, vp, i32, vp]
        lib.sprk_check_ids.argtypes = [vp, vp]
        lib.sprk_destroy.argtypes = [vp]
        lib.sprk_destroy.restype = None
        lib.sprk_embedding_gather.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp]
        lib.sprk_cross_hash.argtypes = [vp, vp, i32, C.c_int64, vp, vp]
        lib.sprk_describe.argtypes = [vp, C.c_char_p, sz]
        lib.sprk_comm_unique_id.argtypes = [C.c_char_p]
        lib.sprk_comm_create.argtypes = [C.c_char_p, i32, i32, C.POINTER(vp)]
        lib.sprk_comm_allgather_scores.argtypes = [vp, vp, vp, sz, vp]
        lib.sprk_comm_destroy.argtypes = [vp]
        lib.sprk_comm_destroy.restype = None
        lib.sprk_peer_create.argtypes = [i32, i32, sz, C.c_char_p, C.POINTER(vp)]
        lib.sprk_peer_connect.argtypes = [vp, C.c_char_p]
        lib.sprk_peer_allgather_scores.argtypes = [vp, vp, sz, C.POINTER(vp), vp]
        lib.sprk_peer_check.argtypes = [vp, vp]
        lib.sprk_peer_memory_kind.argtypes = [vp]
        lib.sprk_peer_memory_kind.restype = C.c_char_p
        lib.sprk_peer_destroy.argtypes = [vp]
        lib.sprk_peer_destroy.restype = None
        lib.sprk_vtable_create.argtypes = [C.c_int64, i32, i32, i32, C.POINTER(vp)]
        lib.sprk_vtable_export.argtypes = [vp, C.POINTER(i32)]
        lib.sprk_vtable_import.argtypes = [vp, i32, i32]
        lib.sprk_vtable_info.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(i32)]
        lib.sprk_vtable_destroy.argtypes = [vp]
        lib.sprk_vtable_destroy.restype = None
        lib.sprk_upload_external.argtypes = [vp, i32, vp, sz]
        lib.sprk_set_many_streams.argtypes = [vp, i32]
        lib.sprk_set_many_batches.argtypes = [vp, i32]
        lib.sprk_pack_csv.argtypes = [C.c_char_p, sz, C.POINTER(CsvCol), i32, C.POINTER(C.c_char_p), i32, i32, vp, vp,
                                      C.POINTER(i32)]
        lib.sprk_pack_csv_mt.argtypes = [C.c_char_p, sz, C.POINTER(CsvCol), i32, C.POINTER(C.c_char_p), i32, i32, i32, vp, vp,
                                         C.POINTER(i32)]
        lib.sprk_pack_csv_device.argtypes = [vp, sz, C.POINTER(CsvCol), i32, C.POINTER(C.c_char_p), i32, i32, vp, vp, C.POINTER(i32), vp]
        lib.sprk_csv_last_path.argtypes = []
        lib.sprk_pack_columns.argtypes = [C.POINTER(PackCol), i32, C.POINTER(PackCol), i32, C.c_char_p, sz, i32, i32, vp, vp]
        lib.sprk_pack_columns_device.argtypes = [C.POINTER(PackCol), i32, C.POINTER(PackCol), i32, C.c_char_p, sz, i32, i32, vp, vp, vp]
        lib.sprk_pack_last_route.argtypes = []
        lib.sprk_emb_rank.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp, vp]
        lib.sprk_emb_topk.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]
        lib.sprk_emb_topk_workspace_bytes.argtypes = [i32, i32, i32]
        lib.sprk_emb_topk_workspace_bytes.restype = sz
        lib.sprk_join_features.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, i32, i32, i32, C.POINTER(JoinCol), i32, C.POINTER(JoinCol), i32,
                                           vp, vp, vp, vp]
        lib.sprk_rank_scores.argtypes = [vp, i32, i32, vp, vp]
        lib.sprk_metrics_state_bytes.argtypes = [i32]
        lib.sprk_metrics_state_bytes.restype = sz
        lib.sprk_metrics_reset.argtypes = [vp, sz, i32, vp]
        lib.sprk_metrics_update.argtypes = [vp, sz, vp, vp, i32, C.c_int64, C.c_int64, vp]
        lib.sprk_exact_auc_workspace_bytes.argtypes = [C.c_int64]
        lib.sprk_exact_auc_workspace_bytes.restype = sz
        lib.sprk_exact_auc_bin_bits.argtypes = [C.c_int64]
        lib.sprk_exact_auc_bin_bits.restype = i32
        lib.sprk_exact_auc.argtypes = [vp, vp, i32, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, sz, vp]   # scores, labels .. n, result, the curve, error word, workspace, stream
        lib.sprk_feature_eng_workspace_bytes.argtypes = [C.c_int64, i32, i32]
        lib.sprk_feature_eng_workspace_bytes.restype = sz
        lib.sprk_feature_eng.argtypes = [vp, vp, vp, vp, C.c_int64, i32, i32, vp, vp, vp, i32, i32,      # ratings, sizes, movie table, n_vocab, hist_len
                                         vp, vp, vp, vp, vp, vp, vp, vp, vp,                             # the sample columns
                                         vp, vp, i32, vp, vp,                                            # the store's tables (or NULL)
                                         vp, vp, vp, sz, vp]                                             # error word, sample count, workspace, stream
        lib.sprk_store_update_workspace_bytes.argtypes = [C.c_int64, i32, i32]
        lib.sprk_store_update_workspace_bytes.restype = sz
        lib.sprk_store_update.argtypes = [vp, vp, vp, vp, C.c_int64, i32, i32, vp, vp, vp, i32, i32,     # ratings, sizes, movie table, n_vocab, hist_len
                                          vp, vp, vp, vp, vp, vp, vp, vp,                                # the state: four arrays per user, four per movie
                                          vp, vp, i32, vp, vp,                                           # the store's tables
                                          vp, vp, sz, vp]                                                # error word, workspace, stream
        lib.sprk_segments_grid.argtypes = [C.c_int64]
        lib.sprk_segments_grid.restype = C.c_int64
        lib.sprk_user_emb_workspace_bytes.argtypes = [C.c_int64, i32]
        lib.sprk_user_emb_workspace_bytes.restype = sz
        lib.sprk_user_emb.argtypes = [vp, vp, C.c_int64, i32, vp, vp, i32, i32, i32,                     # ratings, sizes, item table, D, item_stride
                                      i32, vp, i32, vp, vp, vp, vp, sz, vp]                              # mode, the three outputs, error word, workspace, stream
        lib.sprk_lsh_hash.argtypes = [vp, vp, C.c_int64, i32, i32, vp, i32, C.c_double, vp, vp]          # table, has, n, D, stride, vectors, T, bucket_length, buckets, stream
        lib.sprk_lsh_build_workspace_bytes.argtypes = [C.c_int64, i32]
        lib.sprk_lsh_build_workspace_bytes.restype = sz
        lib.sprk_lsh_build.argtypes = [vp, C.c_int64, i32, vp, vp, vp, sz, vp]                         # buckets, n, T, the index, workspace, stream
        lib.sprk_lsh_query.argtypes = [vp, vp, C.c_int64, i32, i32, vp, i32, C.c_double, vp, vp, vp,     # sprk_lsh_hash's first eight, buckets, the index
                                       vp, vp, i32, i32, i32, vp, vp, vp, vp]                           # queries, query_has, Q, query_stride, K, dist, rows, count, stream
        lib.sprk_split_plan_workspace_bytes.argtypes = [C.c_int64]
        lib.sprk_split_plan_workspace_bytes.restype = sz
        lib.sprk_split_plan.argtypes = [vp, i32, vp, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, i32,   # key, key_kind, timestamp, n, seed, T(sample), T(train), train, mode
                                        vp, vp, vp, vp, sz, vp]                                                   # the two index lists, the five words, workspace, stream
        lib.sprk_take_rows.argtypes = [C.POINTER(SplitCol), i32, vp, C.c_int64, C.c_int64, vp]                    # columns, n_cols, index, n_index, n_rows, stream
        lib.sprk_rank_eval_workspace_bytes.argtypes = [C.c_int64, C.c_int64, i32, i32]
        lib.sprk_rank_eval_workspace_bytes.restype = sz
        lib.sprk_rank_eval.argtypes = [vp, i32, i32, i32, vp, vp, vp, C.c_int64, vp, vp, C.c_int64, i32,   # lists, Q, list_len, stride, query_user, truth, seen, n_users
                                       C.POINTER(i32), i32, vp, vp, vp, vp, vp, vp, vp,                    # ks (host), n_ks, gain, gain_sum, the five outputs
                                       vp, vp, sz, vp]                                                    # error word, workspace, stream
        lib.sprk_catalog_build_workspace_bytes.argtypes = [C.c_int64, i32, C.c_int64]
        lib.sprk_catalog_build_workspace_bytes.restype = sz
        lib.sprk_catalog_build.argtypes = [vp, vp, C.c_int64, i32, vp, vp, vp, vp, vp, i32,                  # ratings, sizes, movie table, n_genres
                                           vp, vp, vp, vp, C.c_int64, vp, vp, sz, vp]                       # the outputs, list_capacity, error word, workspace, stream
        lib.sprk_catalog_similar.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, C.c_int64,           # queries, movie table, n_genres, the lists
                                             i32, i32, i32, i32, i32, vp, vp, i32, vp, vp]                  # mode, top_n, extra_n, score_kind, size, the outputs, stream
        lib.sprk_als_workspace_bytes.argtypes = [C.c_int64, i32, i32, i32]
        lib.sprk_als_workspace_bytes.restype = sz
        lib.sprk_als_fit.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, C.c_double, i32,                  # ratings, sizes, rank, reg, iters
                                     vp, i32, vp, i32, vp, i32, vp, vp, vp, vp,                              # init_user, the factor tables, has, counts
                                     vp, vp, sz, vp]                                                         # error word, workspace, stream
        lib.sprk_als_predict.argtypes = [vp, vp, C.c_int64, vp, i32, vp, vp, i32, vp, i32, i32, i32, vp, vp]
        lib.sprk_als_topk_workspace_bytes.argtypes = [i32, i32, i32]
        lib.sprk_als_topk_workspace_bytes.restype = sz
        lib.sprk_als_topk.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, sz, vp]
        lib.sprk_item_sequences_workspace_bytes.argtypes = [C.c_int64, i32, i32]
        lib.sprk_item_sequences_workspace_bytes.restype = sz
        lib.sprk_item_sequences.argtypes = [vp, vp, vp, vp, C.c_int64, i32, i32, vp, vp, vp, vp, vp, sz, vp]
        lib.sprk_item_walks_workspace_bytes.argtypes = [C.c_int64, i32, i32, C.c_int64, i32]
        lib.sprk_item_walks_workspace_bytes.restype = sz
        lib.sprk_item_walks.argtypes = [vp, vp, C.c_int64, i32, i32, C.c_int64, i32, C.c_uint64, vp, vp, vp, vp, sz, vp]
        lib.sprk_skipgram_workspace_bytes.argtypes = [C.c_int64, i32, i32, C.c_int64, i32, i32, i32]
        lib.sprk_skipgram_workspace_bytes.restype = sz
        lib.sprk_skipgram_fit.argtypes = [vp, vp, C.c_int64, i32, vp, i32, i32, C.c_int64, vp, vp, vp,          # sequences, the vocabulary's tables
                                          vp, i32, vp, vp, i32, i32, i32, C.c_double, i32, i32, C.c_uint64, i32,  # init, the two tables, D .. max_sentence
                                          vp, i32, vp, vp, vp, vp, sz, vp]                                       # vectors, syn1, loss, error word, workspace, stream
        lib.sprk_train_workspace_bytes.argtypes = [C.POINTER(TrainModel), C.c_int64, i32, i32]
        lib.sprk_train_workspace_bytes.restype = sz
        lib.sprk_train_fit.argtypes = [C.POINTER(TrainModel), vp, vp, vp, vp, C.c_int64, i32, i32, i32, vp, C.c_float, C.c_float, C.c_float,   # model .. epsilon
                                       vp, vp, vp, vp, vp, vp, sz, vp]                              # params, m, v, p, error word, workspace, stream
        lib.sprk_train_fm_workspace_bytes.argtypes = [C.POINTER(TrainFmModel), C.c_int64, i32, i32]
        lib.sprk_train_fm_workspace_bytes.restype = sz
        lib.sprk_train_fm_fit.argtypes = [C.POINTER(TrainFmModel)] + lib.sprk_train_fit.argtypes[1:]             # sprk_train_fit's argument list
        lib.sprk_train_din_workspace_bytes.argtypes = [C.POINTER(TrainDinModel), C.c_int64, i32, i32]
        lib.sprk_train_din_workspace_bytes.restype = sz
        lib.sprk_train_din_fit.argtypes = [C.POINTER(TrainDinModel)] + lib.sprk_train_fit.argtypes[1:]           # sprk_train_fit's argument list
        lib.sprk_train_dien_workspace_bytes.argtypes = [C.POINTER(TrainDienModel), C.c_int64, i32, i32]
        lib.sprk_train_dien_workspace_bytes.restype = sz
        lib.sprk_train_dien_fit.argtypes = [C.POINTER(TrainDienModel)] + lib.sprk_train_fit.argtypes[1:]         # sprk_train_fit's argument list
        lib.sprk_train_wide_workspace_bytes.argtypes = [C.POINTER(TrainWideModel), C.c_int64, i32, i32]
        lib.sprk_train_wide_workspace_bytes.restype = sz
        lib.sprk_train_wide_fit.argtypes = [C.POINTER(TrainWideModel)] + lib.sprk_train_fit.argtypes[1:]         # sprk_train_fit's argument list
        lib.sprk_train_pair_workspace_bytes.argtypes = [C.POINTER(TrainPairModel), C.c_int64, i32, i32]
        lib.sprk_train_pair_workspace_bytes.restype = sz
        lib.sprk_train_pair_fit.argtypes = [C.POINTER(TrainPairModel)] + lib.sprk_train_fit.argtypes[1:]         # sprk_train_fit's argument list
        lib.sprk_train_tower_workspace_bytes.argtypes = [C.POINTER(TrainTowerModel), C.c_int64, i32, i32]
        lib.sprk_train_tower_workspace_bytes.restype = sz
        a = lib.sprk_train_fit.argtypes
        lib.sprk_train_tower_fit.argtypes = [C.POINTER(TrainTowerModel), a[1]] + a[3:]                          # sprk_train_fit's argument list less `dense`
        lib.sprk_tower_rows.argtypes = [C.POINTER(TrainTowerModel), vp, i32, i32, vp, C.c_int64, vp]
        for name in EXPORTED_SYMBOLS:
            if name not in ("sprk_train_tower_workspace_bytes", "sprk_train_din_workspace_bytes", "sprk_train_dien_workspace_bytes", "sprk_train_wide_workspace_bytes", "sprk_train_pair_workspace_bytes","sprk_segments_grid", "sprk_rank_eval_workspace_bytes", "sprk_exact_auc_workspace_bytes", "sprk_exact_auc_bin_bits", "sprk_lsh_build_workspace_bytes", "sprk_train_fm_workspace_bytes","sprk_train_workspace_bytes", "sprk_item_sequences_workspace_bytes", "sprk_item_walks_workspace_bytes", "sprk_skipgram_workspace_bytes", "sprk_als_workspace_bytes", "sprk_als_topk_workspace_bytes", "sprk_catalog_build_workspace_bytes", "sprk_last_error", "sprk_destroy", "sprk_workspace_bytes", "sprk_emb_topk_workspace_bytes", "sprk_metrics_state_bytes", "sprk_feature_eng_workspace_bytes", "sprk_user_emb_workspace_bytes", "sprk_comm_destroy", "sprk_peer_destroy", "sprk_peer_memory_kind", "sprk_vtable_destroy"):
                getattr(lib, name).restype = C.c_int
        _lib = lib
        return lib


class SparrowHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libsparrow_hip error %d: %s" % (code, message))
        self.code = code


def check(rc: int):
    if rc != OK:
        msg = load_library().sprk_last_error().decode("utf-8", "replace")
        if rc == ERANGE:
            raise ValueError(msg)
        raise SparrowHipError(rc, msg)


def runtime_info():
    lib = load_library()
    info = (C.c_int32 * 4)()
    check(lib.sprk_runtime_info(C.byref(info)))
    return {"abi_version": info[0], "device_count": info[1], "compute_units": info[2], "is_gfx950": bool(info[3])}
