/*
 * sparrow_hip.h -- C ABI of libsparrow_hip.so: the MI355X (gfx950) CTR-ranking forward pass
 * for SparrowRecSys's TFRecModel models.
 *
 * The reference has NO native/FFI interface for this path: every model is a stand-alone Keras
 * script and the boundary a maintainer sees is `model.predict(x)` (reference
 * TFRecModel/src/com/sparrowrecsys/offline/tensorflow/DeepFM.py:131, DIN.py:185,
 * NeuralCF.py:91) and the TF-Serving REST call of the Jetty server
 * (src/main/java/com/sparrowrecsys/online/recprocess/RecForYouProcess.java:113-138).
 * This header is therefore the NEW seam those two call into: each entry
 * point below names the reference construct it replaces.  The Python host
 * (sparrowrecsys_amd/_lib.py) binds it with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative
 * SPRK_E* code and never throws; sprk_last_error() returns a thread-local message.
 * `ids`, `dense`, `aux`, `out`, `workspace` are DEVICE pointers owned by the caller (torch
 * tensors in the Python host); the library owns only the tables/weights it was given through
 * sprk_upload().  A finalized handle is immutable: sprk_forward*() may run concurrently on
 * distinct streams; sprk_upload()/sprk_finalize() must not race with them.
 */
#ifndef SPARROW_HIP_H
#define SPARROW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* [r6] The library is built with -fvisibility=hidden: the entry points declared between this push and its pop are its WHOLE dynamic symbol table
 * (tests/test_cabi.py compares `nm -D` with this header). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define SPRK_ABI_VERSION 2

#define SPRK_OK 0
#define SPRK_EINVAL (-1)    /* bad argument / malformed plan            */
#define SPRK_EHIP (-2)      /* a HIP runtime call failed                */
#define SPRK_ESTATE (-3)    /* wrong call order (e.g. forward before finalize) */
#define SPRK_ERANGE (-4)    /* an id was outside its table (see sprk_check_ids) */
#define SPRK_EKIND (-5)     /* forward_<model> called on a handle of another model */

#define SPRK_TILE_M 64      /* samples per workgroup tile                */
#define SPRK_MAX_SEGS 40
#define SPRK_MAX_OPS 24
#define SPRK_MAX_TAPS 8
#define SPRK_MAX_PAIRS 32
#define SPRK_MAX_BUFS 3

/* model_kind: which reference script the plan restates (checked by sprk_forward_<model>) */
enum sprk_model_kind {
    SPRK_MODEL_GENERIC = 0,
    SPRK_MODEL_EMBEDDING_MLP = 1, /* EmbeddingMLP.py:72-77  */
    SPRK_MODEL_WIDE_DEEP = 2,     /* WideNDeep.py:99-108    */
    SPRK_MODEL_NEURALCF = 3,      /* NeuralCF.py:45-70      */
    SPRK_MODEL_DEEPFM = 4,        /* DeepFM.py:91-115       */
    SPRK_MODEL_DEEPFM_V2 = 5,     /* DeepFM_v2.py:98-157    */
    SPRK_MODEL_DIN = 6,           /* DIN.py:125-169         */
    SPRK_MODEL_DIEN = 7           /* DIEN.py:114-259 (y_pred) */
};

/* Gather segments: how one sample's row of activation buffer 0 is assembled.  Together they
 * replace tf.keras.layers.DenseFeatures + tf.feature_column.{embedding,indicator,numeric,
 * crossed}_column (DeepFM.py:54-97, WideNDeep.py:72-73). */
enum sprk_seg_kind {
    SPRK_SEG_ROWS = 0,         /* embedding_column: copy table[id] (nvec float4); id<0 -> zeros */
    SPRK_SEG_SCALAR = 1,       /* indicator_column x Dense(1): one weight table[id]; id<0 -> 0   */
    SPRK_SEG_DENSE = 2,        /* numeric_column(s): copy `count` floats of the dense row       */
    SPRK_SEG_ZERO = 3,         /* zero-fill `count` floats (K padding)                           */
    SPRK_SEG_CROSS_SCALAR = 4, /* indicator(crossed_column) x Dense(1): table[hash(a,b) % vocab] */
    SPRK_SEG_CROSS_ROWS = 5,   /* embedding_column(crossed_column): row table[hash(a,b) % vocab] */
    SPRK_SEG_AUX = 6           /* copy `count` floats of the aux row (DIN pooled history)        */
};

typedef struct sprk_seg {
    int32_t kind;
    int32_t slot;       /* weight slot holding the table (ROWS/SCALAR/CROSS_*)            */
    int32_t field;      /* ids column | first dense column | first aux column             */
    int32_t field2;     /* second ids column (CROSS_*)                                    */
    int32_t row_stride; /* floats per table row (multiple of 4 for ROWS)                  */
    int32_t count;      /* ROWS/CROSS_ROWS: float4 per row; DENSE/ZERO/AUX: floats        */
    int32_t dst;        /* destination float offset inside buffer 0 (multiple of 4 for ROWS) */
    int32_t vocab;      /* table rows (bounds check) | number of hash buckets             */
} sprk_seg;

enum sprk_op_kind {
    SPRK_OP_DENSE = 0,    /* tf.keras.layers.Dense: dst = act(src @ W + b) on fp32 MFMA        */
    SPRK_OP_FM_SUMSQ = 1, /* DeepFM_v2.py:147-152: (sum_g v_g)^2 - sum_g v_g^2 over `groups`    */
    SPRK_OP_PAIR_DOT = 2  /* tf.keras.layers.Dot(axes=1) for the plan's pair list (DeepFM.py:100-103) */
};
enum sprk_act { SPRK_ACT_NONE = 0, SPRK_ACT_RELU = 1, SPRK_ACT_PRELU = 2 };

typedef struct sprk_op {
    int32_t kind;
    int32_t src_buf, src_off;
    int32_t K;           /* DENSE: input width (multiple of 4); FM_SUMSQ: width per group; PAIR_DOT: vector length */
    int32_t dst_buf, dst_off;
    int32_t N;           /* DENSE: output width (multiple of 16)                           */
    int32_t w_slot;      /* DENSE: W transposed+padded, [N][ldw] floats                    */
    int32_t ldw;         /* DENSE: floats per W^T row (multiple of 4, >= K)                */
    int32_t b_slot;      /* DENSE: bias [N]                                                */
    int32_t alpha_slot;  /* DENSE+PRELU: alpha [N]                                         */
    int32_t act;
    int32_t groups;      /* FM_SUMSQ: number of fields                                     */
    int32_t group_stride;/* FM_SUMSQ: floats between consecutive fields                    */
} sprk_op;

/* Output layer: z = head_bias + sum_t scale_t * (bias_t + sum_j w_t[j] * buf_t[off_t + j]);
 * score = sigmoid(z).  Replaces the final concatenate + Dense(1, sigmoid)
 * (DeepFM.py:111-113, DeepFM_v2.py:154-155, DIN.py:167, ...). */
typedef struct sprk_tap {
    int32_t buf, off, len;
    int32_t w_slot;      /* weights [len]; -1 -> all ones                                  */
    float scale;
    float bias;
} sprk_tap;

/* DIN activation unit + weighted sum pooling (DIN.py:132-158), run by its own kernel before
 * the tile kernel; its [B, out_cols] result is what SPRK_SEG_AUX segments read. */
typedef struct sprk_din {
    int32_t enabled;
    int32_t T;           /* history length                                                 */
    int32_t hist_col;    /* first of T consecutive ids columns                             */
    int32_t cand_col;    /* candidate movieId ids column                                   */
    int32_t table_slot;  /* shared movie Embedding table                                   */
    int32_t row_stride;  /* floats per row (= Dp, multiple of 4)                           */
    int32_t vocab;
    int32_t hidden;      /* attention hidden width (multiple of 16; reference 32)          */
    int32_t w_slot;      /* att0 kernel transposed [hidden][4*Dp] in [h-c | h | c | h*c] blocks */
    int32_t b_slot;      /* att0 bias [hidden]                                             */
    int32_t alpha_slot;  /* PReLU alpha [T][hidden]                                        */
    int32_t w2_slot;     /* att1 kernel [hidden]                                           */
    float b2;            /* att1 bias                                                      */
    /* enabled == 2: DIEN's interest-evolution stage instead (DIEN.py:163-250: Embedding mask -> GRU -> attention gate ->
     * AUGRU; its final state [B, row_stride] is what SPRK_SEG_AUX reads).  Uses T, hist_col, cand_col, table_slot,
     * row_stride, vocab, hidden (= 32) and the two fields below; w_slot .. b2 are ignored. */
    int32_t emb_dim;     /* D: Embedding / GRU / AUGRU width (10 or 16)                    */
    int32_t seq_slot;    /* packed weights, strides padded to 4 floats (Dq = pad4(D), N3 = pad4(3D)):
                          *   GRU kernel [D][N3] | recurrent kernel [D][N3] | bias [2][N3]  (z | r | h columns, reset_after)
                          *   | attention Dense(32) kernel [D][32] | bias [32] | Dense(1) kernel [32] | bias [4]
                          *   | for gate in (R_t, Z_t, H_t_next): input_w kernel [D][Dq] | bias [Dq] | hidden_w kernel [D][Dq]
                          *     | Dense_sigmoid / Dense_tanh kernel [D][Dq] | bias [Dq]
                          *   | AUGRU initial state h0 [Dq]; the whole image zero-padded to a multiple of 64 floats */
} sprk_din;

typedef struct sprk_plan {
    int32_t abi_version;               /* SPRK_ABI_VERSION */
    int32_t model_kind;
    int32_t n_id_cols;                 /* F: int32 columns per ids row   */
    int32_t n_dense;                   /* N: floats per dense row        */
    int32_t n_aux;                     /* floats per aux row (0 if none) */
    int32_t n_slots;                   /* weight slots used              */
    int32_t n_bufs;
    int32_t buf_width[SPRK_MAX_BUFS];  /* floats per sample in each LDS activation buffer */
    int32_t n_segs;
    sprk_seg segs[SPRK_MAX_SEGS];
    int32_t n_ops;
    sprk_op ops[SPRK_MAX_OPS];
    int32_t n_pairs;                   /* pair list of the PAIR_DOT op (offsets in src buffer) */
    int32_t pair_a[SPRK_MAX_PAIRS];
    int32_t pair_b[SPRK_MAX_PAIRS];
    int32_t n_taps;
    sprk_tap taps[SPRK_MAX_TAPS];
    float head_bias;
    sprk_din din;
} sprk_plan;

typedef struct sprk_engine* sprk_handle;

/* Library / device facts.  info[0]=ABI version, [1]=HIP device count (0 when no GPU is
 * visible; never an error), [2]=compute units of the current device, [3]=1 if it is gfx950. */
int sprk_runtime_info(int32_t info[4]);

/* Replaces building the Keras graph (`tf.keras.Model(inputs, output_layer)`, DeepFM.py:115):
 * validates and copies `plan`. */
int sprk_create(const sprk_plan* plan, sprk_handle* out);

/* Replaces Keras weight loading (`model.set_weights` / SavedModel restore, NeuralCF.py:97-105):
 * copies `bytes` from `src` (host OR device pointer) into library-owned device memory for
 * weight slot `slot`.  Layouts are the device layouts documented in DESIGN.md (tables padded
 * to a multiple of 4 floats per row, Dense kernels transposed). */
int sprk_upload(sprk_handle h, int32_t slot, const void* src, size_t bytes);

/* Resolves slots to device pointers; must follow the last sprk_upload. */
int sprk_finalize(sprk_handle h);

/* Bytes of caller-provided device scratch sprk_forward needs for a batch of B (0 for models
 * without a DIN stage). */
size_t sprk_workspace_bytes(sprk_handle h, int32_t B);

/* Replaces `model.predict(x)` for one device-resident batch (DeepFM.py:131):
 *   ids   [B, n_id_cols] int32 row-major, -1 = missing / out-of-vocabulary (-> zero row)
 *   dense [B, n_dense]   float32 row-major
 *   out   [B]            float32 sigmoid scores
 * Asynchronous on `stream` (a hipStream_t; NULL = default stream). */
int sprk_forward(sprk_handle h, const int32_t* ids, const float* dense, float* out, int32_t B,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Replaces `model.predict(dataset)` looping over the dataset's batches (DeepFM.py:131 over the
 * tf.data pipeline of DeepFM.py:14-22): enqueues n_batches forwards of B rows each on `stream`,
 * batch i reading ids[i] / dense[i] and writing out[i] (arrays of DEVICE pointers held in HOST
 * memory).  Exactly equivalent to n_batches calls of sprk_forward; it exists so that a serving or
 * evaluation loop pays one foreign-function call per pass instead of one per batch. */
int sprk_forward_many(sprk_handle h, int32_t n_batches, const int32_t* const* ids, const float* const* dense,
                      float* const* out, int32_t B, void* workspace, size_t workspace_bytes, void* stream);

/* How sprk_forward_many enqueues its batches.  n = 0 (default): all on `stream`, strictly one after the other -- on this
 * stack even an empty kernel costs ~3.3 us per launch in such a dependent chain.  n = 2..4: independent batches alternate
 * over n library-owned helper streams forked from `stream` and joined back into it, so that one kernel's dispatch / drain
 * overlaps its neighbours' execution (config 2: 8.9 -> 6.8 us per 65 536-row batch).  Results are identical; completion is
 * still ordered on `stream`.  Models with a workspace (DIN) fan out only when `workspace_bytes` holds one 256-byte-aligned
 * slice of sprk_workspace_bytes(B) per stream. */
int sprk_set_many_streams(sprk_handle h, int32_t n);

/* How many of sprk_forward_many's batches ONE kernel launch scores (1 = a launch per batch, the default; up to 64).  Each
 * batch keeps its own ids / dense / out buffers of B rows; the launch walks the tasks of all of them, so the fixed cost of
 * a launch is spent once per n batches.  Bit-identical results.  Honoured, with 16-byte aligned buffers, by the fused DeepFM_v2
 * and embedding-rows kernels (up to 64 per launch) and by the pair-dot DeepFM, EmbeddingMLP / Wide&Deep and DIN kernels (up to
 * 16); every other case silently goes batch by batch (and takes sprk_set_many_streams into account). */
int sprk_set_many_batches(sprk_handle h, int32_t n);

/* sprk_forward_many with both knobs as ARGUMENTS of the call: `batches_per_launch` (1..64) and `helper_streams` (0, 2..4) mean
 * what sprk_set_many_batches / sprk_set_many_streams set, but nothing is stored in the handle -- a finalized handle stays
 * immutable, so threads sharing one can each use their own settings (round 2's setters changed state under a handle the
 * header called immutable; they remain as the DEFAULTS sprk_forward_many uses and must not be called while another thread is
 * inside a forward).  With helper_streams >= 2 the call uses the handle's helper streams and fork / join events: that form is
 * not re-entrant on one handle; helper_streams = 0 is.  What `model.predict(dataset)` (DeepFM.py:131) replays per batch. */
int sprk_forward_many_opts(sprk_handle h, int32_t n_batches, const int32_t* const* ids, const float* const* dense,
                           float* const* out, int32_t B, void* workspace, size_t workspace_bytes, void* stream,
                           int32_t batches_per_launch, int32_t helper_streams);

/* Per-model entry points: identical to sprk_forward but fail with
 * SPRK_EKIND unless the handle was created from that model's plan. */
int sprk_forward_embedding_mlp(sprk_handle h, const int32_t* ids, const float* dense, float* out, int32_t B, void* ws, size_t ws_bytes, void* stream);
int sprk_forward_widedeep(sprk_handle h, const int32_t* ids, const float* dense, float* out, int32_t B, void* ws, size_t ws_bytes, void* stream);
int sprk_forward_neuralcf(sprk_handle h, const int32_t* ids, const float* dense, float* out, int32_t B, void* ws, size_t ws_bytes, void* stream);
int sprk_forward_deepfm(sprk_handle h, const int32_t* ids, const float* dense, float* out, int32_t B, void* ws, size_t ws_bytes, void* stream);
int sprk_forward_deepfm_v2(sprk_handle h, const int32_t* ids, const float* dense, float* out, int32_t B, void* ws, size_t ws_bytes, void* stream);
int sprk_forward_din(sprk_handle h, const int32_t* ids, const float* dense, float* out, int32_t B, void* ws, size_t ws_bytes, void* stream);
int sprk_forward_dien(sprk_handle h, const int32_t* ids, const float* dense, float* out, int32_t B, void* ws, size_t ws_bytes, void* stream);

/* DIN stage alone (DIN.py:132-158): pooled [B, row_stride] and, if att != NULL, the attention
 * weights att [B, T].  For a DIEN handle: the final AUGRU state [B, row_stride]; att must be NULL. */
int sprk_din_pool(sprk_handle h, const int32_t* ids, float* pooled, float* att, int32_t B, void* stream);

/* Replaces TF's assert_greater_or_equal_0 / assert_less_than_num_buckets
 * (categorical_column_with_identity, DeepFM.py:54,59): synchronises `stream` and returns
 * SPRK_ERANGE if any forward since the last call saw an id >= its table size or < -1. */
int sprk_check_ids(sprk_handle h, void* stream);

/* Which kernels a finalized handle dispatches to (no reference counterpart; Keras would answer `model.summary()`).  Writes a
 * NUL-terminated "key=value;..." line into buf: kernel = the fused kernel instantiation that scores a batch, or k_tile_forward
 * when no fused kernel matched the plan and the generic plan interpreter runs it (fused=0: several times slower -- a shape that
 * silently fell off the fast path is visible here); stage = the history stage of DIN / DIEN handles (k_din_attn, k_din_pool,
 * k_dien_seq) or empty; uploaded_bytes / derived_bytes = device memory of the uploaded slots and of the tables derived from them
 * at finalize (folded rows, split halfs, per-id terms); first_dense_fold = embedding columns folded into the first Dense layer;
 * split_f16 = the sites of that route and stage whose operand runs as hi + lo f16 halves under a STATIC power-of-two scale chosen
 * at finalize, comma separated (v2, pairs_e, rows_unf, tail_unf, dyn_w1, dyn_w0, dyn_w0p, din_attn, dien_seq) --
 * a site that a range guard, a non-finite weight or a switch refused is absent and runs f32; empty = everything f32.
 * SPRK_EINVAL when the buffer is too small (512 bytes always suffice). */
int sprk_describe(sprk_handle h, char* buf, size_t buf_bytes);

void sprk_destroy(sprk_handle h);

/* ---- stand-alone operators (same kernels' building blocks, for parity tests / reuse) ---- */

/* tf.keras.layers.Embedding / embedding_column row gather (DIN.py:132-136, DeepFM.py:55):
 * out[b, 0:D] = table[ids[b], 0:D]; ids[b] < 0 -> zeros.  table is [V, row_stride] floats,
 * out is [B, D] floats; D and row_stride multiples of 4.  Bit-exact copy. */
int sprk_embedding_gather(const float* table, int32_t V, int32_t D, int32_t row_stride,
                          const int32_t* ids, int32_t B, float* out, void* stream);

/* tf.feature_column.crossed_column([a, b], num_buckets) hashing (WideNDeep.py:72-73):
 * out[b] = FingerprintCat64(FingerprintCat64(0xDECAFCAFFE, a[b]), b[b]) mod num_buckets. */
int sprk_cross_hash(const int32_t* a, const int32_t* b, int32_t B, int64_t num_buckets,
                    int64_t* out, void* stream);

/* The reference's "emb" ranker: RecForYouProcess.java:69-92 (ranker, case "emb") with
 * calculateEmbSimilarScore :100-105, SimilarMovieProcess.java:121-136,167-172, Embedding.calculateSimilarity
 * (Embedding.java:33-47).  For query u (a user's embedding, or a movie's) and its C candidate movies
 *   scores[u][c] = dot / (sqrt(n1) * sqrt(n2)), float products summed into doubles in index order exactly as the Java
 *                  loop does (bit-exact doubles; an all-zero vector gives NaN as in Java);
 *                  -1.0 if the query has no embedding (query_has[u] == 0), cand[u][c] is outside [0, n_items) (a Movie
 *                  unknown to the table) or that item has none (item_has[id] == 0) -- Embedding.java:34-37.
 *   order[u][0..C) (optional, C <= 4096): candidate POSITIONS in the order of
 *                  `sorted(Map.Entry.comparingByValue(Comparator.reverseOrder()))`: descending in Double.compareTo
 *                  order (NaN first, 0.0 before -0.0); equal scores stay in candidate order (Java: unspecified).
 * All pointers are device memory; item_emb [n_items][item_stride], query_emb [n_queries][query_stride] floats (first D
 * used), cand [n_queries][C]; item_has / query_has may be NULL (= all present). */
int sprk_emb_rank(const float* item_emb, const uint8_t* item_has, int32_t n_items, int32_t D, int32_t item_stride,
                  const float* query_emb, const uint8_t* query_has, int32_t n_queries, int32_t query_stride,
                  const int32_t* cand, int32_t C, double* scores, int32_t* order, void* stream);

/* Embedding RECALL, exact, over the whole table: SimilarMovieProcess.retrievalCandidatesByEmbedding (SimilarMovieProcess.java:91-112) --
 * score EVERY movie against the query embedding (calculateEmbSimilarScore :167-172, Embedding.java:33-47), sort, keep `size`.
 * For every query u the result is exactly what sprk_emb_rank gives for cand[u] = 0, 1, .., n_items-1, cut to the first K:
 *   items[u][k]  = the table row of the k-th entry;
 *   scores[u][k] = its score, the same doubles bit for bit (-1.0 for a row with item_has == 0 or a query with query_has == 0, NaN for an
 *                  all-zero vector).
 * largest = 1: descending Double.compareTo order (NaN first, 0.0 before -0.0), equal scores by ascending row -- the ranker's order
 *              (`comparingByValue(Comparator.reverseOrder())`, SimilarMovieProcess.java:135), i.e. the K MOST similar rows.
 * largest = 0: ascending Double.compareTo order, equal scores again by ascending row.  This is what the Java literally does:
 *              retrievalCandidatesByEmbedding sorts with `Map.Entry.comparingByValue()` and NO reverseOrder (:104), so the reference
 *              returns the `size` LEAST similar movies.
 * (score, row) is a total order: the answer is unique and does not depend on how the table is chunked or merged.  A query without an
 * embedding gets rows 0 .. K-1 with score -1.0 in both directions.
 * Limits: 1 <= K <= 1024 and K <= n_items; 1 <= D <= 1024, strides >= D; largest 0 or 1; item_emb, query_emb, scores, items not NULL;
 * `workspace` (device memory, 8-byte aligned) of at least the bytes the workspace function below names for (n_items, n_queries, K), which
 * is 0 -- and the pointer may be NULL -- when the table fits one chunk of 4096 rows.  Anything else returns SPRK_EINVAL BEFORE any device
 * call (the message names the bytes needed).  n_queries == 0 does nothing.  Asynchronous on `stream`: no host synchronisation, no memory
 * owned by the library; all index arithmetic in 64 bits.  All pointers are device memory, laid out as for sprk_emb_rank; scores and items
 * are [n_queries][K].  SPRK_EMB_TOPK_CHUNK = a power of two in [64, 4096] shortens the chunk (tests), for both functions. */
size_t sprk_emb_topk_workspace_bytes(int32_t n_items, int32_t n_queries, int32_t K);
int sprk_emb_topk(const float* item_emb, const uint8_t* item_has, int32_t n_items, int32_t D, int32_t item_stride,
                  const float* query_emb, const uint8_t* query_has, int32_t n_queries, int32_t query_stride,
                  int32_t K, int32_t largest,
                  double* scores /* [n_queries][K] */, int32_t* items /* [n_queries][K] */,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- host ingest (no GPU involved): the step before the path ----
 * Replaces `tf.data.experimental.make_csv_dataset(..., na_value="0", ignore_errors=True)` of the reference's
 * get_dataset (DeepFM.py:14-22) plus the feature-column id resolution (DeepFM.py:54-76) for a CSV text held in
 * memory: header line + rows -> the two packed arrays sprk_forward reads.  Identity columns: empty -> 0, values
 * outside [0, vocab) -> SPRK_ERANGE (TF: assert_less_than_num_buckets); genre columns: position in the 19-entry
 * vocabulary of DeepFM.py:64-66, anything else (empty, unknown) -> -1; dense columns: empty -> 0.0.  Rows whose
 * field count differs from the header's are skipped (ignore_errors).  `ids_out` is [max_rows, n_id] int32,
 * `dense_out` [max_rows, n_dense] float32 (HOST memory); *rows_out receives the number of rows packed. */
typedef struct sprk_csv_col {
    const char* name;    /* CSV header name (reference schema key)                  */
    int32_t kind;        /* 0 = categorical_column_with_identity, 1 = genre vocabulary */
    int32_t vocab;       /* buckets / vocabulary size                                */
} sprk_csv_col;
int sprk_pack_csv(const char* text, size_t len, const sprk_csv_col* id_cols, int32_t n_id,
                  const char* const* dense_names, int32_t n_dense, int32_t max_rows,
                  int32_t* ids_out, float* dense_out, int32_t* rows_out);
/* The same on n_threads host threads (clamped to [1, 256]; the body is cut at line boundaries, chunks are parsed
 * concurrently and stitched in file order): identical outputs, identical first error, for any thread count. */
int sprk_pack_csv_mt(const char* text, size_t len, const sprk_csv_col* id_cols, int32_t n_id,
                     const char* const* dense_names, int32_t n_dense, int32_t max_rows, int32_t n_threads,
                     int32_t* ids_out, float* dense_out, int32_t* rows_out);
/* The same packing ON THE DEVICE ("GPU-side tokenizer"): `text_dev` is the CSV text in device
 * memory (16-byte aligned; e.g. the file read straight into a pinned buffer and copied once), `ids_dev` / `dense_dev` are
 * DEVICE arrays [max_rows, n_id] / [max_rows, n_dense].  Same rules and the same bits as sprk_pack_csv for every field that is
 * empty or a plain decimal of at most 15 significant digits with a decimal exponent within +-22 (strtod's exact fast path) --
 * every value the reference's sample files hold (quoted fields are split as the host tokenizer splits them; the files spell
 * an empty string "").  It never guesses: a numeric field outside that shape ("inf", hex, blanks, 16+ digits, text, an escaped
 * quote) fails with SPRK_EKIND and names the first such row; ids outside
 * their bucket range fail with SPRK_ERANGE like the host tokenizer (first bad row in file order).  Synchronises `stream`
 * (the row count comes back to the host).  Device scratch (8 bytes per line + 4 per 4-KB chunk of text) is allocated on first
 * use, grows to the largest text seen and is kept for the calling thread's lifetime. */
int sprk_pack_csv_device(const char* text_dev, size_t len, const sprk_csv_col* id_cols, int32_t n_id,
                         const char* const* dense_names, int32_t n_dense, int32_t max_rows,
                         int32_t* ids_dev, float* dense_dev, int32_t* rows_out, void* stream);
/* Which kernels the calling thread's last sprk_pack_csv_device ran the text through (diagnostics / tests): 1 = the optimistic
 * pass alone (every line of the text is a row: line i is output row i - 1), 2 = the exact keep -> scan -> parse sequence (some
 * line is empty or has another field count than the header: ignore_errors=True drops it), -1 = no call yet / no data line / the
 * call failed early.  The packed arrays are the same bits whichever ran. */
int sprk_csv_last_path(void);

/* ---- column ingest: a dict of feature columns -> the two packed arrays (what `model.predict(features_dict)` runs first) ----
 * Replaces the feature-column resolution of the reference's Keras inputs (DeepFM.py:30-76) for columns that are already in
 * memory: every output column of `ids [rows, n_id] int32` / `dense [rows, n_dense] float32` is described by one sprk_pack_col.
 * The rule is CONVERT OR DECLINE, NEVER GUESS: the cases below are converted with the bits of the Python packer
 * (schema.pack_ids / pack_dense); a batch that holds anything else is DECLINED -- SPRK_EKIND, sprk_last_error names the column
 * and the row -- and the caller runs it through its next route.  The one error raised here is an identity id outside
 * [0, vocab), and only when nothing in the batch was declined: SPRK_ERANGE with the Python packer's message, chosen as it
 * chooses it (first column in id_cols order that holds a bad value, first bad row of that column).
 *   identity  integer / bool -> the value; float -> NaN = 0, else truncation (outside int64: declined); string -> empty = 0,
 *             else (long long) of the parsed double
 *   genre     integer -> the value, -1 outside [0, vocab); string -> position in the 19-entry vocabulary (DeepFM.py:64-66)
 *             below vocab, else -1; float / bool columns: declined
 *   dense     integer -> (float), one rounding; float -> NaN = 0.0, else (float); string -> empty = 0.0, else (float) of the
 *             parsed double
 * A numeric string is [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)? and nothing else (no blanks, "inf", "nan",
 * hex, "_"; a result of +-inf is declined).  The element of a fixed-width column is what is in front of its trailing NULs; an
 * embedded NUL is part of the value; a code point above 127 matches no genre and is declined in a numeric column.  Text
 * columns share ONE block of bytes: the columns' fields one after the other, column by column, EVERY field terminated by
 * '\n' (fields are raw: no quotes, no '\r' stripping); field i of text column k is line k * rows + i.  A block whose newline
 * count is not (text columns) * rows is declined. */
#define SPRK_COL_BOOL 0
#define SPRK_COL_I8 1
#define SPRK_COL_I16 2
#define SPRK_COL_I32 3
#define SPRK_COL_I64 4
#define SPRK_COL_U8 5
#define SPRK_COL_U16 6
#define SPRK_COL_U32 7
#define SPRK_COL_F32 8
#define SPRK_COL_F64 9
#define SPRK_COL_BYTES 10   /* fixed-width bytes, NUL padded (numpy S<width>)                  */
#define SPRK_COL_UCS4 11    /* fixed-width native-endian UCS4, NUL padded (numpy U<width>)     */
#define SPRK_COL_TEXT 12    /* fields of the shared text block                                 */
#define SPRK_RULE_IDENTITY 0
#define SPRK_RULE_GENRE 1
#define SPRK_RULE_DENSE 2
#define SPRK_PACK_MAX_COLS 128   /* id + dense columns of one sprk_pack_columns_device call    */
typedef struct sprk_pack_col {
    const void* data;    /* first element (NULL for SPRK_COL_TEXT)                              */
    int64_t stride;      /* bytes from one row's element to the next (any sign)                 */
    int32_t storage;     /* SPRK_COL_*                                                          */
    int32_t width;       /* BYTES: bytes, UCS4: code points per element (1 .. 65535); TEXT: the column's index in the block */
    int32_t on_device;   /* 0 = `data` is host memory, 1 = device memory (sprk_pack_columns_device only) */
    int32_t rule;        /* SPRK_RULE_*: id columns IDENTITY or GENRE, dense columns DENSE      */
    int32_t vocab;       /* buckets / vocabulary size (unused for DENSE)                        */
    int32_t reserved;    /* 0                                                                   */
    const char* name;    /* for messages (reference schema key)                                 */
} sprk_pack_col;
/* On the host (no GPU involved; every column and the outputs are HOST memory).  Rows are cut into chunks over n_threads host
 * threads (clamped to [1, 256], one thread below 16384 rows); outputs, the decline and the range error are identical for
 * any thread count.  Bad arguments (NULL pointers, unknown storage / rule, width 0, negative rows) -> SPRK_EINVAL. */
int sprk_pack_columns(const sprk_pack_col* id_cols, int32_t n_id, const sprk_pack_col* dense_cols, int32_t n_dense,
                      const char* text, size_t text_len, int32_t rows, int32_t n_threads, int32_t* ids_out, float* dense_out);
/* The same ON THE DEVICE (k_pack_columns.h), same bits: `ids_dev` / `dense_dev` are DEVICE arrays (16-byte aligned).  Columns
 * marked on_device are read where they are, with their stride; host columns (and the text block, always host memory) are
 * compacted into a pinned buffer on n_threads host threads and sent with ONE asynchronous copy; the buffer and its device
 * twin are kept per calling thread and grow to the largest batch seen.  At most SPRK_PACK_MAX_COLS columns, strides below
 * 2^31.  Numeric strings are converted on strtod's exact path only (at most 15 significant digits, decimal exponent within
 * +-22); the rest is declined, and sprk_pack_columns converts it.  Synchronises `stream`.  Arguments are validated before
 * any device call. */
int sprk_pack_columns_device(const sprk_pack_col* id_cols, int32_t n_id, const sprk_pack_col* dense_cols, int32_t n_dense,
                             const char* text, size_t text_len, int32_t rows, int32_t n_threads, int32_t* ids_dev,
                             float* dense_dev, void* stream);
/* What the calling thread's last column pack did (diagnostics / tests): 2 = converted on the device, 1 = converted on the
 * host, 0 = declined (SPRK_EKIND), -1 = no call yet / the call failed before converting anything.  A call that ends in
 * SPRK_ERANGE converted the batch (1 or 2). */
int sprk_pack_last_route(void);

/* ---- feature store in HBM: (userId, movieId) pairs -> the two packed arrays, and the sort behind the scores ----
 * The reference's ranking request carries {"userId": u, "movieId": m} x 800 and nothing else (RecForYouProcess.java:113-138); every other
 * model input comes from two per-entity maps, the `uf:<userId>` / `mf:<movieId>` hashes that FeatureEngForRecModel.scala:127-174,208-259
 * writes (the columns of each user's and each movie's latest sample).  Here the two maps are device tables indexed by id (row = id,
 * `pitch` dwords per row, a multiple of 4; one `has` byte per row), holding for every column exactly the 32 bits schema.pack_ids /
 * pack_dense produce (sparrowrecsys_amd/featurestore.py lays them out).  sprk_join_features writes output row q * C + c of
 * `ids_out [Q*C, n_id] int32` / `dense_out [Q*C, n_dense] float32` -- the format sprk_forward* reads -- for user_ids[q] and movie_ids[q][c]
 * (shared_candidates = 1: movie_ids[c], one list of C for every query); pairs are C = 1.  Every output column is one sprk_join_col:
 *   source  SPRK_JOIN_PAIR_USER / PAIR_MOVIE: the pair's own id; SPRK_JOIN_USER_ROW / MOVIE_ROW: dword `offset` of that table's row
 *   rule    SPRK_RULE_IDENTITY  the value as it is; one outside [0, vocab) is still written, and reported (below)
 *           SPRK_RULE_GENRE     the value, -1 outside [0, vocab)
 *           SPRK_RULE_DENSE     the 32 bits as they are (dense columns only; id columns are IDENTITY or GENRE, the pair's ids IDENTITY)
 * A user (movie) id outside [0, n_users) ([0, n_movies)), or one whose `has` byte is 0, reads the default row -- identity 0, genre -1,
 * dense 0.0 -- and nothing of the table; its own id still goes to the PAIR columns.  `range_key` is ONE caller-provided device word,
 * set to ~0 before the call: the kernel atomicMin's (id column index << 32 | output row) of every identity value outside its range into
 * it, so afterwards it names the error schema.pack_ids would raise for the same rows (first column in id_cols order, then first row).
 * All pointers but the descriptor lists are device memory; tables and outputs 16-byte aligned; at most SPRK_PACK_MAX_COLS columns;
 * Q * C < 2^31.  Anything else returns SPRK_EINVAL BEFORE any device call.  Asynchronous on `stream`: no synchronisation, no memory owned
 * by the library; all index arithmetic in 64 bits.  Q, C or the column count 0: nothing is done. */
#define SPRK_JOIN_PAIR_USER 0
#define SPRK_JOIN_PAIR_MOVIE 1
#define SPRK_JOIN_USER_ROW 2
#define SPRK_JOIN_MOVIE_ROW 3
typedef struct sprk_join_col {
    int32_t source;      /* SPRK_JOIN_*                                                          */
    int32_t offset;      /* USER_ROW / MOVIE_ROW: dword offset in the row (PAIR_*: unused)       */
    int32_t rule;        /* SPRK_RULE_*                                                          */
    int32_t vocab;       /* buckets / vocabulary size (unused for DENSE)                         */
} sprk_join_col;
int sprk_join_features(const int32_t* user_rows, const uint8_t* user_has, int32_t n_users, int32_t user_pitch,
                       const int32_t* movie_rows, const uint8_t* movie_has, int32_t n_movies, int32_t movie_pitch,
                       const int32_t* user_ids /* [Q] */, const int32_t* movie_ids /* [Q][C], or [C] shared */,
                       int32_t Q, int32_t C, int32_t shared_candidates,
                       const sprk_join_col* id_cols, int32_t n_id, const sprk_join_col* dense_cols, int32_t n_dense,
                       int32_t* ids_out, float* dense_out, uint64_t* range_key, void* stream);
/* order[q][0..C) = the candidate POSITIONS of scores[q][0..C) (float32, device memory) in the order of
 * `sorted(comparingByValue(reverseOrder()))` (RecForYouProcess.java:69-92): descending in Float.compare order -- every NaN one greatest
 * value, 0.0 before -0.0 -- and equal scores in candidate order: sprk_emb_rank's convention.  1 <= C <= 4096, Q >= 0, pointers not
 * NULL, else SPRK_EINVAL before any device call.  Asynchronous on `stream`; owns no memory. */
int sprk_rank_scores(const float* scores, int32_t Q, int32_t C, int32_t* order, void* stream);

/* ---- model.evaluate's accumulators in device memory ----
 * Every reference script ends with `model.evaluate(test_dataset)` -> [loss, accuracy, roc_auc, pr_auc] (DeepFM.py:117-133): binary
 * cross-entropy, accuracy at 0.5 and tf.keras.metrics.AUC(num_thresholds=200) for ROC and PR.  Keras keeps each metric as a handful of
 * accumulators that are updated batch by batch; here they live in ONE caller-owned block of device memory, and an update folds n
 * float32 scores and their labels into it on the caller's stream -- no score and no label crosses to the host, and the host reads
 * the few KB of state once, at the end (sparrowrecsys_amd/metrics.py DeviceMetrics turns it into the four numbers).
 * The state is sprk_metrics_state_bytes(T) bytes, 16-byte aligned, laid out as 8-byte words:
 *   [0] T (thresholds)   [1] n (samples)   [2] n_correct   [3] loss_sum (double)
 *   pos[T + 1], neg[T + 1] (uint64)   th[T] (double)   partial[1024] (double: one update's per-workgroup loss sums, scratch)
 * th is the table Keras compares against -- th[0] = 0 - 1e-7, th[i] = i / (T - 1), th[T - 1] = 1 + 1e-7, in float64 -- and a sample
 * with score p (float32 widened to double) and label y counts in pos (y != 0) or neg (y == 0) at
 *   bucket = the number of thresholds t with !(p <= t):  0 .. T; a NaN score in T, -inf in 0, +inf in T,
 * so that true positives at threshold i = the sum of pos[b] over b > i, false positives likewise over neg.
 * n_correct counts ((p > 0.5 ? 1 : 0) == y); loss_sum adds -(y log(pc) + (1 - y) log(1 - pc)) with pc = p clipped to
 * [1e-7, 1 - 1e-7], in double (a NaN score makes it NaN).  The counts are integer sums and exact.  loss_sum takes no floating-point
 * atomic: after an update it is a function of the word before, the inputs and n alone, the same bits on every run.
 * sprk_metrics_reset zeroes the counters and writes T and th.  sprk_metrics_update reads T from the state ON THE DEVICE (the host
 * never reads the state): on a state that was never reset, or that is shorter than its own T needs, the update does nothing.
 * label_storage is SPRK_COL_F32 / I32 / I64 / U8 / BOOL (the column packer's storage kinds, above), label_stride the distance in BYTES between two labels, a positive multiple of the label's size: a column of a
 * wider row-major array is read in place.  n >= 0; n == 0 does nothing.  ONE STATE IS NOT RE-ENTRANT: the calls on it must be ordered
 * on one stream (or by events); different states are independent.  NULL or misaligned pointers (state 16 bytes, scores 4, labels
 * their own size), a short state, an unknown storage, a bad stride or a negative n return SPRK_EINVAL BEFORE any device call.
 * Asynchronous on `stream`; no memory owned by the library; all index arithmetic in 64 bits. */
#define SPRK_METRICS_MAX_THRESHOLDS 1024
size_t sprk_metrics_state_bytes(int32_t num_thresholds);   /* 0 for num_thresholds outside [2, 1024] */
int sprk_metrics_reset(void* state, size_t state_bytes, int32_t num_thresholds, void* stream);
int sprk_metrics_update(void* state, size_t state_bytes, const float* scores, const void* labels, int32_t label_storage,
                        int64_t label_stride /* bytes */, int64_t n, void* stream);

/* ---- the exact areas under the ROC and the PR curve, over every distinct score ----
 * offline/spark/evaluate/Evaluator.scala of the reference reports BinaryClassificationMetrics' areaUnderROC and areaUnderPR: the areas
 * over EVERY distinct score, not Keras' 200 thresholds.  sparrowrecsys_amd/metrics.py exact_auc_host defines every number (DESIGN.md
 * section 5.15, with the rules read out of Spark 2.4 and the deviations); this call gives its bits from n float32 scores and their
 * labels in device memory.  scores: any finite float32; the threshold of a score is its float32 value, -0.0 taken as +0.0.  labels as
 * sprk_metrics_update takes them (label_storage, label_stride in bytes); a sample is positive iff label > 0.5.  Groups g = 1 .. G are
 * the distinct thresholds in DESCENDING order, tp_g / fp_g the positives / negatives with a score >= the group's, P = tp_G, N = fp_G:
 *   roc_numerator  = sum over g of neg_g (2 tp_{g-1} + pos_g), an integer (the rank statistic with ties at one half, times 2)
 *   area_under_roc = (double)roc_numerator / (double)(2 P N); 1.0 when N = 0, else 0.0 when P = 0
 *   pr_sum         = sum over g of (double)pos_g (prec_g + prec_{g-1}), prec_g = (double)tp_g / (double)(tp_g + fp_g), prec_0 := prec_1,
 *                    added in runs of 1024 consecutive groups, each from +0.0 in group order, the run sums from +0.0 in run order
 *   area_under_pr  = pr_sum / (double)(2 P); 0.0 when P = 0
 * Every operation is rounded on its own; no floating-point atomic: the result is a function of the inputs alone, whatever the grid,
 * the sort capacity, the bin width or the order of arrival.  The curve -- thresholds[g], tp[g], fp[g] (cumulative) for the G groups --
 * goes to the three arrays, each of which may be NULL and otherwise holds n elements, of which the first n_groups are written.
 * Errors are found before anything is computed: *error_key, which the caller sets to ~0 (= none), takes the LEAST of
 * kind << 32 | row over the rows in error -- kind 1: the score is not finite; kind 2: a float label is not finite -- and every later
 * kernel of the call returns at once, so result and the curve arrays keep what they held.  The caller reads the word.
 * 1 <= n < 2^31 - 1.  The workspace is what the _workspace_bytes call reports for n (0 for an n outside the range), 16-byte
 * aligned; rows go to bins by the leading _bin_bits(n) bits of their key (SPRK_EXACT_AUC_BIN_BITS = an integer in [1, 24], read at each call,
 * overrides the rule), bins are sorted in LDS up to 4096 keys (SPRK_FE_SORT_CAP, below) and by chunks and merge passes beyond.
 * NULL or misaligned pointers (result and error word 8 bytes), an n outside the range, an unknown storage, a bad stride, a short or
 * misaligned workspace (the message names sprk_exact_auc_workspace_bytes) return SPRK_EINVAL BEFORE any device call.  Asynchronous on
 * `stream`: no synchronisation, no memory owned by the library. */
typedef struct {
    int64_t n, n_pos, n_groups;
    uint64_t roc_numerator;
    double pr_sum, area_under_roc, area_under_pr;
} sprk_exact_auc_result;
size_t sprk_exact_auc_workspace_bytes(int64_t n);
int32_t sprk_exact_auc_bin_bits(int64_t n);                 /* 0 for an n outside the range */
int sprk_exact_auc(const float* scores, const void* labels, int32_t label_storage, int64_t label_stride /* bytes */, int64_t n,
                   sprk_exact_auc_result* result, float* thresholds, uint32_t* tp, uint32_t* fp,
                   uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* ---- feature engineering on the device: ratings -> training samples and the feature store's rows ----
 * The arithmetic of the reference's Spark job (FeatureEngForRecModel.scala:21-130): label = rating >= 3.5; per movie over ALL ratings
 * count / average / sample stddev; per user, in (timestamp, input row) order, the window of the previous 100 ratings -- its size, average,
 * stddev, its label-1 movies most recent first, the five genres its label-1 movies carry most often -- and the samples whose window
 * holds more than one rating.  The definition, rule by rule, is sparrowrecsys_amd/featureeng.py samples_host;
 * this call gives the same bits.  Averages and deviations are rounded to hundredths in INTEGER arithmetic (round half to even of the
 * exact rational, 128-bit products where a movie's count needs them) and stored as float32(h / 100.0); every sum is an integer
 * atomic, so the result is a function of the input alone.
 * In, device memory: the rating columns user_id, movie_id (int32), rating (float32, on the half-star scale 0, 0.5 .. 10), timestamp
 * (int64), n_ratings rows in any order; the movie table, n_movies rows indexed by movie id: movie_year (releaseYear; 1990 for a movie
 * the table does not hold), movie_genre3 [n_movies][3] (movieGenre1..3 as vocabulary index or -1), movie_genre_mask (bit g = the movie
 * carries genre g of a dictionary of at most 32 genres whose first n_vocab entries are the vocabulary).
 * Out, device memory, each holding n_ratings rows of which the first *n_kept are written, in (userId, timestamp, input row) order:
 * out_user, out_movie, out_rating, out_timestamp, out_label, out_source_row (the input row), out_genres [.][8] (movieGenre1..3,
 * userGenre1..5; a genre past n_vocab is -1 in its place), out_history [.][hist_len] (userRatedMovie1.., missing 0), out_dense [.][7]
 * (releaseYear, movieRatingCount, movieAvgRating, movieRatingStddev, userRatingCount, userAvgRating, userRatingStddev).
 * *n_kept = the sum over users of max(0, ratings of the user - 2).  Optionally the store in sparrowrecsys_amd/featurestore.py's layout,
 * every row written: user_rows [n_users][user_pitch], user_has [n_users], movie_rows [n_movies][8], movie_has [n_movies] -- all four
 * or none (NULL).  `error_key` is ONE caller-provided device word, set to ~0 before the call: the kernels atomicMin
 * (kind << 32 | input row) into it, kind 1 = user_id outside [0, n_users), 2 = movie_id outside [0, n_movies), 3 = rating off the
 * half-star scale; when it is not ~0 afterwards the outputs hold no result.  Such rows take no further part, so no index leaves its
 * array.  The workspace is sprk_feature_eng_workspace_bytes(n_ratings, n_users, n_movies) bytes, 16-byte aligned (0 for sizes the call
 * rejects).  A user's ratings are sorted in LDS up to 4096 of them (SPRK_FE_SORT_CAP = a power of two in [64, 4096], read at each call,
 * lowers that) and by chunked sort + merge passes in global memory beyond; any length up to n_ratings works.
 * 0 <= n_ratings < 2^31 - 1, 0 <= n_users < 2^31 - 1, n_movies >= 0, 1 <= hist_len <= 100, 0 <= n_vocab <= 32, user_pitch >= hist_len + 8,
 * no NULL or misaligned pointer, a sufficient workspace: anything else returns SPRK_EINVAL BEFORE any device call.  Asynchronous on
 * `stream`: no synchronisation, no memory owned by the library; all index arithmetic in 64 bits. */
size_t sprk_feature_eng_workspace_bytes(int64_t n_ratings, int32_t n_users, int32_t n_movies);
int sprk_feature_eng(const int32_t* user_id, const int32_t* movie_id, const float* rating, const int64_t* timestamp, int64_t n_ratings,
                     int32_t n_users, int32_t n_movies, const int32_t* movie_year, const int32_t* movie_genre3, const uint32_t* movie_genre_mask,
                     int32_t n_vocab, int32_t hist_len,
                     int32_t* out_user, int32_t* out_movie, float* out_rating, int64_t* out_timestamp, int32_t* out_label, int32_t* out_source_row,
                     int32_t* out_genres, int32_t* out_history, float* out_dense,
                     int32_t* user_rows, uint8_t* user_has, int32_t user_pitch, int32_t* movie_rows, uint8_t* movie_has,
                     uint64_t* error_key, int64_t* n_kept, void* workspace, size_t workspace_bytes, void* stream);

/* ---- new ratings applied to a feature store on the device, equal to a rebuild ----
 * Let R be the concatenation, in call order, of every ratings batch applied to one store and its state (the state of no ratings:
 * user_count, ring_movie, ring_r2, movie_count, movie_sum, movie_sumsq, movie_flag all zero, user_last_ts INT64_MIN in every element;
 * the tables of no ratings: user_has / movie_has 0 and every row the NA defaults, which is what sprk_feature_eng writes for
 * n_ratings = 0).  After each call the first n_users / n_movies rows of user_rows, user_has, movie_rows, movie_has are byte for byte
 * what sprk_feature_eng writes from R with the same movie table, n_vocab, hist_len and table sizes -- PROVIDED every new rating's
 * timestamp is >= the latest timestamp of its user applied by an EARLIER call (rows of one call may come in any order).  The
 * definition is sparrowrecsys_amd/featureeng.py update_host; DESIGN.md section 5.14 has the argument.
 * State, device memory, owned by the caller and changed by this call alone: user_count [n_users] (ratings applied), user_last_ts
 * [n_users], ring_movie / ring_r2 [n_users][100] (the user's last 100 ratings as movie id and 2 * rating, the rating at position p of
 * the user's (timestamp, row in R) order in slot p % 100), movie_count / movie_sum / movie_sumsq [n_movies] (n, the sum of 2 * rating
 * and of its square over all ratings), movie_flag [n_movies] (a rating of the movie sits at a user position >= 2: a kept sample names it).
 * The rating columns, the movie table, n_vocab, hist_len, the tables and user_pitch are sprk_feature_eng's.  The caller keeps the sum of
 * n_new over all calls below 2^31 - 1.
 * `error_key` is ONE caller-provided device word, set to ~0 before the call: the first kernel atomicMins (kind << 32 | row of this
 * batch) into it, kinds 1 - 3 as for sprk_feature_eng and 4 = timestamp older than the user's latest; it writes nothing else, and every
 * later kernel returns at once when the word is set: then NO byte of the state or of the tables has changed.
 * The workspace is sprk_store_update_workspace_bytes(n_new, n_users, n_movies) bytes, 16-byte aligned (0 for sizes the call rejects).
 * 0 <= n_new < 2^31 - 1, 0 <= n_users < 2^31 - 1, n_movies >= 0, 1 <= hist_len <= 100, 0 <= n_vocab <= 32, user_pitch >= hist_len + 8, no
 * NULL or misaligned pointer, a sufficient workspace: anything else returns SPRK_EINVAL BEFORE any device call.  Asynchronous on
 * `stream`: no synchronisation, no memory owned by the library; integer sums only, so the result is a function of the input alone. */
size_t sprk_store_update_workspace_bytes(int64_t n_new, int32_t n_users, int32_t n_movies);
int sprk_store_update(const int32_t* user_id, const int32_t* movie_id, const float* rating, const int64_t* timestamp, int64_t n_new,
                      int32_t n_users, int32_t n_movies, const int32_t* movie_year, const int32_t* movie_genre3, const uint32_t* movie_genre_mask,
                      int32_t n_vocab, int32_t hist_len,
                      uint32_t* user_count, int64_t* user_last_ts, int32_t* ring_movie, uint8_t* ring_r2,
                      uint32_t* movie_count, uint64_t* movie_sum, uint64_t* movie_sumsq, uint8_t* movie_flag,
                      int32_t* user_rows, uint8_t* user_has, int32_t user_pitch, int32_t* movie_rows, uint8_t* movie_has,
                      uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* The workgroups (of 256 threads) that the ratings pipelines and the trainers launch for a loop over `items` elements:
 * max(1, ceil(items / 256)), at most 2048; every such loop strides by the grid, and the work queues (sprk_als_fit's half sweeps,
 * sprk_user_emb's sums) are capped likewise.  SPRK_FE_MAX_GRID = an integer in [1, 2048], read at each call, lowers the cap (anything
 * else is ignored); it exists for the tests, which take the loops' second round at small sizes: no result depends on the grid.  No
 * device call. */
int64_t sprk_segments_grid(int64_t items);

/* ---- user embeddings on the device: ratings + item embeddings -> one vector per user ----
 * The arithmetic of the reference's Embedding.generateUserEmb (Embedding.scala:53-101), which writes userEmb.csv, the "emb" ranker's user
 * side.  The definition, rule by rule, is sparrowrecsys_amd/userembedding.py user_emb_host; this call gives the
 * same bits.  Per user: acc = +0.0f in every dimension; the user's rating rows are walked in INPUT ORDER FROM THE LAST TO THE FIRST (the
 * Scala folds with foldRight) and every row whose item has an embedding does acc = acc + item_emb[row], one float32 add per dimension
 * per row, never reassociated (no float atomics, nothing split along a user's rows: the result is a function of the input alone).  A
 * row "has an embedding" when 0 <= item_row[i] < n_items and item_has[item_row[i]] != 0; any other row is skipped -- no zero row is
 * added, a table row with item_has == 0 may hold anything -- and is no error.  Subnormals are kept.
 *   mode 0 (the Scala)        user_count = ALL the user's rows, user_emb = acc / (float)user_count (IEEE division, round to nearest even)
 *   mode 1 (the PySpark twin) user_count = the user's rows that have an embedding, user_emb = acc
 * user_has = (user_count > 0); a user whose count is 0 gets zeros.  So in mode 0 a user none of whose items has an embedding has
 * user_has 1 and an all-zero vector.
 * In, device memory: user_id and item_row (int32, the item table's row of the rated movie), n_ratings rows in any order; item_emb
 * [n_items][item_stride] float32 of which D per row are read, item_has [n_items].  Out, device memory, EVERY row written: user_emb
 * [n_users][user_stride] (D floats per row; the floats between D and user_stride are left alone), user_has [n_users], user_count
 * [n_users].  `error_key` is ONE caller-provided device word, set to ~0 before the call: the kernels atomicMin (1 << 32 | input row)
 * into it for a user_id outside [0, n_users); such a row takes no further part, and when the word is not ~0 afterwards the outputs
 * hold no result.  Input that is grouped by user (every user's rows adjacent) is summed where it lies; any other input is scattered
 * into per-user segments and sorted by input row -- in LDS up to 4096 rows of one user (SPRK_FE_SORT_CAP, as for sprk_feature_eng),
 * by chunked sort + merge passes beyond.  The workspace is sprk_user_emb_workspace_bytes(n_ratings, n_users) bytes, 16-byte aligned
 * (0 for sizes the call rejects).
 * 0 <= n_ratings < 2^31 - 1, 0 <= n_users < 2^31 - 1, n_items >= 0, 1 <= D <= 1024, item_stride >= D, user_stride >= D, mode 0 or 1, no
 * NULL or misaligned pointer, a sufficient workspace (the message names the bytes needed): anything else returns SPRK_EINVAL BEFORE
 * any device call.  Asynchronous on `stream`: no synchronisation, no memory owned by the library; all index arithmetic in 64 bits. */
size_t sprk_user_emb_workspace_bytes(int64_t n_ratings, int32_t n_users);
int sprk_user_emb(const int32_t* user_id, const int32_t* item_row, int64_t n_ratings, int32_t n_users,
                  const float* item_emb, const uint8_t* item_has, int32_t n_items, int32_t D, int32_t item_stride,
                  int32_t mode, float* user_emb, int32_t user_stride, uint8_t* user_has, int32_t* user_count,
                  uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* ---- embedding LSH on the device: random-projection buckets, a sorted index per hash table, approximate top-K ----
 * The reference's Embedding.embeddingLSH (Embedding.scala:230-252): Spark's BucketedRandomProjectionLSH, its transform and its single-probe
 * approxNearestNeighbors.  The definition, rule by rule, is sparrowrecsys_amd/lsh.py hash_host / approx_nearest_host (DESIGN.md section
 * 5.16); these calls give the same bits.  All arithmetic is double, every operation rounded on its own (no fused multiply-add), in index
 * order; no float or double atomics, so every output is a function of the input alone.
 *
 * sprk_lsh_hash (`transform`).  In, device memory: emb [n][stride] float32 of which D per row are read, has [n] (NULL: every row has an
 * embedding), vectors [T][D] float64 (the caller's: random_unit_vectors in lsh.py, or any).  Out: buckets [n][T] int64, every word written.
 * For row x and table t: dot = ((+0.0 + x_0 r_t0) + x_1 r_t1) + ..., bucket = floor(dot / bucket_length) clamped to [-2^62, 2^62]; a dot
 * that is not finite, and every table of a row with has == 0, gives SPRK_LSH_NO_BUCKET: the row is in no bucket of that table.  A row
 * with a non-finite coordinate has no bucket in any table.
 *
 * sprk_lsh_build.  In: buckets [n][T].  Out: idx_bucket [T][n] int64 and idx_row [T][n] int32 -- table t's n (bucket, row) pairs
 * sorted by (bucket, row) ascending, one segment per table: in LDS up to 4096 rows (SPRK_FE_SORT_CAP, as for sprk_feature_eng), by
 * chunked sort + merge passes beyond.  The workspace is sprk_lsh_build_workspace_bytes(n, T) bytes, 16-byte aligned (0 for sizes the
 * call rejects).
 *
 * sprk_lsh_query (`approxNearestNeighbors`, one probe).  In: the table, has, vectors and bucket_length as given to sprk_lsh_hash, its
 * buckets, sprk_lsh_build's index; queries [Q][query_stride] float32, query_has [Q] (NULL: every query counts).  The candidates of a
 * query are the rows with has != 0 whose bucket equals the query's in at least one table (SPRK_LSH_NO_BUCKET equals nothing), each
 * once; dist = sqrt(sum_i (x_i - y_i)^2) from +0.0 in index order with a correctly rounded square root; candidates are ordered by
 * (dist, row) ascending.  Out, every word written: dist [Q][K] float64 and rows [Q][K] int32, the first K candidates; count [Q] int32,
 * the number of candidates, which may exceed K.  Places past count, and every place of a query with query_has == 0 (count 0), hold NaN
 * (0x7ff8000000000000) / -1.  One workgroup per query walks the bucket's range of every table and keeps the best K next to the new
 * pairs in an LDS buffer of 4096 pairs, sorted and cut to K when full; SPRK_LSH_CHUNK = a power of two in [64, 4096], read at each
 * call, shortens the buffer (for the tests).  No workspace.
 *
 * 0 <= n < 2^31 - 1, Q >= 0, 1 <= D <= 1024, 1 <= T <= 16, strides >= D, 1 <= K <= 1024 and K < the buffer's pairs, bucket_length finite
 * and > 0, no NULL (but has / query_has) or misaligned pointer, a sufficient workspace (the message names the bytes needed): anything
 * else returns SPRK_EINVAL BEFORE any device call.  Asynchronous on `stream`: no synchronisation, no memory owned by the library; all
 * index arithmetic in 64 bits; the element-wise loops stride by sprk_segments_grid's grid. */
#define SPRK_LSH_NO_BUCKET INT64_MIN
int sprk_lsh_hash(const float* emb, const uint8_t* has, int64_t n, int32_t D, int32_t stride, const double* vectors, int32_t T,
                  double bucket_length, int64_t* buckets, void* stream);
size_t sprk_lsh_build_workspace_bytes(int64_t n, int32_t T);
int sprk_lsh_build(const int64_t* buckets, int64_t n, int32_t T, int64_t* idx_bucket, int32_t* idx_row,
                   void* workspace, size_t workspace_bytes, void* stream);
int sprk_lsh_query(const float* emb, const uint8_t* has, int64_t n, int32_t D, int32_t stride, const double* vectors, int32_t T,
                   double bucket_length, const int64_t* buckets, const int64_t* idx_bucket, const int32_t* idx_row,
                   const float* queries, const uint8_t* query_has, int32_t Q, int32_t query_stride, int32_t K,
                   double* dist, int32_t* rows, int32_t* count, void* stream);

/* ---- the held-out split on the device: a sample of the rows, cut at random or at a quantile of the timestamps ----
 * The reference's splitAndSaveTrainingTestSamples and ...ByTimeStamp (FeatureEngForRecModel.scala:176-205): a 10 % sample cut 80 / 20.
 * The definition, rule by rule, is sparrowrecsys_amd/featureeng.py split_host; these calls give the same bytes.
 *
 * sprk_split_plan.  In, device memory: key [n] -- int32 (key_kind 1) or int64 (key_kind 2) -- or nothing (key_kind 0: a row's key is its
 * position); timestamp [n] int64 (mode 1 only; unread in mode 0).  For key k and stream s (0 = sample, 1 = split), modulo 2^64:
 *   x = seed + 0x9E3779B97F4A7C15 (2 k + s + 1);  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;
 *   x ^= x >> 31;  u = x >> 11
 * A row is sampled where its stream-0 u < t_sample.  mode 0 (random): a sampled row is training where its stream-1 u < t_train, else
 * test.  mode 1 (time): with r = ceil(train * (double)n_sampled), the call's only float arithmetic, split_timestamp = the sampled rows'
 * timestamp at ascending position max(r, 1) - 1, found exactly by a radix select (sign bit flipped, eight passes of eight bits, most
 * significant first: a 256-bin histogram per pass and a one-workgroup pick between passes); sampled rows with timestamp <=
 * split_timestamp are training, the others test.  t_sample and t_train are the caller's floor(fraction * 2^53) (2^53 for a fraction of 1).
 * Out: index_train [n] and index_test [n] int32, of which the first n_train / n_test are written: the parts' source positions,
 * ascending -- a row's place is decided by per-tile counts, a scan and ballots, by no atomic, so the lists are the same on every run.
 * words [5] int64: words[0] is the error word, set to ~0 (-1) by the caller BEFORE the call; the call writes words[1 .. 4] = n_sampled,
 * n_train, n_test, split_timestamp (0 in mode 0 and where no row is sampled).  A negative key does atomicMin (1 << 32 | row) into the
 * error word; every kernel returns at once when the word is not ~0, so the lists and the other four words then hold no result.
 * The workspace is sprk_split_plan_workspace_bytes of n, 16-byte aligned (0 for an n the call rejects).
 * 0 <= n < 2^31 - 1, key_kind 0 / 1 / 2, mode 0 / 1, thresholds <= 2^53, 0 <= train <= 1, no NULL (but key at key_kind 0 and timestamp in
 * mode 0) or misaligned pointer, a sufficient workspace (the message names the bytes needed): anything else returns SPRK_EINVAL BEFORE
 * any device call.
 *
 * sprk_take_rows: dst[j] = src[index[j]], j in [0, n_index), for each of n_cols columns.  A column is a sprk_split_col: its source (row
 * i at src + i * src_stride bytes, so a column of a wider matrix is taken where it lies), the bytes of a row (a positive multiple of
 * 4) and a dense destination of n_index rows.  A thread makes 16 bytes of a destination, stored as one 128-bit word where the
 * destination is 16-byte aligned and loaded as one where row_bytes, src and src_stride are multiples of 16.  n_rows = the rows of the
 * sources: an index outside [0, n_rows) leaves its destination row unwritten.  Pointers 4-byte aligned, src_stride a multiple of 4 and
 * >= 0, 0 <= n_index, n_rows < 2^31 - 1, else SPRK_EINVAL BEFORE any device call.  No workspace.
 *
 * Both are asynchronous on `stream`: no synchronisation, no memory owned by the library; all index arithmetic in 64 bits; the loops
 * stride by sprk_segments_grid's grid. */
typedef struct {
    const void* src;
    int64_t src_stride;                /* bytes from a source row to the next */
    int32_t row_bytes;                 /* a multiple of 4 */
    int32_t reserved;                  /* 0 */
    void* dst;
} sprk_split_col;
size_t sprk_split_plan_workspace_bytes(int64_t n);
int sprk_split_plan(const void* key, int32_t key_kind, const int64_t* timestamp, int64_t n, uint64_t seed, uint64_t t_sample, uint64_t t_train,
                    double train, int32_t mode, int32_t* index_train, int32_t* index_test, int64_t* words,
                    void* workspace, size_t workspace_bytes, void* stream);
int sprk_take_rows(const sprk_split_col* cols, int32_t n_cols, const int32_t* index, int64_t n_index, int64_t n_rows, void* stream);

/* ---- ranking metrics on the device: top-K lists against held-out (user, item) pairs ----
 * Spark's RankingMetrics (precisionAt, recallAt, ndcgAt, meanAveragePrecisionAt) plus hit rate and reciprocal rank, the lists first
 * cleared of what the user has already seen.  The definition, rule by rule, is sparrowrecsys_amd/rankeval.py rank_eval_host (DESIGN.md
 * section 5.18); this call gives the same bytes.
 *
 * In, device memory: pred [n_queries][pred_stride] int32 of which list_len per row are read -- item ids, best first, a negative entry
 * is no entry; query_user [n_queries] int32 (NULL: query q is user q's); the truth pairs truth_user / truth_item [n_truth] and the seen
 * pairs seen_user / seen_item [n_seen] int32, in any order, duplicates allowed (n_seen 0: nothing is dropped); gain [1024] and
 * gain_sum [1025] float64, the CALLER's: gain[i] = 1.0 / log(i + 2) and gain_sum[c] = gain[0] + .. + gain[c - 1] added in order from
 * +0.0, made on the host (rankeval.py gain_table) -- no logarithm is taken on the device.  In, HOST memory: ks [n_ks] int32, the cut-offs.
 *
 * Per query q of user u: T = the distinct truth items of u, R = |T|; E = pred[q] in order without negative entries and without the
 * entries among u's seen items, L = len(E).  A truth item that is also seen stays in T; duplicate entries of pred each count.  For a
 * cut-off k, with n = min(L, k) and the hits = the places i < n with E[i] in T:
 *   precision = hits / k;  recall = hits / R;  ndcg = dcg / gain_sum[min(R, k)], dcg = the sum of gain[i] over the hits in list order
 *   from +0.0;  ap = (the sum over the hits, in order, of cnt_i / (i + 1)) / min(R, k), cnt_i = the running hit count;  hit = 1.0 where
 *   hits > 0;  rr = 1 / (i0 + 1) for the first hit i0, else 0.0.
 * All float64, every operation rounded on its own (no fused multiply-add), `/` correctly rounded.  A query with R == 0 scores +0.0 six
 * times and is not counted in counts[1].
 * Out, device memory: per_query [n_queries][n_ks][6] float64 in the order above; n_relevant [n_queries] (R) and n_ranked [n_queries]
 * (L) int32; sums [n_ks][6] float64 -- per (k, metric) the partial sums over 256 consecutive queries from +0.0 in query order, then the
 * partials in order from +0.0; counts [2] int64 = (n_queries, the queries with R > 0).  No float or double atomics and no cross-lane
 * float reduction: every output is a function of the input alone.
 *
 * The error word is set to ~0 by the caller BEFORE the call.  A truth row (kind 1) or a seen row (kind 2) whose user lies outside
 * [0, n_users) or whose item is negative, and a query (kind 3) whose user lies outside [0, n_users), do atomicMin (kind << 32 | row)
 * into it; when it is not ~0 as the metrics start, none of the five outputs is written.
 *
 * Stages: per side, counts per user, the scan, a scatter and the segment sort by (item, input row) (in LDS up to 4096 rows,
 * SPRK_FE_SORT_CAP as for sprk_feature_eng; chunked sort + merge passes beyond); one wave per query -- rounds of 64 entries, two
 * binary searches a lane, two ballots, the float64 terms added in list order by a walk over the hit mask; the two-level sums.  The
 * workspace is sprk_rank_eval_workspace_bytes(n_truth, n_seen, n_users, n_queries) bytes, 16-byte aligned (0 for sizes the call rejects).
 *
 * 0 <= n_truth, n_seen, n_users < 2^31 - 1, n_queries >= 0, 1 <= list_len <= 65536, pred_stride >= list_len, 1 <= n_ks <= 8, every k in
 * [1, 1024] (independent of list_len), no NULL (but query_user; the truth or seen columns of an empty side; pred and the per-query
 * outputs at n_queries 0) or misaligned pointer, a sufficient workspace (the message names the bytes needed): anything else returns
 * SPRK_EINVAL BEFORE any device call.  Asynchronous on `stream`: no synchronisation, no memory owned by the library; all index
 * arithmetic in 64 bits; the loops stride by sprk_segments_grid's grid. */
size_t sprk_rank_eval_workspace_bytes(int64_t n_truth, int64_t n_seen, int32_t n_users, int32_t n_queries);
int sprk_rank_eval(const int32_t* pred, int32_t n_queries, int32_t list_len, int32_t pred_stride, const int32_t* query_user,
                   const int32_t* truth_user, const int32_t* truth_item, int64_t n_truth,
                   const int32_t* seen_user, const int32_t* seen_item, int64_t n_seen, int32_t n_users,
                   const int32_t* ks, int32_t n_ks, const double* gain, const double* gain_sum,
                   double* per_query, int32_t* n_relevant, int32_t* n_ranked, double* sums, int64_t* counts,
                   uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the movie catalogue on the device: average ratings, sorted lists, candidates and the default similarity ranker ----
 * The arithmetic of the reference's DataManager and SimilarMovieProcess (Movie.java:93-98, DataManager.java:253-283,
 * SimilarMovieProcess.java:39-83 and :145-159).  The definition, rule by rule, is sparrowrecsys_amd/catalog.py catalog_host / similar_host
 * (DESIGN.md section 5.9); these calls give the same bits.
 *
 * sprk_catalog_build.  In, device memory: the rating columns movie_id (int32) and rating (float32), n_ratings rows in input order; the
 * movie table, n_movies rows indexed by movie id: movie_genre_mask (bit g = genre g of a dictionary of n_genres <= 32 genres), movie_has
 * (the table holds the movie), movie_year (DataManager's releaseYear, 0 = none), movie_file_pos (the movie's position in movies.csv) and
 * movie_hash_pos (its position in the iteration order of Java's HashMap), the last two permutations of [0, movies held) over the
 * movies held.  A rating whose movie lies outside the table, or is not held, is skipped (movieMap.get == null): no error.
 * Out, device memory, every row written: avg_rating [n_movies] float64 -- per movie, over its ratings in input order from avg = 0.0,
 * n = 0: avg = (avg * (double)n + (double)rating) / (double)(n + 1), one multiply, one add and one IEEE division per rating, never fused
 * or reassociated, which is NOT sum / n in general; 0.0 for a movie without a rating -- and rating_count [n_movies].  The 2 (G + 1)
 * lists, G = n_genres, as list_offsets [2 (G + 1) + 1] into list_movies [list_capacity]: list g < G = the movies of genre g by
 * average rating, list G = every movie held by average rating, list G + 1 + g = genre g by year, list 2 G + 1 = every movie by year;
 * all descending (the rating in Double.compare order), ties by file position in a genre list and by hash position in the whole
 * catalogue's, as Java's stable sort leaves them.  list_capacity >= the lists' total, 2 (sum of the movies' genre counts + movies
 * held); the entries past the total are -1.  Input grouped by movie (every movie's rows adjacent) is walked where it lies; any other
 * input is scattered into per-movie segments and sorted by input row, in LDS up to 4096 rows of one movie (SPRK_FE_SORT_CAP, as for
 * the feature engineering call) and by chunked sort + merge passes beyond; so are the lists.  A movie of fewer than 128 ratings is
 * walked by one lane, a longer one by a wave of its own.
 * `error_key` is ONE caller-provided device word, set to ~0 before the call: the kernels atomicMin (3 << 32 | input row) into it for a
 * rating that is not finite (the row takes no further part) and (4 << 32) when the lists do not fit list_capacity (every list is then
 * empty); when it is not ~0 afterwards the outputs hold no result.
 * 0 <= n_ratings < 2^31 - 1, 0 <= n_movies < 2^31 - 1, 0 <= list_capacity < 2^31 - 1, 0 <= n_genres <= 32, no NULL or misaligned pointer, a
 * workspace of sprk_catalog_build_workspace_bytes bytes (0 for sizes the call rejects; the message names the bytes needed), 16-byte
 * aligned: anything else returns SPRK_EINVAL BEFORE any device call.
 *
 * sprk_catalog_similar: one workgroup per query movie.  In: query_movie [n_queries]; the table columns above with movie_n_genres
 * (uint8, the movie's number of genres) and the build's avg_rating, list_offsets and list_movies (list_entries of them).
 * mode 0 (candidateGenerator): the union over the query's genres of the first top_n entries of that genre's rating list; mode 1
 * (multipleRetrievalCandidates): those, the first extra_n of the whole catalogue's rating list and the first extra_n of its year
 * list; minus the query itself, in ascending movie id order.  A query the table does not hold has no candidates.
 * score_kind 0: out_ids [n_queries][out_stride] = the candidates, padded with -1, out_count = their number (ids past out_stride are
 * not written: a count above out_stride tells); out_scores is not used.  score_kind 1: per candidate c of query q, in doubles, every
 * operation rounded on its own: same = popcount(mask_q & mask_c), score = ((same / (n_genres_q + n_genres_c)) / 2.0) * 0.7 +
 * (avg_c / 5.0) * 0.3 (0 / 0 = NaN); the candidates sorted by score descending in Double.compare order (every NaN one greatest value,
 * written as 0x7ff8000000000000), equal scores by ascending id; the first `size` ids and scores are written, padded with -1 / 0.0, and
 * out_count = min(size, candidates).  n_queries >= 0, n_movies >= 0, 0 <= n_genres <= 32, top_n >= 0, extra_n >= 0,
 * 32 top_n + 2 extra_n <= 4096, out_stride >= 1, 0 <= size (<= out_stride for score_kind 1), no NULL or misaligned pointer: anything else
 * returns SPRK_EINVAL BEFORE any device call.  No workspace.
 * Both are asynchronous on `stream`: no synchronisation, no memory owned by the library; all index arithmetic in 64 bits. */
size_t sprk_catalog_build_workspace_bytes(int64_t n_ratings, int32_t n_movies, int64_t list_capacity);
int sprk_catalog_build(const int32_t* movie_id, const float* rating, int64_t n_ratings, int32_t n_movies,
                       const uint32_t* movie_genre_mask, const uint8_t* movie_has, const int32_t* movie_year,
                       const int32_t* movie_file_pos, const int32_t* movie_hash_pos, int32_t n_genres,
                       double* avg_rating, int32_t* rating_count, int32_t* list_offsets, int32_t* list_movies, int64_t list_capacity,
                       uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);
int sprk_catalog_similar(const int32_t* query_movie, int32_t n_queries, int32_t n_movies,
                         const uint32_t* movie_genre_mask, const uint8_t* movie_has, const uint8_t* movie_n_genres, const double* avg_rating, int32_t n_genres,
                         const int32_t* list_offsets, const int32_t* list_movies, int64_t list_entries,
                         int32_t mode, int32_t top_n, int32_t extra_n, int32_t score_kind, int32_t size,
                         int32_t* out_ids, double* out_scores, int32_t out_stride, int32_t* out_count, void* stream);

/* ---- ALS collaborative filtering on the device: ratings -> factors, scores and a top-K for every row ----
 * The reference's offline/spark/model/CollaborativeFiltering.scala (Spark ALS, explicit feedback, no non-negativity, maxIter 5, regParam
 * 0.01, rank 10; then the RMSE of held-out pairs, recommendForAllUsers and recommendForAllItems).  The definition, rule by rule, is
 * sparrowrecsys_amd/als.py als_host / predict_host / topk_host (with the deviations from Spark); these calls give
 * the same bits.
 *
 * sprk_als_fit.  Every iteration recomputes the item factors from the user factors, then the user factors from the new item factors, so
 * only the initial USER factors are read.  One destination row (a movie, then a user) walks its ratings in ascending order of the
 * other side's id, a repeated pair by ascending input row, and accumulates in doubles from +0.0, with x = the other side's factor row
 * widened to double: the packed upper triangle ata[i, j] += x[i] * x[j] (entry (i, j), i <= j, at j (j + 1) / 2 + i) and atb[i] +=
 * (double)rating * x[i], the product rounded, then the sum; adds (double)n * reg (n = the row's ratings) to the diagonal; factors
 * U^T U = ata column by column (netlib's dpptrf), solves by forward and back substitution (dpptrs) in als.py cholesky_solve_host's
 * operation order, nothing fused, division and square root correctly rounded; and rounds the solution to float32.  A row's ratings
 * are never split and there is no float or double atomic: the result is a function of the input alone.  A row without ratings gets
 * has 0 and zeros.
 * In, device memory: user_id, movie_id (int32) and rating (float32), n_ratings rows in any order; init_user [n_users][init_stride]
 * float32 of which `rank` per row are read.  Out, device memory, EVERY row written: user_factors [n_users][user_stride] and item_factors
 * [n_items][item_stride] (`rank` floats per row; the floats between rank and the stride are left alone), user_has / item_has (the row
 * has a rating), user_count / item_count.  iters = 0 writes init_user to user_factors, zeros to item_factors, and has and the counts.
 * `error_key` is ONE caller-provided device word, set to ~0 before the call, into which the kernels atomicMin (kind << 32 | index):
 * kind 1, 2, 3 = a user id outside [0, n_users), a movie id outside [0, n_items), a rating that is not finite, index = the input row
 * (such a row takes no further part); kind 7 = a value of init_user that is not finite, index = its row; kind 5 / 6 = the normal
 * equations of a user / a movie are not positive definite (some d = A[j, j] - sum is not > 0; with reg = 0 and fewer ratings than rank
 * the ordinary outcome), index = the id, the smallest of the first half-sweep that has one.  Once the word is set no further half-sweep
 * runs; when it is not ~0 afterwards the outputs hold no result.  The ratings are scattered into per-movie and per-user segments once
 * and sorted by (other id, input row) -- in LDS up to 4096 ratings of one row (SPRK_FE_SORT_CAP, as for the feature engineering call), by
 * chunked sort + merge passes beyond.  The workspace is sprk_als_workspace_bytes bytes, 16-byte aligned (0 for sizes the call rejects).
 * 0 <= n_ratings < 2^31 - 1, 0 <= n_users < 2^31 - 1, 0 <= n_items < 2^31 - 1, 1 <= rank <= 16, iters >= 0, reg finite and >= 0, every
 * stride >= rank, no NULL or misaligned pointer, a sufficient workspace (the message names the bytes needed): anything else returns
 * SPRK_EINVAL BEFORE any device call.
 *
 * sprk_als_predict: out[i] = the float32 dot of user_factors[user[i]] and item_factors[item[i]] in index order from 0.0f, every product
 * and every sum rounded on its own (ALSModel's sdot); NaN (0x7fc00000) when either id lies outside its table or has has == 0 -- Spark's
 * cold-start NaN, which coldStartStrategy = "drop" drops.  n >= 0, n_users >= 0, n_items >= 0, 1 <= rank <= 16, strides >= rank.
 *
 * sprk_als_topk: for every row of query [n_queries][query_stride] the K rows of table [n_rows][table_stride] with the largest such dot:
 * descending score, equal scores by ascending row (a NaN score, possible only with non-finite factors, sorts greatest); table rows with
 * table_has == 0 are left out.  scores / rows [n_queries][K]; the places past the rows available, and every place of a query with
 * query_has == 0, hold NaN (0x7fc00000) / -1.  The selection is sprk_emb_topk's: chunks of 4096 rows (SPRK_EMB_TOPK_CHUNK) sorted in
 * LDS, then a merge tree.  1 <= K <= 1024, 1 <= rank <= 16, n_rows >= 0, n_queries >= 0; the workspace is
 * sprk_als_topk_workspace_bytes bytes (0 when the table is one chunk, and for sizes the call rejects), 16-byte aligned.
 * All are asynchronous on `stream`: no synchronisation, no memory owned by the library; all index arithmetic in 64 bits. */
size_t sprk_als_workspace_bytes(int64_t n_ratings, int32_t n_users, int32_t n_items, int32_t rank);
int sprk_als_fit(const int32_t* user_id, const int32_t* movie_id, const float* rating, int64_t n_ratings,
                 int32_t n_users, int32_t n_items, int32_t rank, double reg, int32_t iters,
                 const float* init_user, int32_t init_stride,
                 float* user_factors, int32_t user_stride, float* item_factors, int32_t item_stride,
                 uint8_t* user_has, uint8_t* item_has, int32_t* user_count, int32_t* item_count,
                 uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);
int sprk_als_predict(const int32_t* user, const int32_t* item, int64_t n,
                     const float* user_factors, int32_t user_stride, const uint8_t* user_has,
                     const float* item_factors, int32_t item_stride, const uint8_t* item_has,
                     int32_t n_users, int32_t n_items, int32_t rank, float* out, void* stream);
size_t sprk_als_topk_workspace_bytes(int32_t n_rows, int32_t n_queries, int32_t K);
int sprk_als_topk(const float* table, const uint8_t* table_has, int32_t n_rows, int32_t rank, int32_t table_stride,
                  const float* query, const uint8_t* query_has, int32_t n_queries, int32_t query_stride,
                  int32_t K, float* scores, int32_t* rows, void* workspace, size_t workspace_bytes, void* stream);

/* ---- item2vec on the device: ratings -> per-user item sequences -> skip-gram item vectors ----
 * The reference's offline/spark/embedding/Embedding.scala (processItemSequence, then Spark Word2Vec: skip-gram with hierarchical
 * softmax) without Spark.  The definitions are sparrowrecsys_amd/item2vec.py sequences_host and skipgram_host (numpy); both calls equal
 * them bit for bit.  DESIGN.md section 5.11 has the rules and the deviations from Spark.  The calls are asynchronous on `stream`, own
 * no memory, check every argument before any device call (SPRK_EINVAL) and report bad input through *error_key, which the caller sets
 * to ~0 first: the least (kind << 32 | row) by atomicMin, kind 1 = user id, 2 = item id out of range, 3 = rating not finite, 4 = the
 * corpus does not hold n_words words (the low word is the number found).
 *
 * sprk_item_sequences: the rows with rating >= 3.5f, per user in ascending (timestamp, input row): seq_offsets [n_users + 1],
 * seq_items (room for n_ratings, seq_offsets[n_users] written) and item_count [n_items] (an item's occurrences among the kept rows).
 *
 * sprk_item_walks: the graph route (generateTransitionMatrix + randomWalk).  The adjacent pairs (prev, next) of every sequence are
 * grouped per prev and sorted by next; sample_count walks of at most sample_length items are drawn in integers from a counter-based
 * generator (item2vec.py walks_host): the start is the item whose pairs hold pair number mulhi64(word, total), a step takes entry
 * mulhi64(word, row_total) of the current item's sorted pairs, an item without successors ends the walk.  walk_offsets
 * [sample_count + 1], walk_items (room for sample_count * sample_length).
 *
 * sprk_skipgram_fit: seq_offsets [n_seq + 1] / seq_items [n_seq_items] as above (or random walks of the same shape); item_vocab
 * [n_items] = an item's vocabulary index or -1; code_len [V], codes [V][40], points [V][40] = the Huffman tables
 * (item2vec.py vocabulary_host); n_words = the corpus' size after the items outside the vocabulary are dropped; init [V][init_stride],
 * exp_table [1000] float32 and loss_table [2][1000] float64 as item2vec.py computes them -- the device calls no transcendental.
 * Sequences are cut into sentences of max_sentence words.  An iteration walks the corpus in rounds of `round` consecutive positions
 * that all read the model as the round found it; a row's updates of one round are added in ascending (centre, context or depth) and
 * scaled by row_cap / n when n > row_cap of them meet.  Outputs: vectors [V][stride] (floats past D untouched), syn1 [V][D], *loss
 * (the mean table loss of every term at the full window under the final model).  D in [1, 64], window in [1, 16].
 * The workspace holds one 12-byte record (twice, for the sort) per (position, context) and (position, depth) pair:
 * sprk_skipgram_workspace_bytes, 16-byte aligned (0 for sizes the call rejects). */
size_t sprk_item_sequences_workspace_bytes(int64_t n_ratings, int32_t n_users, int32_t n_items);
int sprk_item_sequences(const int32_t* user_id, const int32_t* movie_id, const float* rating, const int64_t* timestamp, int64_t n_ratings,
                        int32_t n_users, int32_t n_items, int32_t* seq_offsets, int32_t* seq_items, int32_t* item_count,
                        uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);
size_t sprk_item_walks_workspace_bytes(int64_t n_seq_items, int32_t n_seq, int32_t n_items, int64_t sample_count, int32_t sample_length);
int sprk_item_walks(const int32_t* seq_offsets, const int32_t* seq_items, int64_t n_seq_items, int32_t n_seq, int32_t n_items,
                    int64_t sample_count, int32_t sample_length, uint64_t seed, int32_t* walk_offsets, int32_t* walk_items,
                    uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);
size_t sprk_skipgram_workspace_bytes(int64_t n_seq_items, int32_t n_seq, int32_t vocab_size, int64_t n_words, int32_t D, int32_t window, int32_t round);
int sprk_skipgram_fit(const int32_t* seq_offsets, const int32_t* seq_items, int64_t n_seq_items, int32_t n_seq,
                      const int32_t* item_vocab, int32_t n_items, int32_t vocab_size, int64_t n_words,
                      const int32_t* code_len, const uint8_t* codes, const int32_t* points,
                      const float* init, int32_t init_stride, const float* exp_table, const double* loss_table,
                      int32_t D, int32_t window, int32_t iters, double lr, int32_t round, int32_t row_cap, uint64_t seed, int32_t max_sentence,
                      float* vectors, int32_t stride, float* syn1, double* loss,
                      uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* ---- multi-GPU: the path's one collective (the reference has no distributed path) ----
 * Batch rows are sharded over one process per GPU, tables and weights replicated; every rank ends with all scores through ONE
 * all-gather of the per-rank score slices over RCCL / xGMI, enqueued on the caller's HIP stream (no host synchronisation).
 * RCCL is loaded at run time on first use.  Rank 0 calls sprk_comm_unique_id and hands the 128 bytes to the other ranks through
 * any host channel (the Python host uses the process group's store); every rank then calls sprk_comm_create (collective).
 * gathered = [world][count] floats, rank r's slice at offset r * count; in-place (local == gathered + rank * count) is allowed. */
#define SPRK_COMM_ID_BYTES 128
typedef struct sprk_comm_s* sprk_comm;
int sprk_comm_unique_id(uint8_t id[SPRK_COMM_ID_BYTES]);
int sprk_comm_create(const uint8_t id[SPRK_COMM_ID_BYTES], int32_t rank, int32_t world, sprk_comm* out);
int sprk_comm_allgather_scores(sprk_comm c, const float* local, float* gathered, size_t count, void* stream);
void sprk_comm_destroy(sprk_comm c);

/* The same exchange as direct peer writes over xGMI: every rank stores its slice straight into all peers'
 * receive buffers (one step on the point-to-point mesh instead of a ring's world-1 dependent hops), then waits for the peers'
 * arrival flags -- two kernels on the caller's stream, no host synchronisation, no RCCL.  Setup: every rank calls
 * sprk_peer_create (allocates its receive buffer [2 parities][world][slot_floats] + flags and returns the 64-byte IPC handle),
 * the handles travel through any host channel, every rank calls sprk_peer_connect with all of them (rank order).
 * sprk_peer_allgather_scores: local [count <= slot_floats] -> *gathered = this rank's receive buffer for this exchange,
 * [world][slot_floats] floats (rank r's slice at r * slot_floats), valid for work enqueued on `stream` until the exchange after
 * the next one on this communicator; one exchange in flight per communicator.  A slice that does not arrive within the deadline
 * (2 s; SPRK_PEER_TIMEOUT_MS) raises a flag that sprk_peer_check (synchronises the stream) reports as SPRK_EHIP. */
#define SPRK_PEER_HANDLE_BYTES 64
typedef struct sprk_peer_s* sprk_peer;
int sprk_peer_create(int32_t rank, int32_t world, size_t slot_floats, uint8_t handle_out[SPRK_PEER_HANDLE_BYTES], sprk_peer* out);
int sprk_peer_connect(sprk_peer c, const uint8_t* handles /* [world][SPRK_PEER_HANDLE_BYTES] */);
int sprk_peer_allgather_scores(sprk_peer c, const float* local, size_t count, const float** gathered, void* stream);
int sprk_peer_check(sprk_peer c, void* stream);
const char* sprk_peer_memory_kind(sprk_peer c);   /* "uncached" | "fine-grained" | "default": how the receive buffer was allocated */
void sprk_peer_destroy(sprk_peer c);

/* [r4] BASELINE.json configs[3]: "DeepFM emb_dim=64, 138 k-movie x 27 M-row synthetic table, ROW-SHARDED across 8 x MI355X" (the
 * reference holds its tables as ordinary tf.Variables of one process -- embedding_column, DeepFM.py:54-60 -- so there is no
 * reference interface to mirror; SURVEY.md section 8(e) names the variant).  A sprk_vtable is an embedding table of rows_total rows
 * whose rows [r S, (r + 1) S) live in rank r's HBM and which EVERY rank sees as one contiguous device array: HIP virtual memory maps
 * the peers' allocations into one reserved range, so the fused kernels gather table[id] unchanged and a row another GPU owns is
 * loaded over the xGMI link between the two -- no collective, no staging pass (the textbook form is an all-to-all of ids and one
 * of rows in front of every forward).  Set-up, once: every rank calls sprk_vtable_create (collective in effect: same geometry
 * everywhere; allocates and zero-fills its own shard), sprk_vtable_export (a POSIX file descriptor of that shard, to be sent to the
 * other ranks of the node with SCM_RIGHTS -- sparrowrecsys_amd/dist.py ShardedTable does it over Unix sockets) and, for each peer's
 * descriptor, sprk_vtable_import.  sprk_vtable_info: the base of the whole table (rank r's rows start at r * shard_rows), rows per
 * rank (ceil(rows_total / world) rounded up so that shards are whole allocation granules), shards mapped so far.  row_bytes must be a
 * multiple of 16.  The table outlives every engine that was given it through sprk_upload_external. */
typedef struct sprk_vtable_s* sprk_vtable;
int sprk_vtable_create(int64_t rows_total, int32_t row_bytes, int32_t world, int32_t rank, sprk_vtable* out);
int sprk_vtable_export(sprk_vtable v, int32_t* fd_out);
int sprk_vtable_import(sprk_vtable v, int32_t peer_rank, int32_t fd);
int sprk_vtable_info(sprk_vtable v, void** base, int64_t* shard_rows, int32_t* ranks_mapped);
void sprk_vtable_destroy(sprk_vtable v);

/* [r4] sprk_upload without the copy: the slot READS `bytes` of caller-owned device memory at dev_ptr (16-byte aligned, in the
 * slot's device layout -- a table as [vocab + 1][Dp] floats with its last row zero) for as long as the handle lives; the engine
 * never frees it.  For tables that are already where they should be: a sprk_vtable, or a 6.9 GB tensor that sprk_upload would
 * duplicate (embedding_column's variable, DeepFM.py:55,60). */
int sprk_upload_external(sprk_handle h, int32_t slot, const void* dev_ptr, size_t bytes);

/* model.fit for the graphs "embedding rows + numerics -> Dense/ReLU stack -> one sigmoid" (NeuralCF arch 1, EmbeddingMLP), with Adam as
 * TensorFlow's ApplyAdam computes it; sparrowrecsys_amd/trainer.py's train_host is the definition of every bit.
 * sprk_train_model: the id columns (vocab; genre != 0: ids may be -1 = no row), the width of every table row, per input row k of the first
 * Dense kernel the id column it comes from (xcol, -1 = a numeric) and its place in the table row or among the numerics (xsub), the hidden
 * widths.  params / m / v: one float vector each -- the tables in column order ([vocab][emb_dim]), then per hidden layer its kernel
 * ([in][out]) and bias, then the head's -- trained in place.  ids [n][n_cols] int32, dense [n][n_dense], labels [n]; order: NULL or a
 * permutation of 0 .. n - 1 (step b takes positions [b batch, (b + 1) batch) of it); alphas [epochs x ceil(n / batch)]: Adam's lr_t per
 * step, a device array like every other pointer; p [epochs][n]: every epoch's training probabilities by position.  Before the first step:
 * an id outside its vocabulary (kind 1), a numeric (2) or a label (3) that is not finite gives *error_key = kind << 32 | row, the least
 * such key (the caller presets ~0), and no parameter changes.  The whole fit is enqueued on `stream`: no synchronisation.
 * n x n_cols must stay below 2^31 - 1 (the schedule's unsigned offsets); tile x (n_x + the widths + 2 x the widest) floats must fit 160 KB. */
#define SPRK_TRAIN_MAX_COLS 16
#define SPRK_TRAIN_MAX_LAYERS 8
#define SPRK_TRAIN_MAX_X 256
#define SPRK_TRAIN_MAX_WIDTH 256
typedef struct {
    int32_t n_cols, n_dense, emb_dim, n_x, n_layers;
    int32_t vocab[SPRK_TRAIN_MAX_COLS], genre[SPRK_TRAIN_MAX_COLS];
    int32_t width[SPRK_TRAIN_MAX_LAYERS];
    int32_t xcol[SPRK_TRAIN_MAX_X], xsub[SPRK_TRAIN_MAX_X];
} sprk_train_model;
size_t sprk_train_workspace_bytes(const sprk_train_model* model, int64_t n, int32_t batch, int32_t tile);
int sprk_train_fit(const sprk_train_model* model, const int32_t* ids, const float* dense, const float* labels, const int32_t* order, int64_t n,
                   int32_t batch, int32_t tile, int32_t epochs, const float* alphas, float one_minus_beta1, float one_minus_beta2, float epsilon,
                   float* params, float* m, float* v, float* p, uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* model.fit for DeepFM_v2: first order + sum-of-squares FM cross over per-field Dense projections + a deep stack, one sigmoid; the rules of the
 * trainer above, sparrowrecsys_amd/trainer_fm.py's train_host is the definition of every bit.
 * sprk_train_fm_model: the fields (vocab; genre != 0: ids may be -1 = no row; fo_off: the field's first row in fo_cat/kernel -- the blocks tile its
 * rows), order[g] = the field of group g < n_order (distinct; the numerics are the last group), emb_dim, proj_dim, the hidden widths.
 * params / m / v: one float vector each -- the emb/ tables in field order ([vocab][emb_dim]), fo_cat/kernel, fo_cat/bias, fo_num/kernel,
 * fo_num/bias, per group proj kernel ([in][proj_dim]) and bias (the numerics' last), per hidden layer kernel ([in][out]) and bias, the head's
 * kernel ([1 + proj_dim + last width]) and bias -- trained in place.  Every other argument, the error word and the enqueue-only contract are
 * those of the fit above.  n x n_fields must stay below 2^31 - 1; one workgroup's LDS (trainer_fm.lds_bytes) must fit 160 KB.
 * A NaN that reaches p, a parameter, m or v is stored as 0x7fc00000. */
#define SPRK_TRAIN_FM_MAX_FIELDS 8
#define SPRK_TRAIN_FM_MAX_LAYERS 8
#define SPRK_TRAIN_FM_MAX_PROJ 128
#define SPRK_TRAIN_FM_MAX_FLAT 1024
#define SPRK_TRAIN_FM_MAX_WIDTH 256
#define SPRK_TRAIN_FM_MAX_IN 256
typedef struct {
    int32_t n_fields, n_dense, emb_dim, proj_dim, n_order, n_layers;
    int32_t vocab[SPRK_TRAIN_FM_MAX_FIELDS], genre[SPRK_TRAIN_FM_MAX_FIELDS], fo_off[SPRK_TRAIN_FM_MAX_FIELDS], order[SPRK_TRAIN_FM_MAX_FIELDS];
    int32_t width[SPRK_TRAIN_FM_MAX_LAYERS];
} sprk_train_fm_model;
size_t sprk_train_fm_workspace_bytes(const sprk_train_fm_model* model, int64_t n, int32_t batch, int32_t tile);
int sprk_train_fm_fit(const sprk_train_fm_model* model, const int32_t* ids, const float* dense, const float* labels, const int32_t* order, int64_t n,
                      int32_t batch, int32_t tile, int32_t epochs, const float* alphas, float one_minus_beta1, float one_minus_beta2, float epsilon,
                      float* params, float* m, float* v, float* p, uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* Training DIN: an attention unit ([h - c | h | c | h c] -> Dense -> PReLU(alpha[slot]) -> Dense(1) -> sigmoid) shared over hist_len history
 * slots, weighted sum pooling, a PReLU tail, one sigmoid; the rules of the trainers above, sparrowrecsys_amd/trainer_din.py's train_host is the
 * definition of every bit.  sprk_train_din_model: the id columns (vocab; genre != 0: ids may be -1 = no row; table:
 * the table the column reads -- column 0 is the candidate, columns 1 .. hist_len the history, all of table 0; tables are numbered 0 .. without a
 * gap and the columns of one table agree in vocab and genre), emb_dim, att_hidden, per input row k of fc0 its source xsrc (an id column
 * outside the history, -1 = a numeric, -2 = the pooled vector) and xsub (the element), the tail's widths.  params / m / v: one float vector each
 * -- the tables in table order ([vocab][emb_dim]), att0 kernel ([4 emb_dim][att_hidden]) and bias, the attention PReLU's alpha
 * ([hist_len][att_hidden]), att1 kernel and bias, per tail layer kernel ([in][out]), bias and alpha, the head's kernel and bias -- trained in place.
 * Every other argument, the error word and the enqueue-only contract are those of sprk_train_fit.  n x n_cols must stay below 2^31 - 1 and
 * batch at or below 2^28 (a schedule key holds position x 16 + column in 32 bits); one workgroup's LDS (trainer_din.lds_bytes) must fit 160 KB. */
#define SPRK_TRAIN_DIN_MAX_COLS 16
#define SPRK_TRAIN_DIN_MAX_LAYERS 8
#define SPRK_TRAIN_DIN_MAX_X 256
#define SPRK_TRAIN_DIN_MAX_WIDTH 256
#define SPRK_TRAIN_DIN_MAX_EMB 64
typedef struct {
    int32_t n_cols, n_dense, emb_dim, hist_len, att_hidden, n_x, n_layers;
    int32_t vocab[SPRK_TRAIN_DIN_MAX_COLS], genre[SPRK_TRAIN_DIN_MAX_COLS], table[SPRK_TRAIN_DIN_MAX_COLS];
    int32_t width[SPRK_TRAIN_DIN_MAX_LAYERS];
    int32_t xsrc[SPRK_TRAIN_DIN_MAX_X], xsub[SPRK_TRAIN_DIN_MAX_X];
} sprk_train_din_model;
size_t sprk_train_din_workspace_bytes(const sprk_train_din_model* model, int64_t n, int32_t batch, int32_t tile);
int sprk_train_din_fit(const sprk_train_din_model* model, const int32_t* ids, const float* dense, const float* labels, const int32_t* order, int64_t n,
                       int32_t batch, int32_t tile, int32_t epochs, const float* alphas, float one_minus_beta1, float one_minus_beta2, float epsilon,
                       float* params, float* m, float* v, float* p, uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* Training DIEN: a Keras GRU (reset_after, gates z | r | h) over hist_len history slots that keeps its state and repeats its output at a slot whose
 * id is 0, a per-slot gate sigmoid(Dense(1)(sigmoid(Dense(att_hidden)(g_t c)))) -- no PReLU and no softmax in the attention --, the reference's AUGRU
 * (per gate r, z, h: Dense_out(Dense_in(g_t) + hid @ hid kernel); hs <- (1 - a_t r_t) hs + a_t r_t h~), a PReLU tail, one sigmoid; tanh is
 * 2 sigmoid_def(2 z) - 1; the rules of the trainers above, sparrowrecsys_amd/trainer_dien.py's train_host is the definition of every bit (DESIGN.md
 * section 5.22).  sprk_train_dien_model: sprk_train_din_model's fields with the same meaning, where xsrc -2 names the AUGRU's last state and column
 * 0's genre must be 0.  params / m / v: one float vector each -- the tables in table order ([vocab][emb_dim]), the GRU's kernel and recurrent kernel
 * ([emb_dim][3 emb_dim] each) and bias ([2][3 emb_dim]), att0 kernel ([emb_dim][att_hidden]) and bias, att1 kernel and bias, per gate r, z, h its
 * in kernel ([emb_dim][emb_dim]), in bias, hid kernel, out kernel and out bias, the AUGRU's initial state ([emb_dim]), per tail layer kernel
 * ([in][out]), bias and alpha, the head's kernel and bias -- trained in place.  Every other argument, the error word and the enqueue-only contract
 * are those of sprk_train_fit; the workspace is laid out as sprk_train_din_fit's.  n x n_cols must stay below 2^31 - 1 and batch at or below 2^28;
 * one workgroup's LDS (trainer_dien.lds_bytes) must fit 160 KB. */
typedef struct {
    int32_t n_cols, n_dense, emb_dim, hist_len, att_hidden, n_x, n_layers;
    int32_t vocab[SPRK_TRAIN_DIN_MAX_COLS], genre[SPRK_TRAIN_DIN_MAX_COLS], table[SPRK_TRAIN_DIN_MAX_COLS];
    int32_t width[SPRK_TRAIN_DIN_MAX_LAYERS];
    int32_t xsrc[SPRK_TRAIN_DIN_MAX_X], xsub[SPRK_TRAIN_DIN_MAX_X];
} sprk_train_dien_model;
size_t sprk_train_dien_workspace_bytes(const sprk_train_dien_model* model, int64_t n, int32_t batch, int32_t tile);
int sprk_train_dien_fit(const sprk_train_dien_model* model, const int32_t* ids, const float* dense, const float* labels, const int32_t* order, int64_t n,
                        int32_t batch, int32_t tile, int32_t epochs, const float* alphas, float one_minus_beta1, float one_minus_beta2, float epsilon,
                        float* params, float* m, float* v, float* p, uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* Training Wide&Deep: EmbeddingMLP's graph (sprk_train_fit's) plus a wide term in the head whose parameter row is FingerprintCat64(0xDECAFCAFFE,
 * ids[cross_a], ids[cross_b]) mod cross_buckets; the rules of the trainers above, sparrowrecsys_amd/trainer_wide.py's train_host is the definition
 * of every bit.  sprk_train_wide_model: sprk_train_model's fields, where the LAST id column (cross_b = n_cols - 1) has a
 * vocabulary and no table and no input row names it, and cross_a < cross_b names a column with a table; cross_dim == 0: the cross is an indicator
 * and its cross_buckets weights are rows [H, H + cross_buckets) of the head's kernel (H = the last hidden width); cross_dim > 0: the cross reads a
 * table [cross_buckets][cross_dim] of its own and the head's kernel has H + cross_dim rows.  params / m / v: one float vector each -- the tables of
 * columns 0 .. n_cols - 2 ([vocab][emb_dim]), per hidden layer its kernel ([in][out]) and bias, the head's BIAS, the head's kernel, then (cross_dim
 * > 0) the cross table -- trained in place.  Every other argument, the error word and the enqueue-only contract are those of sprk_train_fit.
 * n x n_cols and (all tables' rows + cross_buckets) must stay below 2^31 - 1; tile x (n_x + the widths + 2 x the widest + cross_dim) floats must
 * fit 160 KB. */
#define SPRK_TRAIN_WIDE_MAX_CROSS_DIM 64
typedef struct {
    int32_t n_cols, n_dense, emb_dim, n_x, n_layers;
    int32_t vocab[SPRK_TRAIN_MAX_COLS], genre[SPRK_TRAIN_MAX_COLS];
    int32_t width[SPRK_TRAIN_MAX_LAYERS];
    int32_t xcol[SPRK_TRAIN_MAX_X], xsub[SPRK_TRAIN_MAX_X];
    int32_t cross_a, cross_b, cross_buckets, cross_dim;
} sprk_train_wide_model;
size_t sprk_train_wide_workspace_bytes(const sprk_train_wide_model* model, int64_t n, int32_t batch, int32_t tile);
int sprk_train_wide_fit(const sprk_train_wide_model* model, const int32_t* ids, const float* dense, const float* labels, const int32_t* order, int64_t n,
                        int32_t batch, int32_t tile, int32_t epochs, const float* alphas, float one_minus_beta1, float one_minus_beta2, float epsilon,
                        float* params, float* m, float* v, float* p, uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* trainer_pair.fit for the pair-dot DeepFM (the reference's DeepFM.py): first-order weights that are rows of the head's kernel, n_pairs explicit dots
 * of FM table rows, a deep stack over deep-only tables (or the FM tables: shared != 0) and the numerics, one sigmoid; the rules of the trainer above,
 * sparrowrecsys_amd/trainer_pair.py's train_host is the definition of every bit.
 * sprk_train_pair_model: the fields (vocab; genre != 0: ids may be -1 = no row; fo_off: the field's first row in the head's kernel -- the blocks tile
 * its first sum(vocab) rows), the pairs (pair_a[p], pair_b[p]: field indices, the same one twice is legal), deep_col[j] = the field of deep table j
 * (distinct), the hidden widths, and per row k < n_x of the first deep kernel xsrc[k] = the deep table it reads (-1: a numeric) and xsub[k] = the
 * element of that table's row or the numeric's index: every element of every deep table's row and every numeric once, n_x = n_deep emb_dim + n_dense.
 * params / m / v: one float vector each -- the FM tables in field order ([vocab][emb_dim]), the deep tables in deep_col order (absent when shared),
 * per hidden layer its kernel ([in][out]) and bias, the head's BIAS, then the head's kernel ([sum(vocab) + n_pairs + last width]) -- trained in
 * place.  Every other argument, the error word and the enqueue-only contract are those of sprk_train_fit.  n x n_fields must stay below 2^31 - 1;
 * one workgroup's LDS (trainer_pair.lds_bytes) must fit 160 KB.  A NaN that reaches p, a parameter, m or v is stored as 0x7fc00000. */
#define SPRK_TRAIN_PAIR_MAX_FIELDS 8
#define SPRK_TRAIN_PAIR_MAX_PAIRS 32
#define SPRK_TRAIN_PAIR_MAX_LAYERS 8
#define SPRK_TRAIN_PAIR_MAX_WIDTH 256
#define SPRK_TRAIN_PAIR_MAX_X 256
#define SPRK_TRAIN_PAIR_MAX_DIM 64
typedef struct {
    int32_t n_fields, n_dense, emb_dim, n_pairs, n_deep, shared, n_x, n_layers;
    int32_t vocab[SPRK_TRAIN_PAIR_MAX_FIELDS], genre[SPRK_TRAIN_PAIR_MAX_FIELDS], fo_off[SPRK_TRAIN_PAIR_MAX_FIELDS];
    int32_t pair_a[SPRK_TRAIN_PAIR_MAX_PAIRS], pair_b[SPRK_TRAIN_PAIR_MAX_PAIRS];
    int32_t deep_col[SPRK_TRAIN_PAIR_MAX_FIELDS];
    int32_t width[SPRK_TRAIN_PAIR_MAX_LAYERS];
    int32_t xsrc[SPRK_TRAIN_PAIR_MAX_X], xsub[SPRK_TRAIN_PAIR_MAX_X];
} sprk_train_pair_model;
size_t sprk_train_pair_workspace_bytes(const sprk_train_pair_model* model, int64_t n, int32_t batch, int32_t tile);
int sprk_train_pair_fit(const sprk_train_pair_model* model, const int32_t* ids, const float* dense, const float* labels, const int32_t* order, int64_t n,
                        int32_t batch, int32_t tile, int32_t epochs, const float* alphas, float one_minus_beta1, float one_minus_beta2, float epsilon,
                        float* params, float* m, float* v, float* p, uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);

/* trainer_tower.fit for the two-tower NeuralCF (the reference's neural_cf_model_2): a Dense/ReLU tower over the movie row, one of the same widths over
 * the user row, their dot -- the float32 dot of sprk_als_predict: from 0.0f in index order, every product and sum rounded on its own --, one Dense unit
 * and a sigmoid; the rules of the trainer above, sparrowrecsys_amd/trainer_tower.py's train_host is the definition of every bit (DESIGN.md section
 * 5.23).  sprk_train_tower_model: emb_dim, the hidden widths (both towers') and vocab = {movieId's, userId's}.  ids = [n][2] (movieId, userId); there
 * are no numerics, so sprk_train_tower_fit takes sprk_train_fit's arguments less `dense`.  params / m / v: one float vector each -- the movie table,
 * the user table ([vocab][emb_dim]), per layer of the item tower its kernel ([in][out]) and bias, the same of the user tower, the head's kernel, the
 * head's bias -- trained in place.  The error word and the enqueue-only contract are those of sprk_train_fit.  n x 2 must stay below 2^31 - 1; one
 * workgroup's LDS (trainer_tower.lds_bytes) must fit 160 KB.  A NaN that reaches p, a parameter, m or v is stored as 0x7fc00000.
 * sprk_tower_rows: every row of table `side` (0 = movieId through the item tower, 1 = userId through the user tower) of such a parameter vector through
 * its tower, by the fit's own forward statements: out[row x out_stride + j], j < the last width; the floats between are left alone.  `tile` rows per
 * workgroup pass (2 x tile x the widest of emb_dim and the layers, in floats rounded up to 4, must fit 160 KB).  Enqueued on `stream`; SPRK_EINVAL
 * before any device call for a bad argument. */
#define SPRK_TRAIN_TOWER_MAX_LAYERS 8
#define SPRK_TRAIN_TOWER_MAX_WIDTH 256
#define SPRK_TRAIN_TOWER_MAX_DIM 128
typedef struct {
    int32_t emb_dim, n_layers;
    int32_t vocab[2];
    int32_t width[SPRK_TRAIN_TOWER_MAX_LAYERS];
} sprk_train_tower_model;
size_t sprk_train_tower_workspace_bytes(const sprk_train_tower_model* model, int64_t n, int32_t batch, int32_t tile);
int sprk_train_tower_fit(const sprk_train_tower_model* model, const int32_t* ids, const float* labels, const int32_t* order, int64_t n,
                         int32_t batch, int32_t tile, int32_t epochs, const float* alphas, float one_minus_beta1, float one_minus_beta2, float epsilon,
                         float* params, float* m, float* v, float* p, uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream);
int sprk_tower_rows(const sprk_train_tower_model* model, const float* params, int32_t side, int32_t tile, float* out, int64_t out_stride, void* stream);

const char* sprk_last_error(void);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SPARROW_HIP_H */
