// host_engine.h -- struct sprk_engine: everything a finalized handle owns.
// Part of sparrow_hip.hip (one translation unit); included there, not compilable on its own.
// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// What sprk_forward launches for one batch, and what sprk_din_pool runs (also the first launch of the two-launch DIN / DIEN forward).
// sprk_finalize sets both once, after the set-ups (choose_route, api_engine.h); everything after finalize switches on them.
enum class Route { Tile, V2Joint, Rows, Pairs, MlpRows, DinTail, DinFused, DienFused };
enum class Stage { None, DinPool, DinCols, DinFusedAttn, DienSeq, DienSeqMfma };

// One function-pointer type per kernel signature.  A set-up picks the instantiation ONCE (its variant table or selector), sets the LDS limit on
// exactly that pointer (set_max_lds) and the launch paths hand it to hipLaunchKernelGGL: the compiler checks every launch against the kernel.
typedef void (*V2JKernel)(const V2JRun, const int*, const float*, float*, int, int*, const float*);        // k_deepfm_v2_joint, k_deepfm_v2_joint1
typedef void (*V2JManyKernel)(const V2JRun, const V2JMany, int, int*, const float*);
typedef void (*V2JManyTabKernel)(const V2JRun, const V2JManyTab, int, int*, const float*);                 // k_deepfm_v2_joint_many_tab
typedef void (*RowsKernel)(const RowsRun, const int*, const float*, float*, int, int*, const float*);       // k_rows_chain, k_rows_chain1
typedef void (*RowsManyKernel)(const RowsRun, const RowsMany, int, int*, const float*);
typedef void (*V1Kernel)(const V1Run, const int*, const float*, float*, int, int*);                         // k_deepfm_pairs, k_deepfm_pairs1
typedef void (*V1ManyKernel)(const V1Run, const V1Many, int, int*);
typedef void (*MlpRowsKernel)(const MlpRowsRun, const int*, const float*, float*, int, int*, const float*);
typedef void (*MlpRowsManyKernel)(const MlpRowsRun, const MlpRowsMany, int, int*, const float*);
typedef void (*DinTailKernel)(const DinTailRun, const int*, const float*, const float*, float*, int, int*, const float*, const DinTailMany);
typedef void (*DinColsKernel)(const DinColsRun, const int*, float*, float*, int, int*, const DinColsOne);
typedef void (*DinColsManyKernel)(const DinColsRun, const int*, float*, float*, int, int*, const DinColsMany);
typedef void (*DinFusedKernel)(const DinFusedRun, const int*, const float*, float*, float*, int, int*, const DinFusedOne);
typedef void (*DinFusedManyKernel)(const DinFusedRun, const int*, const float*, float*, float*, int, int*, const DinFusedMany);
typedef void (*DienSeqKernel)(const DienRun, const int*, float*, int, int*);                                // k_dien_seq, k_dien_seq_mfma
typedef void (*DienFusedKernel)(const DienRun, const DinTailRun, const int*, const float*, float*, int, int*, const float*, float*);
// k_din_attn_cols<KC, MB> and k_din_fused<KC, MB, TAIL> for one KC: one batch, several batches
struct DinColsKernels { DinColsKernel one; DinColsManyKernel many; };
struct DinFusedKernels { DinFusedKernel one; DinFusedManyKernel many; };
// the one owner of a kernel's dynamic-LDS limit
template <class Kernel> static int set_max_lds(Kernel k, size_t bytes) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return SPRK_OK;
}

struct sprk_engine {
    sprk_plan plan;
    std::vector<void*> slot_ptr;
    std::vector<size_t> slot_bytes;
    std::vector<char> slot_external;      // [r4] sprk_upload_external: the slot reads caller-owned device memory (never freed here)
    DevPlan* dev_plan = nullptr;
    int* dev_err = nullptr;
    bool finalized = false;
    Route route = Route::Tile;
    Stage stage = Stage::None;
    int device = 0;
    int num_cus = 256;
    int buf_stride[SPRK_MAX_BUFS] = {0, 0, 0};
    int buf_base[SPRK_MAX_BUFS] = {0, 0, 0};
    size_t tile_lds_bytes = 0;
    int ids_base = 0;              // float offset of the tile's ids block inside the tile kernel's LDS
    std::vector<int> idc;          // ids columns read by the gather segments (compact staging order)
    int tile_grid_cap = 0;
    // sprk_forward_many fan-out: independent batches alternate over helper streams (hardware queues), so that one
    // kernel's dispatch / drain (3.3 us even for an empty kernel in a dependent launch chain) overlaps its neighbours
    int many_streams = 0;
    hipStream_t many_stream[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t many_fork = nullptr, many_join[4] = {nullptr, nullptr, nullptr, nullptr};
    // register-chained pairwise-dot DeepFM (k_deepfm_pairs); -1 = not set up
    int v1_variant = -1;
    V1Kernel v1_kernel = nullptr;         // the split-f16 or the f32 form, as the set-up's fragments came out
    V1Kernel v1_one_kernel = nullptr;     // one-batch launches use k_deepfm_pairs1 (one task per wave, four waves per SIMD); nullptr: the looped kernel
    V1ManyKernel v1_many_kernel = nullptr;
    V1Run v1_run;
    // DenseFeatures -> Dense -> Dense -> Dense(1) graphs with every embedding column folded through the first layer, genre tables
    // in LDS (k_mlp_rows); -1 = not set up
    int mlp_rows_nbig = -1;
    MlpRowsRun mlp_rows_run;
    MlpRowsKernel mlp_rows_kernel = nullptr;
    MlpRowsManyKernel mlp_rows_many_kernel = nullptr;   // [r6] several batches per launch (nullptr: batch by batch)
    float* mlp_rows_image = nullptr;
    float* mlp_rows_small = nullptr;
    size_t mlp_rows_lds = 0;
    // register-chained DIN tail (k_din_tail); -1 = not set up
    int din_tail_variant = -1;
    DinTailRun din_tail_run;
    DinTailKernel din_tail_kernel = nullptr, din_tail_many_kernel = nullptr;   // the f32, split-f16 or raw-row (UNF) form the set-up reached
    int din_tail_waves = 0;               // waves per workgroup of that form (16 with raw embedding rows for emb_dim <= 16)
    float* din_tail_image = nullptr;
    // DIN launch geometry
    int din_ms = 0;
    size_t din_lds_bytes = 0;
    int din_grid_cap = 0;
    DienRun dien_run{};
    float* dien_frag = nullptr;          // k_dien_seq_mfma's fragment image (NULL: the lane-per-sample kernel)
    size_t dien_frag_floats = 0;
    DienSeqKernel dien_seq_kernel = nullptr;   // k_dien_seq_mfma or k_dien_seq for the plan's emb_dim, as h->stage says (choose_route)
    SprkTuning tune;               // the environment's switches as sprk_finalize found them
    // attention on k_din_attn_cols (16 samples per MFMA tile, static weight operand; k_din_cols.h); din_cols_kc = 0: not set up
    int din_cols_kc = 0;
    DinColsRun din_cols_run;
    DinColsKernels din_cols_kernels{};
    // the whole DIN forward in one launch (k_din_fused: attention + pooling + tail; k_din_fused.h)
    bool din_fused = false;        // TAIL instantiations usable (attention on the cols formulation AND the 128 / 64 tail recognised)
    bool din_fused_attn = false;   // TAIL = false instantiations replace k_din_attn_cols (sprk_din_pool, the unfused two-launch path)
    DinFusedRun din_fused_run;
    DinFusedKernels din_fused_kernels[2]{};   // k_din_fused for din_cols_kc: [0] pooled vectors out (the attention stage alone), [1] scores out (TAIL)
    DinFusedKernel din_fused_att_kernel = nullptr;   // ... attention weights out as well
    float* din_fused_image = nullptr;
    bool dien_fused = false;       // DIEN in one launch (k_dien_fused.h): dien_frag AND the 128 / 64 tail on raw split rows
    DienFusedKernel dien_fused_kernel = nullptr;
    size_t dien_fused_lds = 0;
    // DeepFM_v2: the parsed plan's shape in kV2Variants (match_v2_chain); -1 = no folded form
    int v2_variant = -1;
    bool v2_rows_ok = false;       // [r6] the parsed DeepFM_v2 plan also fits k_rows_chain (where it goes when the joint set-up refuses it)
    V2Args v2;                     // (w1[] in first-order order, the order of fo_col[] / fo_vocab[], wherever it is read)
    const float* v2_w1_grp[V2_MAX_FIELDS] = {};   // the same first-order weights in embedding-group order (host only: the folded set-up)
    V2Run v2run;
    int v2_grid_cap = 0;
    float* v2_image = nullptr;     // pre-packed LDS weight image (device)
    float* v2_fo_all = nullptr;    // concatenated first-order weight blocks (device)
    float* v2_folded = nullptr;    // projected tables of all fields, back to back (device)
    size_t v2_fo_floats = 0;
    // ... with the small-vocabulary fields folded into one joint table (k_deepfm_v2_joint); -1 = not set up
    int v2j_variant = -1;
    V2JKernel v2j1_kernel = nullptr;      // k_deepfm_v2_joint1 (one task per wave), HOIST or not; nullptr = shape not available
    float* v2j1_image = nullptr;          // its LDS image
    size_t v2j1_lds_bytes = 0;
    int v2j1_waves = 8;                   // waves per workgroup of the form chosen (V2J1_WAVES_OF)
    int many_batches = 1;                 // sprk_forward_many: batches scored per launch (sprk_set_many_batches)
    // "one row per id" chain (k_rows_chain): DeepFM_v2 with projections wider than 16 (the reference's Dense(64)) and NeuralCF; -1 = not set up
    // (the kernels stay in kRowsVariants[rows_variant]: one-batch launches of up to V2J1_MAX_TASKS tasks use fn_one = k_rows_chain1)
    int rows_variant = -1;
    bool rows_from_v2 = false;            // set by match_v2_chain: h->v2 holds the parsed DeepFM_v2 plan, tables still to build
    int rows_g_emb = 0;
    RowsRun rows_run;
    float* rows_tab = nullptr;            // big fields' rows {P | Q}
    float* rows_scal = nullptr;           // big fields' per-id scalars
    float* rows_small = nullptr;          // small fields' LDS rows (device image)
    float* rows_image = nullptr;          // weight image
    size_t rows_lds_bytes = 0;
    int n_acc_folded = 0;                 // embedding columns folded into the first Dense layer (fold_first_dense)
    size_t derived_bytes = 0;             // device memory of tables DERIVED at finalize (folded rows, split halfs, per-id terms)
    V2JRun v2j_run;
    float* v2j_tab = nullptr;      // small fields' LDS rows (device image)
    size_t v2j_lds_bytes = 0;
    float* v2j_big = nullptr;      // HALF: split-half rows of the big fields (device)
    // The per-batch pointer table of a one-launch sprk_forward_many call (k_deepfm_v2_joint_many_tab; api_forward.h: launch_v2j_table).
    // `stage` is the pinned host copy the upload reads and, afterwards, the record of what `dev` holds: a call whose pointers equal the
    // table uploaded last on the same stream (a replayed prepared run) launches without an upload.  Two slots in alternation, and `busy`
    // is recorded behind every launch that reads a slot: a new table waits for the slot's last reader before it overwrites either copy.
    struct V2JTable {
        V2JBatch* stage = nullptr;
        V2JBatch* dev = nullptr;
        size_t cap = 0;                   // entries both copies hold
        size_t n = 0;                     // entries of the table in them (0: none yet)
        hipStream_t stream = nullptr;     // the stream the upload was enqueued on
        hipEvent_t busy = nullptr;
        bool used = false;                // `busy` has been recorded
    };
    V2JTable v2j_table[2];
    int v2j_table_last = -1;              // the slot uploaded last
    // every device allocation of finalize (dev_alloc / table_alloc below); the pointers above are views into them.  vmm_size != 0: a
    // hipMemCreate allocation mapped at a reserved range, else hipMalloc's
    struct DevAlloc { void* p; size_t vmm_size; hipMemGenericAllocationHandle_t handle; };
    std::vector<DevAlloc> allocs;
};

// Device memory of an engine: dev_alloc (hipMalloc) and table_alloc record every allocation in h->allocs, dev_free releases one early
// (a set-up that refuses after it allocated), sprk_destroy all the others.
static void release(const sprk_engine::DevAlloc& a) {
    if (!a.vmm_size) { (void)hipFree(a.p); return; }
    (void)hipMemUnmap(a.p, a.vmm_size);
    (void)hipMemRelease(a.handle);
    (void)hipMemAddressFree(a.p, a.vmm_size);
}
template <class T> static int dev_alloc(sprk_engine* h, T** out, size_t bytes) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    h->allocs.push_back(sprk_engine::DevAlloc{p, 0, nullptr});
    *out = static_cast<T*>(p);
    return SPRK_OK;
}
static void dev_free(sprk_engine* h, void* p) {
    if (!p) return;
    for (size_t i = 0; i < h->allocs.size(); ++i)
        if (h->allocs[i].p == p) {
            release(h->allocs[i]);
            h->allocs.erase(h->allocs.begin() + (long)i);
            return;
        }
}
// an uploaded slot's own copy (a slot of sprk_upload_external reads the caller's memory: not freed here)
static void free_slot(sprk_engine* h, size_t slot) {
    if (h->slot_ptr[slot] && !h->slot_external[slot]) (void)hipFree(h->slot_ptr[slot]);
}

// [r6, VERDICT r05 item 4 (i)] A gather table the engine derives at finalize (folded / split rows).  From 256 MB on -- beyond the Infinity Cache,
// where every row of a batch is its own HBM access AND its own translation -- it is ONE physical allocation (hipMemCreate) mapped at a 1 GB-aligned
// virtual address, not hipMalloc's memory: scripts/ubench/row_gather.hip (`... vmm`) measures the random 128-byte-row gather over a 3.2 GB table
// at 7.15 instead of 7.46 us per 65 536 x 3 rows (8.37 instead of 8.69 with the fused kernel's staging and LDS traffic around it;
// profiles/r06/experiments/r06_15): the one handle lets the driver describe the range with larger page-table fragments.  SPRK_VMM_TABLES=0, any
// failure of the API, or a smaller table: hipMalloc.
template <class T> static int table_alloc(sprk_engine* h, T** out, size_t bytes) {
    *out = nullptr;
    if (h->tune.vmm_tables && bytes >= ((size_t)256 << 20)) {
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = h->device;
        size_t gran = 0;
        if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) == hipSuccess) {
            if (gran < ((size_t)2 << 20)) gran = (size_t)2 << 20;
            const size_t total = (bytes + gran - 1) / gran * gran;
            void* va = nullptr;
            hipMemGenericAllocationHandle_t hnd;
            if (hipMemAddressReserve(&va, total, (size_t)1 << 30, nullptr, 0) == hipSuccess) {
                if (hipMemCreate(&hnd, total, &prop, 0) == hipSuccess) {
                    hipMemAccessDesc acc = {};
                    acc.location = prop.location;
                    acc.flags = hipMemAccessFlagsProtReadWrite;
                    if (hipMemMap(va, total, 0, hnd, 0) == hipSuccess) {
                        if (hipMemSetAccess(va, total, &acc, 1) == hipSuccess) {
                            h->allocs.push_back(sprk_engine::DevAlloc{va, total, hnd});
                            *out = static_cast<T*>(va);
                            return SPRK_OK;
                        }
                        (void)hipMemUnmap(va, total);
                    }
                    (void)hipMemRelease(hnd);
                }
                (void)hipMemAddressFree(va, total);
            }
        }
        (void)hipGetLastError();                                  // (the fall-back below is not an error)
    }
    return dev_alloc(h, out, bytes);
}

