// api_forward.h -- C ABI: sprk_din_pool, sprk_forward, sprk_forward_many, sprk_describe, sprk_check_ids, sprk_destroy, operators, emb ranker.
// Part of sparrow_hip.hip (one translation unit); included there, not compilable on its own.
// k_din_attn_cols: `n` batches of B rows (n = 1: ids / pooled; n > 1: the per-batch pointers of `many`)
static int launch_din_cols(sprk_handle h, const int32_t* ids, float* pooled, float* att, int32_t B, const DinColsMany* many, hipStream_t st) {
    DinColsRun c = h->din_cols_run;
    const long long ntasks = (long long)(many ? many->n : 1) * ((B + 15) / 16);
    // time slices per task: keep about four waves per SIMD on the chip when one launch has few tasks
    const long long slots = (long long)h->num_cus * 16;
    c.ts = (c.T >= 16 && ntasks * 4 <= slots) ? 4 : ((c.T >= 8 && ntasks * 2 <= slots) ? 2 : 1);
    if (h->tune.din_cols_ts) c.ts = h->tune.din_cols_ts;
    if (many) c.ts = 1;                                        // several batches: the persistent form, one wave per task (k_din_fused.h)
    c.ts_log2 = c.ts == 4 ? 2 : (c.ts == 2 ? 1 : 0);
    c.ql = (c.T + 3) / 4;
    const int EL = 4 * h->din_cols_kc;
    const size_t lds = ((size_t)2 * 64 * 36 + (size_t)DC_WAVES * 16 * c.idp + (size_t)DC_WAVES * 2 * 64 * EL) * sizeof(float);
    const long long grid = (ntasks * c.ts + DC_WAVES - 1) / DC_WAVES;
    if (many)
        hipLaunchKernelGGL(h->din_cols_kernels.many, dim3((unsigned)grid), dim3(DC_WAVES * 64), lds, st, c, nullptr, nullptr, nullptr, B, h->dev_err, *many);
    else
        hipLaunchKernelGGL(h->din_cols_kernels.one, dim3((unsigned)grid), dim3(DC_WAVES * 64), lds, st, c, ids, pooled, att, B, h->dev_err, DinColsOne{});
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

// k_din_fused: `n` batches of B rows (n = 1: ids / dense / out; n > 1: the per-batch pointers of `many`).  tail: scores out (the whole
// DIN forward); else pooled vectors out (the attention stage alone: sprk_din_pool, the two-launch path)
static int launch_din_fused(sprk_handle h, const int32_t* ids, const float* dense, float* out, float* att, int32_t B, const DinFusedMany* many,
                            bool tail, hipStream_t st) {
    DinFusedRun c = h->din_fused_run;
    const long long ntasks = (long long)(many ? many->n : 1) * ((B + 15) / 16);
    // time slices per task: one 8-wave workgroup per CU; spread a small launch over the chip
    const long long slots = (long long)h->num_cus * DF_WAVES;
    c.ts = (c.T >= 16 && ntasks * 4 <= slots) ? 4 : ((c.T >= 8 && ntasks * 2 <= slots) ? 2 : 1);
    if (h->tune.din_cols_ts) c.ts = h->tune.din_cols_ts;
    c.ts_log2 = c.ts == 4 ? 2 : (c.ts == 2 ? 1 : 0);
    c.ql = ((c.T + 3) / 4 + 3) & ~3;                          // slots per quarter, a multiple of four: a trip of the slot loop (two pairs) never straddles one
    const int kc = h->din_cols_kc;
    const size_t lds = ((size_t)DF_COEF_FLOATS + (tail ? (size_t)DinFusedImg::dma_floats : 0) + (size_t)DF_WAVES * 16 * c.idp +
                        (size_t)DF_WAVES * (tail ? 1 : 2) * 64 * 4 * kc) * sizeof(float);   // (k_din_fused.h: PREG)
    long long grid = (ntasks * c.ts + DF_WAVES - 1) / DF_WAVES;
    if (many && grid > h->num_cus) grid = h->num_cus;         // persistent: the waves walk the tasks
    const DinFusedKernels& k = h->din_fused_kernels[tail];
    if (many)
        hipLaunchKernelGGL(k.many, dim3((unsigned)grid), dim3(DF_WAVES * 64), lds, st, c, nullptr, nullptr, nullptr, nullptr, B, h->dev_err, *many);
    else                                                        // (attention weights out -- tests, inspection -- is its own instantiation)
        hipLaunchKernelGGL((att && !tail) ? h->din_fused_att_kernel : k.one, dim3((unsigned)grid), dim3(DF_WAVES * 64), lds, st, c, ids, dense, out, att, B, h->dev_err,
                           DinFusedOne{});
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

// the history stage (h->stage): DIEN's sequence stage (GRU -> attention gate -> AUGRU), DIN's attention + weighted-sum pooling
static int launch_din(sprk_handle h, const int32_t* ids, float* pooled, float* att, int32_t B, hipStream_t st) {
    if (att && (h->stage == Stage::DienSeq || h->stage == Stage::DienSeqMfma)) return fail(SPRK_EINVAL, "DIEN stage has no attention output");
    switch (h->stage) {
    case Stage::DinFusedAttn: return launch_din_fused(h, ids, nullptr, pooled, att, B, nullptr, false, st);
    case Stage::DinCols: return launch_din_cols(h, ids, pooled, att, B, nullptr, st);
    case Stage::DinPool: {
        const int nchunks = (B + h->din_ms - 1) / h->din_ms;
        const int grid = nchunks < h->din_grid_cap ? nchunks : h->din_grid_cap;
        hipLaunchKernelGGL(k_din_pool, dim3(grid), dim3(256), h->din_lds_bytes, st, h->dev_plan, ids, pooled, att, B, h->din_ms, h->dev_err);
        break;
    }
    case Stage::DienSeqMfma: {                                    // sixteen samples per MFMA tile
        DienRun run = h->dien_run;
        run.image = h->dien_frag;
        const int ntiles = (B + 15) / 16;
        int gridm = (ntiles + DM_WAVES - 1) / DM_WAVES;
        if (gridm > h->num_cus * 8) gridm = h->num_cus * 8;
        hipLaunchKernelGGL(h->dien_seq_kernel, dim3(gridm), dim3(DM_WAVES * 64), h->dien_frag_floats * sizeof(float), st, run, ids, pooled, B, h->dev_err);
        break;
    }
    case Stage::DienSeq: {                                        // one lane per sample
        int grid = (B + 63) / 64;
        if (grid > h->num_cus * 8) grid = h->num_cus * 8;
        hipLaunchKernelGGL(h->dien_seq_kernel, dim3(grid), dim3(64), 0, st, h->dien_run, ids, pooled, B, h->dev_err);
        break;
    }
    case Stage::None: return fail(SPRK_EKIND, "handle has no DIN stage");
    }
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

int sprk_din_pool(sprk_handle h, const int32_t* ids, float* pooled, float* att, int32_t B, void* stream) {
    RoctxRange roctx_range_("sprk_din_pool");
    if (!h || !ids || !pooled) return fail(SPRK_EINVAL, "NULL argument");
    if (!h->finalized) return fail(SPRK_ESTATE, "din_pool before finalize");
    if (!h->plan.din.enabled) return fail(SPRK_EKIND, "handle has no DIN stage");
    if (B <= 0) return B == 0 ? SPRK_OK : fail(SPRK_EINVAL, "negative batch");
    return launch_din(h, ids, pooled, att, B, (hipStream_t)stream);
}

int sprk_forward(sprk_handle h, const int32_t* ids, const float* dense, float* out, int32_t B,
                 void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_forward");
    if (!h) return fail(SPRK_EINVAL, "handle is NULL");
    if (!h->finalized) return fail(SPRK_ESTATE, "forward before finalize");
    if (B < 0) return fail(SPRK_EINVAL, "negative batch");
    if (B == 0) return SPRK_OK;
    if (!out) return fail(SPRK_EINVAL, "out is NULL");
    if (h->plan.n_id_cols > 0 && !ids) return fail(SPRK_EINVAL, "ids is NULL");
    if (h->plan.n_dense > 0 && !dense) return fail(SPRK_EINVAL, "dense is NULL");
    hipStream_t st = (hipStream_t)stream;
    const float* aux = nullptr;
    if (h->plan.din.enabled) {
        const size_t need = sprk_workspace_bytes(h, B);
        if (!workspace || workspace_bytes < need) return fail(SPRK_EINVAL, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
        // DIN in one launch: attention + pooling + tail (k_din_fused); the workspace contract stays, the buffer is not touched.  One
        // 8-wave workgroup per CU carries the tail's weights: up to ONE round of workgroups (16 rows x 8 waves x CUs = 32 768 rows on an
        // MI355X: BASELINE config 3, and every latency-bound request below it) a wave owns one task; a larger batch goes to the
        // persistent form (a "several batches" launch of one batch: every wave walks its tasks, tables staged once)
        // (this branch must stay UNCONDITIONAL on the route: forward_many hands it the caller's whole workspace, not a per-stream slice)
        if (h->route == Route::DinFused) {
            if ((long long)((B + 15) / 16) <= (long long)h->num_cus * DF_WAVES) return launch_din_fused(h, ids, dense, out, nullptr, B, nullptr, true, st);
            DinFusedMany fm;
            memset(&fm, 0, sizeof(fm));
            fm.n = 1; fm.ids[0] = ids; fm.dense[0] = dense; fm.out[0] = out;
            return launch_din_fused(h, nullptr, nullptr, nullptr, nullptr, B, &fm, true, st);
        }
        // DIEN in one launch (k_dien_fused): as above, the workspace is not touched and the branch is unconditional on the route
        if (h->route == Route::DienFused) {
            DienRun run = h->dien_run;
            run.image = h->dien_frag;
            const int ntiles = (B + 15) / 16;
            int grid = (ntiles + DNF_WAVES - 1) / DNF_WAVES;
            if (grid > h->num_cus) grid = h->num_cus;              // one 16-wave workgroup per CU (both weight images in its LDS)
            hipLaunchKernelGGL(h->dien_fused_kernel, dim3(grid), dim3(DNF_WAVES * 64), h->dien_fused_lds, st, run, h->din_tail_run, ids, dense, out, B, h->dev_err,
                               h->din_tail_image, (float*)workspace);
            HIP_TRY(hipGetLastError());
            return SPRK_OK;
        }
        SPRK_TRY(launch_din(h, ids, (float*)workspace, nullptr, B, st));
        aux = (const float*)workspace;
    }
    const int ntasks = (B + 15) / 16;
    const int unaligned = (((uintptr_t)ids | (uintptr_t)dense) & 15) ? 1 : 0;   // unaligned inputs: element-wise staging
    switch (h->route) {
    case Route::V2Joint: {
        const V2JVariant& jv = kV2JVariants[h->v2j_variant];
        V2JRun jr = h->v2j_run;
        jr.flags = unaligned;
        if (h->v2j1_kernel && ntasks <= V2J1_MAX_TASKS) {          // one strict launch of one batch: one task per wave, four waves per SIMD (k_chain_v2j1.h)
            hipLaunchKernelGGL(h->v2j1_kernel, dim3((ntasks + h->v2j1_waves - 1) / h->v2j1_waves), dim3(h->v2j1_waves * 64), h->v2j1_lds_bytes, st, jr, ids,
                               dense, out, B, h->dev_err, h->v2j1_image);
            break;
        }
        int grid = (ntasks + V2_WAVES - 1) / V2_WAVES;
        if (grid > h->v2_grid_cap) grid = h->v2_grid_cap;
        hipLaunchKernelGGL(jv.fn, dim3(grid), dim3(V2_WAVES * 64), h->v2j_lds_bytes, st, jr, ids, dense, out, B, h->dev_err, h->v2_image);
        break;
    }
    case Route::Rows: {
        const RowsVariant& rv = kRowsVariants[h->rows_variant];
        int grid = (ntasks + RC_WAVES - 1) / RC_WAVES;
        const bool one = ntasks <= V2J1_MAX_TASKS;                 // k_rows_chain1: one task per wave, no cap (the joint1 family's threshold serves here too)
        if (!one && grid > h->num_cus) grid = h->num_cus;          // looped: one 8-wave workgroup per CU (2 waves per SIMD)
        RowsRun rr = h->rows_run;
        rr.flags = unaligned;
        hipLaunchKernelGGL(one ? rv.fn_one : rv.fn, dim3(grid), dim3(RC_WAVES * 64), h->rows_lds_bytes, st, rr, ids, dense, out, B, h->dev_err, h->rows_image);
        break;
    }
    case Route::Pairs: {
        int grid = (ntasks + V1_WAVES - 1) / V1_WAVES;
        const bool one = h->v1_one_kernel && ntasks <= V1_ONE_MAX_TASKS;
        if (!one && grid > h->num_cus) grid = h->num_cus;          // looped: one 8-wave workgroup per CU (2 waves per SIMD; 3 per SIMD measured slower at B = 65 536)
        hipLaunchKernelGGL(one ? h->v1_one_kernel : h->v1_kernel, dim3(grid), dim3(V1_WAVES * 64), kV1Variants[h->v1_variant].lds_bytes, st, h->v1_run, ids,
                           dense, out, B, h->dev_err);
        break;
    }
    case Route::MlpRows: {
        int grid = (ntasks + MR_WAVES - 1) / MR_WAVES;
        if (grid > h->num_cus) grid = h->num_cus;                  // one 8-wave workgroup per CU (the LDS holds weights + genre tables)
        MlpRowsRun rr = h->mlp_rows_run;
        rr.flags = (rr.flags & ~1) | unaligned;
        hipLaunchKernelGGL(h->mlp_rows_kernel, dim3(grid), dim3(MR_WAVES * 64), h->mlp_rows_lds, st, rr, ids, dense, out, B, h->dev_err, (const float*)h->mlp_rows_image);
        break;
    }
    case Route::DinTail: {
        const int tw = h->din_tail_waves;
        int grid = (ntasks + tw - 1) / tw;
        if (grid > h->num_cus) grid = h->num_cus;                  // one workgroup per CU (8 waves, or 16 with raw embedding rows)
        hipLaunchKernelGGL(h->din_tail_kernel, dim3(grid), dim3(tw * 64), kDinTailVariants[h->din_tail_variant].lds_bytes, st, h->din_tail_run, ids, dense, aux,
                           out, B, h->dev_err, h->din_tail_image, DinTailMany{});
        break;
    }
    default: {                                                     // Route::Tile (the one-launch DIN / DIEN routes returned above)
        const int ntiles = (B + SPRK_TILE_M - 1) / SPRK_TILE_M;
        const int grid = ntiles < h->tile_grid_cap ? ntiles : h->tile_grid_cap;
        hipLaunchKernelGGL(k_tile_forward, dim3(grid), dim3(256), h->tile_lds_bytes, st, h->dev_plan, ids, dense, aux, out, B, h->dev_err);
    }
    }
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

// sprk_forward_many's helper streams: streams 0 .. S-1 wait for what `st` holds so far (fork); `st` waits for all their work (join)
static int fork_helpers(sprk_handle h, int S, hipStream_t st) {
    HIP_TRY(hipEventRecord(h->many_fork, st));
    for (int s = 0; s < S; ++s) HIP_TRY(hipStreamWaitEvent(h->many_stream[s], h->many_fork, 0));
    return SPRK_OK;
}
static int join_helpers(sprk_handle h, int S, hipStream_t st) {
    for (int s = 0; s < S; ++s) {
        HIP_TRY(hipEventRecord(h->many_join[s], h->many_stream[s]));
        HIP_TRY(hipStreamWaitEvent(st, h->many_join[s], 0));
    }
    return SPRK_OK;
}

// n_batches batches in launches of at most `per`: group g's *Many struct (count, per-batch pointers; dense = NULL: none) goes to launch(m, g)
extern "C++" {
template <class Many, class Launch>
static int launch_groups(int32_t n_batches, int per, const int32_t* const* ids, const float* const* dense, float* const* out, Launch launch) {
    int g = 0;
    for (int32_t i0 = 0; i0 < n_batches; i0 += per, ++g) {
        Many m;
        memset(&m, 0, sizeof(m));
        m.n = n_batches - i0 < per ? n_batches - i0 : per;
        for (int j = 0; j < m.n; ++j) { m.ids[j] = ids[i0 + j]; m.dense[j] = dense ? dense[i0 + j] : nullptr; m.out[j] = out[i0 + j]; }
        SPRK_TRY(launch(m, g));
        HIP_TRY(hipGetLastError());
    }
    return SPRK_OK;
}
template <class Ok> static bool every_batch(int32_t n_batches, Ok ok) {
    for (int32_t i = 0; i < n_batches; ++i)
        if (!ok(i)) return false;
    return true;
}
}  // extern "C++"

// DeepFM_v2, a call of more batches than one kernel-argument table holds: the table goes to device memory and ONE launch of
// k_deepfm_v2_joint_many_tab scores the whole call (host_engine.h: V2JTable).  *done = false: not this way (the caller launches groups).
static int launch_v2j_table(sprk_handle h, int32_t n_batches, const int32_t* const* ids, const float* const* dense, float* const* out, int32_t B,
                            hipStream_t st, bool* done) {
    *done = false;
    const int ntpb = (B + 15) / 16;
    long long grid = ((long long)n_batches * ntpb + V2_WAVES - 1) / V2_WAVES;
    if (grid > h->v2_grid_cap) grid = h->v2_grid_cap;
    // task indices are 32-bit in the kernel, and a wave looks four strides past its last task
    if ((long long)n_batches * ntpb + 4 * grid * V2_WAVES >= (1LL << 31)) return SPRK_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); return SPRK_OK; }
    if (cap != hipStreamCaptureStatusNone) return SPRK_OK;       // a captured launch would replay whatever the slot holds by then
    const size_t n = (size_t)n_batches;
    int slot = h->v2j_table_last;
    bool same = slot >= 0 && h->v2j_table[slot].n == n && h->v2j_table[slot].stream == st;
    if (same) {
        const V2JBatch* last = h->v2j_table[slot].stage;
        for (size_t i = 0; i < n && same; ++i) same = last[i].ids == ids[i] && last[i].dense == dense[i] && last[i].out == out[i];
    }
    if (!same) {
        slot = h->v2j_table_last == 0 ? 1 : 0;
        sprk_engine::V2JTable& t = h->v2j_table[slot];
        if (!t.busy) HIP_TRY(hipEventCreateWithFlags(&t.busy, hipEventDisableTiming));
        if (t.used) HIP_TRY(hipEventSynchronize(t.busy));        // the slot's last reader (its upload, too) has finished
        if (t.cap < n) {
            // (room for 4 096 batches from the start, doubling beyond: pinning host memory and hipFree cost about half a millisecond, which
            // a caller's first long call must not pay again because a shorter one came first)
            size_t want = t.cap ? 2 * t.cap : 4096;
            if (want < n) want = n;
            if (t.stage) (void)hipHostFree(t.stage);
            if (t.dev) (void)hipFree(t.dev);
            t.stage = nullptr; t.dev = nullptr; t.cap = 0; t.n = 0;
            HIP_TRY(hipHostMalloc((void**)&t.stage, want * sizeof(V2JBatch), hipHostMallocDefault));
            HIP_TRY(hipMalloc((void**)&t.dev, want * sizeof(V2JBatch)));
            t.cap = want;
        }
        t.n = 0;                                                   // (a failure below leaves no table to compare with)
        for (size_t i = 0; i < n; ++i) t.stage[i] = V2JBatch{ids[i], dense[i], out[i], nullptr};
        HIP_TRY(hipMemcpyAsync(t.dev, t.stage, n * sizeof(V2JBatch), hipMemcpyHostToDevice, st));
        t.n = n;
        t.stream = st;
        h->v2j_table_last = slot;
    }
    sprk_engine::V2JTable& t = h->v2j_table[slot];
    V2JRun jr = h->v2j_run;
    jr.flags = 0;
    const V2JManyTab m = {t.dev, n_batches, ntpb};
    hipLaunchKernelGGL(kV2JVariants[h->v2j_variant].fn_many_tab, dim3((int)grid), dim3(V2_WAVES * 64), h->v2j_lds_bytes, st, jr, m, B, h->dev_err, h->v2_image);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t.busy, st));
    t.used = true;
    *done = true;
    return SPRK_OK;
}

// `many_batches` / `many_streams`: batches per launch and helper streams of THIS call (the handle itself is not touched)
static int forward_many_impl(sprk_handle h, int32_t n_batches, const int32_t* const* ids, const float* const* dense,
                             float* const* out, int32_t B, void* workspace, size_t workspace_bytes, void* stream,
                             int many_batches, int many_streams) {
    RoctxRange roctx_range_("sprk_forward_many");
    if (!h) return fail(SPRK_EINVAL, "handle is NULL");
    if (n_batches < 0) return fail(SPRK_EINVAL, "negative batch count");
    if (n_batches > 0 && !out) return fail(SPRK_EINVAL, "out is NULL");
    int S = (h->finalized && n_batches > 1) ? many_streams : 0;
    // a model with a workspace (DIN: attention kernel -> pooled vectors -> tail kernel) needs one workspace slice per
    // stream; with a single slice its forwards stay in strict order
    const size_t ws_need = (sprk_workspace_bytes(h, B) + 255) & ~(size_t)255;
    const bool ws_untouched = h->finalized && (h->route == Route::DinFused || h->route == Route::DienFused);   // (sprk_forward's one-launch branches: unconditional, see there)
    if (S >= 2 && ws_need > 0 && !ws_untouched) {
        while (S >= 2 && (!workspace || workspace_bytes < (size_t)S * ws_need)) --S;
        if (S < 2) S = 0;
    }
    hipStream_t st = (hipStream_t)stream;
    // several batches per launch (sprk_set_many_batches): the fused kernels take up to their *_MB batches' buffers and walk their tasks
    // as one grid; everything else (other models, unaligned buffers, tracing) goes batch by batch at the end
    const bool grouped = h->finalized && many_batches > 1 && n_batches > 1 && B > 0 && ids;
    const int ntpb = (B + 15) / 16;
    auto aligned = [&](int32_t i, const float* d) { return !(((uintptr_t)ids[i] | (uintptr_t)d) & 15); };
    auto present = [&](int32_t i) { return ids[i] && dense[i] && out[i]; };
    if (grouped && dense && h->route == Route::V2Joint && every_batch(n_batches, [&](int32_t i) { return present(i) && aligned(i, dense[i]); })) {
        const V2JVariant& jv = kV2JVariants[h->v2j_variant];
        V2JRun jr = h->v2j_run;
        jr.flags = 0;
        // more batches than one launch's kernel-argument table takes: one launch for the whole call, the table in device memory
        if (n_batches > many_batches) {
            bool done = false;
            SPRK_TRY(launch_v2j_table(h, n_batches, ids, dense, out, B, st, &done));
            if (done) return SPRK_OK;
        }
        return launch_groups<V2JMany>(n_batches, many_batches, ids, dense, out, [&](V2JMany& m, int) {
            m.ntpb = ntpb;
            long long grid = ((long long)m.n * ntpb + V2_WAVES - 1) / V2_WAVES;
            if (grid > h->v2_grid_cap) grid = h->v2_grid_cap;
            hipLaunchKernelGGL(jv.fn_many, dim3((int)grid), dim3(V2_WAVES * 64), h->v2j_lds_bytes, st, jr, m, B, h->dev_err, h->v2_image);
            return SPRK_OK;
        });
    }
    // k_rows_chain: up to RC_MB batches per launch
    const float* const* rows_dense = h->plan.n_dense ? dense : nullptr;
    if (grouped && (dense || h->plan.n_dense == 0) && h->route == Route::Rows &&
        every_batch(n_batches, [&](int32_t i) { return ids[i] && out[i] && (!rows_dense || rows_dense[i]) && aligned(i, rows_dense ? rows_dense[i] : nullptr); })) {
        const RowsVariant& rv = kRowsVariants[h->rows_variant];
        RowsRun rr = h->rows_run;
        rr.flags = 0;
        return launch_groups<RowsMany>(n_batches, many_batches < RC_MB ? many_batches : RC_MB, ids, rows_dense, out, [&](RowsMany& m, int) {
            m.ntpb = ntpb;
            long long grid = ((long long)m.n * ntpb + RC_WAVES - 1) / RC_WAVES;
            if (grid > h->num_cus) grid = h->num_cus;
            hipLaunchKernelGGL(rv.fn_many, dim3((int)grid), dim3(RC_WAVES * 64), h->rows_lds_bytes, st, rr, m, B, h->dev_err, h->rows_image);
            return SPRK_OK;
        });
    }
    // [r6] k_mlp_rows (EmbeddingMLP / Wide&Deep): up to MR_MB batches per launch
    if (grouped && dense && h->route == Route::MlpRows && h->mlp_rows_many_kernel &&
        every_batch(n_batches, [&](int32_t i) { return present(i) && aligned(i, dense[i]); })) {
        MlpRowsRun rr = h->mlp_rows_run;
        rr.flags &= ~1;
        return launch_groups<MlpRowsMany>(n_batches, many_batches < MR_MB ? many_batches : MR_MB, ids, dense, out, [&](MlpRowsMany& m, int) {
            long long grid = ((long long)m.n * ntpb + MR_WAVES - 1) / MR_WAVES;
            if (grid > h->num_cus) grid = h->num_cus;
            hipLaunchKernelGGL(h->mlp_rows_many_kernel, dim3((int)grid), dim3(MR_WAVES * 64), h->mlp_rows_lds, st, rr, m, B, h->dev_err,
                               (const float*)h->mlp_rows_image);
            return SPRK_OK;
        });
    }
    // the pairwise-dot DeepFM kernel: up to V1_MB batches per launch
    if (grouped && dense && h->route == Route::Pairs && every_batch(n_batches, present)) {
        const size_t lds = kV1Variants[h->v1_variant].lds_bytes;
        return launch_groups<V1Many>(n_batches, many_batches < V1_MB ? many_batches : V1_MB, ids, dense, out, [&](V1Many& m, int) {
            m.ntpb = ntpb;
            long long grid = ((long long)m.n * ntpb + V1_WAVES - 1) / V1_WAVES;
            if (grid > h->num_cus) grid = h->num_cus;
            hipLaunchKernelGGL(h->v1_many_kernel, dim3((int)grid), dim3(V1_WAVES * 64), lds, st, h->v1_run, m, B, h->dev_err);
            return SPRK_OK;
        });
    }
    // DIN on k_din_fused: up to DF_MB batches per launch, one PERSISTENT launch does everything (k_din_fused.h: tables staged once, the
    // waves walk the tasks on their own); groups alternate over the helper streams.  32.2 us per batch of BASELINE config 3 against
    // 33.4 for the two-launch pipeline below on the same box (profiles/r04; SPRK_DIN_FUSED_MB=0 brings the pipeline back)
    if (grouped && dense && h->route == Route::DinFused && h->tune.din_fused_mb && every_batch(n_batches, present)) {
        const int SG = S >= 2 ? S : 1;
        if (SG >= 2) SPRK_TRY(fork_helpers(h, SG, st));
        SPRK_TRY(launch_groups<DinFusedMany>(n_batches, many_batches < DF_MB ? many_batches : DF_MB, ids, dense, out, [&](DinFusedMany& m, int g) {
            return launch_din_fused(h, nullptr, nullptr, nullptr, nullptr, B, &m, true, SG >= 2 ? h->many_stream[g % SG] : st);
        }));
        if (SG >= 2) SPRK_TRY(join_helpers(h, SG, st));
        return SPRK_OK;
    }
    // DIN (k_din_attn_cols -> pooled vectors -> k_din_tail): the attention launches of a group of batches, then ONE tail launch for
    // the group; a workspace slice per batch of the group.  Groups alternate over the helper streams when there are slices for that.
    const bool cols = h->stage == Stage::DinCols || h->stage == Stage::DinFusedAttn;
    if (grouped && dense && workspace && ws_need > 0 && cols && (h->route == Route::DinTail || h->route == Route::DinFused)) {
        int per = many_batches < DIN_MB ? many_batches : DIN_MB;
        if ((size_t)per * ws_need > workspace_bytes) per = (int)(workspace_bytes / ws_need);
        if (per >= 2 && every_batch(n_batches, present)) {
            int SG = S >= 2 ? S : 1;                                   // streams the groups alternate over
            while (SG > 1 && (size_t)SG * per * ws_need > workspace_bytes) --SG;
            if (SG >= 2) SPRK_TRY(fork_helpers(h, SG, st));
            const size_t tail_lds = kDinTailVariants[h->din_tail_variant].lds_bytes;
            const int tw = h->din_tail_waves;
            int g = 0;
            for (int32_t i0 = 0; i0 < n_batches; i0 += per, ++g) {
                const int n = n_batches - i0 < per ? n_batches - i0 : per;
                hipStream_t sg = SG >= 2 ? h->many_stream[g % SG] : st;
                char* wbase = (char*)workspace + (size_t)(g % SG) * per * ws_need;
                DinTailMany tm;
                memset(&tm, 0, sizeof(tm));
                tm.n = n; tm.ntpb = ntpb;
                for (int j = 0; j < n; ++j) {
                    float* pooled = (float*)(wbase + (size_t)j * ws_need);
                    tm.ids[j] = ids[i0 + j]; tm.dense[j] = dense[i0 + j]; tm.aux[j] = pooled; tm.out[j] = out[i0 + j];
                }
                // ONE attention launch for the group (k_din_attn_cols<..., MB = true>: no launch boundary and no partial last round of
                // waves between the batches), then one tail launch
                if (n <= DC_MB) {
                    DinColsMany cm;
                    memset(&cm, 0, sizeof(cm));
                    cm.n = n;
                    for (int j = 0; j < n; ++j) { cm.ids[j] = tm.ids[j]; cm.pooled[j] = const_cast<float*>(tm.aux[j]); }
                    SPRK_TRY(launch_din_cols(h, nullptr, nullptr, nullptr, B, &cm, sg));
                } else {
                    for (int j = 0; j < n; ++j) SPRK_TRY(launch_din_cols(h, tm.ids[j], const_cast<float*>(tm.aux[j]), nullptr, B, nullptr, sg));
                }
                long long tg = ((long long)n * ntpb + tw - 1) / tw;
                if (tg > h->num_cus) tg = h->num_cus;
                hipLaunchKernelGGL(h->din_tail_many_kernel, dim3((int)tg), dim3(tw * 64), tail_lds, sg, h->din_tail_run, nullptr, nullptr, nullptr, nullptr, B,
                                   h->dev_err, h->din_tail_image, tm);
                HIP_TRY(hipGetLastError());
            }
            if (SG >= 2) SPRK_TRY(join_helpers(h, SG, st));
            return SPRK_OK;
        }
    }
    if (S >= 2) SPRK_TRY(fork_helpers(h, S, st));
    for (int32_t i = 0; i < n_batches; ++i) {
        // (one workspace slice per stream -- except for the one-launch DIN, whose S was NOT reduced to the slices the buffer holds because
        //  its forward never touches the buffer: it gets the caller's buffer and size unchanged, never an offset past its end [ADVICE r04])
        const bool sliced = S >= 2 && ws_need > 0 && !ws_untouched;
        void* wsi = sliced ? (void*)((char*)workspace + (size_t)(i % S) * ws_need) : workspace;
        SPRK_TRY(sprk_forward(h, ids ? ids[i] : nullptr, dense ? dense[i] : nullptr, out[i], B, wsi,
                              sliced ? ws_need : workspace_bytes, S >= 2 ? (void*)h->many_stream[i % S] : stream));
    }
    if (S >= 2) SPRK_TRY(join_helpers(h, S, st));
    return SPRK_OK;
}

int sprk_forward_many(sprk_handle h, int32_t n_batches, const int32_t* const* ids, const float* const* dense,
                      float* const* out, int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return fail(SPRK_EINVAL, "handle is NULL");
    return forward_many_impl(h, n_batches, ids, dense, out, B, workspace, workspace_bytes, stream, h->many_batches, h->many_streams);
}

int sprk_forward_many_opts(sprk_handle h, int32_t n_batches, const int32_t* const* ids, const float* const* dense,
                           float* const* out, int32_t B, void* workspace, size_t workspace_bytes, void* stream,
                           int32_t batches_per_launch, int32_t helper_streams) {
    if (!h) return fail(SPRK_EINVAL, "handle is NULL");
    if (batches_per_launch < 1 || batches_per_launch > V2J_MB) return fail(SPRK_EINVAL, "batches per launch %d outside [1,%d]", batches_per_launch, V2J_MB);
    if (helper_streams < 0 || helper_streams > 4) return fail(SPRK_EINVAL, "stream count %d outside [0,4]", helper_streams);
    return forward_many_impl(h, n_batches, ids, dense, out, B, workspace, workspace_bytes, stream, batches_per_launch,
                             helper_streams < 2 ? 0 : helper_streams);
}

#define SPRK_FORWARD_KIND(name, kind)                                                                      \
    int name(sprk_handle h, const int32_t* ids, const float* dense, float* out, int32_t B, void* ws,      \
             size_t ws_bytes, void* stream) {                                                              \
        if (!h) return fail(SPRK_EINVAL, "handle is NULL");                                                \
        if (h->plan.model_kind != kind) return fail(SPRK_EKIND, #name ": handle holds model kind %d", h->plan.model_kind); \
        return sprk_forward(h, ids, dense, out, B, ws, ws_bytes, stream);                                  \
    }
SPRK_FORWARD_KIND(sprk_forward_embedding_mlp, SPRK_MODEL_EMBEDDING_MLP)
SPRK_FORWARD_KIND(sprk_forward_widedeep, SPRK_MODEL_WIDE_DEEP)
SPRK_FORWARD_KIND(sprk_forward_neuralcf, SPRK_MODEL_NEURALCF)
SPRK_FORWARD_KIND(sprk_forward_deepfm, SPRK_MODEL_DEEPFM)
SPRK_FORWARD_KIND(sprk_forward_deepfm_v2, SPRK_MODEL_DEEPFM_V2)
SPRK_FORWARD_KIND(sprk_forward_din, SPRK_MODEL_DIN)
SPRK_FORWARD_KIND(sprk_forward_dien, SPRK_MODEL_DIEN)

int sprk_set_many_streams(sprk_handle h, int32_t n) {
    if (!h) return fail(SPRK_EINVAL, "handle is NULL");
    if (!h->finalized) return fail(SPRK_ESTATE, "set_many_streams before finalize");
    if (n < 0 || n > 4) return fail(SPRK_EINVAL, "stream count %d outside [0,4]", n);
    h->many_streams = n < 2 ? 0 : n;
    return SPRK_OK;
}

int sprk_set_many_batches(sprk_handle h, int32_t n) {
    if (!h) return fail(SPRK_EINVAL, "handle is NULL");
    if (!h->finalized) return fail(SPRK_ESTATE, "set_many_batches before finalize");
    if (n < 1 || n > V2J_MB) return fail(SPRK_EINVAL, "batches per launch %d outside [1,%d]", n, V2J_MB);   // (DIN caps at DIN_MB)
    h->many_batches = n;
    return SPRK_OK;
}

int sprk_describe(sprk_handle h, char* buf, size_t buf_bytes) {
    if (!h || !buf || buf_bytes == 0) return fail(SPRK_EINVAL, "describe: NULL argument");
    if (!h->finalized) return fail(SPRK_ESTATE, "describe before finalize");
    char kern[160];
    switch (h->route) {
    case Route::V2Joint: {
        const V2JVariant& jv = kV2JVariants[h->v2j_variant];
        snprintf(kern, sizeof(kern), "k_deepfm_v2_joint<G_BIG=%d,NJF=%d,KPC=%d,%s>", jv.g_big, jv.njf, jv.kpc, jv.half ? "split-f16" : "f32");
        break;
    }
    case Route::Pairs:
        snprintf(kern, sizeof(kern), "k_deepfm_pairs<NF=%d,NV=%d>", kV1Variants[h->v1_variant].nf, kV1Variants[h->v1_variant].nv);
        break;
    case Route::Rows: {
        const RowsVariant& rv = kRowsVariants[h->rows_variant];
        snprintf(kern, sizeof(kern), "k_rows_chain<KPC=%d,H0C=%d,H1C=%d,G_BIG=%d,NJF=%d%s>", rv.kpc, rv.h0c, rv.h1c, rv.g_big, rv.njf,
                 rv.unf ? ",UNF" : "");
        break;
    }
    case Route::MlpRows:
        snprintf(kern, sizeof(kern), "k_mlp_rows<8,8,NBIG=%d,NSMALL=%d>", h->mlp_rows_nbig, h->mlp_rows_run.n_small);
        break;
    case Route::DinTail: {
        const DinTailVariant& tv = kDinTailVariants[h->din_tail_variant];
        snprintf(kern, sizeof(kern), "k_din_tail<%d,%d,%d%s>", tv.n0c, tv.n1c, tv.kpc, h->din_tail_run.e_unscale != 0.f ? ",UNF" : "");
        break;
    }
    case Route::DinFused: snprintf(kern, sizeof(kern), "k_din_fused<KC=%d,tail 128/64>", h->din_cols_kc); break;
    case Route::DienFused: snprintf(kern, sizeof(kern), "k_dien_fused<D=%d,tail 128/64>", h->plan.din.emb_dim); break;
    case Route::Tile: snprintf(kern, sizeof(kern), "k_tile_forward"); break;
    }
    // stage: what sprk_din_pool runs, in the order of enum Stage
    static const char* const kStageName[] = {"", "k_din_pool", "k_din_attn_cols", "k_din_fused", "k_dien_seq", "k_dien_seq_mfma"};
    const bool cols = h->stage == Stage::DinCols || h->stage == Stage::DinFusedAttn;
    size_t uploaded = 0;
    for (size_t b : h->slot_bytes) uploaded += b;
#ifndef SPRK_BUILD_DEFINES_STR
#define SPRK_BUILD_DEFINES_STR ""                             // (_lib.build_library passes the experiment defines of SPRK_BUILD_DEFINES; the product build has none)
#endif
    // split_f16: the sites of the route and stage in use whose operand runs as hi + lo f16 halves with a STATIC scale chosen at finalize (a
    // site a range guard, a non-finite weight or a switch refused is absent: it runs f32; empty = everything f32).  v2 = DeepFM_v2's folded
    // rows and W0; pairs_e = the pair-dot deep tables; rows_unf = the rows chain's raw rows and projection weights; tail_unf = the DIN / DIEN
    // tail's raw rows and fc0 columns; dyn_w1 / dyn_w0 / dyn_w0p = weight fragments of the per-sample dynamic chains (make_dyn_fragments);
    // din_attn = the attention tables; dien_seq = DIEN's sequence stage
    char split[96] = "";
    auto site = [&](bool on, const char* name) {
        if (!on) return;
        if (split[0]) strncat(split, ",", sizeof(split) - strlen(split) - 1);
        strncat(split, name, sizeof(split) - strlen(split) - 1);
    };
    switch (h->route) {
    case Route::V2Joint: site(kV2JVariants[h->v2j_variant].half, "v2"); break;
    case Route::Pairs:
        site(h->v1_run.w1frag != nullptr, "dyn_w1"); site(h->v1_run.w0frag != nullptr, "dyn_w0"); site(h->v1_run.e_scale != 0.f, "pairs_e");
        break;
    case Route::Rows: site(kRowsVariants[h->rows_variant].unf, "rows_unf"); break;
    case Route::MlpRows: site(h->mlp_rows_run.inv_w1_scale != 0.f, "dyn_w1"); break;
    case Route::DinTail: case Route::DinFused: case Route::DienFused:
        site(h->din_tail_run.inv_w1_scale != 0.f, "dyn_w1"); site(h->din_tail_run.inv_w0p_scale != 0.f, "dyn_w0p");
        site(h->din_tail_run.e_unscale != 0.f, "tail_unf");
        break;
    case Route::Tile: break;
    }
    site(cols, "din_attn");
    site(h->stage == Stage::DienSeqMfma, "dien_seq");
    const int n = snprintf(buf, buf_bytes, "kernel=%s;stage=%s;stage_waves_per_workgroup=%d;fused=%d;uploaded_bytes=%zu;derived_bytes=%zu;first_dense_fold=%d;split_f16=%s;build_defines=%s", kern,
                           kStageName[(int)h->stage], cols ? DC_WAVES : 0, h->route != Route::Tile ? 1 : 0, uploaded, h->derived_bytes, h->n_acc_folded, split, SPRK_BUILD_DEFINES_STR);
    if (n < 0 || (size_t)n >= buf_bytes) return fail(SPRK_EINVAL, "describe: buffer of %zu bytes is too small", buf_bytes);
    return SPRK_OK;
}

int sprk_check_ids(sprk_handle h, void* stream) {
    if (!h) return fail(SPRK_EINVAL, "handle is NULL");
    if (!h->finalized) return fail(SPRK_ESTATE, "check_ids before finalize");
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, h->dev_err, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (flag) {
        HIP_TRY(hipMemsetAsync(h->dev_err, 0, sizeof(int), (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return fail(SPRK_ERANGE, "an id was outside its table (TF would raise InvalidArgumentError: assert_less_than_num_buckets) [flag 0x%x]", flag);
    }
    return SPRK_OK;
}

void sprk_destroy(sprk_handle h) {
    if (!h) return;
    for (size_t i = 0; i < h->slot_ptr.size(); ++i) free_slot(h, i);
    for (const sprk_engine::DevAlloc& a : h->allocs) release(a);
    if (h->v2j_tab) (void)hipFree(h->v2j_tab);
    for (sprk_engine::V2JTable& t : h->v2j_table) {
        if (t.used) (void)hipEventSynchronize(t.busy);
        if (t.stage) (void)hipHostFree(t.stage);
        if (t.dev) (void)hipFree(t.dev);
        if (t.busy) (void)hipEventDestroy(t.busy);
    }
    for (int i = 0; i < 4; ++i) { if (h->many_stream[i]) (void)hipStreamDestroy(h->many_stream[i]); if (h->many_join[i]) (void)hipEventDestroy(h->many_join[i]); }
    if (h->many_fork) (void)hipEventDestroy(h->many_fork);
    delete h;
}

int sprk_embedding_gather(const float* table, int32_t V, int32_t D, int32_t row_stride, const int32_t* ids,
                          int32_t B, float* out, void* stream) {
    if (!table || !ids || !out) return fail(SPRK_EINVAL, "NULL argument");
    if (V <= 0 || D <= 0 || (D & 3) || row_stride < D || (row_stride & 3)) return fail(SPRK_EINVAL, "bad gather geometry V=%d D=%d row_stride=%d", V, D, row_stride);
    if (B < 0) return fail(SPRK_EINVAL, "negative batch");
    if (B == 0) return SPRK_OK;
    const long long total = (long long)B * (D / 4);
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_embedding_gather, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, table, V, D / 4, row_stride, ids, B, out);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

