// api_engine.h -- C ABI: sprk_last_error .. sprk_create / sprk_upload / sprk_finalize / sprk_workspace_bytes.
// Part of sparrow_hip.hip (one translation unit); included there, not compilable on its own.

// What a finalized handle launches, from what the set-ups left behind.  The history stage follows from the DIN / DIEN set-up alone; of
// the forward routes at most one is set up (each runs only where the ones before it refused), and the one-launch DIN / DIEN forms take
// precedence over the tail they are built on.
static void choose_route(sprk_engine* h) {
    const int din = h->plan.din.enabled;
    if (din == 2) {
        const bool d10 = h->plan.din.emb_dim == 10;
        h->stage = h->dien_frag ? Stage::DienSeqMfma : Stage::DienSeq;
        h->dien_seq_kernel = h->dien_frag ? (d10 ? &k_dien_seq_mfma<10, 32> : &k_dien_seq_mfma<16, 32>) : (d10 ? &k_dien_seq<10, 32> : &k_dien_seq<16, 32>);
    } else if (din == 1) h->stage = h->din_fused_attn ? Stage::DinFusedAttn : (h->din_cols_kc ? Stage::DinCols : Stage::DinPool);
    else h->stage = Stage::None;
    if (din == 1 && h->din_fused) h->route = Route::DinFused;
    else if (din == 2 && h->dien_fused) h->route = Route::DienFused;
    else if (h->v2j_variant >= 0) h->route = Route::V2Joint;
    else if (h->rows_variant >= 0) h->route = Route::Rows;
    else if (h->v1_variant >= 0) h->route = Route::Pairs;
    else if (h->mlp_rows_nbig >= 0) h->route = Route::MlpRows;
    else if (h->din_tail_variant >= 0) h->route = Route::DinTail;
    else h->route = Route::Tile;
}

extern "C" {

const char* sprk_last_error(void) { return g_err.c_str(); }

int sprk_runtime_info(int32_t info[4]) {
    if (!info) return fail(SPRK_EINVAL, "info is NULL");
    info[0] = SPRK_ABI_VERSION;
    info[1] = info[2] = info[3] = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    info[1] = n;
    if (n > 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) {
            info[2] = prop.multiProcessorCount;
            info[3] = strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
        }
    }
    return SPRK_OK;
}

int sprk_create(const sprk_plan* plan, sprk_handle* out) {
    if (!plan || !out) return fail(SPRK_EINVAL, "plan/out is NULL");
    *out = nullptr;
    int rc = validate_plan(*plan);
    if (rc) return rc;
    sprk_engine* h = new (std::nothrow) sprk_engine();
    if (!h) return fail(SPRK_EHIP, "out of host memory");
    h->plan = *plan;
    h->slot_ptr.assign(plan->n_slots, nullptr);
    h->slot_bytes.assign(plan->n_slots, 0);
    h->slot_external.assign(plan->n_slots, 0);
    int off = 0;
    for (int b = 0; b < plan->n_bufs; ++b) {
        h->buf_stride[b] = lds_stride(plan->buf_width[b]);
        h->buf_base[b] = off;
        off += SPRK_TILE_M * h->buf_stride[b];
    }
    // the tile's ids block [64][columns some gather segment reads]
    auto use_col = [&](int c) {
        for (int x : h->idc) if (x == c) return;
        h->idc.push_back(c);
    };
    for (int i = 0; i < plan->n_segs; ++i) {
        const sprk_seg& sg = plan->segs[i];
        if (sg.kind == SPRK_SEG_ROWS || sg.kind == SPRK_SEG_SCALAR || sg.kind == SPRK_SEG_CROSS_ROWS || sg.kind == SPRK_SEG_CROSS_SCALAR) use_col(sg.field);
        if (sg.kind == SPRK_SEG_CROSS_ROWS || sg.kind == SPRK_SEG_CROSS_SCALAR) use_col(sg.field2);
    }
    h->ids_base = off;
    off += (SPRK_TILE_M * (int)h->idc.size() + 3) & ~3;
    h->tile_lds_bytes = (size_t)off * sizeof(float);
    if (h->tile_lds_bytes > 160 * 1024) {
        size_t need = h->tile_lds_bytes;
        delete h;
        return fail(SPRK_EINVAL, "plan needs %zu bytes of LDS per tile (> 160 KiB)", need);
    }
    *out = h;
    return SPRK_OK;
}

int sprk_upload(sprk_handle h, int32_t slot, const void* src, size_t bytes) {
    if (!h || !src || bytes == 0) return fail(SPRK_EINVAL, "bad upload arguments");
    if (slot < 0 || slot >= h->plan.n_slots) return fail(SPRK_EINVAL, "slot %d outside [0,%d)", slot, h->plan.n_slots);
    if (h->finalized) return fail(SPRK_ESTATE, "upload after finalize");
    free_slot(h, slot);
    h->slot_ptr[slot] = nullptr;
    h->slot_external[slot] = 0;
    // 16 spare bytes so a float4 tail read of a [len]-float vector never leaves the allocation
    HIP_TRY(hipMalloc(&h->slot_ptr[slot], bytes + 16));
    HIP_TRY(hipMemset(h->slot_ptr[slot], 0, bytes + 16));
    HIP_TRY(hipMemcpy(h->slot_ptr[slot], src, bytes, hipMemcpyDefault));
    h->slot_bytes[slot] = bytes;
    return SPRK_OK;
}

int sprk_finalize(sprk_handle h) {
    RoctxRange roctx_range_("sprk_finalize");
    if (!h) return fail(SPRK_EINVAL, "handle is NULL");
    if (h->finalized) return SPRK_OK;
    h->tune = SprkTuning::from_env();                     // the ONE place an engine reads the environment
    struct TuneScope { const SprkTuning*& slot; ~TuneScope() { slot = nullptr; } } tune_scope{g_finalize_tune};
    g_finalize_tune = &h->tune;
    const sprk_plan& p = h->plan;
    DevPlan* dp = new (std::nothrow) DevPlan();
    if (!dp) return fail(SPRK_EHIP, "out of host memory");
    memset(dp, 0, sizeof(DevPlan));
    struct Guard { DevPlan* p; ~Guard() { delete p; } } guard{dp};
    // 1. the plan as the interpreter reads it
    dp->F = p.n_id_cols; dp->ND = p.n_dense; dp->NA = p.n_aux;
    dp->n_segs = p.n_segs; dp->n_ops = p.n_ops; dp->n_taps = p.n_taps; dp->n_pairs = p.n_pairs; dp->n_bufs = p.n_bufs;
    dp->head_bias = p.head_bias;
    for (int b = 0; b < SPRK_MAX_BUFS; ++b) { dp->buf_stride[b] = h->buf_stride[b]; dp->buf_base[b] = h->buf_base[b]; }
    dp->ids_base = h->ids_base;
    dp->n_idc = (int)h->idc.size();
    for (size_t i = 0; i < h->idc.size(); ++i) dp->idc[i] = h->idc[i];
    auto compact = [&](int c) { for (size_t i = 0; i < h->idc.size(); ++i) if (h->idc[i] == c) return (int)i; return 0; };
    for (int i = 0; i < p.n_pairs; ++i) { dp->pair_a[i] = p.pair_a[i]; dp->pair_b[i] = p.pair_b[i]; }
    int rc;
    for (int i = 0; i < p.n_segs; ++i) {
        const sprk_seg& s = p.segs[i];
        DevSeg& d = dp->segs[i];
        d.kind = s.kind; d.field = s.field; d.field2 = s.field2; d.row_stride = s.row_stride; d.count = s.count; d.dst = s.dst; d.vocab = s.vocab;
        if (s.kind == SPRK_SEG_ROWS || s.kind == SPRK_SEG_SCALAR || s.kind == SPRK_SEG_CROSS_ROWS || s.kind == SPRK_SEG_CROSS_SCALAR) d.field = compact(s.field);
        if (s.kind == SPRK_SEG_CROSS_ROWS || s.kind == SPRK_SEG_CROSS_SCALAR) d.field2 = compact(s.field2);
        d.table = nullptr;
        if (s.kind == SPRK_SEG_ROWS || s.kind == SPRK_SEG_CROSS_ROWS) {
            if ((rc = need_bytes(h, s.slot, (size_t)s.vocab * s.row_stride * 4, "embedding table"))) return rc;
            d.table = (const float*)h->slot_ptr[s.slot];
        } else if (s.kind == SPRK_SEG_SCALAR || s.kind == SPRK_SEG_CROSS_SCALAR) {
            if ((rc = need_bytes(h, s.slot, (size_t)s.vocab * 4, "first-order table"))) return rc;
            d.table = (const float*)h->slot_ptr[s.slot];
        }
    }
    for (int i = 0; i < p.n_ops; ++i) {
        const sprk_op& o = p.ops[i];
        DevOp& d = dp->ops[i];
        d.kind = o.kind; d.src_buf = o.src_buf; d.src_off = o.src_off; d.K = o.K; d.dst_buf = o.dst_buf; d.dst_off = o.dst_off;
        d.N = o.N; d.ldw = o.ldw; d.act = o.act; d.groups = o.groups; d.group_stride = o.group_stride;
        if (o.kind == SPRK_OP_DENSE) {
            if ((rc = need_bytes(h, o.w_slot, (size_t)o.N * o.ldw * 4, "Dense kernel"))) return rc;
            if ((rc = need_bytes(h, o.b_slot, (size_t)o.N * 4, "Dense bias"))) return rc;
            d.W = (const float*)h->slot_ptr[o.w_slot];
            d.bias = (const float*)h->slot_ptr[o.b_slot];
            if (o.act == SPRK_ACT_PRELU) {
                if ((rc = need_bytes(h, o.alpha_slot, (size_t)o.N * 4, "PReLU alpha"))) return rc;
                d.alpha = (const float*)h->slot_ptr[o.alpha_slot];
            }
        }
    }
    for (int i = 0; i < p.n_taps; ++i) {
        const sprk_tap& t = p.taps[i];
        DevTap& d = dp->taps[i];
        d.buf = t.buf; d.off = t.off; d.len = t.len; d.scale = t.scale; d.bias = t.bias; d.w = nullptr;
        if (t.w_slot >= 0) {
            if ((rc = need_bytes(h, t.w_slot, (size_t)t.len * 4, "tap weights"))) return rc;
            d.w = (const float*)h->slot_ptr[t.w_slot];
        }
    }
    // 2. the device
    HIP_TRY(hipGetDevice(&h->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, h->device));
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // 3. the history stage (host_setup_din.h)
    if (p.din.enabled == 2 && (rc = setup_dien_stage(h, dp->din))) return rc;
    if (p.din.enabled == 1 && (rc = setup_din_stage(h, dp->din))) return rc;
    // 4. the forward routes: the interpreter (every plan's fall-back), then each fused form only where the ones before it refused
    SPRK_TRY(set_max_lds(k_tile_forward, h->tile_lds_bytes));
    h->tile_grid_cap = lds_grid_cap(h, h->tile_lds_bytes);
    if (!h->tune.force_interpreter && match_v2_chain(h) && (rc = setup_v2_fold(h))) return rc;
    const bool v2_on = h->v2j_variant >= 0;
    if (!h->tune.force_interpreter && !v2_on) {
        if (h->rows_from_v2 && (rc = setup_rows_v2(h))) return rc;
        if (h->rows_variant < 0 && (rc = setup_rows_ncf(h))) return rc;
    }
    const bool chain_on = v2_on || h->rows_variant >= 0;
    if (!chain_on && (rc = setup_deepfm_pairs(h))) return rc;
    if (!chain_on && h->v1_variant < 0 && !h->tune.force_interpreter && (rc = setup_mlp_rows(h))) return rc;
    const bool tile_on = !chain_on && h->mlp_rows_nbig < 0;
    if (tile_on && h->v1_variant < 0 && (rc = fold_first_dense(h, dp))) return rc;
    if (tile_on && (rc = setup_din_tail(h, dp))) return rc;
    if ((rc = setup_dien_fused(h))) return rc;
    // 5. route and stage
    choose_route(h);
    // 6. what every route shares: the device plan, the id-range flag, the helper streams of sprk_forward_many's fan-out
    //    (sprk_set_many_streams; SPRK_MANY_STREAMS presets it: 0 = strict stream order, the default; 2..4 = fan out)
    SPRK_TRY(dev_alloc(h, &h->dev_plan, sizeof(DevPlan)));
    HIP_TRY(hipMemcpy(h->dev_plan, dp, sizeof(DevPlan), hipMemcpyHostToDevice));
    SPRK_TRY(dev_alloc(h, &h->dev_err, sizeof(int)));
    HIP_TRY(hipMemset(h->dev_err, 0, sizeof(int)));
    HIP_TRY(hipEventCreateWithFlags(&h->many_fork, hipEventDisableTiming));
    for (int i = 0; i < 4; ++i) {
        HIP_TRY(hipStreamCreateWithFlags(&h->many_stream[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&h->many_join[i], hipEventDisableTiming));
    }
    h->many_streams = h->tune.many_streams;
    h->finalized = true;
    return SPRK_OK;
}

size_t sprk_workspace_bytes(sprk_handle h, int32_t B) {
    if (!h || B <= 0 || !h->plan.din.enabled) return 0;
    return (size_t)B * h->plan.n_aux * sizeof(float);
}

