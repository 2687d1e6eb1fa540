// api_train_dien.h -- C ABI: sprk_train_dien_workspace_bytes / sprk_train_dien_fit (k_train_dien.h; sparrowrecsys_amd/trainer_dien.py has the definition).
// As api_train_din.h: every argument is checked before any device call; the whole fit -- the schedule once (k_tr_check, k_te_count, k_te_scatter, the
// segment sort), then three launches per step -- is enqueued on the caller's stream and the call returns: no synchronisation, no memory of its own.
// The workspace is DIN's (TrainDinWorkspace), carved over the schedule's view of the model.
namespace {
// the model as the kernels take it: `out` for k_te_step, `sched` for DIN's schedule kernels and its carver; false: a field out of range
bool train_dien_dims(const sprk_train_dien_model* mo, DienDims* out, DinDims* sched) {
    if (!mo) return false;
    DienDims d;
    memset(&d, 0, sizeof(d));
    if (mo->hist_len < 1 || mo->hist_len > TD_MAX_COLS - 4 || mo->n_cols < mo->hist_len + 1 || mo->n_cols > TD_MAX_COLS || mo->emb_dim < 1 || mo->emb_dim > TD_MAX_EMB ||
        mo->att_hidden < 1 || mo->att_hidden > TD_MAX_WIDTH || mo->n_layers < 1 || mo->n_layers > TD_MAX_LAYERS || mo->n_x < 1 || mo->n_x > TD_MAX_X ||
        mo->n_dense < 0 || mo->n_dense > TD_MAX_X || mo->genre[0] != 0)
        return false;
    d.n_cols = mo->n_cols; d.n_dense = mo->n_dense; d.emb_dim = mo->emb_dim; d.hist = mo->hist_len; d.att = mo->att_hidden; d.n_x = mo->n_x; d.n_layers = mo->n_layers;
    const int D = d.emb_dim;
    d.staged = D <= TE_STAGE_EMB ? 1 : 0;
    DinDims s;
    memset(&s, 0, sizeof(s));
    int first_col[TD_MAX_COLS];
    for (int c = 0; c < d.n_cols; ++c) {
        const int t = mo->table[c];
        if (mo->vocab[c] < 1 || t < 0 || t > d.n_tables || (c <= d.hist && t != 0)) return false;                // tables appear in order, without a gap
        if (t == d.n_tables) first_col[d.n_tables++] = c;
        else if (mo->vocab[first_col[t]] != mo->vocab[c] || (mo->genre[first_col[t]] != 0) != (mo->genre[c] != 0)) return false;
        d.table[c] = t; s.table[c] = t;
    }
    long long at = 0, rows = 0;
    for (int t = 0; t < d.n_tables; ++t) {
        d.tab_off[t] = at; s.tab_off[t] = at; s.row_base[t] = rows;
        at += (long long)mo->vocab[first_col[t]] * D; rows += mo->vocab[first_col[t]];
    }
    d.tab_off[d.n_tables] = at; s.tab_off[d.n_tables] = at; s.row_base[d.n_tables] = rows;
    if (rows >= 0x7fffffffll) return false;
    d.n_table = at;
    // fc0's input rows: the AUGRU's state and the candidate once each, every column behind the history once, numerics inside their range
    int seen[TD_MAX_COLS + 1][TD_MAX_EMB];
    memset(seen, 0, sizeof(seen));
    for (int k = 0; k < d.n_x; ++k) {
        const int src = mo->xsrc[k], sub = mo->xsub[k];
        if (src == TD_SRC_NUMERIC) { if (sub < 0 || sub >= d.n_dense) return false; }
        else if (src == TD_SRC_POOLED || src == 0 || (src > d.hist && src < d.n_cols)) {
            if (sub < 0 || sub >= D || seen[src == TD_SRC_POOLED ? TD_MAX_COLS : src][sub]++) return false;
            if (src == TD_SRC_POOLED) d.prow[sub] = (short)k;
            if (src == 0) d.crow[sub] = (short)k;
        } else return false;
        d.xsrc[k] = (short)src; d.xsub[k] = (short)sub;
    }
    for (int c = 0; c <= TD_MAX_COLS; ++c) {
        const bool must = c == TD_MAX_COLS || c == 0 || (c > d.hist && c < d.n_cols);
        for (int x = 0; x < D; ++x)
            if (must && !seen[c][x]) return false;
    }
    d.gru = at; at += (long long)2 * D * 3 * D + 2 * 3 * D;
    d.att0_ker = at; at += (long long)D * d.att;
    d.att0_bias = at; at += d.att;
    d.att1_ker = at; at += d.att;
    d.att1_bias = at; at += 1;
    d.aug = at; at += (long long)3 * (3 * D * D + 2 * D);
    d.h0 = at; at += D;
    int fan = d.n_x, wide = 1;
    for (int l = 0; l <= d.n_layers; ++l) {
        const int h = l < d.n_layers ? mo->width[l] : 1;
        if (h < 1 || h > TD_MAX_WIDTH) return false;
        d.width[l] = h; d.fan[l] = fan;
        d.ker_off[l] = at; at += (long long)fan * h;
        d.bias_off[l] = at; at += h;
        if (l < d.n_layers) { d.alpha_off[l] = at; at += h; if (h > wide) wide = h; }
        fan = h;
    }
    d.wide = wide;
    d.n_params = at;
    s.n_cols = d.n_cols; s.n_dense = d.n_dense; s.emb_dim = D; s.hist = d.hist; s.att = d.att; s.n_x = d.n_x; s.n_layers = d.n_layers; s.n_tables = d.n_tables;
    s.n_table = d.n_table; s.n_params = d.n_params;
    *out = d;
    *sched = s;
    return true;
}
// trainer_dien.lds_bytes
inline size_t train_dien_lds_bytes(const DienDims& d, int tile) {
    const size_t T = (size_t)d.hist, D = (size_t)d.emb_dim, H = (size_t)d.att;
    size_t per = (T + 1) * D + 21 * T * D + 2 * T * H + 2 * T + 8 * D + 2 * (size_t)d.n_x + 2 * (size_t)d.wide;
    for (int l = 0; l < d.n_layers; ++l) per += 2 * (size_t)d.width[l];
    const size_t once = d.staged ? 15 * D * D + 12 * D : 0;
    return (per * (size_t)tile + once) * sizeof(float);
}
inline bool train_dien_sizes_ok(const DienDims& d, int64_t n, int32_t batch, int32_t tile) {
    return n >= 0 && batch >= 1 && batch <= (1 << 28) && tile >= 1 && n * d.n_cols < 0x7fffffffll && train_dien_lds_bytes(d, tile) <= 160 * 1024;
}
}  // namespace

extern "C" {

size_t sprk_train_dien_workspace_bytes(const sprk_train_dien_model* model, int64_t n, int32_t batch, int32_t tile) {
    DienDims d;
    DinDims s;
    if (!train_dien_dims(model, &d, &s) || !train_dien_sizes_ok(d, n, batch, tile)) return 0;
    return train_din_carve(nullptr, s, n, batch, tile).bytes;
}

int sprk_train_dien_fit(const sprk_train_dien_model* model, const int32_t* ids, const float* dense, const float* labels, const int32_t* order, int64_t n,
                        int32_t batch, int32_t tile, int32_t epochs, const float* alphas, float one_minus_beta1, float one_minus_beta2, float epsilon,
                        float* params, float* m, float* v, float* p, uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_train_dien_fit");
    DienDims d;
    DinDims s;
    if (!train_dien_dims(model, &d, &s))
        return fail(SPRK_EINVAL, "train_dien_fit: bad model (need hist_len 1..%d, hist_len + 1 .. %d id columns of which the candidate and the history read table 0 and "
                                 "hold ids from 0, tables numbered without a gap whose columns agree in vocab and genre, emb_dim 1..%d, att_hidden 1..%d, 1..%d tail layers "
                                 "of 1..%d units, 1..%d fc0 input rows that hold the AUGRU's state, the candidate and every column behind the history once each, 0..%d "
                                 "numerics, all tables' rows < 2^31 - 1)",
                    TD_MAX_COLS - 4, TD_MAX_COLS, TD_MAX_EMB, TD_MAX_WIDTH, TD_MAX_LAYERS, TD_MAX_WIDTH, TD_MAX_X, TD_MAX_X);
    if (n < 0 || batch < 1 || tile < 1 || epochs < 0) return fail(SPRK_EINVAL, "train_dien_fit: n = %lld, batch = %d, tile = %d, epochs = %d", (long long)n, batch, tile, epochs);
    if (batch > (1 << 28)) return fail(SPRK_EINVAL, "train_dien_fit: batch = %d: a schedule key holds position x 16 + column in 32 bits, so a batch has up to 2^28 rows", batch);
    if (n * d.n_cols >= 0x7fffffffll)
        return fail(SPRK_EINVAL, "train_dien_fit: n x id columns = %lld: the schedule's unsigned offsets and the sort take fewer than 2^31 - 1 entries", (long long)(n * d.n_cols));
    if (train_dien_lds_bytes(d, tile) > 160 * 1024)
        return fail(SPRK_EINVAL, "train_dien_fit: tile = %d needs %zu bytes of LDS for this model, more than %d", tile, train_dien_lds_bytes(d, tile), 160 * 1024);
    if (!error_key) return fail(SPRK_EINVAL, "train_dien_fit: NULL error word");
    if ((uintptr_t)error_key & 7) return fail(SPRK_EINVAL, "train_dien_fit: misaligned error word");
    if (!params || !m || !v) return fail(SPRK_EINVAL, "train_dien_fit: NULL parameters or moments");
    if (n > 0 && (!ids || !labels || (d.n_dense > 0 && !dense))) return fail(SPRK_EINVAL, "train_dien_fit: NULL ids, dense or labels");
    if (n > 0 && epochs > 0 && (!alphas || !p)) return fail(SPRK_EINVAL, "train_dien_fit: NULL alphas or p");
    if (((uintptr_t)ids & 3) || ((uintptr_t)dense & 3) || ((uintptr_t)labels & 3) || ((uintptr_t)order & 3) || ((uintptr_t)alphas & 3) || ((uintptr_t)params & 3) ||
        ((uintptr_t)m & 3) || ((uintptr_t)v & 3) || ((uintptr_t)p & 3))
        return fail(SPRK_EINVAL, "train_dien_fit: misaligned array");
    const TrainDinWorkspace w = train_din_carve(workspace, s, n, batch, tile);
    SPRK_TRY(check_workspace("train_dien_fit", "sprk_train_dien_workspace_bytes", workspace, workspace_bytes, w.bytes));
    if (n == 0 || epochs == 0) return SPRK_OK;
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* err = (unsigned long long*)error_key;

    TrainDims sched;                                                         // what k_tr_check, k_tr_count and k_tr_dense_adam read of a model
    memset(&sched, 0, sizeof(sched));
    sched.n_cols = d.n_cols; sched.n_dense = d.n_dense; sched.emb_dim = d.emb_dim;
    for (int c = 0; c < d.n_cols; ++c) { sched.vocab[c] = model->vocab[c]; sched.genre[c] = model->genre[c] ? 1 : 0; }
    sched.n_table = d.n_table; sched.n_params = d.n_params;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    hipLaunchKernelGGL(k_tr_check, dim3(fe_grid_capped(n)), dim3(TR_THREADS), 0, st, (long long)n, ids, dense, labels, sched, err);
    hipLaunchKernelGGL(k_te_count, dim3(fe_grid_capped(w.entries)), dim3(TR_THREADS), 0, st, (long long)n, (int)batch, ids, order, d.n_cols, d.hist, w.off);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_scan(w.off, w.n_batches + 1, w.tops, w.scan_tiles, FeScanKept<false>{}, st));
    hipLaunchKernelGGL(k_te_scatter, dim3(fe_grid_capped(w.entries)), dim3(TR_THREADS), 0, st, (long long)n, (int)batch, ids, order, s, (const unsigned*)w.off, w.cursor,
                       w.key, w.val, (const unsigned long long*)err);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_sort(cap, w.entries, (int)w.n_batches, w.off, w.key, w.val, w.tmp_key, w.tmp_val, w.long_list, w.words, nullptr, st));

    const size_t lds = train_dien_lds_bytes(d, tile);
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_te_step), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long long ndp = d.n_params - d.n_table;
    const unsigned dense_grid = fe_grid_capped(ndp), table_grid = fe_grid_capped(d.n_table);
    long long step = 0;
    for (int ep = 0; ep < epochs; ++ep)
        for (long long b = 0; b < w.n_batches; ++b, ++step) {
            const long long first = b * batch;
            const int nb = (int)(n - first < batch ? n - first : batch);
            const int tiles = (nb + tile - 1) / tile;
            hipLaunchKernelGGL(k_te_step, dim3((unsigned)tiles), dim3(TR_THREADS), lds, st, d, ids, dense, labels, order, first, nb, (int)tile, (const float*)params,
                               p + (size_t)ep * (size_t)n + (size_t)first, w.drow, w.partial, (const unsigned long long*)err);
            hipLaunchKernelGGL(k_tr_dense_adam, dim3(dense_grid), dim3(TR_THREADS), 0, st, sched, tiles, (const float*)w.partial, params, m, v, alphas, step,
                               one_minus_beta1, one_minus_beta2, epsilon, (const unsigned long long*)err);
            hipLaunchKernelGGL(k_td_table_adam, dim3(table_grid), dim3(TR_THREADS), 0, st, s, (int)tile, (const unsigned*)w.off, b, (const long long*)w.key,
                               (const float*)w.drow, params, m, v, alphas, step, one_minus_beta1, one_minus_beta2, epsilon, (const unsigned long long*)err);
            HIP_TRY(hipGetLastError());
        }
    return SPRK_OK;
}

}  // extern "C"
