// api_train_pair.h -- C ABI: sprk_train_pair_workspace_bytes / sprk_train_pair_fit (k_train_pair.h; sparrowrecsys_amd/trainer_pair.py has the definition).
// As api_train_fm.h: every argument is checked before any device call; the whole fit -- k_train.h's schedule once, then three launches per step -- is
// enqueued on the caller's stream and the call returns: no synchronisation, no memory of its own.
namespace {
struct TrainPairWorkspace {
    unsigned* off;                 // [n_batches + 1]  entries per batch, then their exclusive scan       [zeroed]
    unsigned* cursor;              // [n_batches]                                                          [zeroed]
    unsigned* words;               // [4]              word 0: the long segments                           [zeroed]
    size_t zeroed_bytes;
    unsigned* tops;                // [n_tiles]
    int* long_list;                // [entries / 64 + 1]
    long long* key;                // [entries]        entries = n x fields
    long long* tmp_key;            // [entries]
    int* val;                      // [entries]
    int* tmp_val;                  // [entries]
    float* de;                     // [batch' x fields x emb_dim]   batch' = min(batch, n)
    float* dd;                     // [batch' x n_deep x emb_dim]   (tables not shared)
    float* dfirst;                 // [batch']
    float* partial;                // [ceil(batch' / tile) x ndp]
    long long n_batches, entries;
    int scan_tiles, step_tiles, rows;
    size_t bytes;
};

// the model as the kernels take it; false: a field out of range
bool train_pair_dims(const sprk_train_pair_model* mo, PairDims* out) {
    if (!mo) return false;
    PairDims d;
    memset(&d, 0, sizeof(d));
    if (mo->n_fields < 1 || mo->n_fields > TP_MAX_FIELDS || mo->n_pairs < 1 || mo->n_pairs > TP_MAX_PAIRS || mo->n_layers < 1 || mo->n_layers > TP_MAX_LAYERS ||
        mo->emb_dim < 1 || mo->emb_dim > TP_MAX_DIM || mo->n_dense < 0 || mo->n_deep < 0 || mo->n_deep > mo->n_fields || mo->n_x < 1 || mo->n_x > TP_MAX_X ||
        (long long)mo->n_deep * mo->emb_dim + mo->n_dense != mo->n_x)
        return false;
    d.n_fields = mo->n_fields; d.n_dense = mo->n_dense; d.emb_dim = mo->emb_dim; d.n_pairs = mo->n_pairs; d.n_deep = mo->n_deep; d.shared = mo->shared ? 1 : 0;
    d.n_x = mo->n_x; d.n_layers = mo->n_layers;
    long long at = 0, rows = 0;
    for (int f = 0; f < d.n_fields; ++f) {
        if (mo->vocab[f] < 1) return false;
        d.vocab[f] = mo->vocab[f]; d.fo_off[f] = mo->fo_off[f]; d.field_slot[f] = -1; d.fo_rank[f] = f;
        d.tab_off[f] = at; d.row_base[f] = rows;
        at += (long long)mo->vocab[f] * d.emb_dim; rows += mo->vocab[f];
    }
    d.row_base[d.n_fields] = rows;
    if (rows >= 0x7fffffffll) return false;
    d.fo_total = (int)rows;
    for (int a = 1; a < d.n_fields; ++a)                                    // the fields by their first-order offset: blocks that tile [0, rows)
        for (int b = a; b > 0 && d.fo_off[d.fo_rank[b]] < d.fo_off[d.fo_rank[b - 1]]; --b) { const int t = d.fo_rank[b]; d.fo_rank[b] = d.fo_rank[b - 1]; d.fo_rank[b - 1] = t; }
    long long want = 0;
    for (int q = 0; q < d.n_fields; ++q) {
        if (d.fo_off[d.fo_rank[q]] != want) return false;
        want += d.vocab[d.fo_rank[q]];
    }
    for (int q = 0; q < d.n_pairs; ++q) {
        if (mo->pair_a[q] < 0 || mo->pair_a[q] >= d.n_fields || mo->pair_b[q] < 0 || mo->pair_b[q] >= d.n_fields) return false;
        d.pair_a[q] = (signed char)mo->pair_a[q]; d.pair_b[q] = (signed char)mo->pair_b[q];
    }
    d.n_emb = at;
    for (int j = 0; j < d.n_deep; ++j) {
        const int f = mo->deep_col[j];
        if (f < 0 || f >= d.n_fields || d.field_slot[f] >= 0) return false;
        d.deep_col[j] = f; d.field_slot[f] = j;
        if (d.shared) d.dtab_off[j] = d.tab_off[f];
        else { d.dtab_off[j] = at; at += (long long)d.vocab[f] * d.emb_dim; }
    }
    d.n_tab = at;
    for (int e = 0; e < d.n_deep * d.emb_dim; ++e) d.xinv[e] = -1;
    int numerics[TP_MAX_X];
    for (int k = 0; k < d.n_dense; ++k) numerics[k] = 0;
    for (int k = 0; k < d.n_x; ++k) {                                        // every element of every deep table's row and every numeric, once each
        const int j = mo->xsrc[k], s = mo->xsub[k];
        if (j < 0) {
            if (j != -1 || s < 0 || s >= d.n_dense || numerics[s]++) return false;
        } else {
            if (j >= d.n_deep || s < 0 || s >= d.emb_dim || d.xinv[j * d.emb_dim + s] >= 0) return false;
            d.xinv[j * d.emb_dim + s] = (short)k;
        }
        d.xsrc[k] = (signed char)j; d.xsub[k] = (short)s;
    }
    int fan = d.n_x, wide = d.n_x;
    for (int l = 0; l < d.n_layers; ++l) {
        const int h = mo->width[l];
        if (h < 1 || h > TP_MAX_WIDTH) return false;
        d.width[l] = h; d.fan[l] = fan;
        d.ker_off[l] = at; at += (long long)fan * h;
        d.bias_off[l] = at; at += h;
        fan = h;
        if (h > wide) wide = h;
    }
    d.wide = wide;
    d.head_bias = at; at += 1;                                               // the head's bias, then its kernel: head/kernel stays one array
    d.nd1 = at - d.n_tab;
    d.head_ker = at; at += d.fo_total;
    d.ndp = d.nd1 + d.n_pairs + fan;
    at += d.n_pairs + fan;
    d.n_params = at;
    *out = d;
    return true;
}
inline size_t train_pair_lds_bytes(const PairDims& d, int tile) {
    size_t f = (size_t)d.n_fields * (size_t)d.emb_dim + (size_t)d.n_x + 2 * (size_t)d.n_pairs + 2 * (size_t)d.wide;
    for (int l = 0; l < d.n_layers; ++l) f += (size_t)d.width[l];
    return f * (size_t)tile * sizeof(float);
}
inline bool train_pair_sizes_ok(const PairDims& d, int64_t n, int32_t batch, int32_t tile) {
    return n >= 0 && batch >= 1 && tile >= 1 && n * d.n_fields < 0x7fffffffll && train_pair_lds_bytes(d, tile) <= 160 * 1024;
}
TrainPairWorkspace train_pair_carve(void* base, const PairDims& d, int64_t n, int32_t batch, int32_t tile) {
    TrainPairWorkspace w;
    Carver c{base};
    w.n_batches = (n + batch - 1) / batch;
    w.entries = n * d.n_fields;
    w.rows = (int)(n < batch ? n : batch);
    w.step_tiles = (w.rows + tile - 1) / tile;
    const size_t nb = (size_t)w.n_batches, ne = (size_t)w.entries;
    w.off = c.take<unsigned>(nb + 1);
    w.cursor = c.take<unsigned>(nb);
    w.words = c.take<unsigned>(4);
    w.zeroed_bytes = c.at;
    w.scan_tiles = seg_scan_tiles(nb);
    w.tops = c.take<unsigned>((size_t)w.scan_tiles);
    w.long_list = c.take<int>(ne / 64 + 1);
    w.key = c.take<long long>(ne);
    w.tmp_key = c.take<long long>(ne);
    w.val = c.take<int>(ne);
    w.tmp_val = c.take<int>(ne);
    w.de = c.take<float>((size_t)w.rows * (size_t)d.n_fields * (size_t)d.emb_dim);
    w.dd = c.take<float>(d.shared ? 0 : (size_t)w.rows * (size_t)d.n_deep * (size_t)d.emb_dim);
    w.dfirst = c.take<float>((size_t)w.rows);
    w.partial = c.take<float>((size_t)w.step_tiles * (size_t)d.ndp);
    w.bytes = c.at;
    return w;
}
}  // namespace

extern "C" {

size_t sprk_train_pair_workspace_bytes(const sprk_train_pair_model* model, int64_t n, int32_t batch, int32_t tile) {
    PairDims d;
    if (!train_pair_dims(model, &d) || !train_pair_sizes_ok(d, n, batch, tile)) return 0;
    return train_pair_carve(nullptr, d, n, batch, tile).bytes;
}

int sprk_train_pair_fit(const sprk_train_pair_model* model, const int32_t* ids, const float* dense, const float* labels, const int32_t* order, int64_t n,
                        int32_t batch, int32_t tile, int32_t epochs, const float* alphas, float one_minus_beta1, float one_minus_beta2, float epsilon,
                        float* params, float* m, float* v, float* p, uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_train_pair_fit");
    PairDims d;
    if (!train_pair_dims(model, &d))
        return fail(SPRK_EINVAL, "train_pair_fit: bad model (need 1..%d fields whose first-order blocks tile the first rows of head/kernel, 1..%d pairs of fields, "
                                 "0..fields distinct deep fields, 1..%d hidden layers of 1..%d units, emb_dim 1..%d, 1..%d deep inputs = every element of every deep "
                                 "table's row and every numeric once, all fields' rows < 2^31 - 1)",
                    TP_MAX_FIELDS, TP_MAX_PAIRS, TP_MAX_LAYERS, TP_MAX_WIDTH, TP_MAX_DIM, TP_MAX_X);
    if (n < 0 || batch < 1 || tile < 1 || epochs < 0) return fail(SPRK_EINVAL, "train_pair_fit: n = %lld, batch = %d, tile = %d, epochs = %d", (long long)n, batch, tile, epochs);
    if (n * d.n_fields >= 0x7fffffffll)
        return fail(SPRK_EINVAL, "train_pair_fit: n x fields = %lld: the schedule's unsigned offsets and the sort take fewer than 2^31 - 1 entries", (long long)(n * d.n_fields));
    if (train_pair_lds_bytes(d, tile) > 160 * 1024)
        return fail(SPRK_EINVAL, "train_pair_fit: tile = %d needs %zu bytes of LDS for this model, more than %d", tile, train_pair_lds_bytes(d, tile), 160 * 1024);
    if (!error_key) return fail(SPRK_EINVAL, "train_pair_fit: NULL error word");
    if ((uintptr_t)error_key & 7) return fail(SPRK_EINVAL, "train_pair_fit: misaligned error word");
    if (!params || !m || !v) return fail(SPRK_EINVAL, "train_pair_fit: NULL parameters or moments");
    if (n > 0 && (!ids || !labels || (d.n_dense > 0 && !dense))) return fail(SPRK_EINVAL, "train_pair_fit: NULL ids, dense or labels");
    if (n > 0 && epochs > 0 && (!alphas || !p)) return fail(SPRK_EINVAL, "train_pair_fit: NULL alphas or p");
    if (((uintptr_t)ids & 3) || ((uintptr_t)dense & 3) || ((uintptr_t)labels & 3) || ((uintptr_t)order & 3) || ((uintptr_t)alphas & 3) || ((uintptr_t)params & 3) ||
        ((uintptr_t)m & 3) || ((uintptr_t)v & 3) || ((uintptr_t)p & 3))
        return fail(SPRK_EINVAL, "train_pair_fit: misaligned array");
    const TrainPairWorkspace w = train_pair_carve(workspace, d, n, batch, tile);
    SPRK_TRY(check_workspace("train_pair_fit", "sprk_train_pair_workspace_bytes", workspace, workspace_bytes, w.bytes));
    if (n == 0 || epochs == 0) return SPRK_OK;
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* err = (unsigned long long*)error_key;
    const unsigned long long* cerr = err;

    TrainDims sched;                                                         // what k_tr_check, k_tr_count and k_tr_scatter read of a model
    memset(&sched, 0, sizeof(sched));
    sched.n_cols = d.n_fields; sched.n_dense = d.n_dense; sched.emb_dim = d.emb_dim;
    for (int f = 0; f < d.n_fields; ++f) { sched.vocab[f] = d.vocab[f]; sched.genre[f] = model->genre[f] ? 1 : 0; sched.row_base[f] = d.row_base[f]; }
    sched.row_base[d.n_fields] = d.row_base[d.n_fields];

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    hipLaunchKernelGGL(k_tr_check, dim3(fe_grid_capped(n)), dim3(TR_THREADS), 0, st, (long long)n, ids, dense, labels, sched, err);
    hipLaunchKernelGGL(k_tr_count, dim3(fe_grid_capped(w.entries)), dim3(TR_THREADS), 0, st, (long long)n, (int)batch, ids, order, d.n_fields, w.off);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_scan(w.off, w.n_batches + 1, w.tops, w.scan_tiles, FeScanKept<false>{}, st));
    hipLaunchKernelGGL(k_tr_scatter, dim3(fe_grid_capped(w.entries)), dim3(TR_THREADS), 0, st, (long long)n, (int)batch, ids, order, sched, (const unsigned*)w.off, w.cursor,
                       w.key, w.val, cerr);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_sort(cap, w.entries, (int)w.n_batches, w.off, w.key, w.val, w.tmp_key, w.tmp_val, w.long_list, w.words, nullptr, st));

    const size_t lds = train_pair_lds_bytes(d, tile);
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tp_step), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned dense_grid = fe_grid_capped(d.ndp), table_grid = fe_grid_capped(d.n_tab + d.fo_total);
    long long step = 0;
    for (int ep = 0; ep < epochs; ++ep)
        for (long long b = 0; b < w.n_batches; ++b, ++step) {
            const long long first = b * batch;
            const int nb = (int)(n - first < batch ? n - first : batch);
            const int tiles = (nb + tile - 1) / tile;
            hipLaunchKernelGGL(k_tp_step, dim3((unsigned)tiles), dim3(TR_THREADS), lds, st, d, ids, dense, labels, order, first, nb, (int)tile, (const float*)params,
                               p + (size_t)ep * (size_t)n + (size_t)first, w.de, w.dd, w.dfirst, w.partial, cerr);
            hipLaunchKernelGGL(k_tp_dense_adam, dim3(dense_grid), dim3(TR_THREADS), 0, st, d.n_tab, d.nd1, (long long)d.fo_total, d.ndp, tiles, (const float*)w.partial, params,
                               m, v, alphas, step, one_minus_beta1, one_minus_beta2, epsilon, cerr);
            hipLaunchKernelGGL(k_tp_table_adam, dim3(table_grid), dim3(TR_THREADS), 0, st, d, (int)tile, (const unsigned*)w.off, b, (const long long*)w.key, (const float*)w.de,
                               (const float*)w.dd, (const float*)w.dfirst, params, m, v, alphas, step, one_minus_beta1, one_minus_beta2, epsilon, cerr);
            HIP_TRY(hipGetLastError());
        }
    return SPRK_OK;
}

}  // extern "C"
