// api_train_tower.h -- C ABI: sprk_train_tower_workspace_bytes / sprk_train_tower_fit / sprk_tower_rows (k_train_tower.h; sparrowrecsys_amd/trainer_tower.py
// has the definition).  As api_train_pair.h: every argument is checked before any device call; the whole fit -- k_train.h's schedule once, then three
// launches per step -- is enqueued on the caller's stream and the call returns: no synchronisation, no memory of its own.
namespace {
struct TrainTowerWorkspace {
    unsigned* off;                 // [n_batches + 1]  entries per batch, then their exclusive scan       [zeroed]
    unsigned* cursor;              // [n_batches]                                                          [zeroed]
    unsigned* words;               // [4]              word 0: the long segments                           [zeroed]
    size_t zeroed_bytes;
    unsigned* tops;                // [n_tiles]
    int* long_list;                // [entries / 64 + 1]
    long long* key;                // [entries]        entries = n x 2
    long long* tmp_key;            // [entries]
    int* val;                      // [entries]
    int* tmp_val;                  // [entries]
    float* dx;                     // [batch' x 2 emb_dim]   batch' = min(batch, n)
    float* partial;                // [ceil(batch' / tile) x Dense parameters]
    long long n_batches, entries;
    int scan_tiles, step_tiles, rows;
    size_t bytes;
};

inline size_t tower_round4(size_t floats) { return (floats + 3) & ~(size_t)3; }

// the model as the kernels take it, without the LDS carves; false: a field out of range
bool train_tower_dims(const sprk_train_tower_model* mo, TowerDims* out) {
    if (!mo) return false;
    TowerDims d;
    memset(&d, 0, sizeof(d));
    if (mo->emb_dim < 1 || mo->emb_dim > TW_MAX_DIM || mo->n_layers < 1 || mo->n_layers > TW_MAX_LAYERS || mo->vocab[0] < 1 || mo->vocab[1] < 1) return false;
    d.emb_dim = mo->emb_dim; d.n_layers = mo->n_layers;
    d.vocab[0] = mo->vocab[0]; d.vocab[1] = mo->vocab[1];
    if ((long long)d.vocab[0] + d.vocab[1] >= 0x7fffffffll) return false;
    d.tab_off[0] = 0; d.tab_off[1] = (long long)d.vocab[0] * d.emb_dim;
    long long at = ((long long)d.vocab[0] + d.vocab[1]) * d.emb_dim;
    d.n_table = at;
    int widest = 0;
    for (int s = 0; s < 2; ++s) {
        int fan = d.emb_dim;
        for (int l = 0; l < d.n_layers; ++l) {
            const int h = mo->width[l];
            if (h < 1 || h > TW_MAX_WIDTH) return false;
            d.width[l] = h; d.fan[l] = fan;
            d.ker_off[s][l] = at; at += (long long)fan * h;
            d.bias_off[s][l] = at; at += h;
            fan = h;
            if (h > widest) widest = h;
        }
    }
    d.wide = 2 * widest;
    d.head_ker = at; at += 1;
    d.head_bias = at; at += 1;
    d.n_params = at;
    *out = d;
    return true;
}
// k_tw_step's carves for a tile, each a multiple of 16 bytes: -> the bytes; `d` (may be null) receives the offsets when they fit the LDS
inline size_t train_tower_lds_bytes(const TowerDims& m, int tile, TowerDims* d) {
    const size_t t = (size_t)tile;
    size_t at = tower_round4(t * 2 * (size_t)m.emb_dim);
    size_t act[2][TW_MAX_LAYERS];
    for (int s = 0; s < 2; ++s)
        for (int l = 0; l < m.n_layers; ++l) { act[s][l] = at; at += tower_round4(t * (size_t)m.width[l]); }
    const size_t dot = at; at += tower_round4(t);
    const size_t dl = at; at += tower_round4(t);
    const size_t g0 = at; at += tower_round4(t * (size_t)m.wide);
    const size_t g1 = at; at += tower_round4(t * (size_t)m.wide);
    if (d && at * sizeof(float) <= 160 * 1024) {
        for (int s = 0; s < 2; ++s)
            for (int l = 0; l < m.n_layers; ++l) d->lds_act[s][l] = (int)act[s][l];
        d->lds_dot = (int)dot; d->lds_dl = (int)dl; d->lds_g0 = (int)g0; d->lds_g1 = (int)g1;
    }
    return at * sizeof(float);
}
inline bool train_tower_sizes_ok(const TowerDims& d, int64_t n, int32_t batch, int32_t tile) {
    return n >= 0 && batch >= 1 && tile >= 1 && n * 2 < 0x7fffffffll && train_tower_lds_bytes(d, tile, nullptr) <= 160 * 1024;
}
TrainTowerWorkspace train_tower_carve(void* base, const TowerDims& d, int64_t n, int32_t batch, int32_t tile) {
    TrainTowerWorkspace w;
    Carver c{base};
    w.n_batches = (n + batch - 1) / batch;
    w.entries = n * 2;
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
    w.dx = c.take<float>((size_t)w.rows * 2 * (size_t)d.emb_dim);
    w.partial = c.take<float>((size_t)w.step_tiles * (size_t)(d.n_params - d.n_table));
    w.bytes = c.at;
    return w;
}
}  // namespace

extern "C" {

size_t sprk_train_tower_workspace_bytes(const sprk_train_tower_model* model, int64_t n, int32_t batch, int32_t tile) {
    TowerDims d;
    if (!train_tower_dims(model, &d) || !train_tower_sizes_ok(d, n, batch, tile)) return 0;
    return train_tower_carve(nullptr, d, n, batch, tile).bytes;
}

int sprk_train_tower_fit(const sprk_train_tower_model* model, const int32_t* ids, const float* labels, const int32_t* order, int64_t n, int32_t batch, int32_t tile,
                         int32_t epochs, const float* alphas, float one_minus_beta1, float one_minus_beta2, float epsilon, float* params, float* m, float* v,
                         float* p, uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_train_tower_fit");
    TowerDims d;
    if (!train_tower_dims(model, &d))
        return fail(SPRK_EINVAL, "train_tower_fit: bad model (need emb_dim 1..%d, 1..%d hidden layers of 1..%d units, two vocabularies >= 1 with fewer than "
                                 "2^31 - 1 rows together)", TW_MAX_DIM, TW_MAX_LAYERS, TW_MAX_WIDTH);
    if (n < 0 || batch < 1 || tile < 1 || epochs < 0) return fail(SPRK_EINVAL, "train_tower_fit: n = %lld, batch = %d, tile = %d, epochs = %d", (long long)n, batch, tile, epochs);
    if (n * 2 >= 0x7fffffffll)
        return fail(SPRK_EINVAL, "train_tower_fit: n x 2 = %lld: the schedule's unsigned offsets and the sort take fewer than 2^31 - 1 entries", (long long)(n * 2));
    const size_t lds = train_tower_lds_bytes(d, tile, &d);
    if (lds > 160 * 1024) return fail(SPRK_EINVAL, "train_tower_fit: tile = %d needs %zu bytes of LDS for this model, more than %d", tile, lds, 160 * 1024);
    if (!error_key) return fail(SPRK_EINVAL, "train_tower_fit: NULL error word");
    if ((uintptr_t)error_key & 7) return fail(SPRK_EINVAL, "train_tower_fit: misaligned error word");
    if (!params || !m || !v) return fail(SPRK_EINVAL, "train_tower_fit: NULL parameters or moments");
    if (n > 0 && (!ids || !labels)) return fail(SPRK_EINVAL, "train_tower_fit: NULL ids or labels");
    if (n > 0 && epochs > 0 && (!alphas || !p)) return fail(SPRK_EINVAL, "train_tower_fit: NULL alphas or p");
    if (((uintptr_t)ids & 3) || ((uintptr_t)labels & 3) || ((uintptr_t)order & 3) || ((uintptr_t)alphas & 3) || ((uintptr_t)params & 3) || ((uintptr_t)m & 3) ||
        ((uintptr_t)v & 3) || ((uintptr_t)p & 3))
        return fail(SPRK_EINVAL, "train_tower_fit: misaligned array");
    const TrainTowerWorkspace w = train_tower_carve(workspace, d, n, batch, tile);
    SPRK_TRY(check_workspace("train_tower_fit", "sprk_train_tower_workspace_bytes", workspace, workspace_bytes, w.bytes));
    if (n == 0 || epochs == 0) return SPRK_OK;
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* err = (unsigned long long*)error_key;
    const unsigned long long* cerr = err;

    TrainDims sched;                                                         // what k_tr_check, k_tr_count and k_tr_scatter read of a model; the towers' inputs
    memset(&sched, 0, sizeof(sched));                                        // as one input of 2 emb_dim rows, movie first
    sched.n_cols = 2; sched.n_dense = 0; sched.emb_dim = d.emb_dim; sched.n_x = 2 * d.emb_dim;
    sched.n_table = d.n_table; sched.n_params = d.n_params;
    for (int c = 0; c < 2; ++c) {
        sched.vocab[c] = d.vocab[c]; sched.tab_off[c] = d.tab_off[c];
        for (int k = 0; k < d.emb_dim; ++k) { sched.xcol[c * d.emb_dim + k] = (short)c; sched.xsub[c * d.emb_dim + k] = (short)k; }
    }
    sched.row_base[1] = d.vocab[0]; sched.row_base[2] = (long long)d.vocab[0] + d.vocab[1];

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    hipLaunchKernelGGL(k_tr_check, dim3(fe_grid_capped(n)), dim3(TR_THREADS), 0, st, (long long)n, ids, (const float*)nullptr, labels, sched, err);
    hipLaunchKernelGGL(k_tr_count, dim3(fe_grid_capped(w.entries)), dim3(TR_THREADS), 0, st, (long long)n, (int)batch, ids, order, 2, w.off);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_scan(w.off, w.n_batches + 1, w.tops, w.scan_tiles, FeScanKept<false>{}, st));
    hipLaunchKernelGGL(k_tr_scatter, dim3(fe_grid_capped(w.entries)), dim3(TR_THREADS), 0, st, (long long)n, (int)batch, ids, order, sched, (const unsigned*)w.off, w.cursor,
                       w.key, w.val, cerr);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_sort(cap, w.entries, (int)w.n_batches, w.off, w.key, w.val, w.tmp_key, w.tmp_val, w.long_list, w.words, nullptr, st));

    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tw_step), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long long ndp = d.n_params - d.n_table;
    const unsigned dense_grid = fe_grid_capped(ndp), table_grid = fe_grid_capped(d.n_table);
    long long step = 0;
    for (int ep = 0; ep < epochs; ++ep)
        for (long long b = 0; b < w.n_batches; ++b, ++step) {
            const long long first = b * batch;
            const int nb = (int)(n - first < batch ? n - first : batch);
            const int tiles = (nb + tile - 1) / tile;
            hipLaunchKernelGGL(k_tw_step, dim3((unsigned)tiles), dim3(TR_THREADS), lds, st, d, ids, labels, order, first, nb, (int)tile, (const float*)params,
                               p + (size_t)ep * (size_t)n + (size_t)first, w.dx, w.partial, cerr);
            hipLaunchKernelGGL(k_tf_dense_adam, dim3(dense_grid), dim3(TR_THREADS), 0, st, d.n_table, ndp, tiles, (const float*)w.partial, params, m, v, alphas, step,
                               one_minus_beta1, one_minus_beta2, epsilon, cerr);
            hipLaunchKernelGGL(k_tw_table_adam, dim3(table_grid), dim3(TR_THREADS), 0, st, d, (int)tile, (const unsigned*)w.off, b, (const long long*)w.key,
                               (const float*)w.dx, params, m, v, alphas, step, one_minus_beta1, one_minus_beta2, epsilon, cerr);
            HIP_TRY(hipGetLastError());
        }
    return SPRK_OK;
}

int sprk_tower_rows(const sprk_train_tower_model* model, const float* params, int32_t side, int32_t tile, float* out, int64_t out_stride, void* stream) {
    RoctxRange roctx_range_("sprk_tower_rows");
    TowerDims d;
    if (!train_tower_dims(model, &d))
        return fail(SPRK_EINVAL, "tower_rows: bad model (need emb_dim 1..%d, 1..%d hidden layers of 1..%d units, two vocabularies >= 1 with fewer than "
                                 "2^31 - 1 rows together)", TW_MAX_DIM, TW_MAX_LAYERS, TW_MAX_WIDTH);
    if (side != 0 && side != 1) return fail(SPRK_EINVAL, "tower_rows: side = %d is neither 0 (item) nor 1 (user)", side);
    if (tile < 1) return fail(SPRK_EINVAL, "tower_rows: tile = %d", tile);
    if (out_stride < d.width[d.n_layers - 1]) return fail(SPRK_EINVAL, "tower_rows: out_stride = %lld below the last width %d", (long long)out_stride, d.width[d.n_layers - 1]);
    if (!params || !out) return fail(SPRK_EINVAL, "tower_rows: NULL parameters or out");
    if (((uintptr_t)params & 3) || ((uintptr_t)out & 3)) return fail(SPRK_EINVAL, "tower_rows: misaligned array");
    int widest = d.emb_dim > d.wide / 2 ? d.emb_dim : d.wide / 2;
    const size_t buf = tower_round4((size_t)tile * (size_t)widest);
    const size_t lds = 2 * buf * sizeof(float);
    if (lds > 160 * 1024) return fail(SPRK_EINVAL, "tower_rows: tile = %d needs %zu bytes of LDS for this model, more than %d", tile, lds, 160 * 1024);
    const long long n_tiles = ((long long)d.vocab[side] + tile - 1) / tile;
    const unsigned grid = (unsigned)(n_tiles < (long long)fe_max_grid() ? n_tiles : (long long)fe_max_grid());
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tw_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_tw_rows, dim3(grid), dim3(TR_THREADS), lds, (hipStream_t)stream, d, (int)side, (int)tile, (int)buf, (int)n_tiles, params, out, (long long)out_stride);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
