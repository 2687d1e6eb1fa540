// api_split.h -- C ABI: sprk_split_plan (+ sprk_split_plan_workspace_bytes) and sprk_take_rows, the held-out split of the samples on the
// device (k_split.h).  From host_segments.h: the carver and the workspace check, the capped grids, the counts-only seg_scan.  Every
// argument is checked before any device call; the calls enqueue their kernels on the caller's stream and return: no synchronisation,
// no memory of their own.
namespace {
// The workspace of sprk_split_plan, carved in this order; every part starts on a 16-byte boundary.  [zeroed] parts are cleared by one
// memset per call.
struct SplitWorkspace {
    unsigned* hist;                // [8][256]          the select's bins, a table per pass                 [zeroed]
    unsigned long long* n_sampled; // [1]                                                                   [zeroed]
    unsigned long long* sel;       // [2]               the digits picked so far, the remaining rank        [zeroed]
    unsigned* gate;                // [1]               the error word was set as the call started          [zeroed]
    unsigned* cnt;                 // [2 n_tiles + 1]   training rows per tile, test rows per tile, then their scan; the last holds the total  [zeroed]
    size_t zeroed_bytes;
    unsigned* tops;                // [scan tiles]
    unsigned char* flags;          // [n]
    int n_tiles, scan_tiles;
    size_t bytes;
};
inline bool split_size_ok(int64_t n) { return n >= 0 && n < 0x7fffffffll; }
SplitWorkspace split_carve(void* base, int64_t n) {
    SplitWorkspace w;
    Carver c{base};
    w.n_tiles = (int)((n + SPLIT_TILE - 1) / SPLIT_TILE);
    w.scan_tiles = seg_scan_tiles(2 * (size_t)w.n_tiles);
    w.hist = c.take<unsigned>(8 * 256);
    w.n_sampled = c.take<unsigned long long>(1);
    w.sel = c.take<unsigned long long>(2);
    w.gate = c.take<unsigned>(1);
    w.cnt = c.take<unsigned>(2 * (size_t)w.n_tiles + 1);
    w.zeroed_bytes = c.at;
    w.tops = c.take<unsigned>((size_t)w.scan_tiles);
    w.flags = c.take<unsigned char>((size_t)n);
    w.bytes = c.at;
    return w;
}
// workgroups for `tiles` tiles, under the grid cap
inline unsigned split_tile_grid(int tiles) { return fe_grid_capped((long long)tiles * FE_THREADS); }
}  // namespace

extern "C" {

size_t sprk_split_plan_workspace_bytes(int64_t n) {
    if (!split_size_ok(n)) return 0;
    return split_carve(nullptr, n).bytes;
}

int sprk_split_plan(const void* key, int32_t key_kind, const int64_t* timestamp, int64_t n, uint64_t seed, uint64_t t_sample, uint64_t t_train, double train,
                    int32_t mode, int32_t* index_train, int32_t* index_test, int64_t* words, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_split_plan");
    // every check before any device call
    if (!split_size_ok(n)) return fail(SPRK_EINVAL, "split_plan: bad size (need 0 <= n < 2^31 - 1)");
    if (mode != SPLIT_RANDOM && mode != SPLIT_TIME) return fail(SPRK_EINVAL, "split_plan: mode = %d (0 = random, 1 = time)", mode);
    if (key_kind != SPLIT_KEY_POSITION && key_kind != SPLIT_KEY_I32 && key_kind != SPLIT_KEY_I64)
        return fail(SPRK_EINVAL, "split_plan: key_kind = %d (0 = the position, 1 = int32, 2 = int64)", key_kind);
    if (t_sample > (1ull << 53) || t_train > (1ull << 53)) return fail(SPRK_EINVAL, "split_plan: a threshold above 2^53");
    if (!(train >= 0.0 && train <= 1.0)) return fail(SPRK_EINVAL, "split_plan: train = %g outside [0, 1]", train);
    if (!words) return fail(SPRK_EINVAL, "split_plan: NULL words");
    if (n > 0 && key_kind != SPLIT_KEY_POSITION && !key) return fail(SPRK_EINVAL, "split_plan: NULL key column");
    if (n > 0 && mode == SPLIT_TIME && !timestamp) return fail(SPRK_EINVAL, "split_plan: mode 1 (time) needs the timestamp column");
    if (n > 0 && (!index_train || !index_test)) return fail(SPRK_EINVAL, "split_plan: NULL index list");
    if (((uintptr_t)words & 7) || ((uintptr_t)timestamp & 7) || ((uintptr_t)key & (key_kind == SPLIT_KEY_I64 ? 7 : 3)) || ((uintptr_t)index_train & 3) ||
        ((uintptr_t)index_test & 3))
        return fail(SPRK_EINVAL, "split_plan: misaligned column, index list or words");
    const SplitWorkspace w = split_carve(workspace, n);
    SPRK_TRY(check_workspace("split_plan", "sprk_split_plan_workspace_bytes", workspace, workspace_bytes, w.bytes));
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long* err = (const unsigned long long*)words;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    if (n > 0) {
        const unsigned rg = fe_grid_capped(n), tg = split_tile_grid(w.n_tiles);
        hipLaunchKernelGGL(k_split_begin, dim3(1), dim3(64), 0, st, err, w.gate);
        hipLaunchKernelGGL(k_split_flags, dim3(rg), dim3(FE_THREADS), 0, st, key, (int)key_kind, (long long)n, (unsigned long long)seed, (unsigned long long)t_sample,
                           (unsigned long long)t_train, (int)mode, w.flags, w.n_sampled, (const unsigned*)w.gate, (unsigned long long*)words);
        HIP_TRY(hipGetLastError());
        if (mode == SPLIT_TIME)
            for (int pass = 0; pass < 8; ++pass) {                          // the exact rank: most significant digit first
                hipLaunchKernelGGL(k_split_hist, dim3(rg), dim3(FE_THREADS), 0, st, (const unsigned char*)w.flags, (const long long*)timestamp, (long long)n, pass,
                                   (const unsigned long long*)w.sel, w.hist, err);
                hipLaunchKernelGGL(k_split_pick, dim3(1), dim3(FE_THREADS), 0, st, pass, train, (const unsigned long long*)w.n_sampled, (const unsigned*)w.hist, w.sel, err);
                HIP_TRY(hipGetLastError());
            }
        hipLaunchKernelGGL(k_split_count, dim3(tg), dim3(FE_THREADS), 0, st, (const unsigned char*)w.flags, (const long long*)timestamp, (long long)n, w.n_tiles, (int)mode,
                           (const unsigned long long*)w.sel, w.cnt, err);
        HIP_TRY(hipGetLastError());
        // (the scan has no error word of its own: on an error it scans the zeroed counts, within the workspace)
        SPRK_TRY(seg_scan(w.cnt, 2 * (long long)w.n_tiles + 1, w.tops, w.scan_tiles, FeScanKept<false>{}, st));
        hipLaunchKernelGGL(k_split_write, dim3(tg), dim3(FE_THREADS), 0, st, (const unsigned char*)w.flags, (const long long*)timestamp, (long long)n, w.n_tiles, (int)mode,
                           (const unsigned long long*)w.sel, (const unsigned*)w.cnt, index_train, index_test, err);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_split_words, dim3(1), dim3(64), 0, st, w.n_tiles, (int)mode, (const unsigned long long*)w.n_sampled, (const unsigned long long*)w.sel,
                       (const unsigned*)w.cnt, (long long*)words);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

int sprk_take_rows(const sprk_split_col* cols, int32_t n_cols, const int32_t* index, int64_t n_index, int64_t n_rows, void* stream) {
    RoctxRange roctx_range_("sprk_take_rows");
    // every check before any device call
    if (n_cols < 0 || (n_cols > 0 && !cols)) return fail(SPRK_EINVAL, "take_rows: n_cols = %d, cols = %p", n_cols, (const void*)cols);
    if (!split_size_ok(n_index) || !split_size_ok(n_rows)) return fail(SPRK_EINVAL, "take_rows: bad sizes (need 0 <= n_index, n_rows < 2^31 - 1)");
    if (n_index > 0 && !index) return fail(SPRK_EINVAL, "take_rows: NULL index");
    if ((uintptr_t)index & 3) return fail(SPRK_EINVAL, "take_rows: misaligned index");
    for (int c = 0; c < n_cols; ++c) {
        const sprk_split_col& col = cols[c];
        if (col.row_bytes < 4 || (col.row_bytes & 3)) return fail(SPRK_EINVAL, "take_rows: column %d: row_bytes = %d must be a positive multiple of 4", c, col.row_bytes);
        if (col.src_stride < 0 || (col.src_stride & 3)) return fail(SPRK_EINVAL, "take_rows: column %d: src_stride = %lld must be a multiple of 4, not negative", c, (long long)col.src_stride);
        if (n_index > 0 && (!col.src || !col.dst)) return fail(SPRK_EINVAL, "take_rows: column %d: NULL source or destination", c);
        if (((uintptr_t)col.src & 3) || ((uintptr_t)col.dst & 3)) return fail(SPRK_EINVAL, "take_rows: column %d: misaligned source or destination", c);
    }
    if (n_index == 0 || n_cols == 0) return SPRK_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int at = 0; at < n_cols; at += SPLIT_MAX_COLS) {
        const int count = n_cols - at < SPLIT_MAX_COLS ? n_cols - at : SPLIT_MAX_COLS;
        SplitColSet set;
        memset(&set, 0, sizeof set);
        long long widest = 4;
        for (int c = 0; c < count; ++c) { set.col[c] = cols[at + c]; widest = cols[at + c].row_bytes > widest ? cols[at + c].row_bytes : widest; }
        const long long units = (n_index * (widest / 4) + 3) / 4;           // of the widest column; the others loop fewer times
        hipLaunchKernelGGL(k_take_rows, dim3(fe_grid_capped(units), (unsigned)count), dim3(FE_THREADS), 0, st, set, index, (long long)n_index, (long long)n_rows);
        HIP_TRY(hipGetLastError());
    }
    return SPRK_OK;
}

}  // extern "C"
