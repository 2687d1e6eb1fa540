// api_exact_auc.h -- C ABI: sprk_exact_auc_workspace_bytes / sprk_exact_auc_bin_bits / sprk_exact_auc, the exact ROC and PR areas over
// device-resident scores (k_exact_auc.h).  Part of sparrow_metrics.hip.  From host_segments.h: the carver and the workspace check, the
// grids, the counts-only seg_scan and the long segments' sort (k_ea_sort_short stands in for seg_sort's first launch).  Every argument is checked before any device call; the call enqueues its kernels on the
// caller's stream and returns: no synchronisation, no memory of its own.
namespace {
// The leading bits of the key that choose a row's bin: SPRK_EXACT_AUC_BIN_BITS = an integer in [1, 24], read at each call (tests and
// measurements), else by n: about n / 4 bins, between 2^8 and 2^22 (docs/exact_auc_results.md has the measurement behind the rule).
int ea_bin_bits(int64_t n) {
    if (const char* e = getenv("SPRK_EXACT_AUC_BIN_BITS")) {
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end != e && *end == 0 && v >= 1 && v <= 24) return (int)v;
    }
    int lg = 0;
    while (lg < 31 && (1ll << lg) < n) ++lg;
    const int bits = lg - 2;
    return bits < 8 ? 8 : (bits > 22 ? 22 : bits);
}

// The workspace, carved in this order; every part starts on a 16-byte boundary.  [zeroed] parts are cleared by one memset per call.
struct EaWorkspace {
    unsigned* bin_off;             // [bins + 1]     counts, then their exclusive scan                    [zeroed]
    unsigned* cursor;              // [bins]         scatter cursors                                      [zeroed]
    unsigned* words;               // [8]            EA_W_*: long segments, the sort's gate, the numerator [zeroed]
    size_t zeroed_bytes;
    unsigned* tops;                // [tiles]        of the longer of the two scans
    int* long_list;                // [n / 64 + 1]
    long long* seg_key;            // [n]            key << 1 | positive
    int* seg_row;                  // [n]
    long long* tmp_key;            // [n]            the merge passes' other side; after the sort: tp[n], fp[n] of the groups
    int* tmp_row;                  // [n]
    unsigned* start;               // [n + 1]        group starts, then their exclusive scan
    unsigned* pos;                 // [n + 1]        positives, likewise
    double* run_sum;               // [ceil(n / EA_PR_RUN)]
    int bits, bin_tiles, row_tiles;
    size_t bins, bytes;
};
inline bool ea_size_ok(int64_t n) { return n >= 1 && n < 0x7fffffffll; }
EaWorkspace ea_carve(void* base, int64_t n) {
    EaWorkspace w;
    Carver c{base};
    const size_t nr = (size_t)n;
    w.bits = ea_bin_bits(n);
    w.bins = (size_t)1 << w.bits;
    w.bin_off = c.take<unsigned>(w.bins + 1);
    w.cursor = c.take<unsigned>(w.bins);
    w.words = c.take<unsigned>(8);
    w.zeroed_bytes = c.at;
    w.bin_tiles = seg_scan_tiles(w.bins);
    w.row_tiles = seg_scan_tiles(nr);
    w.tops = c.take<unsigned>((size_t)(w.bin_tiles > w.row_tiles ? w.bin_tiles : w.row_tiles));
    w.long_list = c.take<int>(nr / 64 + 1);
    w.seg_key = c.take<long long>(nr);
    w.seg_row = c.take<int>(nr);
    w.tmp_key = c.take<long long>(nr);
    w.tmp_row = c.take<int>(nr);
    w.start = c.take<unsigned>(nr + 1);
    w.pos = c.take<unsigned>(nr + 1);
    w.run_sum = c.take<double>((nr + EA_PR_RUN - 1) / EA_PR_RUN);
    w.bytes = c.at;
    return w;
}
}  // namespace

extern "C" {

size_t sprk_exact_auc_workspace_bytes(int64_t n) {
    if (!ea_size_ok(n)) return 0;
    return ea_carve(nullptr, n).bytes;
}

int32_t sprk_exact_auc_bin_bits(int64_t n) { return ea_size_ok(n) ? ea_bin_bits(n) : 0; }

int sprk_exact_auc(const float* scores, const void* labels, int32_t label_storage, int64_t label_stride, int64_t n,
                   sprk_exact_auc_result* result, float* thresholds, uint32_t* tp, uint32_t* fp,
                   uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_exact_auc");
    static_assert(sizeof(EaResult) == sizeof(sprk_exact_auc_result), "k_exact_auc.h's result is the header's");
    // every check before any device call
    if (n < 0) return fail(SPRK_EINVAL, "exact_auc: negative n");
    if (!ea_size_ok(n)) return fail(SPRK_EINVAL, "exact_auc: n = %lld (need 1 <= n < 2^31 - 1)", (long long)n);
    int elem = 0;
    switch (label_storage) {
        case SPRK_COL_F32: case SPRK_COL_I32: elem = 4; break;
        case SPRK_COL_I64: elem = 8; break;
        case SPRK_COL_U8: case SPRK_COL_BOOL: elem = 1; break;
        default: return fail(SPRK_EINVAL, "exact_auc: label_storage = %d (float32, int32, int64, uint8 or bool labels)", label_storage);
    }
    if (label_stride <= 0 || label_stride % elem) return fail(SPRK_EINVAL, "exact_auc: label_stride = %lld is no positive multiple of the %d-byte label", (long long)label_stride, elem);
    if (label_stride > INT64_MAX / n) return fail(SPRK_EINVAL, "exact_auc: label_stride * n beyond 2^63 - 1");
    if (!scores) return fail(SPRK_EINVAL, "exact_auc: NULL scores");
    if (!labels) return fail(SPRK_EINVAL, "exact_auc: NULL labels");
    if (!result) return fail(SPRK_EINVAL, "exact_auc: NULL result");
    if (!error_key) return fail(SPRK_EINVAL, "exact_auc: NULL error word");
    if ((uintptr_t)scores & 3) return fail(SPRK_EINVAL, "exact_auc: misaligned scores");
    if ((uintptr_t)labels & (uintptr_t)(elem - 1)) return fail(SPRK_EINVAL, "exact_auc: misaligned labels");
    if (((uintptr_t)result & 7) || ((uintptr_t)error_key & 7)) return fail(SPRK_EINVAL, "exact_auc: misaligned result or error word");
    if (((uintptr_t)thresholds & 3) || ((uintptr_t)tp & 3) || ((uintptr_t)fp & 3)) return fail(SPRK_EINVAL, "exact_auc: misaligned curve array");
    const EaWorkspace w = ea_carve(workspace, n);
    if ((uintptr_t)workspace & 15) return fail(SPRK_EINVAL, "exact_auc: the workspace (sprk_exact_auc_workspace_bytes: %zu bytes) must start on a 16-byte boundary", w.bytes);
    SPRK_TRY(check_workspace("exact_auc", "sprk_exact_auc_workspace_bytes", workspace, workspace_bytes, w.bytes));
    const int cap = fe_sort_cap(), shift = 32 - w.bits;
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* lab = (const unsigned char*)labels;
    unsigned long long* err = (unsigned long long*)error_key;
    unsigned long long* roc = (unsigned long long*)(w.words + EA_W_ROC);
    unsigned* g_tp = (unsigned*)w.tmp_key;
    unsigned* g_fp = g_tp + n;
    const unsigned row_grid = fe_grid_capped(n);

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    hipLaunchKernelGGL(k_ea_count, dim3(row_grid), dim3(FE_THREADS), 0, st, (long long)n, scores, lab, (int)label_storage, (long long)label_stride, shift, w.bin_off, err);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_scan(w.bin_off, (long long)w.bins + 1, w.tops, w.bin_tiles, FeScanKept<false>{}, st));
    hipLaunchKernelGGL(k_ea_gate, dim3(1), dim3(64), 0, st, w.words, (const unsigned long long*)err);
    hipLaunchKernelGGL(k_ea_scatter, dim3(row_grid), dim3(FE_THREADS), 0, st, (long long)n, scores, lab, (int)label_storage, (long long)label_stride, shift,
                       (const unsigned*)w.bin_off, w.cursor, w.seg_key, w.seg_row, (const unsigned long long*)err);
    HIP_TRY(hipGetLastError());
    // seg_sort with k_ea_sort_short in k_fe_sort_short's place
    const unsigned sort_grid = fe_grid_own_cap((unsigned)(w.bins < 65536u * 16u ? w.bins : 65536u * 16u));
    hipLaunchKernelGGL(k_ea_sort_short, dim3(sort_grid), dim3(FE_THREADS), (size_t)cap * 12, st, (int)w.bins, cap, (const unsigned*)w.bin_off, w.seg_key, w.seg_row, w.long_list,
                       w.words + EA_W_LONG, (const unsigned*)(w.words + EA_W_GATE));
    HIP_TRY(hipGetLastError());
    SPRK_TRY(fe_sort_long_segments(cap, n, w.bin_off, w.seg_key, w.seg_row, w.tmp_key, w.tmp_row, w.long_list, w.words + EA_W_LONG, st));
    hipLaunchKernelGGL(k_ea_flags, dim3(fe_grid_capped(n + 1)), dim3(FE_THREADS), 0, st, (long long)n, (const long long*)w.seg_key, w.start, w.pos, (const unsigned long long*)err);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_scan(w.start, (long long)n + 1, w.tops, w.row_tiles, FeScanKept<false>{}, st));
    SPRK_TRY(seg_scan(w.pos, (long long)n + 1, w.tops, w.row_tiles, FeScanKept<false>{}, st));
    hipLaunchKernelGGL(k_ea_groups, dim3(row_grid), dim3(FE_THREADS), 0, st, (long long)n, (const long long*)w.seg_key, (const unsigned*)w.start, (const unsigned*)w.pos, g_tp, g_fp,
                       thresholds, (unsigned*)tp, (unsigned*)fp, (const unsigned long long*)err);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ea_roc, dim3(row_grid), dim3(FE_THREADS), 0, st, (const unsigned*)(w.start + n), (const unsigned*)g_tp, (const unsigned*)g_fp, roc, (const unsigned long long*)err);
    const long long run_groups = ((n + EA_PR_RUN - 1) / EA_PR_RUN + FE_THREADS / 64 - 1) / (FE_THREADS / 64);
    const unsigned run_grid = run_groups < (long long)fe_max_grid() ? (unsigned)run_groups : fe_max_grid();
    hipLaunchKernelGGL(k_ea_pr_runs, dim3(run_grid), dim3(FE_THREADS), 0, st, (const unsigned*)(w.start + n), (const unsigned*)g_tp, (const unsigned*)g_fp, w.run_sum,
                       (const unsigned long long*)err);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ea_finish, dim3(1), dim3(64), 0, st, (long long)n, (const unsigned*)(w.start + n), (const unsigned*)(w.pos + n), (const double*)w.run_sum,
                       (const unsigned long long*)roc, (EaResult*)result, (const unsigned long long*)err);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
