// api_rank_eval.h -- C ABI: sprk_rank_eval / sprk_rank_eval_workspace_bytes, ranking metrics of top-K lists against held-out pairs on the
// device (k_rank_eval.h).  From host_segments.h: the carver and the workspace check, the capped grids, the counts-only seg_scan and
// seg_sort with its long path.  Every argument is checked before any device call; the call enqueues its kernels on the caller's stream
// and returns: no synchronisation, no memory of its own.
namespace {
// One side's pairs (the truth, or the seen) as per-user segments sorted by (item, input row).
struct ReSide {
    unsigned* off;                 // [n_users + 1]  len, then its exclusive scan                       [zeroed]
    unsigned* cursor;              // [n_users]      scatter cursors                                    [zeroed]
    unsigned* n_long;              // [1]            segments beyond the LDS sort                       [zeroed]
    int* long_list;                // [n / 64 + 1]
    long long* key;                // [n]            the item
    long long* tmp_key;            // [n]
    int* row;                      // [n]            the input row
    int* tmp_row;                  // [n]
};
// The workspace, carved in this order; every part starts on a 16-byte boundary.  [zeroed] parts are cleared by one memset per call.
struct ReWorkspace {
    ReSide truth, seen;
    size_t zeroed_bytes;
    unsigned* tops;                // [n_tiles]      the scan's, used by one side after the other
    double* partial;               // [n_chunks][n_ks x 6], sized for RE_MAX_KS
    unsigned* with_truth;          // [n_chunks]
    int n_tiles;
    long long n_chunks;
    size_t bytes;
};
inline bool re_sizes_ok(int64_t n_truth, int64_t n_seen, int32_t n_users, int32_t n_queries) {
    return n_truth >= 0 && n_truth < 0x7fffffffll && n_seen >= 0 && n_seen < 0x7fffffffll && n_users >= 0 && n_users < 0x7fffffff && n_queries >= 0;
}
ReWorkspace re_carve(void* base, int64_t n_truth, int64_t n_seen, int32_t n_users, int32_t n_queries) {
    ReWorkspace w;
    Carver c{base};
    const size_t nu = (size_t)n_users;
    ReSide* side[2] = {&w.truth, &w.seen};
    const size_t rows[2] = {(size_t)n_truth, (size_t)n_seen};
    for (int s = 0; s < 2; ++s) {
        side[s]->off = c.take<unsigned>(nu + 1);
        side[s]->cursor = c.take<unsigned>(nu);
        side[s]->n_long = c.take<unsigned>(1);
    }
    w.zeroed_bytes = c.at;
    w.n_tiles = seg_scan_tiles(nu);
    w.n_chunks = ((long long)n_queries + RE_CHUNK - 1) / RE_CHUNK;
    w.tops = c.take<unsigned>((size_t)w.n_tiles);
    w.partial = c.take<double>((size_t)w.n_chunks * RE_MAX_KS * RE_METRICS);
    w.with_truth = c.take<unsigned>((size_t)w.n_chunks);
    for (int s = 0; s < 2; ++s) {
        side[s]->long_list = c.take<int>(rows[s] / 64 + 1);
        side[s]->key = c.take<long long>(rows[s]);
        side[s]->tmp_key = c.take<long long>(rows[s]);
        side[s]->row = c.take<int>(rows[s]);
        side[s]->tmp_row = c.take<int>(rows[s]);
    }
    w.bytes = c.at;
    return w;
}
// counts -> offsets -> scatter -> sort, for one side; n > 0
int re_segments(const ReSide& s, const int* user, const int* item, long long n, int n_users, unsigned long long kind, unsigned* tops, int n_tiles,
                unsigned long long* err, hipStream_t st) {
    const unsigned g = fe_grid_capped(n);
    hipLaunchKernelGGL(k_re_count, dim3(g), dim3(FE_THREADS), 0, st, n, user, item, n_users, kind, s.off, err);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_scan(s.off, (long long)n_users + 1, tops, n_tiles, FeScanKept<false>{}, st));
    hipLaunchKernelGGL(k_re_scatter, dim3(g), dim3(FE_THREADS), 0, st, n, user, item, n_users, (const unsigned*)s.off, s.cursor, s.key, s.row);
    HIP_TRY(hipGetLastError());
    return seg_sort(fe_sort_cap(), n, n_users, s.off, s.key, s.row, s.tmp_key, s.tmp_row, s.long_list, s.n_long, nullptr, st);
}
}  // namespace

extern "C" {

size_t sprk_rank_eval_workspace_bytes(int64_t n_truth, int64_t n_seen, int32_t n_users, int32_t n_queries) {
    if (!re_sizes_ok(n_truth, n_seen, n_users, n_queries)) return 0;
    return re_carve(nullptr, n_truth, n_seen, n_users, n_queries).bytes;
}

int sprk_rank_eval(const int32_t* pred, int32_t n_queries, int32_t list_len, int32_t pred_stride, const int32_t* query_user,
                   const int32_t* truth_user, const int32_t* truth_item, int64_t n_truth,
                   const int32_t* seen_user, const int32_t* seen_item, int64_t n_seen, int32_t n_users,
                   const int32_t* ks, int32_t n_ks, const double* gain, const double* gain_sum,
                   double* per_query, int32_t* n_relevant, int32_t* n_ranked, double* sums, int64_t* counts,
                   uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_rank_eval");
    // every check before any device call
    if (!re_sizes_ok(n_truth, n_seen, n_users, n_queries))
        return fail(SPRK_EINVAL, "rank_eval: bad sizes (need 0 <= n_truth, n_seen, n_users < 2^31 - 1 and n_queries >= 0)");
    if (list_len < 1 || list_len > RE_MAX_LIST) return fail(SPRK_EINVAL, "rank_eval: list_len = %d outside [1, %d]", list_len, RE_MAX_LIST);
    if (pred_stride < list_len) return fail(SPRK_EINVAL, "rank_eval: pred_stride = %d, a list holds list_len = %d entries", pred_stride, list_len);
    if (n_ks < 1 || n_ks > RE_MAX_KS) return fail(SPRK_EINVAL, "rank_eval: n_ks = %d outside [1, %d]", n_ks, RE_MAX_KS);
    if (!ks) return fail(SPRK_EINVAL, "rank_eval: NULL ks (a host array of n_ks cut-offs)");
    ReCutoffs cut;
    memset(&cut, 0, sizeof cut);
    for (int j = 0; j < n_ks; ++j) {
        if (ks[j] < 1 || ks[j] > RE_MAX_K) return fail(SPRK_EINVAL, "rank_eval: ks[%d] = %d outside [1, %d]", j, ks[j], RE_MAX_K);
        cut.k[j] = ks[j];
    }
    if (!error_key) return fail(SPRK_EINVAL, "rank_eval: NULL error word");
    if (!gain || !gain_sum) return fail(SPRK_EINVAL, "rank_eval: NULL gain table (gain [%d] and gain_sum [%d], made on the host)", RE_MAX_K, RE_MAX_K + 1);
    if (!sums || !counts) return fail(SPRK_EINVAL, "rank_eval: NULL sums or counts");
    if (n_queries > 0 && (!pred || !per_query || !n_relevant || !n_ranked)) return fail(SPRK_EINVAL, "rank_eval: NULL lists or per-query output");
    if (n_truth > 0 && (!truth_user || !truth_item)) return fail(SPRK_EINVAL, "rank_eval: NULL truth column");
    if (n_seen > 0 && (!seen_user || !seen_item)) return fail(SPRK_EINVAL, "rank_eval: NULL seen column");
    if (((uintptr_t)error_key & 7) || ((uintptr_t)gain & 7) || ((uintptr_t)gain_sum & 7) || ((uintptr_t)per_query & 7) || ((uintptr_t)sums & 7) || ((uintptr_t)counts & 7))
        return fail(SPRK_EINVAL, "rank_eval: misaligned 8-byte array (error word, gain tables, per_query, sums, counts)");
    if (((uintptr_t)pred & 3) || ((uintptr_t)query_user & 3) || ((uintptr_t)truth_user & 3) || ((uintptr_t)truth_item & 3) || ((uintptr_t)seen_user & 3) ||
        ((uintptr_t)seen_item & 3) || ((uintptr_t)n_relevant & 3) || ((uintptr_t)n_ranked & 3))
        return fail(SPRK_EINVAL, "rank_eval: misaligned int32 column");
    const ReWorkspace w = re_carve(workspace, n_truth, n_seen, n_users, n_queries);
    SPRK_TRY(check_workspace("rank_eval", "sprk_rank_eval_workspace_bytes", workspace, workspace_bytes, w.bytes));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* err = (unsigned long long*)error_key;
    const int width = n_ks * RE_METRICS;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    // (a side without rows keeps its zeroed offsets: every segment is empty.  n_users == 0: every row and every query is an error)
    if (n_truth > 0) SPRK_TRY(re_segments(w.truth, truth_user, truth_item, n_truth, n_users, RE_ERR_TRUTH, w.tops, w.n_tiles, err, st));
    if (n_seen > 0) SPRK_TRY(re_segments(w.seen, seen_user, seen_item, n_seen, n_users, RE_ERR_SEEN, w.tops, w.n_tiles, err, st));
    if (n_queries > 0) {
        hipLaunchKernelGGL(k_re_users, dim3(fe_grid_capped(n_queries)), dim3(FE_THREADS), 0, st, (long long)n_queries, query_user, (int)n_users, err);
        hipLaunchKernelGGL(k_re_eval, dim3(fe_grid_capped((long long)n_queries * 64)), dim3(FE_THREADS), 0, st, pred, (long long)n_queries, (int)list_len, (long long)pred_stride,
                           query_user, (const unsigned*)w.truth.off, (const long long*)w.truth.key, (const unsigned*)w.seen.off, (const long long*)w.seen.key, cut, (int)n_ks, gain,
                           gain_sum, per_query, n_relevant, n_ranked, (const unsigned long long*)err);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_re_partial, dim3(fe_grid_capped(w.n_chunks * (width + 1))), dim3(FE_THREADS), 0, st, (long long)n_queries, width, (const double*)per_query,
                           (const int*)n_relevant, w.partial, w.with_truth, (const unsigned long long*)err);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_re_total, dim3(1), dim3(FE_THREADS), 0, st, (long long)n_queries, width, (const double*)w.partial, (const unsigned*)w.with_truth, sums, (long long*)counts,
                       (const unsigned long long*)err);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
