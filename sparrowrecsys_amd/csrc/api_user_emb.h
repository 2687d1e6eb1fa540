// api_user_emb.h -- C ABI: sprk_user_emb / sprk_user_emb_workspace_bytes, ratings + item embeddings -> user embeddings on the device
// (k_user_emb.h).  From host_segments.h: the carver and the workspace check, the grids, the counts-only seg_scan, seg_sort behind the
// `ungrouped` word.  Every argument is checked before any device call; the call enqueues its kernels on the caller's stream and
// returns: no synchronisation, no memory of its own.
namespace {
// The workspace, carved in this order; every part starts on a 16-byte boundary.  [zeroed] parts are cleared by one memset per call.
struct UeWorkspace {
    unsigned* seg_off;             // [n_users + 1]  len, then its exclusive scan                       [zeroed]
    unsigned* runs;                // [n_users]      runs of the user's rows in the input               [zeroed]
    unsigned* cursor;              // [n_users]      scatter cursors                                    [zeroed]
    unsigned* words;               // [4]            UE_W_*: long segments, ungrouped, next user        [zeroed]
    size_t zeroed_bytes;
    unsigned* first;               // [n_users]      the first row of the user's (only) run
    unsigned* tops;                // [n_tiles]
    int* long_list;                // [n / 64 + 1]
    int* seg_item;                 // [n]
    int* tmp_item;                 // [n]
    long long* seg_key;            // [n]
    long long* tmp_key;            // [n]
    int n_tiles;
    size_t bytes;
};
inline bool ue_sizes_ok(int64_t n, int32_t n_users) { return n >= 0 && n < 0x7fffffffll && n_users >= 0 && n_users < 0x7fffffff; }
UeWorkspace ue_carve(void* base, int64_t n, int32_t n_users) {
    UeWorkspace w;
    Carver c{base};
    const size_t nu = (size_t)n_users, nr = (size_t)n;
    w.seg_off = c.take<unsigned>(nu + 1);
    w.runs = c.take<unsigned>(nu);
    w.cursor = c.take<unsigned>(nu);
    w.words = c.take<unsigned>(4);
    w.zeroed_bytes = c.at;
    w.n_tiles = seg_scan_tiles(nu);
    w.first = c.take<unsigned>(nu);
    w.tops = c.take<unsigned>((size_t)w.n_tiles);
    w.long_list = c.take<int>(nr / 64 + 1);
    w.seg_item = c.take<int>(nr);
    w.tmp_item = c.take<int>(nr);
    w.seg_key = c.take<long long>(nr);
    w.tmp_key = c.take<long long>(nr);
    w.bytes = c.at;
    return w;
}
}  // namespace

extern "C" {

size_t sprk_user_emb_workspace_bytes(int64_t n_ratings, int32_t n_users) {
    if (!ue_sizes_ok(n_ratings, n_users)) return 0;
    return ue_carve(nullptr, n_ratings, n_users).bytes;
}

int sprk_user_emb(const int32_t* user_id, const int32_t* item_row, int64_t n_ratings, int32_t n_users,
                  const float* item_emb, const uint8_t* item_has, int32_t n_items, int32_t D, int32_t item_stride,
                  int32_t mode, float* user_emb, int32_t user_stride, uint8_t* user_has, int32_t* user_count,
                  uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_user_emb");
    // every check before any device call
    if (!ue_sizes_ok(n_ratings, n_users)) return fail(SPRK_EINVAL, "user_emb: bad sizes (need 0 <= n_ratings < 2^31 - 1, 0 <= n_users < 2^31 - 1)");
    if (n_items < 0) return fail(SPRK_EINVAL, "user_emb: n_items = %d", n_items);
    if (D < 1 || D > UE_MAX_D) return fail(SPRK_EINVAL, "user_emb: D = %d outside [1, %d]", D, UE_MAX_D);
    if (item_stride < D || user_stride < D) return fail(SPRK_EINVAL, "user_emb: item_stride = %d, user_stride = %d, a row holds D = %d floats", item_stride, user_stride, D);
    if (mode != 0 && mode != 1) return fail(SPRK_EINVAL, "user_emb: mode = %d (0 = mean over the user's rows, 1 = sum)", mode);
    if (!error_key) return fail(SPRK_EINVAL, "user_emb: NULL error word");
    if ((uintptr_t)error_key & 7) return fail(SPRK_EINVAL, "user_emb: misaligned error word");
    if (n_ratings > 0 && (!user_id || !item_row)) return fail(SPRK_EINVAL, "user_emb: NULL rating column");
    if (n_items > 0 && (!item_emb || !item_has)) return fail(SPRK_EINVAL, "user_emb: NULL item table");
    if (n_users > 0 && (!user_emb || !user_has || !user_count)) return fail(SPRK_EINVAL, "user_emb: NULL output");
    if (((uintptr_t)user_id & 3) || ((uintptr_t)item_row & 3) || ((uintptr_t)item_emb & 3) || ((uintptr_t)user_emb & 3) || ((uintptr_t)user_count & 3))
        return fail(SPRK_EINVAL, "user_emb: misaligned column");
    const UeWorkspace w = ue_carve(workspace, n_ratings, n_users);
    SPRK_TRY(check_workspace("user_emb", "sprk_user_emb_workspace_bytes", workspace, workspace_bytes, w.bytes));
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_ratings;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_ue_count, dim3(fe_grid_capped(n)), dim3(UE_THREADS), 0, st, n, user_id, (int)n_users, w.seg_off, w.runs, w.first, w.words, (unsigned long long*)error_key);
        HIP_TRY(hipGetLastError());
    }
    if (n_users == 0) return SPRK_OK;                                       // no row to write (every rating was an error, and is reported)
    SPRK_TRY(seg_scan(w.seg_off, (long long)n_users + 1, w.tops, w.n_tiles, FeScanKept<false>{}, st));
    if (n > 0) {                                                            // each of these does nothing unless k_ue_count raised `ungrouped`
        hipLaunchKernelGGL(k_ue_scatter, dim3(fe_grid_capped(n)), dim3(UE_THREADS), 0, st, n, user_id, item_row, (int)n_users, (const unsigned*)w.seg_off, w.cursor, w.seg_key, w.seg_item,
                           (const unsigned*)w.words);
        HIP_TRY(hipGetLastError());
        SPRK_TRY(seg_sort(cap, n, n_users, w.seg_off, w.seg_key, w.seg_item, w.tmp_key, w.tmp_item, w.long_list, w.words + UE_W_LONG, w.words + UE_W_UNGROUPED, st));
    }
    const bool narrow = D <= 16;                                            // 16 lanes a user, four users a wave; else a wave a user
    const long long groups = ((long long)n_users + (narrow ? 15 : 3)) / (narrow ? 16 : 4);       // workgroups that give every user its own lanes
    const unsigned sg = groups < (long long)fe_max_grid() ? (unsigned)groups : fe_max_grid();
    if (narrow)
        hipLaunchKernelGGL(k_ue_sum<16>, dim3(sg), dim3(UE_THREADS), 0, st, (int)n_users, (const unsigned*)w.seg_off, (const unsigned*)w.first, (const int*)w.seg_item, item_row, item_emb,
                           item_has, (int)n_items, (int)D, (int)item_stride, (int)mode, user_emb, (int)user_stride, user_has, user_count, w.words);
    else
        hipLaunchKernelGGL(k_ue_sum<64>, dim3(sg), dim3(UE_THREADS), 0, st, (int)n_users, (const unsigned*)w.seg_off, (const unsigned*)w.first, (const int*)w.seg_item, item_row, item_emb,
                           item_has, (int)n_items, (int)D, (int)item_stride, (int)mode, user_emb, (int)user_stride, user_has, user_count, w.words);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
