// api_user_emb.h -- C ABI: sprk_user_emb / sprk_user_emb_workspace_bytes, ratings + item embeddings -> user embeddings on the device
// (k_user_emb.h).  Part of sparrow_feature_eng.hip, after api_feature_eng.h, whose sort capacity, grids and long-segment sort it uses.
// Every argument is checked before any device call; the call enqueues its kernels on the caller's stream and returns: no
// synchronisation, no memory of its own.
namespace {
// The workspace, carved in this order; every part starts on a 16-byte boundary.  [zeroed] parts are cleared by one memset per call.
struct UeWorkspace {
    unsigned* seg_off;             // [n_users + 1]  len, then its exclusive scan                       [zeroed]
    unsigned* runs;                // [n_users]      runs of the user's rows in the input               [zeroed]
    unsigned* cursor;              // [n_users]      scatter cursors                                    [zeroed]
    unsigned* words;               // [4]            UE_W_*: long segments, ungrouped, next user        [zeroed]
    size_t zeroed_bytes;
    unsigned* first;               // [n_users]      the first row of the user's (only) run
    unsigned* kept_off;            // [n_users + 1]  k_fe_scan_*'s second scan, unused here
    unsigned* tops;                // [2 * n_tiles]
    long long* n_kept;             // [2]            k_fe_scan_add's total, unused here
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
    size_t o = 0;
    auto take = [&](size_t count, size_t elem) { const size_t at = o; o += (count * elem + 15) / 16 * 16; return (unsigned char*)base + at; };
    const size_t nu = (size_t)n_users, nr = (size_t)n;
    w.seg_off = (unsigned*)take(nu + 1, 4);
    w.runs = (unsigned*)take(nu, 4);
    w.cursor = (unsigned*)take(nu, 4);
    w.words = (unsigned*)take(4, 4);
    w.zeroed_bytes = o;
    w.n_tiles = (int)((nu + 1 + FE_SCAN_TILE - 1) / FE_SCAN_TILE);
    w.first = (unsigned*)take(nu, 4);
    w.kept_off = (unsigned*)take(nu + 1, 4);
    w.tops = (unsigned*)take(2 * (size_t)w.n_tiles, 4);
    w.n_kept = (long long*)take(2, 8);
    w.long_list = (int*)take(nr / 64 + 1, 4);
    w.seg_item = (int*)take(nr, 4);
    w.tmp_item = (int*)take(nr, 4);
    w.seg_key = (long long*)take(nr, 8);
    w.tmp_key = (long long*)take(nr, 8);
    w.bytes = o;
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
    if (!workspace || workspace_bytes < w.bytes)
        return fail(SPRK_EINVAL, "user_emb: needs a workspace of %zu bytes (sprk_user_emb_workspace_bytes), got %zu", w.bytes, workspace ? workspace_bytes : (size_t)0);
    if ((uintptr_t)workspace & 15) return fail(SPRK_EINVAL, "user_emb: the workspace must start on a 16-byte boundary");
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_ratings, count = (long long)n_users + 1;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_ue_count, dim3(fe_grid_capped(n)), dim3(UE_THREADS), 0, st, n, user_id, (int)n_users, w.seg_off, w.runs, w.first, w.words, (unsigned long long*)error_key);
        HIP_TRY(hipGetLastError());
    }
    if (n_users == 0) return SPRK_OK;                                       // no row to write (every rating was an error, and is reported)
    hipLaunchKernelGGL(k_fe_scan_tiles, dim3((unsigned)w.n_tiles), dim3(FE_THREADS), 0, st, w.seg_off, w.kept_off, count, w.tops, w.n_tiles);
    hipLaunchKernelGGL(k_fe_scan_tops, dim3(1), dim3(FE_THREADS), 0, st, w.tops, w.n_tiles);
    hipLaunchKernelGGL(k_fe_scan_add, dim3(fe_grid(count)), dim3(FE_THREADS), 0, st, w.seg_off, w.kept_off, count, (const unsigned*)w.tops, w.n_tiles, w.n_kept);
    HIP_TRY(hipGetLastError());
    if (n > 0) {                                                            // each of these does nothing unless k_ue_count raised `ungrouped`
        hipLaunchKernelGGL(k_ue_scatter, dim3(fe_grid_capped(n)), dim3(UE_THREADS), 0, st, n, user_id, item_row, (int)n_users, (const unsigned*)w.seg_off, w.cursor, w.seg_key, w.seg_item,
                           (const unsigned*)w.words);
        HIP_TRY(hipGetLastError());
        const unsigned ug = (unsigned)n_users < 65536u * 16u ? (unsigned)n_users : 65536u * 16u;
        hipLaunchKernelGGL(k_ue_sort_short, dim3(ug), dim3(FE_THREADS), (size_t)cap * 12, st, (int)n_users, cap, (const unsigned*)w.seg_off, w.seg_key, w.seg_item, w.long_list, w.words);
        HIP_TRY(hipGetLastError());
        SPRK_TRY(fe_sort_long_segments(cap, n, w.seg_off, w.seg_key, w.seg_item, w.tmp_key, w.tmp_item, w.long_list, w.words + UE_W_LONG, st));
    }
    const bool narrow = D <= 16;                                            // 16 lanes a user, four users a wave; else a wave a user
    const long long groups = ((long long)n_users + (narrow ? 15 : 3)) / (narrow ? 16 : 4);       // workgroups that give every user its own lanes
    const unsigned sg = groups < FE_MAX_GRID ? (unsigned)groups : (unsigned)FE_MAX_GRID;
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
