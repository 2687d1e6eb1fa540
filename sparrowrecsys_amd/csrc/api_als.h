// api_als.h -- C ABI: sprk_als_fit / sprk_als_workspace_bytes (ratings -> ALS factors on the device) and sprk_als_predict (factors ->
// scores), k_als.h.  From host_segments.h: the carver and the workspace check, the grids, and for each of the two sides the counts-only
// seg_scan and seg_sort.  Every argument is checked before any device call; the calls enqueue their kernels on the caller's stream and
// return: no synchronisation, no memory of their own.
namespace {
// The workspace, carved in this order; every part starts on a 16-byte boundary.  [zeroed] parts are cleared by one memset per call.
struct AlsWorkspace {
    unsigned* off_user;            // [n_users + 1]  len, then its exclusive scan                       [zeroed]
    unsigned* off_movie;           // [n_items + 1]                                                     [zeroed]
    unsigned* cur_user;            // [n_users]      scatter cursors                                    [zeroed]
    unsigned* cur_movie;           // [n_items]                                                         [zeroed]
    unsigned* words;               // [4]            ALS_W_*: long segments of either side, next row, stop   [zeroed]
    size_t zeroed_bytes;
    unsigned* tops;                // [n_tiles]      (the larger side's)
    int* long_user;                // [n / 64 + 1]
    int* long_movie;               // [n / 64 + 1]
    int* val_user;                 // [n]            the rating's bits, in the user's segment
    int* val_movie;                // [n]
    int* tmp_val;                  // [n]
    long long* key_user;           // [n]            movie << 32 | input row
    long long* key_movie;          // [n]            user << 32 | input row
    long long* tmp_key;            // [n]
    int tiles_user, tiles_movie;
    size_t bytes;
};
inline bool als_sizes_ok(int64_t n, int32_t n_users, int32_t n_items, int32_t rank) {
    return n >= 0 && n < 0x7fffffffll && n_users >= 0 && n_users < 0x7fffffff && n_items >= 0 && n_items < 0x7fffffff && rank >= 1 && rank <= ALS_MAX_RANK;
}
AlsWorkspace als_carve(void* base, int64_t n, int32_t n_users, int32_t n_items) {
    AlsWorkspace w;
    Carver c{base};
    const size_t nu = (size_t)n_users, ni = (size_t)n_items, nr = (size_t)n;
    w.off_user = c.take<unsigned>(nu + 1);
    w.off_movie = c.take<unsigned>(ni + 1);
    w.cur_user = c.take<unsigned>(nu);
    w.cur_movie = c.take<unsigned>(ni);
    w.words = c.take<unsigned>(4);
    w.zeroed_bytes = c.at;
    w.tiles_user = seg_scan_tiles(nu);
    w.tiles_movie = seg_scan_tiles(ni);
    w.tops = c.take<unsigned>((size_t)(w.tiles_user > w.tiles_movie ? w.tiles_user : w.tiles_movie));
    w.long_user = c.take<int>(nr / 64 + 1);
    w.long_movie = c.take<int>(nr / 64 + 1);
    w.val_user = c.take<int>(nr);
    w.val_movie = c.take<int>(nr);
    w.tmp_val = c.take<int>(nr);
    w.key_user = c.take<long long>(nr);
    w.key_movie = c.take<long long>(nr);
    w.tmp_key = c.take<long long>(nr);
    w.bytes = c.at;
    return w;
}

int als_half_sweep(int n_dst, int rank, double reg, const unsigned* off, const long long* key, const int* val, const float* src, int src_stride, float* dst,
                   int dst_stride, unsigned long long fail_kind, unsigned* words, unsigned long long* err, hipStream_t st) {
    if (n_dst == 0) return SPRK_OK;
    hipLaunchKernelGGL(k_als_begin, dim3(1), dim3(1), 0, st, words, (const unsigned long long*)err);
    constexpr int ROWS_PER_GROUP = ALS_THREADS / ALS_G;                     // rows a workgroup draws at once
    const long long groups = ((long long)n_dst + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP;
    const unsigned g = groups < (long long)fe_max_grid() ? (unsigned)groups : fe_max_grid();
    const int acc = rank * (rank + 1) / 2 + rank;                            // chains per lane = ceil(acc / 16): 2 up to rank 6, 5 up to rank 10, 10 beyond
    if (acc <= 2 * ALS_G)
        hipLaunchKernelGGL(k_als_half_sweep<2>, dim3(g), dim3(ALS_THREADS), 0, st, n_dst, rank, reg, off, key, val, src, src_stride, dst, dst_stride, fail_kind, words, err);
    else if (acc <= 5 * ALS_G)
        hipLaunchKernelGGL(k_als_half_sweep<5>, dim3(g), dim3(ALS_THREADS), 0, st, n_dst, rank, reg, off, key, val, src, src_stride, dst, dst_stride, fail_kind, words, err);
    else
        hipLaunchKernelGGL(k_als_half_sweep<10>, dim3(g), dim3(ALS_THREADS), 0, st, n_dst, rank, reg, off, key, val, src, src_stride, dst, dst_stride, fail_kind, words, err);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}
}  // namespace

extern "C" {

size_t sprk_als_workspace_bytes(int64_t n_ratings, int32_t n_users, int32_t n_items, int32_t rank) {
    if (!als_sizes_ok(n_ratings, n_users, n_items, rank)) return 0;
    return als_carve(nullptr, n_ratings, n_users, n_items).bytes;
}

int sprk_als_fit(const int32_t* user_id, const int32_t* movie_id, const float* rating, int64_t n_ratings,
                 int32_t n_users, int32_t n_items, int32_t rank, double reg, int32_t iters,
                 const float* init_user, int32_t init_stride,
                 float* user_factors, int32_t user_stride, float* item_factors, int32_t item_stride,
                 uint8_t* user_has, uint8_t* item_has, int32_t* user_count, int32_t* item_count,
                 uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_als_fit");
    // every check before any device call
    if (rank < 1 || rank > ALS_MAX_RANK) return fail(SPRK_EINVAL, "als_fit: rank = %d outside [1, %d]", rank, ALS_MAX_RANK);
    if (!als_sizes_ok(n_ratings, n_users, n_items, rank))
        return fail(SPRK_EINVAL, "als_fit: bad sizes (need 0 <= n_ratings < 2^31 - 1, 0 <= n_users < 2^31 - 1, 0 <= n_items < 2^31 - 1)");
    if (iters < 0) return fail(SPRK_EINVAL, "als_fit: iters = %d is negative", iters);
    if (!(reg >= 0.0) || reg > 1.7976931348623157e308) return fail(SPRK_EINVAL, "als_fit: reg must be finite and >= 0");
    if (init_stride < rank || user_stride < rank || item_stride < rank)
        return fail(SPRK_EINVAL, "als_fit: init_stride = %d, user_stride = %d, item_stride = %d, a row holds rank = %d floats", init_stride, user_stride, item_stride, rank);
    if (!error_key) return fail(SPRK_EINVAL, "als_fit: NULL error word");
    if ((uintptr_t)error_key & 7) return fail(SPRK_EINVAL, "als_fit: misaligned error word");
    if (n_ratings > 0 && (!user_id || !movie_id || !rating)) return fail(SPRK_EINVAL, "als_fit: NULL rating column");
    if (n_users > 0 && (!init_user || !user_factors || !user_has || !user_count)) return fail(SPRK_EINVAL, "als_fit: NULL user table");
    if (n_items > 0 && (!item_factors || !item_has || !item_count)) return fail(SPRK_EINVAL, "als_fit: NULL item table");
    if (((uintptr_t)user_id & 3) || ((uintptr_t)movie_id & 3) || ((uintptr_t)rating & 3) || ((uintptr_t)init_user & 3) || ((uintptr_t)user_factors & 3) ||
        ((uintptr_t)item_factors & 3) || ((uintptr_t)user_count & 3) || ((uintptr_t)item_count & 3))
        return fail(SPRK_EINVAL, "als_fit: misaligned column");
    const AlsWorkspace w = als_carve(workspace, n_ratings, n_users, n_items);
    SPRK_TRY(check_workspace("als_fit", "sprk_als_workspace_bytes", workspace, workspace_bytes, w.bytes));
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_ratings;
    unsigned long long* err = (unsigned long long*)error_key;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_als_count, dim3(fe_grid_capped(n)), dim3(ALS_THREADS), 0, st, n, user_id, movie_id, rating, (int)n_users, (int)n_items, w.off_user, w.off_movie, err);
        HIP_TRY(hipGetLastError());
    }
    SPRK_TRY(seg_scan(w.off_user, (long long)n_users + 1, w.tops, w.tiles_user, FeScanKept<false>{}, st));
    SPRK_TRY(seg_scan(w.off_movie, (long long)n_items + 1, w.tops, w.tiles_movie, FeScanKept<false>{}, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_als_scatter, dim3(fe_grid_capped(n)), dim3(ALS_THREADS), 0, st, n, user_id, movie_id, rating, (int)n_users, (int)n_items,
                           (const unsigned*)w.off_user, (const unsigned*)w.off_movie, w.cur_user, w.cur_movie, w.key_user, w.val_user, w.key_movie, w.val_movie);
        HIP_TRY(hipGetLastError());
        SPRK_TRY(seg_sort(cap, n, n_users, w.off_user, w.key_user, w.val_user, w.tmp_key, w.tmp_val, w.long_user, w.words + ALS_W_LONG_USER, nullptr, st));
        SPRK_TRY(seg_sort(cap, n, n_items, w.off_movie, w.key_movie, w.val_movie, w.tmp_key, w.tmp_val, w.long_movie, w.words + ALS_W_LONG_MOVIE, nullptr, st));
    }
    if (n_users > 0 || n_items > 0) {
        hipLaunchKernelGGL(k_als_init, dim3(fe_grid_capped(n_users > n_items ? n_users : n_items)), dim3(ALS_THREADS), 0, st, (int)n_users, (int)n_items, (int)rank,
                           (const unsigned*)w.off_user, (const unsigned*)w.off_movie, init_user, (int)init_stride, user_factors, (int)user_stride, item_factors,
                           (int)item_stride, user_has, item_has, user_count, item_count, err);
        HIP_TRY(hipGetLastError());
    }
    for (int it = 0; it < iters; ++it) {
        SPRK_TRY(als_half_sweep(n_items, rank, reg, w.off_movie, w.key_movie, w.val_movie, user_factors, user_stride, item_factors, item_stride, ALS_ERR_MOVIE_SOLVE, w.words, err, st));
        SPRK_TRY(als_half_sweep(n_users, rank, reg, w.off_user, w.key_user, w.val_user, item_factors, item_stride, user_factors, user_stride, ALS_ERR_USER_SOLVE, w.words, err, st));
    }
    return SPRK_OK;
}

int sprk_als_predict(const int32_t* user, const int32_t* item, int64_t n,
                     const float* user_factors, int32_t user_stride, const uint8_t* user_has,
                     const float* item_factors, int32_t item_stride, const uint8_t* item_has,
                     int32_t n_users, int32_t n_items, int32_t rank, float* out, void* stream) {
    RoctxRange roctx_range_("sprk_als_predict");
    if (n < 0 || n_users < 0 || n_items < 0) return fail(SPRK_EINVAL, "als_predict: bad sizes (n, n_users and n_items must be >= 0)");
    if (rank < 1 || rank > ALS_MAX_RANK) return fail(SPRK_EINVAL, "als_predict: rank = %d outside [1, %d]", rank, ALS_MAX_RANK);
    if (user_stride < rank || item_stride < rank) return fail(SPRK_EINVAL, "als_predict: user_stride = %d, item_stride = %d, a row holds rank = %d floats", user_stride, item_stride, rank);
    if (n > 0 && (!user || !item || !out)) return fail(SPRK_EINVAL, "als_predict: NULL ids or output");
    if (n_users > 0 && (!user_factors || !user_has)) return fail(SPRK_EINVAL, "als_predict: NULL user table");
    if (n_items > 0 && (!item_factors || !item_has)) return fail(SPRK_EINVAL, "als_predict: NULL item table");
    if (((uintptr_t)user & 3) || ((uintptr_t)item & 3) || ((uintptr_t)out & 3) || ((uintptr_t)user_factors & 3) || ((uintptr_t)item_factors & 3))
        return fail(SPRK_EINVAL, "als_predict: misaligned column");
    if (n == 0) return SPRK_OK;
    hipLaunchKernelGGL(k_als_predict, dim3(fe_grid_capped(n)), dim3(ALS_THREADS), 0, (hipStream_t)stream, (long long)n, user, item, user_factors, (int)user_stride, user_has,
                       item_factors, (int)item_stride, item_has, (int)n_users, (int)n_items, (int)rank, out);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
