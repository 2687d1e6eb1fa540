// api_store_update.h -- C ABI: sprk_store_update / sprk_store_update_workspace_bytes, new ratings applied to a feature store and its
// state on the device (k_store_update.h).  From host_segments.h: the carver and the workspace check, the grids, seg_scan, seg_sort.
// Every argument is checked before any device call; the call enqueues its kernels on the caller's stream and returns: no
// synchronisation, no memory of its own.
namespace {
// The workspace, carved in this order; every part starts on a 16-byte boundary.  [zeroed] parts are cleared by one memset per call.
struct SuWorkspace {
    unsigned* seg_off;             // [n_users + 1]  new ratings per user, then their exclusive scan     [zeroed]
    unsigned* cursor;              // [n_users]      scatter cursors                                    [zeroed]
    unsigned char* mv_touched;     // [n_movies]     the batch names the movie                          [zeroed]
    unsigned* n_long;              // [4]            segments on the long sort path                     [zeroed]
    size_t zeroed_bytes;
    unsigned* tops;                // [n_tiles]
    int* long_list;                // [n / 64 + 1]
    int* seg_row;                  // [n]
    int* seg_user;                 // [n]
    int* tmp_row;                  // [n]
    long long* seg_ts;             // [n]
    long long* tmp_ts;             // [n]
    int n_tiles;
    size_t bytes;
};
SuWorkspace su_carve(void* base, int64_t n, int32_t n_users, int32_t n_movies) {
    SuWorkspace w;
    Carver c{base};
    const size_t nu = (size_t)n_users, nm = (size_t)n_movies, nr = (size_t)n;
    w.seg_off = c.take<unsigned>(nu + 1);
    w.cursor = c.take<unsigned>(nu);
    w.mv_touched = c.take<unsigned char>(nm);
    w.n_long = c.take<unsigned>(4);
    w.zeroed_bytes = c.at;
    w.n_tiles = seg_scan_tiles(nu);
    w.tops = c.take<unsigned>((size_t)w.n_tiles);
    w.long_list = c.take<int>(nr / 64 + 1);
    w.seg_row = c.take<int>(nr);
    w.seg_user = c.take<int>(nr);
    w.tmp_row = c.take<int>(nr);
    w.seg_ts = c.take<long long>(nr);
    w.tmp_ts = c.take<long long>(nr);
    w.bytes = c.at;
    return w;
}
}  // namespace

extern "C" {

size_t sprk_store_update_workspace_bytes(int64_t n_new, int32_t n_users, int32_t n_movies) {
    if (!fe_sizes_ok(n_new, n_users, n_movies)) return 0;
    return su_carve(nullptr, n_new, n_users, n_movies).bytes;
}

int sprk_store_update(const int32_t* user_id, const int32_t* movie_id, const float* rating, const int64_t* timestamp, int64_t n_new,
                      int32_t n_users, int32_t n_movies, const int32_t* movie_year, const int32_t* movie_genre3, const uint32_t* movie_genre_mask,
                      int32_t n_vocab, int32_t hist_len,
                      uint32_t* user_count, int64_t* user_last_ts, int32_t* ring_movie, uint8_t* ring_r2,
                      uint32_t* movie_count, uint64_t* movie_sum, uint64_t* movie_sumsq, uint8_t* movie_flag,
                      int32_t* user_rows, uint8_t* user_has, int32_t user_pitch, int32_t* movie_rows, uint8_t* movie_has,
                      uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_store_update");
    // every check before any device call
    if (!fe_sizes_ok(n_new, n_users, n_movies))
        return fail(SPRK_EINVAL, "store_update: bad sizes (need 0 <= n_new < 2^31 - 1, 0 <= n_users < 2^31 - 1, n_movies >= 0)");
    if (hist_len < 1 || hist_len > FE_WINDOW) return fail(SPRK_EINVAL, "store_update: hist_len = %d outside [1, %d]", hist_len, FE_WINDOW);
    if (n_vocab < 0 || n_vocab > 32) return fail(SPRK_EINVAL, "store_update: n_vocab = %d outside [0, 32]", n_vocab);
    if (!error_key) return fail(SPRK_EINVAL, "store_update: NULL error word");
    if ((uintptr_t)error_key & 7) return fail(SPRK_EINVAL, "store_update: misaligned error word");
    if (n_new > 0 && (!user_id || !movie_id || !rating || !timestamp)) return fail(SPRK_EINVAL, "store_update: NULL rating column");
    if (n_movies > 0 && (!movie_year || !movie_genre3 || !movie_genre_mask)) return fail(SPRK_EINVAL, "store_update: NULL movie table");
    if ((n_users > 0 && (!user_count || !user_last_ts || !ring_movie || !ring_r2)) || (n_movies > 0 && (!movie_count || !movie_sum || !movie_sumsq || !movie_flag)))
        return fail(SPRK_EINVAL, "store_update: NULL state array");
    if ((n_users > 0 && (!user_rows || !user_has)) || (n_movies > 0 && (!movie_rows || !movie_has))) return fail(SPRK_EINVAL, "store_update: NULL store table");
    if (user_pitch < hist_len + 8) return fail(SPRK_EINVAL, "store_update: user_pitch = %d, a user row holds %d dwords", user_pitch, hist_len + 8);
    if (((uintptr_t)user_id & 3) || ((uintptr_t)movie_id & 3) || ((uintptr_t)rating & 3) || ((uintptr_t)timestamp & 7) || ((uintptr_t)movie_year & 3) ||
        ((uintptr_t)movie_genre3 & 3) || ((uintptr_t)movie_genre_mask & 3) || ((uintptr_t)user_count & 3) || ((uintptr_t)user_last_ts & 7) || ((uintptr_t)ring_movie & 3) ||
        ((uintptr_t)movie_count & 3) || ((uintptr_t)movie_sum & 7) || ((uintptr_t)movie_sumsq & 7) || ((uintptr_t)user_rows & 3) || ((uintptr_t)movie_rows & 3))
        return fail(SPRK_EINVAL, "store_update: misaligned column");
    const SuWorkspace w = su_carve(workspace, n_new, n_users, n_movies);
    SPRK_TRY(check_workspace("store_update", "sprk_store_update_workspace_bytes", workspace, workspace_bytes, w.bytes));
    if (n_new == 0) return SPRK_OK;                                            // nothing to apply
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_new;
    const unsigned long long* err = (const unsigned long long*)error_key;
    const unsigned* u_cnt = (const unsigned*)user_count;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    hipLaunchKernelGGL(k_su_check, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, user_id, movie_id, rating, (const long long*)timestamp, (int)n_users, (int)n_movies,
                       (const long long*)user_last_ts, (unsigned long long*)error_key);
    hipLaunchKernelGGL(k_su_count, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, user_id, w.seg_off, err);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_scan(w.seg_off, (long long)n_users + 1, w.tops, w.n_tiles, FeScanKept<false>{}, st));
    hipLaunchKernelGGL(k_su_scatter, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, user_id, (const long long*)timestamp, (const unsigned*)w.seg_off, w.cursor, w.seg_ts,
                       w.seg_row, w.seg_user, err);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_sort(cap, n, n_users, w.seg_off, w.seg_ts, w.seg_row, w.tmp_ts, w.tmp_row, w.long_list, w.n_long, nullptr, st));
    hipLaunchKernelGGL(k_su_positions, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, (const unsigned*)w.seg_off, (const int*)w.seg_row, (const int*)w.seg_user, movie_id, rating,
                       u_cnt, (unsigned*)movie_count, (unsigned long long*)movie_sum, (unsigned long long*)movie_sumsq, movie_flag, w.mv_touched, err);
    hipLaunchKernelGGL(k_su_users, dim3(fe_grid_capped(n_users)), dim3(FE_THREADS), 0, st, (int)n_users, (const unsigned*)w.seg_off, (const int*)w.seg_row, movie_id, rating,
                       (const unsigned*)movie_genre_mask, u_cnt, (const int*)ring_movie, (const unsigned char*)ring_r2, (int)n_vocab, (int)hist_len, (int)user_pitch, user_rows,
                       user_has, err);
    hipLaunchKernelGGL(k_su_ring, dim3(fe_grid_capped(n_users)), dim3(FE_THREADS), 0, st, (int)n_users, (const unsigned*)w.seg_off, (const long long*)w.seg_ts, (const int*)w.seg_row,
                       movie_id, rating, (unsigned*)user_count, (long long*)user_last_ts, ring_movie, ring_r2, err);
    hipLaunchKernelGGL(k_su_movies, dim3(fe_grid_capped(n_movies)), dim3(FE_THREADS), 0, st, (int)n_movies, (const unsigned char*)w.mv_touched, movie_year, movie_genre3,
                       (const unsigned*)movie_count, (const unsigned long long*)movie_sum, (const unsigned long long*)movie_sumsq, (const unsigned char*)movie_flag, movie_rows,
                       movie_has, err);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
