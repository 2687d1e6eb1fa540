// api_feature_eng.h -- C ABI: sprk_feature_eng / sprk_feature_eng_workspace_bytes, ratings -> samples and the feature store's rows on the
// device (k_feature_eng.h).  From host_segments.h: the carver and the workspace check, the grids, seg_scan with its `kept` half, seg_sort.
// Every argument is checked before any device call; the call enqueues its kernels on the caller's stream and returns: no
// synchronisation, no memory of its own.
namespace {
// The workspace, carved in this order; every part starts on a 16-byte boundary.  [zeroed] parts are cleared by one memset per call.
struct FeWorkspace {
    unsigned* seg_off;             // [n_users + 1]  len, then its exclusive scan                       [zeroed]
    unsigned* cursor;              // [n_users]      scatter cursors                                    [zeroed]
    unsigned* mv_cnt;              // [n_movies]                                                        [zeroed]
    unsigned* mv_flag;             // [n_movies]     a kept sample names the movie                      [zeroed]
    unsigned long long* mv_S;      // [n_movies]                                                        [zeroed]
    unsigned long long* mv_Q;      // [n_movies]                                                        [zeroed]
    unsigned* n_long;              // [4]            segments on the long sort path                     [zeroed]
    size_t zeroed_bytes;
    unsigned* kept_off;            // [n_users + 1]
    unsigned* tops;                // [2 * n_tiles]
    float* mv_dense;               // [n_movies][4]
    int* long_list;                // [n / 64 + 1]
    int* seg_row;                  // [n]
    int* seg_user;                 // [n]
    int* tmp_row;                  // [n]
    long long* seg_ts;             // [n]
    long long* tmp_ts;             // [n]
    int n_tiles;
    size_t bytes;
};
inline bool fe_sizes_ok(int64_t n, int32_t n_users, int32_t n_movies) { return n >= 0 && n < 0x7fffffffll && n_users >= 0 && n_users < 0x7fffffff && n_movies >= 0; }
FeWorkspace fe_carve(void* base, int64_t n, int32_t n_users, int32_t n_movies) {
    FeWorkspace w;
    Carver c{base};
    const size_t nu = (size_t)n_users, nm = (size_t)n_movies, nr = (size_t)n;
    w.seg_off = c.take<unsigned>(nu + 1);
    w.cursor = c.take<unsigned>(nu);
    w.mv_cnt = c.take<unsigned>(nm);
    w.mv_flag = c.take<unsigned>(nm);
    w.mv_S = c.take<unsigned long long>(nm);
    w.mv_Q = c.take<unsigned long long>(nm);
    w.n_long = c.take<unsigned>(4);
    w.zeroed_bytes = c.at;
    w.n_tiles = seg_scan_tiles(nu);
    w.kept_off = c.take<unsigned>(nu + 1);
    w.tops = c.take<unsigned>(2 * (size_t)w.n_tiles);
    w.mv_dense = c.take<float>(nm * 4);
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

int64_t sprk_segments_grid(int64_t items) { return (int64_t)fe_grid_capped(items); }

size_t sprk_feature_eng_workspace_bytes(int64_t n_ratings, int32_t n_users, int32_t n_movies) {
    if (!fe_sizes_ok(n_ratings, n_users, n_movies)) return 0;
    return fe_carve(nullptr, n_ratings, n_users, n_movies).bytes;
}

int sprk_feature_eng(const int32_t* user_id, const int32_t* movie_id, const float* rating, const int64_t* timestamp, int64_t n_ratings,
                     int32_t n_users, int32_t n_movies, const int32_t* movie_year, const int32_t* movie_genre3, const uint32_t* movie_genre_mask,
                     int32_t n_vocab, int32_t hist_len,
                     int32_t* out_user, int32_t* out_movie, float* out_rating, int64_t* out_timestamp, int32_t* out_label, int32_t* out_source_row,
                     int32_t* out_genres, int32_t* out_history, float* out_dense,
                     int32_t* user_rows, uint8_t* user_has, int32_t user_pitch, int32_t* movie_rows, uint8_t* movie_has,
                     uint64_t* error_key, int64_t* n_kept, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_feature_eng");
    // every check before any device call
    if (!fe_sizes_ok(n_ratings, n_users, n_movies))
        return fail(SPRK_EINVAL, "feature_eng: bad sizes (need 0 <= n_ratings < 2^31 - 1, 0 <= n_users < 2^31 - 1, n_movies >= 0)");
    if (hist_len < 1 || hist_len > FE_WINDOW) return fail(SPRK_EINVAL, "feature_eng: hist_len = %d outside [1, %d]", hist_len, FE_WINDOW);
    if (n_vocab < 0 || n_vocab > 32) return fail(SPRK_EINVAL, "feature_eng: n_vocab = %d outside [0, 32]", n_vocab);
    if (!error_key || !n_kept) return fail(SPRK_EINVAL, "feature_eng: NULL error word / sample count");
    if (((uintptr_t)error_key & 7) || ((uintptr_t)n_kept & 7)) return fail(SPRK_EINVAL, "feature_eng: misaligned error word / sample count");
    if (n_ratings > 0 && (!user_id || !movie_id || !rating || !timestamp)) return fail(SPRK_EINVAL, "feature_eng: NULL rating column");
    if (n_movies > 0 && (!movie_year || !movie_genre3 || !movie_genre_mask)) return fail(SPRK_EINVAL, "feature_eng: NULL movie table");
    if (n_ratings > 0 && (!out_user || !out_movie || !out_rating || !out_timestamp || !out_label || !out_source_row || !out_genres || !out_history || !out_dense))
        return fail(SPRK_EINVAL, "feature_eng: NULL output column");
    const bool store = user_rows || user_has || movie_rows || movie_has;
    if (store) {
        if ((n_users > 0 && (!user_rows || !user_has)) || (n_movies > 0 && (!movie_rows || !movie_has)))
            return fail(SPRK_EINVAL, "feature_eng: the store's four tables come together or not at all");
        if (user_pitch < hist_len + 8) return fail(SPRK_EINVAL, "feature_eng: user_pitch = %d, a user row holds %d dwords", user_pitch, hist_len + 8);
    }
    if (((uintptr_t)user_id & 3) || ((uintptr_t)movie_id & 3) || ((uintptr_t)rating & 3) || ((uintptr_t)timestamp & 7) || ((uintptr_t)out_timestamp & 7) ||
        ((uintptr_t)movie_year & 3) || ((uintptr_t)movie_genre3 & 3) || ((uintptr_t)movie_genre_mask & 3) || ((uintptr_t)user_rows & 3) || ((uintptr_t)movie_rows & 3))
        return fail(SPRK_EINVAL, "feature_eng: misaligned column");
    const FeWorkspace w = fe_carve(workspace, n_ratings, n_users, n_movies);
    SPRK_TRY(check_workspace("feature_eng", "sprk_feature_eng_workspace_bytes", workspace, workspace_bytes, w.bytes));
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_ratings;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_fe_hist, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, user_id, movie_id, rating, (int)n_users, (int)n_movies, w.seg_off, w.mv_cnt, w.mv_S, w.mv_Q,
                           (unsigned long long*)error_key);
        HIP_TRY(hipGetLastError());
    }
    SPRK_TRY(seg_scan(w.seg_off, (long long)n_users + 1, w.tops, w.n_tiles, FeScanKept<true>{w.kept_off, (long long*)n_kept}, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_fe_scatter, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, user_id, movie_id, rating, (const long long*)timestamp, (int)n_users, (int)n_movies,
                           (const unsigned*)w.seg_off, w.cursor, w.seg_ts, w.seg_row, w.seg_user);
        HIP_TRY(hipGetLastError());
        SPRK_TRY(seg_sort(cap, n, n_users, w.seg_off, w.seg_ts, w.seg_row, w.tmp_ts, w.tmp_row, w.long_list, w.n_long, nullptr, st));
    }
    if (n_movies > 0) {
        hipLaunchKernelGGL(k_fe_movie_stats, dim3(fe_grid(n_movies)), dim3(FE_THREADS), 0, st, (int)n_movies, movie_year, (const unsigned*)w.mv_cnt, (const unsigned long long*)w.mv_S,
                           (const unsigned long long*)w.mv_Q, w.mv_dense);
        HIP_TRY(hipGetLastError());
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_fe_window, dim3(fe_grid(n)), dim3(FE_THREADS), 0, st, (const unsigned*)w.seg_off, (const unsigned*)w.kept_off, (int)n_users, (const long long*)w.seg_ts,
                           (const int*)w.seg_row, (const int*)w.seg_user, movie_id, rating, movie_genre3, (const unsigned*)movie_genre_mask, (const float*)w.mv_dense, w.mv_flag,
                           (int)n_vocab, (int)hist_len, out_user, out_movie, out_rating, (long long*)out_timestamp, out_label, out_source_row, out_genres, out_history, out_dense);
        HIP_TRY(hipGetLastError());
    }
    if (store && (n_users > 0 || n_movies > 0)) {
        hipLaunchKernelGGL(k_fe_store, dim3(fe_grid(n_users > n_movies ? n_users : n_movies)), dim3(FE_THREADS), 0, st, (int)n_users, (int)n_movies, (int)hist_len, (int)user_pitch,
                           (const unsigned*)w.kept_off, (const int*)out_genres, (const int*)out_history, (const float*)out_dense, movie_genre3, (const float*)w.mv_dense,
                           (const unsigned*)w.mv_flag, user_rows, user_has, movie_rows, movie_has);
        HIP_TRY(hipGetLastError());
    }
    return SPRK_OK;
}

}  // extern "C"
