// api_catalog.h -- C ABI: sprk_catalog_build / sprk_catalog_build_workspace_bytes (ratings + the movie table -> average ratings and the
// sorted lists) and sprk_catalog_similar (candidates and the default similarity ranker for Q queries), on the device (k_catalog.h).
// From host_segments.h: the carver and the workspace check, the grids, the counts-only seg_scan, and seg_sort twice: the ratings per movie
// behind the `ungrouped` word, then the 2 (G + 1) lists.
// Every argument is checked before any device call; the calls enqueue their kernels on the caller's stream and return: no
// synchronisation, no memory of their own.
namespace {
// The workspace, carved in this order; every part starts on a 16-byte boundary.  [zeroed] parts are cleared by one memset per call.
struct CatWorkspace {
    unsigned* seg_off;             // [n_movies + 1]  ratings per movie, then their exclusive scan                 [zeroed]
    unsigned* runs;                // [n_movies]      runs of the movie's rows in the input                       [zeroed]
    unsigned* cursor;              // [n_movies]      scatter cursors                                             [zeroed]
    unsigned* words;               // [4]             UE_W_LONG, UE_W_UNGROUPED                                   [zeroed]
    unsigned* lwords;              // [4]             the lists' long segments                                    [zeroed]
    unsigned* lcnt;                // [G + 1]         members per genre, movies held                              [zeroed]
    unsigned* lcursor;             // [2 (G + 1)]     the genre lists' scatter cursors                            [zeroed]
    int* inv_file;                 // [n_movies]      file position -> movie                                      [zeroed]
    int* inv_hash;                 // [n_movies]      hash position -> movie                                      [zeroed]
    size_t zeroed_bytes;
    unsigned* first;               // [n_movies]      the first row of the movie's (only) run
    unsigned* tops;                // [n_tiles]
    int* long_list;                // [n / 64 + 1]
    int* seg_rating;               // [n]             float32 bits
    int* tmp_rating;               // [n]
    long long* seg_key;            // [n]
    long long* tmp_key;            // [n]
    unsigned* lseg_off;            // [2 (G + 1) + 1]
    int* llong_list;               // [2 (G + 1)]
    int* lrow;                     // [capacity]
    int* ltmp_row;                 // [capacity]
    long long* lkey;               // [capacity]
    long long* ltmp_key;           // [capacity]
    int n_tiles;
    size_t bytes;
};
inline bool cat_sizes_ok(int64_t n, int32_t n_movies, int64_t capacity) {
    return n >= 0 && n < 0x7fffffffll && n_movies >= 0 && n_movies < 0x7fffffff && capacity >= 0 && capacity < 0x7fffffffll;
}
CatWorkspace cat_carve(void* base, int64_t n, int32_t n_movies, int64_t capacity) {
    CatWorkspace w;
    Carver c{base};
    const size_t nm = (size_t)n_movies, nr = (size_t)n, nl = (size_t)capacity, L = 2 * (CAT_MAX_GENRES + 1);
    w.seg_off = c.take<unsigned>(nm + 1);
    w.runs = c.take<unsigned>(nm);
    w.cursor = c.take<unsigned>(nm);
    w.words = c.take<unsigned>(4);
    w.lwords = c.take<unsigned>(4);
    w.lcnt = c.take<unsigned>(CAT_MAX_GENRES + 1);
    w.lcursor = c.take<unsigned>(L);
    w.inv_file = c.take<int>(nm);
    w.inv_hash = c.take<int>(nm);
    w.zeroed_bytes = c.at;
    w.n_tiles = seg_scan_tiles(nm);
    w.first = c.take<unsigned>(nm);
    w.tops = c.take<unsigned>((size_t)w.n_tiles);
    w.long_list = c.take<int>(nr / 64 + 1);
    w.seg_rating = c.take<int>(nr);
    w.tmp_rating = c.take<int>(nr);
    w.seg_key = c.take<long long>(nr);
    w.tmp_key = c.take<long long>(nr);
    w.lseg_off = c.take<unsigned>(L + 1);
    w.llong_list = c.take<int>(L);
    w.lrow = c.take<int>(nl);
    w.ltmp_row = c.take<int>(nl);
    w.lkey = c.take<long long>(nl);
    w.ltmp_key = c.take<long long>(nl);
    w.bytes = c.at;
    return w;
}
}  // namespace

extern "C" {

size_t sprk_catalog_build_workspace_bytes(int64_t n_ratings, int32_t n_movies, int64_t list_capacity) {
    if (!cat_sizes_ok(n_ratings, n_movies, list_capacity)) return 0;
    return cat_carve(nullptr, n_ratings, n_movies, list_capacity).bytes;
}

int sprk_catalog_build(const int32_t* movie_id, const float* rating, int64_t n_ratings, int32_t n_movies,
                       const uint32_t* movie_genre_mask, const uint8_t* movie_has, const int32_t* movie_year,
                       const int32_t* movie_file_pos, const int32_t* movie_hash_pos, int32_t n_genres,
                       double* avg_rating, int32_t* rating_count, int32_t* list_offsets, int32_t* list_movies, int64_t list_capacity,
                       uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_catalog_build");
    // every check before any device call
    if (!cat_sizes_ok(n_ratings, n_movies, list_capacity))
        return fail(SPRK_EINVAL, "catalog_build: bad sizes (need 0 <= n_ratings < 2^31 - 1, 0 <= n_movies < 2^31 - 1, 0 <= list_capacity < 2^31 - 1)");
    if (n_genres < 0 || n_genres > CAT_MAX_GENRES) return fail(SPRK_EINVAL, "catalog_build: n_genres = %d outside [0, %d]", n_genres, CAT_MAX_GENRES);
    if (!error_key) return fail(SPRK_EINVAL, "catalog_build: NULL error word");
    if ((uintptr_t)error_key & 7) return fail(SPRK_EINVAL, "catalog_build: misaligned error word");
    if (n_ratings > 0 && (!movie_id || !rating)) return fail(SPRK_EINVAL, "catalog_build: NULL rating column");
    if (n_movies > 0 && (!movie_genre_mask || !movie_has || !movie_year || !movie_file_pos || !movie_hash_pos)) return fail(SPRK_EINVAL, "catalog_build: NULL movie table");
    if (n_movies > 0 && (!avg_rating || !rating_count)) return fail(SPRK_EINVAL, "catalog_build: NULL output");
    if (!list_offsets || (list_capacity > 0 && !list_movies)) return fail(SPRK_EINVAL, "catalog_build: NULL list output");
    if (((uintptr_t)movie_id & 3) || ((uintptr_t)rating & 3) || ((uintptr_t)movie_genre_mask & 3) || ((uintptr_t)movie_year & 3) || ((uintptr_t)movie_file_pos & 3) ||
        ((uintptr_t)movie_hash_pos & 3) || ((uintptr_t)avg_rating & 7) || ((uintptr_t)rating_count & 3) || ((uintptr_t)list_offsets & 3) || ((uintptr_t)list_movies & 3))
        return fail(SPRK_EINVAL, "catalog_build: misaligned column");
    const CatWorkspace w = cat_carve(workspace, n_ratings, n_movies, list_capacity);
    SPRK_TRY(check_workspace("catalog_build", "sprk_catalog_build_workspace_bytes", workspace, workspace_bytes, w.bytes));
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_ratings;
    const int G = n_genres, L = 2 * (G + 1);

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_cat_count, dim3(fe_grid_capped(n)), dim3(CAT_THREADS), 0, st, n, movie_id, rating, (int)n_movies, movie_has, w.seg_off, w.runs, w.first, w.words,
                           (unsigned long long*)error_key);
        HIP_TRY(hipGetLastError());
    }
    if (n_movies > 0) {
        SPRK_TRY(seg_scan(w.seg_off, (long long)n_movies + 1, w.tops, w.n_tiles, FeScanKept<false>{}, st));
        if (n > 0) {                                                        // each of these does nothing unless k_cat_count raised `ungrouped`
            hipLaunchKernelGGL(k_cat_scatter, dim3(fe_grid_capped(n)), dim3(CAT_THREADS), 0, st, n, movie_id, rating, (int)n_movies, movie_has, (const unsigned*)w.seg_off, w.cursor,
                               w.seg_key, w.seg_rating, (const unsigned*)w.words);
            HIP_TRY(hipGetLastError());
            SPRK_TRY(seg_sort(cap, n, n_movies, w.seg_off, w.seg_key, w.seg_rating, w.tmp_key, w.tmp_rating, w.long_list, w.words + UE_W_LONG, w.words + UE_W_UNGROUPED, st));
        }
        const unsigned mg = fe_grid_capped(n_movies);
        hipLaunchKernelGGL(k_cat_avg_short, dim3(mg), dim3(CAT_THREADS), 0, st, (int)n_movies, (const unsigned*)w.seg_off, (const unsigned*)w.first, (const int*)w.seg_rating, rating,
                           (const unsigned*)w.words, avg_rating, rating_count);
        const long long waves = ((long long)n_movies + CAT_THREADS / 64 - 1) / (CAT_THREADS / 64);          // workgroups that give every movie its own wave
        hipLaunchKernelGGL(k_cat_avg_wave, dim3(fe_grid_own_cap((unsigned)(waves < 65536 * 4 ? waves : 65536 * 4))), dim3(CAT_THREADS), 0, st, (int)n_movies, (const unsigned*)w.seg_off,
                           (const unsigned*)w.first, (const int*)w.seg_rating, rating, (const unsigned*)w.words, avg_rating);
        hipLaunchKernelGGL(k_cat_list_count, dim3(mg), dim3(CAT_THREADS), 0, st, (int)n_movies, (const unsigned*)movie_genre_mask, movie_has, G, w.lcnt);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cat_list_scan, dim3(1), dim3(64), 0, st, G, (const unsigned*)w.lcnt, (long long)list_capacity, w.lseg_off, list_offsets, (unsigned long long*)error_key);
    HIP_TRY(hipGetLastError());
    if (n_movies > 0 && list_capacity > 0) {
        hipLaunchKernelGGL(k_cat_list_scatter, dim3(fe_grid_capped(n_movies)), dim3(CAT_THREADS), 0, st, (int)n_movies, (const unsigned*)movie_genre_mask, movie_has, movie_year,
                           movie_file_pos, movie_hash_pos, (const double*)avg_rating, G, (const unsigned*)w.lseg_off, w.lcursor, w.lkey, w.lrow, w.inv_file, w.inv_hash);
        HIP_TRY(hipGetLastError());
        SPRK_TRY(seg_sort(cap, (long long)list_capacity, L, w.lseg_off, w.lkey, w.lrow, w.ltmp_key, w.ltmp_row, w.llong_list, w.lwords, nullptr, st));
    }
    if (list_capacity > 0) {
        const unsigned wg = fe_grid_own_cap(fe_grid_capped(list_capacity) < 256u ? fe_grid_capped(list_capacity) : 256u);
        hipLaunchKernelGGL(k_cat_list_write, dim3(wg, (unsigned)L), dim3(CAT_THREADS), 0, st, G, (int)n_movies, (const unsigned*)w.lseg_off, (const int*)w.lrow, (const int*)w.inv_file,
                           (const int*)w.inv_hash, list_movies, (long long)list_capacity);
        HIP_TRY(hipGetLastError());
    }
    return SPRK_OK;
}

int sprk_catalog_similar(const int32_t* query_movie, int32_t n_queries, int32_t n_movies,
                         const uint32_t* movie_genre_mask, const uint8_t* movie_has, const uint8_t* movie_n_genres, const double* avg_rating, int32_t n_genres,
                         const int32_t* list_offsets, const int32_t* list_movies, int64_t list_entries,
                         int32_t mode, int32_t top_n, int32_t extra_n, int32_t score_kind, int32_t size,
                         int32_t* out_ids, double* out_scores, int32_t out_stride, int32_t* out_count, void* stream) {
    RoctxRange roctx_range_("sprk_catalog_similar");
    // every check before any device call
    if (n_queries < 0 || n_movies < 0 || list_entries < 0 || list_entries >= 0x7fffffffll)
        return fail(SPRK_EINVAL, "catalog_similar: bad sizes (need n_queries >= 0, n_movies >= 0, 0 <= list_entries < 2^31 - 1)");
    if (n_genres < 0 || n_genres > CAT_MAX_GENRES) return fail(SPRK_EINVAL, "catalog_similar: n_genres = %d outside [0, %d]", n_genres, CAT_MAX_GENRES);
    if (mode != 0 && mode != 1) return fail(SPRK_EINVAL, "catalog_similar: mode = %d (0 = candidateGenerator, 1 = multipleRetrievalCandidates)", mode);
    if (score_kind != 0 && score_kind != 1) return fail(SPRK_EINVAL, "catalog_similar: score_kind = %d (0 = the candidates, 1 = the default ranker)", score_kind);
    if (top_n < 0 || extra_n < 0 || 32ll * top_n + 2ll * extra_n > CAT_MAX_CAND)
        return fail(SPRK_EINVAL, "catalog_similar: top_n = %d, extra_n = %d: need both >= 0 and 32 top_n + 2 extra_n <= %d", top_n, extra_n, CAT_MAX_CAND);
    if (out_stride < 1) return fail(SPRK_EINVAL, "catalog_similar: out_stride = %d", out_stride);
    if (size < 0 || (score_kind == 1 && size > out_stride)) return fail(SPRK_EINVAL, "catalog_similar: size = %d outside [0, out_stride = %d]", size, out_stride);
    if (n_queries > 0 && (!query_movie || !out_ids || !out_count || (score_kind == 1 && !out_scores))) return fail(SPRK_EINVAL, "catalog_similar: NULL query column or output");
    if (n_movies > 0 && (!movie_genre_mask || !movie_has || !movie_n_genres || !avg_rating)) return fail(SPRK_EINVAL, "catalog_similar: NULL movie table");
    if (!list_offsets || (list_entries > 0 && !list_movies)) return fail(SPRK_EINVAL, "catalog_similar: NULL lists");
    if (((uintptr_t)query_movie & 3) || ((uintptr_t)movie_genre_mask & 3) || ((uintptr_t)avg_rating & 7) || ((uintptr_t)list_offsets & 3) || ((uintptr_t)list_movies & 3) ||
        ((uintptr_t)out_ids & 3) || ((uintptr_t)out_scores & 7) || ((uintptr_t)out_count & 3))
        return fail(SPRK_EINVAL, "catalog_similar: misaligned column");
    if (n_queries == 0) return SPRK_OK;
    const long long most = (long long)n_genres * top_n + (mode == 1 ? 2ll * extra_n : 0ll);                  // <= CAT_MAX_CAND
    int B = 2;
    while (B < most) B <<= 1;
    hipLaunchKernelGGL(k_cat_similar, dim3((unsigned)n_queries), dim3(CAT_THREADS), cat_similar_lds(B), (hipStream_t)stream, query_movie, (int)n_movies,
                       (const unsigned*)movie_genre_mask, movie_has, movie_n_genres, avg_rating, (int)n_genres, list_offsets, list_movies, (long long)list_entries, (int)mode,
                       (int)top_n, (int)extra_n, (int)score_kind, (int)size, B, out_ids, out_scores, (int)out_stride, out_count);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
