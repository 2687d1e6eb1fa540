// api_catalog.h -- C ABI: sprk_catalog_build / sprk_catalog_build_workspace_bytes (ratings + the movie table -> average ratings and the
// sorted lists) and sprk_catalog_similar (candidates and the default similarity ranker for Q queries), on the device (k_catalog.h).
// Part of sparrow_feature_eng.hip, after api_user_emb.h: the sort capacity, the grids and the long-segment sort are api_feature_eng.h's.
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
    unsigned* kept_off;            // [n_movies + 1]  k_fe_scan_*'s second scan, unused here
    unsigned* tops;                // [2 * n_tiles]
    long long* n_kept;             // [2]             k_fe_scan_add's total, unused here
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
    size_t o = 0;
    auto take = [&](size_t count, size_t elem) { const size_t at = o; o += (count * elem + 15) / 16 * 16; return (unsigned char*)base + at; };
    const size_t nm = (size_t)n_movies, nr = (size_t)n, nl = (size_t)capacity, L = 2 * (CAT_MAX_GENRES + 1);
    w.seg_off = (unsigned*)take(nm + 1, 4);
    w.runs = (unsigned*)take(nm, 4);
    w.cursor = (unsigned*)take(nm, 4);
    w.words = (unsigned*)take(4, 4);
    w.lwords = (unsigned*)take(4, 4);
    w.lcnt = (unsigned*)take(CAT_MAX_GENRES + 1, 4);
    w.lcursor = (unsigned*)take(L, 4);
    w.inv_file = (int*)take(nm, 4);
    w.inv_hash = (int*)take(nm, 4);
    w.zeroed_bytes = o;
    w.n_tiles = (int)((nm + 1 + FE_SCAN_TILE - 1) / FE_SCAN_TILE);
    w.first = (unsigned*)take(nm, 4);
    w.kept_off = (unsigned*)take(nm + 1, 4);
    w.tops = (unsigned*)take(2 * (size_t)w.n_tiles, 4);
    w.n_kept = (long long*)take(2, 8);
    w.long_list = (int*)take(nr / 64 + 1, 4);
    w.seg_rating = (int*)take(nr, 4);
    w.tmp_rating = (int*)take(nr, 4);
    w.seg_key = (long long*)take(nr, 8);
    w.tmp_key = (long long*)take(nr, 8);
    w.lseg_off = (unsigned*)take(L + 1, 4);
    w.llong_list = (int*)take(L, 4);
    w.lrow = (int*)take(nl, 4);
    w.ltmp_row = (int*)take(nl, 4);
    w.lkey = (long long*)take(nl, 8);
    w.ltmp_key = (long long*)take(nl, 8);
    w.bytes = o;
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
    if (!workspace || workspace_bytes < w.bytes)
        return fail(SPRK_EINVAL, "catalog_build: needs a workspace of %zu bytes (sprk_catalog_build_workspace_bytes), got %zu", w.bytes, workspace ? workspace_bytes : (size_t)0);
    if ((uintptr_t)workspace & 15) return fail(SPRK_EINVAL, "catalog_build: the workspace must start on a 16-byte boundary");
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_ratings, count = (long long)n_movies + 1;
    const int G = n_genres, L = 2 * (G + 1);
    const size_t sort_lds = (size_t)cap * 12;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_cat_count, dim3(fe_grid_capped(n)), dim3(CAT_THREADS), 0, st, n, movie_id, rating, (int)n_movies, movie_has, w.seg_off, w.runs, w.first, w.words,
                           (unsigned long long*)error_key);
        HIP_TRY(hipGetLastError());
    }
    if (n_movies > 0) {
        hipLaunchKernelGGL(k_fe_scan_tiles, dim3((unsigned)w.n_tiles), dim3(FE_THREADS), 0, st, w.seg_off, w.kept_off, count, w.tops, w.n_tiles);
        hipLaunchKernelGGL(k_fe_scan_tops, dim3(1), dim3(FE_THREADS), 0, st, w.tops, w.n_tiles);
        hipLaunchKernelGGL(k_fe_scan_add, dim3(fe_grid(count)), dim3(FE_THREADS), 0, st, w.seg_off, w.kept_off, count, (const unsigned*)w.tops, w.n_tiles, w.n_kept);
        HIP_TRY(hipGetLastError());
        if (n > 0) {                                                        // each of these does nothing unless k_cat_count raised `ungrouped`
            hipLaunchKernelGGL(k_cat_scatter, dim3(fe_grid_capped(n)), dim3(CAT_THREADS), 0, st, n, movie_id, rating, (int)n_movies, movie_has, (const unsigned*)w.seg_off, w.cursor,
                               w.seg_key, w.seg_rating, (const unsigned*)w.words);
            HIP_TRY(hipGetLastError());
            const unsigned ug = (unsigned)n_movies < 65536u * 16u ? (unsigned)n_movies : 65536u * 16u;
            hipLaunchKernelGGL(k_ue_sort_short, dim3(ug), dim3(FE_THREADS), sort_lds, st, (int)n_movies, cap, (const unsigned*)w.seg_off, w.seg_key, w.seg_rating, w.long_list, w.words);
            HIP_TRY(hipGetLastError());
            SPRK_TRY(fe_sort_long_segments(cap, n, w.seg_off, w.seg_key, w.seg_rating, w.tmp_key, w.tmp_rating, w.long_list, w.words + UE_W_LONG, st));
        }
        const unsigned mg = fe_grid_capped(n_movies);
        hipLaunchKernelGGL(k_cat_avg_short, dim3(mg), dim3(CAT_THREADS), 0, st, (int)n_movies, (const unsigned*)w.seg_off, (const unsigned*)w.first, (const int*)w.seg_rating, rating,
                           (const unsigned*)w.words, avg_rating, rating_count);
        const long long waves = ((long long)n_movies + CAT_THREADS / 64 - 1) / (CAT_THREADS / 64);          // workgroups that give every movie its own wave
        hipLaunchKernelGGL(k_cat_avg_wave, dim3((unsigned)(waves < 65536 * 4 ? waves : 65536 * 4)), dim3(CAT_THREADS), 0, st, (int)n_movies, (const unsigned*)w.seg_off,
                           (const unsigned*)w.first, (const int*)w.seg_rating, rating, (const unsigned*)w.words, avg_rating);
        hipLaunchKernelGGL(k_cat_list_count, dim3(mg), dim3(CAT_THREADS), 0, st, (int)n_movies, (const unsigned*)movie_genre_mask, movie_has, G, w.lcnt);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cat_list_scan, dim3(1), dim3(64), 0, st, G, (const unsigned*)w.lcnt, (long long)list_capacity, w.lseg_off, list_offsets, (unsigned long long*)error_key);
    HIP_TRY(hipGetLastError());
    if (n_movies > 0 && list_capacity > 0) {
        hipLaunchKernelGGL(k_cat_list_scatter, dim3(fe_grid_capped(n_movies)), dim3(CAT_THREADS), 0, st, (int)n_movies, (const unsigned*)movie_genre_mask, movie_has, movie_year,
                           movie_file_pos, movie_hash_pos, (const double*)avg_rating, G, (const unsigned*)w.lseg_off, w.lcursor, w.lkey, w.lrow, w.inv_file, w.inv_hash);
        hipLaunchKernelGGL(k_fe_sort_short, dim3((unsigned)L), dim3(FE_THREADS), sort_lds, st, L, cap, (const unsigned*)w.lseg_off, w.lkey, w.lrow, w.llong_list, w.lwords);
        HIP_TRY(hipGetLastError());
        SPRK_TRY(fe_sort_long_segments(cap, (long long)list_capacity, w.lseg_off, w.lkey, w.lrow, w.ltmp_key, w.ltmp_row, w.llong_list, w.lwords, st));
    }
    if (list_capacity > 0) {
        const unsigned wg = fe_grid_capped(list_capacity) < 256u ? fe_grid_capped(list_capacity) : 256u;
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
