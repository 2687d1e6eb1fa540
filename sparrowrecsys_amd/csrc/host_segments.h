// host_segments.h -- the host side of k_segments.h, shared by the entry points of sparrow_feature_eng.hip (api_feature_eng.h, api_store_update.h,
// api_user_emb.h, api_catalog.h, api_als.h, api_item2vec.h, api_lsh.h, api_split.h, api_rank_eval.h): the sort capacity and the grids, the workspace carver and the workspace check, seg_scan
// (counts -> offsets) and seg_sort (every segment of one side by its key).  Everything is enqueued on the caller's stream.
namespace {
// LDS sort capacity: FE_SORT_CAP, or SPRK_FE_SORT_CAP = a power of two in [64, FE_SORT_CAP], read at each call (tests: the long path at small sizes)
int fe_sort_cap() {
    if (const char* e = getenv("SPRK_FE_SORT_CAP")) {
        const int v = atoi(e);
        if (v >= 64 && v <= FE_SORT_CAP && (v & (v - 1)) == 0) return v;
    }
    return FE_SORT_CAP;
}
inline unsigned fe_grid(long long items) {
    const long long g = (items + FE_THREADS - 1) / FE_THREADS;
    return (unsigned)(g < 1 ? 1 : g);
}
// Grid cap: FE_MAX_GRID, or SPRK_FE_MAX_GRID = an integer in [1, FE_MAX_GRID], read at each call (tests: a grid-stride loop's second round and a
// work queue's second draw at small sizes; results do not depend on the grid).  fe_max_grid_env() = that value, 0 where the variable is unset
// or anything else: the launches with a cap of their own (k_fe_sort_short, k_cat_avg_wave, k_cat_list_write) keep it then.
inline unsigned fe_max_grid_env() {
    if (const char* e = getenv("SPRK_FE_MAX_GRID")) {
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end != e && *end == 0 && v >= 1 && v <= FE_MAX_GRID) return (unsigned)v;
    }
    return 0;
}
inline unsigned fe_max_grid() { const unsigned v = fe_max_grid_env(); return v ? v : (unsigned)FE_MAX_GRID; }
inline unsigned fe_grid_capped(long long items) { const unsigned g = fe_grid(items), cap = fe_max_grid(); return g < cap ? g : cap; }
// a launch with a cap of its own: `g` workgroups as the launch sizes them, under SPRK_FE_MAX_GRID where that is set
inline unsigned fe_grid_own_cap(unsigned g) { const unsigned v = fe_max_grid_env(); return v && v < g ? v : g; }

// A workspace handed out part by part, in order; every part starts on a 16-byte boundary.  at = the bytes taken so far.
struct Carver {
    void* base;
    size_t at = 0;
    template <class T> T* take(size_t count) {
        T* p = (T*)((unsigned char*)base + at);
        at += (count * sizeof(T) + 15) / 16 * 16;
        return p;
    }
};

// the caller's workspace against the size `bytes_fn` reports: call = the entry point's short name in its messages
int check_workspace(const char* call, const char* bytes_fn, const void* workspace, size_t given, size_t needed) {
    if (!workspace || given < needed)
        return fail(SPRK_EINVAL, "%s: needs a workspace of %zu bytes (%s), got %zu", call, needed, bytes_fn, workspace ? given : (size_t)0);
    if ((uintptr_t)workspace & 15) return fail(SPRK_EINVAL, "%s: the workspace must start on a 16-byte boundary", call);
    return SPRK_OK;
}

// tiles of a scan over ids [0, n_ids) and the total past them
inline int seg_scan_tiles(size_t n_ids) { return (int)((n_ids + 1 + FE_SCAN_TILE - 1) / FE_SCAN_TILE); }

// off[0 .. count) from counts to their exclusive scan, in place.  FeScanKept<false>{}: that alone, tops holds n_tiles words.
// FeScanKept<true>{kept_off, n_kept}: also kept_off[i] = the exclusive scan of max(0, count_i - 2) and its total to *n_kept; 2 n_tiles words.
template <bool KEPT> int seg_scan(unsigned* off, long long count, unsigned* tops, int n_tiles, FeScanKept<KEPT> second, hipStream_t st) {
    hipLaunchKernelGGL(k_fe_scan_tiles<KEPT>, dim3((unsigned)n_tiles), dim3(FE_THREADS), 0, st, off, count, tops, n_tiles, second);
    hipLaunchKernelGGL(k_fe_scan_tops<KEPT>, dim3(1), dim3(FE_THREADS), 0, st, tops, n_tiles);
    hipLaunchKernelGGL(k_fe_scan_add<KEPT>, dim3(fe_grid(count)), dim3(FE_THREADS), 0, st, off, count, (const unsigned*)tops, n_tiles, second);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

// The segments k_fe_sort_short listed (longer than `cap`), sorted where they are: chunks of `cap` in LDS, then merge passes between
// (seg_ts, seg_row) and (tmp_ts, tmp_row), and a copy back after an odd number of passes.  n = all keys: no segment is longer.
int fe_sort_long_segments(int cap, long long n, const unsigned* seg_off, long long* seg_ts, int* seg_row, long long* tmp_ts, int* tmp_row, const int* long_list,
                          const unsigned* n_long, hipStream_t st) {
    if (n <= cap) return SPRK_OK;                                           // no segment can be longer than the LDS sort holds
    const size_t sort_lds = (size_t)cap * 12;
    const unsigned lg = fe_grid_capped(n);
    const unsigned cg = (unsigned)((n + cap - 1) / cap) < fe_max_grid() ? (unsigned)((n + cap - 1) / cap) : fe_max_grid();
    hipLaunchKernelGGL(k_fe_sort_long_chunks, dim3(cg), dim3(FE_THREADS), sort_lds, st, cap, seg_off, seg_ts, seg_row, long_list, n_long);
    HIP_TRY(hipGetLastError());
    long long* ts[2] = {seg_ts, tmp_ts};
    int* row[2] = {seg_row, tmp_row};
    int at = 0;
    for (long long width = cap; width < n; width *= 2, at ^= 1) {
        hipLaunchKernelGGL(k_fe_merge_pass, dim3(lg), dim3(FE_THREADS), 0, st, width, seg_off, (const long long*)ts[at], (const int*)row[at], ts[at ^ 1], row[at ^ 1], long_list, n_long);
        HIP_TRY(hipGetLastError());
    }
    if (at) {
        hipLaunchKernelGGL(k_fe_long_copy, dim3(lg), dim3(FE_THREADS), 0, st, seg_off, (const long long*)tmp_ts, (const int*)tmp_row, seg_ts, seg_row, long_list, n_long);
        HIP_TRY(hipGetLastError());
    }
    return SPRK_OK;
}

// Every segment of one side by (key, val): in LDS up to `cap` keys, chunks and merge passes beyond.  n = the keys of all n_segs segments;
// long_list has room for every segment longer than 64 keys (n / 64 + 1, or n_segs) and *n_long counts them from 0; tmp_key / tmp_val hold
// n keys; gate: k_fe_sort_short's (null: always sort).
int seg_sort(int cap, long long n, int n_segs, const unsigned* off, long long* key, int* val, long long* tmp_key, int* tmp_val, int* long_list, unsigned* n_long,
             const unsigned* gate, hipStream_t st) {
    if (n_segs == 0) return SPRK_OK;
    const unsigned g = fe_grid_own_cap((unsigned)n_segs < 65536u * 16u ? (unsigned)n_segs : 65536u * 16u);
    hipLaunchKernelGGL(k_fe_sort_short, dim3(g), dim3(FE_THREADS), (size_t)cap * 12, st, n_segs, cap, off, key, val, long_list, n_long, gate);
    HIP_TRY(hipGetLastError());
    return fe_sort_long_segments(cap, n, off, key, val, tmp_key, tmp_val, long_list, n_long, st);
}
}  // namespace
