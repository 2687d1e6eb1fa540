// api_als_topk.h -- C ABI: sprk_als_topk / sprk_als_topk_workspace_bytes, the K best rows of a factor table for every query factor row
// (k_als_topk.h).  Uses api_emb_topk.h's chunk length (SPRK_EMB_TOPK_CHUNK), merge plan, workspace split and merge tree driver (et_plan, et_split, et_merge_levels).
namespace {
inline bool at_sizes_ok(int32_t n_rows, int32_t n_queries, int32_t K) { return n_rows >= 0 && n_queries >= 0 && K >= 1 && K <= 1024; }
// the workspace: the merge tree's runs (api_emb_topk.h's layout), then the last level's [n_queries][K] doubles and rows; 0 when the table is one chunk
size_t at_tree_bytes(const EtPlan& p, int32_t n_queries) { return ((size_t)n_queries * (p.pairs[0] + p.pairs[1]) * 12 + 15) / 16 * 16; }
size_t at_workspace_bytes(const EtPlan& p, int32_t n_queries, int32_t K) {
    if (p.n_levels == 1) return 0;
    return at_tree_bytes(p, n_queries) + (size_t)n_queries * K * 12;
}
}  // namespace

extern "C" {

size_t sprk_als_topk_workspace_bytes(int32_t n_rows, int32_t n_queries, int32_t K) {
    if (!at_sizes_ok(n_rows, n_queries, K) || n_rows == 0) return 0;
    return at_workspace_bytes(et_plan(n_rows, K, et_chunk_len()), n_queries, K);
}

int sprk_als_topk(const float* table, const uint8_t* table_has, int32_t n_rows, int32_t rank, int32_t table_stride,
                  const float* query, const uint8_t* query_has, int32_t n_queries, int32_t query_stride,
                  int32_t K, float* scores, int32_t* rows, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_als_topk");
    // every check before any device call
    if (n_rows < 0 || n_queries < 0 || rank < 1 || rank > 16 || table_stride < rank || query_stride < rank)
        return fail(SPRK_EINVAL, "als_topk: bad sizes (need n_rows >= 0, n_queries >= 0, 1 <= rank <= 16, strides >= rank)");
    if (K < 1 || K > 1024) return fail(SPRK_EINVAL, "als_topk: K = %d outside [1, 1024]", K);
    if (n_rows > 0 && (!table || !table_has)) return fail(SPRK_EINVAL, "als_topk: NULL table");
    if (n_queries > 0 && (!query || !query_has || !scores || !rows)) return fail(SPRK_EINVAL, "als_topk: NULL queries / scores / rows");
    if (((uintptr_t)table & 3) || ((uintptr_t)query & 3) || ((uintptr_t)scores & 3) || ((uintptr_t)rows & 3)) return fail(SPRK_EINVAL, "als_topk: misaligned column");
    const int CH = et_chunk_len();
    const EtPlan p = n_rows > 0 ? et_plan(n_rows, K, CH) : EtPlan();
    const size_t need = n_rows > 0 ? at_workspace_bytes(p, n_queries, K) : 0;
    if (need && (!workspace || workspace_bytes < need))
        return fail(SPRK_EINVAL, "als_topk: needs a workspace of %zu bytes (sprk_als_topk_workspace_bytes), got %zu", need, workspace ? workspace_bytes : (size_t)0);
    if (need && ((uintptr_t)workspace & 15)) return fail(SPRK_EINVAL, "als_topk: the workspace must start on a 16-byte boundary");
    if (n_queries == 0) return SPRK_OK;
    hipStream_t st = (hipStream_t)stream;
    const long long n_out = (long long)n_queries * K;
    const unsigned fg = (unsigned)((n_out + ET_THREADS - 1) / ET_THREADS < 2048 ? (n_out + ET_THREADS - 1) / ET_THREADS : 2048);
    if (n_rows == 0) {                                                      // no candidate: every place is -1 / NaN
        hipLaunchKernelGGL(k_als_topk_finish, dim3(fg), dim3(ET_THREADS), 0, st, (const int*)nullptr, n_out, (int)K, 0, table, (int)rank, (int)table_stride, query,
                           (int)query_stride, scores, rows);
        HIP_TRY(hipGetLastError());
        return SPRK_OK;
    }
    // workspace: the tree's places (et_split) | last level: doubles | rows
    const EtRuns r = et_split(workspace, p, n_queries);
    double* last_score = (double*)((unsigned char*)workspace + at_tree_bytes(p, n_queries));
    int* last_row = (int*)(last_score + (size_t)n_out);
    const bool one = p.n_levels == 1;
    {
        const EtLevel& l0 = p.lv[0];
        const int P = et_pow2(n_rows < CH ? n_rows : CH);
        const size_t lds = (size_t)P * 12 + (size_t)rank * 4;
        for (int u0 = 0; u0 < n_queries; u0 += 65535) {
            const int nq = n_queries - u0 < 65535 ? n_queries - u0 : 65535;
            hipLaunchKernelGGL(k_als_topk_chunk, dim3((unsigned)l0.n_runs, (unsigned)nq), dim3(ET_THREADS), lds, st, table, table_has, (int)n_rows, (int)rank, (int)table_stride,
                               query, query_has, (int)query_stride, u0, CH, P, (int)K, one ? 0 : l0.slot, r.keys[0], r.rows[0], scores, rows);
        }
        HIP_TRY(hipGetLastError());
    }
    if (one) return SPRK_OK;
    SPRK_TRY(et_merge_levels(p, r, n_queries, n_rows, K, 1, table, rank, table_stride, query, query_stride, last_score, last_row, st));
    hipLaunchKernelGGL(k_als_topk_finish, dim3(fg), dim3(ET_THREADS), 0, st, (const int*)last_row, n_out, (int)K, (int)(n_rows < K ? n_rows : K), table, (int)rank,
                       (int)table_stride, query, (int)query_stride, scores, rows);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
