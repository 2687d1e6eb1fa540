// api_emb_topk.h -- C ABI: sprk_emb_topk / sprk_emb_topk_workspace_bytes, exact top-K embedding recall over a whole table (k_emb_topk.h).
// Part of sparrow_hip.hip (one translation unit); included there, not compilable on its own.
namespace {
// rows per chunk: ET_CH, or SPRK_EMB_TOPK_CHUNK = a power of two in [64, ET_CH] (tests: deep merge trees at a few thousand rows)
int et_chunk_len() {
    if (const char* e = getenv("SPRK_EMB_TOPK_CHUNK")) {
        const int v = atoi(e);
        if (v >= 64 && v <= ET_CH && (v & (v - 1)) == 0) return v;
    }
    return ET_CH;
}

// The merge tree of one query.  Level 0 = the chunks; a run of level l covers `span` consecutive rows and sits in a place of `slot` =
// min(K, span) pairs; F = 4096 / slot runs merge into one run of the next level; the last level has one run and no place (it is the output).
struct EtLevel { int n_runs; int slot; long long span; };
struct EtPlan {
    int n_levels = 0;
    EtLevel lv[34];
    size_t pairs[2] = {0, 0};             // per query: places of the even / odd levels (they alternate between two buffers)
};
EtPlan et_plan(int n_items, int K, int CH) {
    EtPlan p;
    EtLevel cur{(int)(((long long)n_items + CH - 1) / CH), K < CH ? K : CH, CH};
    while (true) {
        p.lv[p.n_levels] = cur;
        if (cur.n_runs == 1) { ++p.n_levels; break; }
        const size_t need = (size_t)cur.n_runs * cur.slot;
        if (need > p.pairs[p.n_levels & 1]) p.pairs[p.n_levels & 1] = need;
        ++p.n_levels;
        const int F = ET_CH / cur.slot;                                    // >= 4: slot <= K <= 1024
        EtLevel nxt;
        nxt.n_runs = (cur.n_runs + F - 1) / F;
        nxt.span = cur.span * F;                                           // < n_items * 4096 while n_runs > 1
        nxt.slot = nxt.span < K ? (int)nxt.span : K;
        cur = nxt;
    }
    return p;
}
inline int et_pow2(long long n) { int p = 2; while (p < n) p <<= 1; return p; }
inline bool et_sizes_ok(int32_t n_items, int32_t n_queries, int32_t K) { return n_queries >= 0 && K >= 1 && K <= 1024 && K <= n_items; }

// the tree's places in a workspace: keys of the even levels | keys of the odd levels | rows of the even levels | rows of the odd levels
struct EtRuns { unsigned long long* keys[2]; int* rows[2]; };
EtRuns et_split(void* workspace, const EtPlan& p, int n_queries) {
    EtRuns r;
    r.keys[0] = (unsigned long long*)workspace;
    r.keys[1] = r.keys[0] + (size_t)n_queries * p.pairs[0];
    r.rows[0] = (int*)(r.keys[1] + (size_t)n_queries * p.pairs[1]);
    r.rows[1] = r.rows[0] + (size_t)n_queries * p.pairs[0];
    return r;
}

// levels 0 -> 1 -> ... -> last of every query's tree over level 0's runs in r; the last level scores its rows again (table, query) and
// writes last_score / last_row.  Nothing for a tree of one level.
int et_merge_levels(const EtPlan& p, const EtRuns& r, int n_queries, int n_rows, int K, int largest, const float* table, int D, int table_stride, const float* query,
                    int query_stride, double* last_score, int* last_row, hipStream_t st) {
    for (int l = 0; l + 1 < p.n_levels; ++l) {
        const EtLevel& in = p.lv[l];
        const EtLevel& out = p.lv[l + 1];
        const bool last = l + 2 == p.n_levels;
        const int F = ET_CH / in.slot;
        const int P = et_pow2((long long)(in.n_runs < F ? in.n_runs : F) * in.slot);
        const size_t lds = (size_t)P * 12;
        for (int u0 = 0; u0 < n_queries; u0 += 65535) {
            const int nq = n_queries - u0 < 65535 ? n_queries - u0 : 65535;
            hipLaunchKernelGGL(k_emb_topk_merge, dim3((unsigned)out.n_runs, (unsigned)nq), dim3(ET_THREADS), lds, st, (const unsigned long long*)r.keys[l & 1],
                               (const int*)r.rows[l & 1], in.n_runs, in.slot, in.span, F, P, n_rows, K, largest, u0, out.slot,
                               last ? (unsigned long long*)nullptr : r.keys[(l + 1) & 1], last ? (int*)nullptr : r.rows[(l + 1) & 1], table, D, table_stride,
                               query, query_stride, last_score, last_row);
        }
        HIP_TRY(hipGetLastError());
    }
    return SPRK_OK;
}
}  // namespace

extern "C" {

size_t sprk_emb_topk_workspace_bytes(int32_t n_items, int32_t n_queries, int32_t K) {
    if (!et_sizes_ok(n_items, n_queries, K)) return 0;
    const EtPlan p = et_plan(n_items, K, et_chunk_len());
    return (size_t)n_queries * (p.pairs[0] + p.pairs[1]) * 12;
}

int sprk_emb_topk(const float* item_emb, const uint8_t* item_has, int32_t n_items, int32_t D, int32_t item_stride,
                  const float* query_emb, const uint8_t* query_has, int32_t n_queries, int32_t query_stride,
                  int32_t K, int32_t largest, double* scores, int32_t* items, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_emb_topk");
    // every check before any device call
    if (n_items < 0 || n_queries < 0 || D < 1 || D > 1024 || item_stride < D || query_stride < D)
        return fail(SPRK_EINVAL, "emb_topk: bad sizes (need 1 <= D <= 1024, strides >= D)");
    if (K < 1 || K > 1024 || K > n_items) return fail(SPRK_EINVAL, "emb_topk: K = %d outside [1, min(1024, n_items = %d)]", K, n_items);
    if (largest != 0 && largest != 1) return fail(SPRK_EINVAL, "emb_topk: largest must be 0 or 1");
    if (!item_emb || !query_emb || !scores || !items) return fail(SPRK_EINVAL, "emb_topk: NULL table / queries / scores / items");
    const int CH = et_chunk_len();
    const EtPlan p = et_plan(n_items, K, CH);
    const size_t need = (size_t)n_queries * (p.pairs[0] + p.pairs[1]) * 12;
    if (need && (!workspace || workspace_bytes < need))
        return fail(SPRK_EINVAL, "emb_topk: needs a workspace of %zu bytes (sprk_emb_topk_workspace_bytes), got %zu", need, workspace ? workspace_bytes : (size_t)0);
    if (need && ((uintptr_t)workspace & 7)) return fail(SPRK_EINVAL, "emb_topk: the workspace must start on an 8-byte boundary");
    if (n_queries == 0) return SPRK_OK;
    hipStream_t st = (hipStream_t)stream;
    const EtRuns r = et_split(workspace, p, n_queries);
    const bool one = p.n_levels == 1;
    {
        const EtLevel& l0 = p.lv[0];
        const int P = et_pow2(n_items < CH ? n_items : CH);
        const size_t lds = (size_t)P * 12 + (size_t)D * 4;
        for (int u0 = 0; u0 < n_queries; u0 += 65535) {
            const int nq = n_queries - u0 < 65535 ? n_queries - u0 : 65535;
            hipLaunchKernelGGL(k_emb_topk_chunk, dim3((unsigned)l0.n_runs, (unsigned)nq), dim3(ET_THREADS), lds, st, item_emb, item_has, n_items, D, item_stride,
                               query_emb, query_has, query_stride, u0, CH, P, K, largest, one ? 0 : l0.slot, r.keys[0], r.rows[0], scores, items);
        }
        HIP_TRY(hipGetLastError());
    }
    return et_merge_levels(p, r, n_queries, n_items, K, largest, item_emb, D, item_stride, query_emb, query_stride, scores, items, st);
}

}  // extern "C"
