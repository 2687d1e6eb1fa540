// k_user_emb.h -- user embeddings from ratings and item embeddings, on the device (Embedding.scala:53-101 generateUserEmb: per user, the
// float32 sum of the embeddings of the movies the user rated, folded from the user's LAST row in file order to the first, divided by the
// number of the user's rows).  The definition these kernels equal bit for bit is sparrowrecsys_amd/userembedding.py user_emb_host;
// DESIGN.md section 5.8 has the rules.  Uses k_segments.h: the counts-only scan, and the segment sort behind the `ungrouped` word.
//
// Stages, one stream, no host synchronisation (api_user_emb.h launches them in this order):
//   k_ue_count      per rating: validate (error word), count the user's ratings; a rating whose predecessor in the input belongs to
//                   another user starts a run: the run's first row is kept, and a user's second run raises the `ungrouped` word
//   k_fe_scan_*<false>  (k_segments.h) exclusive scan over users of the counts: segment offsets
//   -- only when `ungrouped` is raised (the kernels read the word and return; the long-path kernels find an empty list) --
//   k_ue_scatter    per rating: (input row, item row) into its user's segment at an atomic cursor, any order
//   k_fe_sort_short (k_segments.h; its gate is the `ungrouped` word) one workgroup per user: fe_sort_lds by input row; longer segments are listed
//   k_fe_sort_long_chunks + k_fe_merge_pass (+ k_fe_long_copy): the listed segments
//   -- always --
//   k_ue_sum        per (user, dimension): the ordered sum and the division
// The sort's key is (input row, item row): the input row sits where feature engineering keeps the timestamp and alone decides the order
// (rows are distinct); the item row rides where feature engineering keeps the input row, so the sum kernel reads a user's item rows
// as one contiguous run -- a segment of seg_row, or, when the input is grouped by user, the input column itself.
// No float atomics and nothing split along a segment: the result is a function of the input alone.

static constexpr int UE_THREADS = 256;
static_assert(UE_THREADS == FE_THREADS, "api_user_emb.h sizes k_ue_count's and k_ue_scatter's grids with fe_grid_capped");
static constexpr int UE_CHUNK = 16;                // item rows per lane and pipeline stage
static constexpr int UE_MAX_D = 1024;
static constexpr unsigned long long UE_ERR_USER = 1;
enum { UE_W_LONG = 0, UE_W_UNGROUPED = 1, UE_W_NEXT_USER = 2 };     // the workspace's control words

__global__ __launch_bounds__(UE_THREADS) void k_ue_count(long long n, const int* __restrict__ user, int n_users, unsigned* __restrict__ len, unsigned* __restrict__ runs,
                                                         unsigned* __restrict__ first, unsigned* __restrict__ words, unsigned long long* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * UE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * UE_THREADS) {
        const int u = user[i];
        if (u < 0 || u >= n_users) { atomicMin(err, UE_ERR_USER << 32 | (unsigned long long)i); continue; }   // (the row takes no further part)
        atomicAdd(&len[u], 1u);
        if (i == 0 || user[i - 1] != u) {
            first[u] = (unsigned)i;                                            // (read only when every user has one run: one writer)
            if (atomicAdd(&runs[u], 1u)) words[UE_W_UNGROUPED] = 1u;
        }
    }
}

__global__ __launch_bounds__(UE_THREADS) void k_ue_scatter(long long n, const int* __restrict__ user, const int* __restrict__ item_row, int n_users,
                                                           const unsigned* __restrict__ seg_off, unsigned* __restrict__ cursor, long long* __restrict__ seg_key,
                                                           int* __restrict__ seg_item, const unsigned* __restrict__ words) {
    if (!words[UE_W_UNGROUPED]) return;
    for (long long i = (long long)blockIdx.x * UE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * UE_THREADS) {
        const int u = user[i];
        if (u < 0 || u >= n_users) continue;                                   // k_ue_count's predicate
        const size_t pos = (size_t)seg_off[u] + atomicAdd(&cursor[u], 1u);     // < seg_off[u + 1]: the same rows were counted
        seg_key[pos] = i;
        seg_item[pos] = item_row[i];
    }
}

// it[k] = the item row k places before the end of items[0 .. j), j > 0; -1 past its start (the load itself is clamped to items[0]: no branch)
__device__ inline void ue_load_items(const int* __restrict__ items, long long j, int (&it)[UE_CHUNK]) {
#pragma unroll
    for (int k = 0; k < UE_CHUNK; ++k) {
        const long long p = j - 1 - k;
        const int r = items[p > 0 ? p : 0];
        it[k] = p >= 0 ? r : -1;
    }
}

// the table's word and `has` byte of every item row, n_items > 0; a row outside the table reads row 0 and clears its bit of `in`.  A row
// with has = 0 is read like any other (its address is the table's).  Nothing here waits for a load: ue_has does, where the row is used.
__device__ inline void ue_load_rows(const int (&it)[UE_CHUNK], const float* __restrict__ emb, const unsigned char* __restrict__ has, int n_items, int stride, int d,
                                    float (&v)[UE_CHUNK], int (&h)[UE_CHUNK], unsigned& in) {
    in = 0;
#pragma unroll
    for (int k = 0; k < UE_CHUNK; ++k) {
        const bool inside = (unsigned)it[k] < (unsigned)n_items;
        const int r = inside ? it[k] : 0;
        in |= inside ? 1u << k : 0u;
        h[k] = (int)has[r];
        v[k] = emb[(size_t)r * stride + d];
    }
}
__device__ inline bool ue_has(const int (&h)[UE_CHUNK], unsigned in, int k) { return h[k] != 0 && (in >> k & 1u); }

// G lanes, one per dimension, walk one user's item rows from the last to the first; a wave holds 64 / G users.  Users are handed out
// through an integer counter, 64 / G at a time per wave, so a wave behind a long user holds up no other.  The loop-carried dependency
// is one v_add_f32 per row: the item rows of the chunk after the next and the table words of the next chunk are in flight while this
// chunk is added, in order.  A row that adds nothing contributes +0.0f: acc is never -0.0f (it starts at +0.0f, and round-to-nearest
// gives +0.0f for every exact cancellation), so acc + (+0.0f) is acc, bit for bit -- the select stays off the dependency chain.
// mode 0 (Scala): count = the user's rows, emb = acc / (float)count, correctly rounded; mode 1 (PySpark): count = the rows that have
// an embedding, emb = acc.  has = count > 0.  D > G: one walk per G dimensions.
template <int G>
__global__ __launch_bounds__(UE_THREADS) void k_ue_sum(int n_users, const unsigned* __restrict__ seg_off, const unsigned* __restrict__ first, const int* __restrict__ seg_item,
                                                       const int* __restrict__ item_row, const float* __restrict__ item_emb, const unsigned char* __restrict__ item_has,
                                                       int n_items, int D, int item_stride, int mode, float* __restrict__ user_emb, int user_stride,
                                                       unsigned char* __restrict__ user_has, int* __restrict__ user_count, unsigned* __restrict__ words) {
    constexpr unsigned PER_WAVE = 64 / G;
    const int lane = threadIdx.x & 63, gl = lane % G;
    const bool ungrouped = words[UE_W_UNGROUPED] != 0;
    for (;;) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&words[UE_W_NEXT_USER], PER_WAVE);
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        if (base >= (unsigned)n_users) break;                                  // (the whole wave)
        const unsigned u = base + (unsigned)(lane / G);
        if (u < (unsigned)n_users) {                                           // (a wave's last draw can pass the end)
            const unsigned lo = seg_off[u], len = seg_off[u + 1] - lo;
            const int* __restrict__ items = ungrouped ? seg_item + lo : item_row + (len ? first[u] : 0u);
            for (int d0 = 0; d0 < D; d0 += G) {
                const int d = d0 + gl;
                const bool live = d < D;
                const int dc = live ? d : 0;
                float acc = 0.0f;
                unsigned n_emb = 0;
                int it[UE_CHUNK], hb[UE_CHUNK], hc[UE_CHUNK];
                float vb[UE_CHUNK], vc[UE_CHUNK];
                unsigned inb = 0, inc = 0;
                long long j = (n_items > 0) ? (long long)len : 0;               // (an empty table: no row has an embedding)
                if (j > 0) {
                    ue_load_items(items, j, it);
                    ue_load_rows(it, item_emb, item_has, n_items, item_stride, dc, vb, hb, inb);
                    if (j > UE_CHUNK) ue_load_items(items, j - UE_CHUNK, it);
                }
                while (j > 0) {
                    if (j > UE_CHUNK) ue_load_rows(it, item_emb, item_has, n_items, item_stride, dc, vc, hc, inc);
                    if (j > 2 * UE_CHUNK) ue_load_items(items, j - 2 * UE_CHUNK, it);
#pragma unroll
                    for (int k = 0; k < UE_CHUNK; ++k) {
                        const bool has = ue_has(hb, inb, k);
                        acc += has ? vb[k] : 0.0f;
                        n_emb += has ? 1u : 0u;
                    }
                    j -= UE_CHUNK;
                    if (j > 0) {
#pragma unroll
                        for (int k = 0; k < UE_CHUNK; ++k) { vb[k] = vc[k]; hb[k] = hc[k]; }
                        inb = inc;
                    }
                }
                const unsigned count = mode == 0 ? len : n_emb;
                if (live) user_emb[(size_t)u * user_stride + d] = (mode == 0 && len) ? acc / (float)len : acc;
                if (d == 0) {
                    user_has[u] = count ? 1 : 0;
                    user_count[u] = (int)count;
                }
            }
        }
    }
}
