// k_emb_topk.h -- embedding RECALL on the GPU: the K table rows closest to (or, as the Java literally does, farthest from) a query embedding,
// exact, over the whole table.  Reference: SimilarMovieProcess.retrievalCandidatesByEmbedding (SimilarMovieProcess.java:91-112): score every
// movie with calculateEmbSimilarScore (:167-172, Embedding.java:33-47), sort, keep `size`.  Included behind k_emb_rank.h (er_key).
//
// The result is DEFINED as what the ranker gives for cand = 0 .. n_items-1, cut to K: the same doubles (float products from __fmul_rn, widened and
// summed with __dadd_rn in index order, correctly rounded sqrt and division, no contraction -- et_score is k_emb_rank's loop), ordered by
// (score in Double.compareTo order, row index ascending).  That pair is a total order, so the answer does not depend on chunking or merging.
//
//   k_emb_topk_chunk  grid = chunks x queries.  One workgroup scores a chunk of at most ET_CH consecutive rows for its query into LDS as
//                     (64-bit sort key, 32-bit row) pairs, sorts them with the bitonic network of the generic k_emb_rank and emits the first
//                     min(K, rows in the chunk): into the workspace as a sorted run, or -- the table is ONE chunk (the serving shape, 881
//                     movies) -- straight into scores / items: one launch.
//   k_emb_topk_merge  one launch per level of the merge tree; a workgroup loads up to 4096 pairs of consecutive runs, sorts, keeps K, and the
//                     last level (one run per query left) writes scores / items.  Levels are separate stream-ordered launches: no flags, no
//                     counters, no workgroup waits for another.
// Sort key: er_key(score) for `largest`, its complement for ascending order, so both directions sort "greater key first, smaller row first".
// Padding = (key 0, row ET_PAD_ROW): key 0 is below every real key of the descending direction and EQUAL to ascending NaN's, and the row
// index above every real one settles that tie -- padding loses against every real entry in both directions.
// The score is recovered from the key (the map is a bijection on non-NaN doubles); a NaN, whose bits the key does not hold, is computed
// again from the row by the same instruction sequence.
// Why the item norm is not hoisted out of the (query, item) loop: at 4096 rows x D = 32 the scoring is ~4 us of a workgroup whose sort
// takes far longer (78 barrier-separated LDS passes); a table of norms would cost a launch and 8 bytes per row of workspace for nothing measurable.

#define ET_THREADS 512
#define ET_CH 4096                      // rows per chunk and pairs per merge: 4096 x 12 B + the query = 48 KB + 4 D of LDS
#define ET_PAD_ROW 0x7fffffff

__device__ __forceinline__ double et_unkey(unsigned long long k) {          // inverse of er_key on non-NaN doubles
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

// Embedding.calculateSimilarity's quotient for one row: k_emb_rank's inner loop, the same operations in the same order
__device__ __forceinline__ double et_score(const float* __restrict__ row, const float* qv, int D, double r1) {
    double dot = 0.0, n2 = 0.0;
    for (int i = 0; i < D; ++i) {
        const float x = row[i];
        dot = __dadd_rn(dot, (double)__fmul_rn(qv[i], x));
        n2 = __dadd_rn(n2, (double)__fmul_rn(x, x));
    }
    return __ddiv_rn(dot, __dmul_rn(r1, __dsqrt_rn(n2)));
}

// the score behind a sorted pair: from the key, or (NaN) again from the row and the query in global memory -- rare, so one thread does it all
__device__ __forceinline__ double et_pair_score(unsigned long long sort_key, int row, int largest, const float* __restrict__ item_emb, int D,
                                                int item_stride, const float* __restrict__ q) {
    const unsigned long long k = largest ? sort_key : ~sort_key;
    if (k != ~0ull) return et_unkey(k);
    double n1 = 0.0;
    for (int i = 0; i < D; ++i) n1 = __dadd_rn(n1, (double)__fmul_rn(q[i], q[i]));
    return et_score(item_emb + (size_t)row * item_stride, q, D, __dsqrt_rn(n1));
}

// bitonic network over P (a power of two) pairs in LDS: "first" = greater key, or equal key and smaller row.  One thread per compare-exchange.
__device__ __forceinline__ void et_sort(unsigned long long* key, int* row, int P, int tid) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += ET_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long ki = key[i], kl = key[l];
                const int ri = row[i], rl = row[l];
                const bool i_first = ki > kl || (ki == kl && ri < rl);
                const bool up = (i & k) == 0;
                if (up ? !i_first : i_first) { key[i] = kl; key[l] = ki; row[i] = rl; row[l] = ri; }
            }
            __syncthreads();
        }
    }
}

// P = padded sort length (power of two >= rows of a chunk); slot = length of a run's place in the workspace, 0 = the table is one chunk and
// the first K pairs are the answer.  u0 = first query of this launch (grid.y covers at most 65535).
static __global__ __launch_bounds__(ET_THREADS) void k_emb_topk_chunk(const float* __restrict__ item_emb, const unsigned char* __restrict__ item_has,
                                                               int n_items, int D, int item_stride, const float* __restrict__ query_emb,
                                                               const unsigned char* __restrict__ query_has, int query_stride, int u0, int CH, int P,
                                                               int K, int largest, int slot, unsigned long long* __restrict__ ws_key,
                                                               int* __restrict__ ws_row, double* __restrict__ scores, int* __restrict__ items) {
    extern __shared__ unsigned long long et_smem[];
    unsigned long long* key = et_smem;                                     // [P]
    int* row = reinterpret_cast<int*>(et_smem + P);                        // [P]
    float* qv = reinterpret_cast<float*>(row + P);                         // [D]
    const int tid = threadIdx.x, c = blockIdx.x, u = u0 + blockIdx.y;
    const long long base = (long long)c * CH;
    const int cnt = (long long)n_items - base < CH ? (int)(n_items - base) : CH;
    const float* q = query_emb + (size_t)u * query_stride;
    const bool q_ok = query_has ? query_has[u] != 0 : true;
    for (int i = tid; i < D; i += ET_THREADS) qv[i] = q[i];
    __syncthreads();
    double n1 = 0.0;
    for (int i = 0; i < D; ++i) n1 = __dadd_rn(n1, (double)__fmul_rn(qv[i], qv[i]));
    const double r1 = __dsqrt_rn(n1);
    for (int i = tid; i < P; i += ET_THREADS) {
        unsigned long long k = 0ull;
        int r = ET_PAD_ROW;
        if (i < cnt) {
            const long long id = base + i;
            double s = -1.0;
            if (q_ok && (item_has ? item_has[id] != 0 : true)) s = et_score(item_emb + (size_t)id * item_stride, qv, D, r1);
            k = er_key(s);
            if (!largest) k = ~k;
            r = (int)id;
        }
        key[i] = k;
        row[i] = r;
    }
    __syncthreads();
    et_sort(key, row, P, tid);
    const int m = K < cnt ? K : cnt;
    if (slot == 0) {                                                       // one chunk: cnt = n_items >= K
        for (int k = tid; k < m; k += ET_THREADS) {
            scores[(size_t)u * K + k] = et_pair_score(key[k], row[k], largest, item_emb, D, item_stride, q);
            items[(size_t)u * K + k] = row[k];
        }
        return;
    }
    const size_t out = ((size_t)u * gridDim.x + c) * slot;                 // m <= min(K, CH) = slot
    for (int k = tid; k < m; k += ET_THREADS) { ws_key[out + k] = key[k]; ws_row[out + k] = row[k]; }
}

// Runs of one level -> runs of the next.  Input run r of a query holds the first min(K, rows it covers) pairs of rows [r span_in, (r + 1) span_in)
// in a place of slot_in pairs; output run g merges input runs g F .. g F + F - 1 (F slot_in <= 4096).  out_key == nullptr: the last level, one
// run per query, written as scores / items.
static __global__ __launch_bounds__(ET_THREADS) void k_emb_topk_merge(const unsigned long long* __restrict__ in_key, const int* __restrict__ in_row, int n_in,
                                                               int slot_in, long long span_in, int F, int P, int n_items, int K, int largest, int u0,
                                                               int slot_out, unsigned long long* __restrict__ out_key, int* __restrict__ out_row,
                                                               const float* __restrict__ item_emb, int D, int item_stride,
                                                               const float* __restrict__ query_emb, int query_stride, double* __restrict__ scores,
                                                               int* __restrict__ items) {
    extern __shared__ unsigned long long et_smem[];
    unsigned long long* key = et_smem;                                     // [P]
    int* row = reinterpret_cast<int*>(et_smem + P);                        // [P]
    const int tid = threadIdx.x, g = blockIdx.x, u = u0 + blockIdx.y;
    const int r0 = g * F;
    const int nr = n_in - r0 < F ? n_in - r0 : F;
    for (int i = tid; i < P; i += ET_THREADS) {
        const int j = i / slot_in, t = i - j * slot_in;
        unsigned long long k = 0ull;
        int r = ET_PAD_ROW;
        if (j < nr) {
            const long long lo = (long long)(r0 + j) * span_in;
            const long long rows = n_items - lo < span_in ? n_items - lo : span_in;
            if (t < (rows < K ? rows : K)) {
                const size_t src = ((size_t)u * n_in + (r0 + j)) * slot_in + t;
                k = in_key[src];
                r = in_row[src];
            }
        }
        key[i] = k;
        row[i] = r;
    }
    __syncthreads();
    et_sort(key, row, P, tid);
    const long long lo = (long long)r0 * span_in, span_out = span_in * F;
    const long long rows = n_items - lo < span_out ? n_items - lo : span_out;
    const int m = rows < K ? (int)rows : K;
    if (!out_key) {                                                        // last level: rows = n_items >= K
        const float* q = query_emb + (size_t)u * query_stride;
        for (int k = tid; k < m; k += ET_THREADS) {
            scores[(size_t)u * K + k] = et_pair_score(key[k], row[k], largest, item_emb, D, item_stride, q);
            items[(size_t)u * K + k] = row[k];
        }
        return;
    }
    const size_t out = ((size_t)u * gridDim.x + g) * slot_out;             // m <= min(K, span_out) = slot_out
    for (int k = tid; k < m; k += ET_THREADS) { out_key[out + k] = key[k]; out_row[out + k] = row[k]; }
}
