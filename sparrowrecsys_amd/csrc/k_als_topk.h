// k_als_topk.h -- ALS recommendations on the GPU: for every query factor row the K rows of the other table with the largest score (the
// reference's recommendForAllUsers / recommendForAllItems, CollaborativeFiltering.scala).  Included behind k_emb_topk.h, whose selection
// it reuses: er_key's sortable 64-bit key, et_sort's bitonic network, the (key, row) runs and k_emb_topk_merge's merge tree.
//
// The score is ALSModel's float32 dot in index order, every product and every sum rounded on its own (als.py predict_host; k_als.h's
// als_dot is the same loop in the other translation unit); widened to double it fits the existing key exactly.  Order: descending score,
// equal scores by ascending row -- a total order, so the answer does not depend on chunking or merging.  A table row with has == 0 and
// every row of a query with has == 0 is no candidate: it becomes the selection's padding (key 0, row ET_PAD_ROW), which loses against every
// real entry, and comes out as -1 / NaN; so does every place past the rows available when K exceeds them.
//
//   k_als_topk_chunk   k_emb_topk_chunk's sibling with this score and this padding; one chunk = the whole table: it writes the answer.
//   k_emb_topk_merge   unchanged, every level; its last level writes (double score, row) pairs into the workspace
//   k_als_topk_finish  those pairs -> the float32 scores (computed again from the row: a NaN score's bits are not in the key) and rows, padded

__device__ __forceinline__ float at_dot(const float* __restrict__ row, const float* qv, int D) {
#pragma clang fp contract(off)
    float acc = 0.0f;
    for (int i = 0; i < D; ++i) {
        const float prod = qv[i] * row[i];
        acc = acc + prod;
    }
    return acc;
}

// P = padded sort length (power of two >= rows of a chunk); slot = length of a run's place in the workspace, 0 = the table is one chunk and
// the first K pairs are the answer.  u0 = first query of this launch (grid.y covers at most 65535).
static __global__ __launch_bounds__(ET_THREADS) void k_als_topk_chunk(const float* __restrict__ table, const unsigned char* __restrict__ table_has, int n_rows, int D,
                                                                      int table_stride, const float* __restrict__ query, const unsigned char* __restrict__ query_has,
                                                                      int query_stride, int u0, int CH, int P, int K, int slot, unsigned long long* __restrict__ ws_key,
                                                                      int* __restrict__ ws_row, float* __restrict__ scores, int* __restrict__ rows) {
    extern __shared__ unsigned long long et_smem[];
    unsigned long long* key = et_smem;                                     // [P]
    int* row = reinterpret_cast<int*>(et_smem + P);                        // [P]
    float* qv = reinterpret_cast<float*>(row + P);                         // [D]
    const int tid = threadIdx.x, c = blockIdx.x, u = u0 + blockIdx.y;
    const long long base = (long long)c * CH;
    const int cnt = (long long)n_rows - base < CH ? (int)(n_rows - base) : CH;
    const float* q = query + (size_t)u * query_stride;
    const bool q_ok = query_has[u] != 0;
    for (int i = tid; i < D; i += ET_THREADS) qv[i] = q[i];
    __syncthreads();
    for (int i = tid; i < P; i += ET_THREADS) {
        unsigned long long k = 0ull;
        int r = ET_PAD_ROW;
        if (i < cnt && q_ok && table_has[base + i] != 0) {
            k = er_key((double)at_dot(table + (size_t)(base + i) * table_stride, qv, D));
            r = (int)(base + i);
        }
        key[i] = k;
        row[i] = r;
    }
    __syncthreads();
    et_sort(key, row, P, tid);
    const int m = K < cnt ? K : cnt;
    if (slot == 0) {                                                       // one chunk: every place of the answer is written here
        for (int k = tid; k < K; k += ET_THREADS) {
            const bool real = k < m && row[k] != ET_PAD_ROW;
            scores[(size_t)u * K + k] = real ? at_dot(table + (size_t)row[k] * table_stride, qv, D) : __uint_as_float(0x7fc00000u);
            rows[(size_t)u * K + k] = real ? row[k] : -1;
        }
        return;
    }
    const size_t out = ((size_t)u * gridDim.x + c) * slot;                 // m <= min(K, CH) = slot
    for (int k = tid; k < m; k += ET_THREADS) { ws_key[out + k] = key[k]; ws_row[out + k] = row[k]; }
}

// in_row [n_queries][K] = k_emb_topk_merge's last level, of which the first m = min(K, n_rows) places per query are written (m = 0: an empty
// table, nothing was launched before)
static __global__ __launch_bounds__(ET_THREADS) void k_als_topk_finish(const int* __restrict__ in_row, long long n_out, int K, int m, const float* __restrict__ table,
                                                                       int D, int table_stride, const float* __restrict__ query, int query_stride,
                                                                       float* __restrict__ scores, int* __restrict__ rows) {
    for (long long i = (long long)blockIdx.x * ET_THREADS + threadIdx.x; i < n_out; i += (long long)gridDim.x * ET_THREADS) {
        const long long u = i / K;
        const int k = (int)(i - u * K);
        const int r = k < m ? in_row[i] : ET_PAD_ROW;
        const bool real = r != ET_PAD_ROW;
        scores[i] = real ? at_dot(table + (size_t)r * table_stride, query + (size_t)u * query_stride, D) : __uint_as_float(0x7fc00000u);
        rows[i] = real ? r : -1;
    }
}
