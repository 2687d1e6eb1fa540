// k_lsh.h -- embedding LSH on the device: random-projection buckets (Spark's BucketedRandomProjectionLSH.transform), a sorted index
// per hash table, and the single-probe approxNearestNeighbors over it.  Reference: Embedding.embeddingLSH (Embedding.scala:230-252).
// The definition, rule by rule, is sparrowrecsys_amd/lsh.py (hash_host, approx_nearest_host); these kernels
// give the same bits: every product, sum, quotient and square root rounded on its own in double, in index order -- __dmul_rn and
// __dadd_rn are plain operators in this toolchain and a product feeding a sum would contract into an fma, so contraction is switched
// off in lsh_bucket and lsh_dist (as in k_catalog.h) --, and no float or double atomics anywhere.
//   k_lsh_hash        one thread per (row, table): bucket = floor(dot(row, vector) / bucket_length), clamped; grid-stride
//   k_lsh_index_init  idx_bucket[t][i] = buckets[i][t], idx_row[t][i] = i, and the words seg_sort starts from; grid-stride.  seg_sort
//                     (k_segments.h) then sorts every table's n (bucket, row) keys: one segment per table
//   k_lsh_query       one workgroup per query: hashes the query, finds the bucket's range in every table's sorted index (two binary
//                     searches a table), walks it -- consecutive threads read consecutive index places --, takes a row found through
//                     table t if has != 0 and it matches in no table t' < t (read from `buckets`: each row counts once, no set structure),
//                     scores it and keeps the best K by (distance bits, row): a finite non-negative double orders as its bit pattern.
//                     New pairs gather behind the running best K in an LDS buffer of `chunk` pairs; a full buffer is sorted (bitonic,
//                     k_emb_topk.h's network in ascending form) and cut to K.  Which slot a pair lands in depends on the order of an
//                     integer LDS counter; the answer does not: (distance, row) is a total order over a fixed set.

#define LSH_THREADS 512
#define LSH_CHUNK 4096                   // pairs of the query kernel's buffer: 4096 x 12 B = 48 KB
#define LSH_MAX_T 16
#define LSH_MAX_D 1024
#define LSH_MAX_K 1024
#define LSH_HASH_STAGE_BYTES 32768       // k_lsh_hash keeps the vectors in LDS up to this size, reads them from global memory beyond
#define LSH_QUERY_STAGE_BYTES 8192       // k_lsh_query likewise: 48 KB of pairs + 4 KB of query + this stay inside 64 KB
#define LSH_PAD_ROW 0x7fffffff
static constexpr long long LSH_NO_BUCKET = (long long)0x8000000000000000ull;
static constexpr double LSH_CLAMP = 4611686018427387904.0;               // 2^62

// the bucket of one row in one table: hash_host's operations in hash_host's order.  x: D floats, r: D doubles.
template <class X>
__device__ __forceinline__ long long lsh_bucket(const X* x, const double* r, int D, double bucket_length) {
#pragma clang fp contract(off)
    double dot = 0.0;
    for (int i = 0; i < D; ++i) {
        const double product = (double)x[i] * r[i];
        dot = dot + product;
    }
    if (!(fabs(dot) <= 1.7976931348623157e308)) return LSH_NO_BUCKET;     // NaN or an infinity
    double h = floor(__ddiv_rn(dot, bucket_length));
    h = h < -LSH_CLAMP ? -LSH_CLAMP : (h > LSH_CLAMP ? LSH_CLAMP : h);
    return (long long)h;
}

// the distance of a table row and the query: approx_nearest_host's operations in its order
__device__ __forceinline__ double lsh_dist(const float* __restrict__ x, const float* y, int D) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = 0; i < D; ++i) {
        const double d = (double)x[i] - (double)y[i];
        const double square = d * d;
        s = s + square;
    }
    return __dsqrt_rn(s);
}

// dynamic LDS: T x D doubles when `stage` (the host decides: T D 8 <= LSH_HASH_STAGE_BYTES)
__global__ __launch_bounds__(FE_THREADS) void k_lsh_hash(const float* __restrict__ emb, const unsigned char* __restrict__ has, long long n, int D, int stride,
                                                         const double* __restrict__ vectors, int T, double bucket_length, int stage,
                                                         long long* __restrict__ buckets) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsh_lds[];
    const double* vec = vectors;
    if (stage) {
        double* sv = (double*)lsh_lds;
        for (int i = threadIdx.x; i < T * D; i += FE_THREADS) sv[i] = vectors[i];
        __syncthreads();
        vec = sv;
    }
    const long long total = n * T;
    for (long long e = (long long)blockIdx.x * FE_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * FE_THREADS) {
        const long long i = e / T;
        const int t = (int)(e - i * T);
        long long b = LSH_NO_BUCKET;
        if (has ? has[i] != 0 : true) b = lsh_bucket(emb + (size_t)i * stride, vec + (size_t)t * D, D, bucket_length);
        buckets[e] = b;
    }
}

// off[0 .. 2) = {0, n}: the one segment of every table; n_long[0 .. T) = 0: seg_sort's count of long segments, one word a table
__global__ __launch_bounds__(FE_THREADS) void k_lsh_index_init(const long long* __restrict__ buckets, long long n, int T, long long* __restrict__ idx_bucket,
                                                               int* __restrict__ idx_row, unsigned* __restrict__ off, unsigned* __restrict__ n_long) {
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)T) n_long[threadIdx.x] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) { off[0] = 0u; off[1] = (unsigned)n; }
    const long long total = n * T;
    for (long long e = (long long)blockIdx.x * FE_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * FE_THREADS) {
        const long long t = e / n, i = e - t * n;                          // consecutive threads write consecutive places
        idx_bucket[e] = buckets[i * T + t];
        idx_row[e] = (int)i;
    }
}

// bitonic network over P (a power of two) pairs in LDS, ascending: "first" = smaller key, or equal key and smaller row
__device__ __forceinline__ void lsh_sort(unsigned long long* key, int* row, int P, int tid) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += LSH_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long ki = key[i], kl = key[l];
                const int ri = row[i], rl = row[l];
                const bool i_first = ki < kl || (ki == kl && ri < rl);
                const bool up = (i & k) == 0;
                if (up ? !i_first : i_first) { key[i] = kl; key[l] = ki; row[i] = rl; row[l] = ri; }
            }
            __syncthreads();
        }
    }
}

// the first place of [0, n) whose bucket is >= b, in one table's sorted index
__device__ __forceinline__ long long lsh_lower_bound(const long long* __restrict__ sorted, long long n, long long b) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (sorted[mid] < b) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Dynamic LDS, in this order: key [chunk] | vectors [T D] doubles when `stage` | hq [16] | lo [16] | hi [16] | row [chunk] | query [D] floats.
// Workgroup w takes queries w, w + grid, ...
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_query(const float* __restrict__ emb, const unsigned char* __restrict__ has, long long n, int D, int stride,
                                                           const double* __restrict__ vectors, int T, double bucket_length, int stage,
                                                           const long long* __restrict__ buckets, const long long* __restrict__ idx_bucket,
                                                           const int* __restrict__ idx_row, const float* __restrict__ queries,
                                                           const unsigned char* __restrict__ query_has, int Q, int query_stride, int K, int chunk,
                                                           double* __restrict__ dist, int* __restrict__ rows, int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsh_lds[];
    __shared__ int s_fill;
    unsigned long long* key = (unsigned long long*)lsh_lds;
    double* sv = (double*)(key + chunk);
    long long* hq = (long long*)(sv + (stage ? T * D : 0));
    long long* lo = hq + LSH_MAX_T;
    long long* hi = lo + LSH_MAX_T;
    int* row = (int*)(hi + LSH_MAX_T);
    float* qv = (float*)(row + chunk);
    const int tid = threadIdx.x;
    const double* vec = vectors;
    if (stage) {
        for (int i = tid; i < T * D; i += LSH_THREADS) sv[i] = vectors[i];
        vec = sv;
    }
    for (int q = blockIdx.x; q < Q; q += gridDim.x) {
        const float* qg = queries + (size_t)q * query_stride;
        for (int i = tid; i < D; i += LSH_THREADS) qv[i] = qg[i];
        if (tid == 0) s_fill = 0;
        __syncthreads();                                                    // the query (and, the first time, the vectors) are in LDS
        if (tid < T) hq[tid] = (query_has ? query_has[q] != 0 : true) ? lsh_bucket(qv, vec + (size_t)tid * D, D, bucket_length) : LSH_NO_BUCKET;
        __syncthreads();
        if (tid < 2 * T) {                                                  // [lo, hi) = the places of the query's bucket in table t
            const int t = tid >> 1;
            const long long b = hq[t];
            long long at = 0;
            if (b != LSH_NO_BUCKET) at = lsh_lower_bound(idx_bucket + (size_t)t * n, n, b + (tid & 1));    // b <= 2^62: b + 1 does not wrap
            ((tid & 1) ? hi : lo)[t] = at;
        }
        __syncthreads();
        long long dropped = 0;                                              // candidates cut from the buffer so far
        for (int t = 0; t < T; ++t) {
            if (hq[t] == LSH_NO_BUCKET) continue;
            const int* walk = idx_row + (size_t)t * n;
            long long p = lo[t];
            const long long end = hi[t];
            while (p < end) {
                int fill = s_fill;
                __syncthreads();                                            // every thread has read the counter before any adds to it
                if (fill == chunk) {                                        // full: the best K stay
                    lsh_sort(key, row, chunk, tid);
                    dropped += chunk - K;
                    fill = K;
                    if (tid == 0) s_fill = K;
                    __syncthreads();
                }
                long long tile = end - p;
                if (tile > chunk - fill) tile = chunk - fill;
                if (tile > LSH_THREADS) tile = LSH_THREADS;
                if (tid < tile) {
                    const int r = walk[p + tid];
                    bool take = has ? has[r] != 0 : true;
                    for (int u = 0; take && u < t; ++u) take = hq[u] == LSH_NO_BUCKET || buckets[(size_t)r * T + u] != hq[u];
                    if (take) {
                        const double d = lsh_dist(emb + (size_t)r * stride, qv, D);
                        const int slot = atomicAdd(&s_fill, 1);             // < fill + tile <= chunk
                        key[slot] = (unsigned long long)__double_as_longlong(d);
                        row[slot] = r;
                    }
                }
                p += tile;
                __syncthreads();
            }
        }
        const int fill = s_fill;
        int P = 2;
        while (P < fill) P <<= 1;                                           // <= chunk
        __syncthreads();
        if (fill > 0) {
            for (int i = fill + tid; i < P; i += LSH_THREADS) { key[i] = ~0ull; row[i] = LSH_PAD_ROW; }
            __syncthreads();
            lsh_sort(key, row, P, tid);
        }
        for (int k = tid; k < K; k += LSH_THREADS) {
            const bool real = k < fill;
            dist[(size_t)q * K + k] = __longlong_as_double(real ? (long long)key[k] : 0x7ff8000000000000ll);
            rows[(size_t)q * K + k] = real ? row[k] : -1;
        }
        if (tid == 0) count[q] = (int)(dropped + fill);
        __syncthreads();                                                    // the buffer and the query are free for the next one
    }
}
