// k_rank_scores.h -- the sort behind a ranking model's scores: for every query the candidate POSITIONS in descending score order, the
// `sorted(comparingByValue(reverseOrder()))` of RecForYouProcess.java:69-92 over the float scores a forward wrote.  Same convention as
// k_emb_rank.h, in Float.compare terms: every NaN is one greatest value, 0.0 sorts before -0.0, equal scores keep candidate order.
// Included inside the kernels' namespace.
//
// One workgroup per query.  A candidate is ONE 64-bit word, (order-preserving 32-bit key << 32) | ~position: a descending sort of the
// words is the ranking, ties included, so the bitonic network compares and swaps single words in LDS (padded to the next power of
// two with 0, which is below every real word: 32 KB at C = 4096).  Reads C floats and writes C ints per query; the 55 (C = 1024)
// to 78 (C = 4096) barrier-separated steps of the network are the time.

#define RS_THREADS 256
#define RS_MAX_SORT 4096

__device__ __forceinline__ unsigned rs_key(float s) {
    const unsigned b = __float_as_uint(s);
    if (s != s) return ~0u;                                                // every NaN is the same, greatest value
    return (b >> 31) ? ~b : (b | 0x80000000u);
}

static __global__ __launch_bounds__(RS_THREADS) void k_rank_scores(const float* __restrict__ scores, int C, int P, int* __restrict__ order) {
    unsigned long long* w = reinterpret_cast<unsigned long long*>(smem);   // [P]
    const int tid = threadIdx.x;
    const float* s = scores + (size_t)blockIdx.x * (size_t)C;
    for (int i = tid; i < P; i += RS_THREADS)
        w[i] = i < C ? ((unsigned long long)rs_key(s[i]) << 32) | (unsigned)~(unsigned)i : 0ull;
    __syncthreads();
    // bitonic network, "first" = the greater word
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += RS_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // the lower index of pair t: bit j clear
                const int l = i | j;
                const unsigned long long a = w[i], b = w[l];
                const bool up = (i & k) == 0;                              // this run sorts "first to the front"
                if (up ? a < b : a > b) { w[i] = b; w[l] = a; }
            }
            __syncthreads();
        }
    }
    int* o = order + (size_t)blockIdx.x * (size_t)C;
    for (int i = tid; i < C; i += RS_THREADS) o[i] = (int)~(unsigned)w[i];
}
