// k_segments.h -- counts per id -> segment offsets, and every segment sorted by a 64-bit key with a 32-bit payload: the device code
// that the ratings pipelines of sparrow_feature_eng.hip share.  host_segments.h launches it (seg_scan, seg_sort).
//   feature engineering (k_feature_eng.h)  segments per user, key (timestamp, input row); the scan with its `kept` half
//   store updates (k_store_update.h)       segments per user of the NEW ratings, key (timestamp, row in the batch)
//   user embeddings (k_user_emb.h)         segments per user, key (input row, item row), the sort behind the `ungrouped` word
//   the catalogue (k_catalog.h)            segments per movie, behind the word likewise, and the 2 (G + 1) lists; fe_block_scan in k_cat_similar
//   ALS (k_als.h)                          segments per user and per movie
//   item2vec (k_item2vec.h)                segments per user, key (timestamp, input row); per `prev` item, key (next, place); per row of
//                                          syn0 / syn1, key (centre, context or depth)
//   ranking metrics (k_rank_eval.h)        segments per user of the truth pairs and of the seen pairs, key (item, input row)
// The kernels keep the names they got in feature engineering, where they were written first: k_fe_* are the names in rocprof traces,
// in the timing tables of docs/*_results.md, in DESIGN.md sections 5.7-5.10 and in the GPU tests' docstrings.
//   k_fe_scan_*     exclusive scan over ids of len (and, KEPT, of kept = max(0, len - 2)): three launches
//   k_fe_sort_short one workgroup per id: segments of up to `cap` keys sorted in LDS; longer ones are listed
//   k_fe_sort_long_chunks + k_fe_merge_pass x ceil(log2(n / cap)) (+ k_fe_long_copy): the listed segments, sorted in chunks of `cap`
//                   and merged in global memory by rank (keys are distinct: rank in the partner run = one binary search)

static constexpr int FE_THREADS = 256;
static constexpr int FE_SORT_CAP = 4096;          // keys of one segment sorted in LDS: 4096 x 12 bytes = 48 KB, three workgroups per CU
static constexpr int FE_SCAN_TILE = 4 * FE_THREADS;
static constexpr int FE_MAX_GRID = 2048;

__device__ inline bool fe_key_less(long long ta, int ra, long long tb, int rb) { return ta < tb || (ta == tb && ra < rb); }

// exclusive scan of one value per thread over the workgroup (FE_THREADS); sh holds FE_THREADS words
__device__ inline unsigned fe_block_scan(unsigned v, unsigned* sh, unsigned* total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < FE_THREADS; d <<= 1) {
        const unsigned a = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const unsigned incl = sh[t];
    *total = sh[FE_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// What the scan's second half writes, the last argument of the three scan kernels: kept[count] and the place of its total.  The
// counts-only scan (KEPT = false) has no such half: its kernels get no pointer to it, and tops holds n_tiles words, not 2 n_tiles.
template <bool KEPT> struct FeScanKept {};
template <> struct FeScanKept<true> { unsigned* __restrict__ kept; long long* __restrict__ n_kept; };

// seg[i] = len_i, kept[i] = (unwritten) for i in [0, count): both become tile-local exclusive scans, the tiles' totals go to tops
template <bool KEPT>
__global__ __launch_bounds__(FE_THREADS) void k_fe_scan_tiles(unsigned* __restrict__ seg, long long count, unsigned* __restrict__ tops, int n_tiles, FeScanKept<KEPT> second) {
    __shared__ unsigned sh[FE_THREADS];
    const long long base = (long long)blockIdx.x * FE_SCAN_TILE + (long long)threadIdx.x * 4;
    unsigned a[4], b[4], sa = 0, sb = 0;
    for (int k = 0; k < 4; ++k) {
        a[k] = base + k < count ? seg[base + k] : 0u;
        b[k] = a[k] > 2 ? a[k] - 2 : 0u;
        sa += a[k]; sb += b[k];
    }
    unsigned ta, tb = 0;
    unsigned ea = fe_block_scan(sa, sh, &ta), eb = 0;
    if constexpr (KEPT) eb = fe_block_scan(sb, sh, &tb);
    for (int k = 0; k < 4; ++k) {
        if (base + k < count) { seg[base + k] = ea; if constexpr (KEPT) second.kept[base + k] = eb; }
        ea += a[k]; eb += b[k];
    }
    if (threadIdx.x == 0) { tops[blockIdx.x] = ta; if constexpr (KEPT) tops[n_tiles + blockIdx.x] = tb; }
}

// one workgroup: tops[0..n_tiles) and, KEPT, tops[n_tiles..2 n_tiles) become exclusive scans
template <bool KEPT>
__global__ __launch_bounds__(FE_THREADS) void k_fe_scan_tops(unsigned* __restrict__ tops, int n_tiles) {
    __shared__ unsigned sh[FE_THREADS];
    for (int w = 0; w < (KEPT ? 2 : 1); ++w) {
        unsigned* t = tops + (size_t)w * n_tiles;
        unsigned carry = 0;
        for (int b0 = 0; b0 < n_tiles; b0 += FE_THREADS) {
            const int i = b0 + threadIdx.x;
            const unsigned v = i < n_tiles ? t[i] : 0u;
            unsigned total;
            const unsigned e = fe_block_scan(v, sh, &total);
            if (i < n_tiles) t[i] = carry + e;
            carry += total;
        }
    }
}

// adds the tiles' offsets; element count - 1 (the one past the last id) then holds the totals: the number of kept samples goes to n_kept
template <bool KEPT>
__global__ __launch_bounds__(FE_THREADS) void k_fe_scan_add(unsigned* __restrict__ seg, long long count, const unsigned* __restrict__ tops, int n_tiles, FeScanKept<KEPT> second) {
    const long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x;
    if (i >= count) return;
    const int tile = (int)(i / FE_SCAN_TILE);
    seg[i] += tops[tile];
    if constexpr (KEPT) {
        const unsigned k = second.kept[i] + tops[n_tiles + tile];
        second.kept[i] = k;
        if (i == count - 1) *second.n_kept = (long long)k;
    }
}

// sorts count <= cap keys at (gts, grow) by (timestamp, input row) in LDS: bitonic over P = the next power of two, padded with keys greater
// than any real one (input rows are < 2^31 - 1)
__device__ inline void fe_sort_lds(long long* __restrict__ gts, int* __restrict__ grow, int count, long long* sts, int* srow) {
    int P = 2;
    while (P < count) P <<= 1;
    for (int i = threadIdx.x; i < P; i += FE_THREADS) {
        sts[i] = i < count ? gts[i] : 0x7fffffffffffffffll;
        srow[i] = i < count ? grow[i] : 0x7fffffff;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += FE_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const long long ta = sts[i], tb = sts[x];
                    const int ra = srow[i], rb = srow[x];
                    const bool up = (i & k) == 0;
                    if (fe_key_less(tb, rb, ta, ra) == up) { sts[i] = tb; sts[x] = ta; srow[i] = rb; srow[x] = ra; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < count; i += FE_THREADS) { gts[i] = sts[i]; grow[i] = srow[i]; }
    __syncthreads();
}

// dynamic LDS: cap x 8 bytes of timestamps, then cap x 4 bytes of rows.  gate: null, or a word that is zero when the segments need no
// sort (k_ue_count's and k_cat_count's `ungrouped`): the whole workgroup returns
__global__ __launch_bounds__(FE_THREADS) void k_fe_sort_short(int n_users, int cap, const unsigned* __restrict__ seg_off, long long* __restrict__ seg_ts, int* __restrict__ seg_row,
                                                              int* __restrict__ long_list, unsigned* __restrict__ n_long, const unsigned* gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fe_lds[];
    if (gate && !*gate) return;
    long long* sts = (long long*)fe_lds;
    int* srow = (int*)(fe_lds + (size_t)cap * 8);
    for (int u = blockIdx.x; u < n_users; u += gridDim.x) {
        const unsigned base = seg_off[u], len = seg_off[u + 1] - base;
        if (len < 2) continue;
        if (len <= (unsigned)cap) fe_sort_lds(seg_ts + base, seg_row + base, (int)len, sts, srow);
        else if (threadIdx.x == 0) long_list[atomicAdd(n_long, 1u)] = u;        // at most n / (cap + 1) users: the list holds n / 64 + 1
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_fe_sort_long_chunks(int cap, const unsigned* __restrict__ seg_off, long long* __restrict__ seg_ts, int* __restrict__ seg_row,
                                                                    const int* __restrict__ long_list, const unsigned* __restrict__ n_long) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fe_lds[];
    long long* sts = (long long*)fe_lds;
    int* srow = (int*)(fe_lds + (size_t)cap * 8);
    const unsigned nl = *n_long;
    for (unsigned s = 0; s < nl; ++s) {
        const int u = long_list[s];
        const unsigned base = seg_off[u], len = seg_off[u + 1] - base;
        const unsigned chunks = (len + cap - 1) / cap;
        for (unsigned c = blockIdx.x; c < chunks; c += gridDim.x) {
            const unsigned o = c * (unsigned)cap, cnt = len - o < (unsigned)cap ? len - o : (unsigned)cap;
            fe_sort_lds(seg_ts + base + o, seg_row + base + o, (int)cnt, sts, srow);
        }
    }
}

// one merge level of every listed segment: sorted runs of `width` keys pair up; a key's place in the merged pair is its index in its own
// run plus its rank in the partner run.  A run without a partner (and a segment of one run) is copied, so all segments move src -> dst together.
__global__ __launch_bounds__(FE_THREADS) void k_fe_merge_pass(long long width, const unsigned* __restrict__ seg_off, const long long* __restrict__ src_ts, const int* __restrict__ src_row,
                                                              long long* __restrict__ dst_ts, int* __restrict__ dst_row, const int* __restrict__ long_list,
                                                              const unsigned* __restrict__ n_long) {
    const unsigned nl = *n_long;
    for (unsigned s = 0; s < nl; ++s) {
        const int u = long_list[s];
        const long long base = seg_off[u], len = (long long)seg_off[u + 1] - base;
        for (long long p = (long long)blockIdx.x * FE_THREADS + threadIdx.x; p < len; p += (long long)gridDim.x * FE_THREADS) {
            const long long run = p / width, rs = run * width, ps = (run ^ 1) * width;
            const long long t = src_ts[base + p];
            const int r = src_row[base + p];
            long long out = p;
            if (ps < len) {
                long long lo = ps, hi = ps + width < len ? ps + width : len;            // the partner's keys less than this one: [ps, lo)
                while (lo < hi) {
                    const long long mid = (lo + hi) >> 1;
                    if (fe_key_less(src_ts[base + mid], src_row[base + mid], t, r)) lo = mid + 1; else hi = mid;
                }
                out = (rs < ps ? rs : ps) + (p - rs) + (lo - ps);                         // < the pair's end <= len
            }
            dst_ts[base + out] = t;
            dst_row[base + out] = r;
        }
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_fe_long_copy(const unsigned* __restrict__ seg_off, const long long* __restrict__ src_ts, const int* __restrict__ src_row,
                                                             long long* __restrict__ dst_ts, int* __restrict__ dst_row, const int* __restrict__ long_list,
                                                             const unsigned* __restrict__ n_long) {
    const unsigned nl = *n_long;
    for (unsigned s = 0; s < nl; ++s) {
        const int u = long_list[s];
        const long long base = seg_off[u], len = (long long)seg_off[u + 1] - base;
        for (long long p = (long long)blockIdx.x * FE_THREADS + threadIdx.x; p < len; p += (long long)gridDim.x * FE_THREADS) {
            dst_ts[base + p] = src_ts[base + p];
            dst_row[base + p] = src_row[base + p];
        }
    }
}
