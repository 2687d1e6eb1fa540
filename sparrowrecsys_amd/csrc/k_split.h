// k_split.h -- the held-out split of the samples (featureeng.py split_host is the definition): a sample of the
// rows, cut into a training and a test part at random or at a quantile of the timestamps, as two ascending lists of source positions,
// and the rows of any columns taken by such a list.  api_split.h launches it.
//   k_split_begin   one thread: gate = the error word is already set as the call starts
//   k_split_flags   per row: the key (error word: a negative key), the two draws -> flag 0 = not sampled, 1 = training, 2 = test
//                   (time mode: 1 = sampled); the sampled rows are counted per workgroup and added to one counter (integer atomic)
//   k_split_hist    time mode, pass p of 8: the sampled timestamps that match the digits picked so far, by their next 8 bits (most
//                   significant first, sign bit flipped): a 256-bin histogram in LDS, added to the pass's global bins (integer atomics)
//   k_split_pick    one workgroup: the bin that holds the remaining rank becomes the next digit; pass 0 first makes the rank from the
//                   count of sampled rows -- r = ceil(train * n_sampled), the call's only float arithmetic -- as max(r, 1) - 1
//   k_split_count   per tile of SPLIT_TILE rows: the training and the test rows, to cnt[tile] and cnt[n_tiles + tile]; the counts-only
//                   seg_scan over cnt[0 .. 2 n_tiles] then gives every tile its first place in either list
//   k_split_write   per tile: the rows' places by ballot and popcount within a wave and the waves' totals in LDS, in row order -- no
//                   atomic decides a place, so the lists are ascending on every run
//   k_split_words   one thread: n_sampled, n_train, n_test, split_timestamp
//   k_take_rows     dst[j] = src[index[j]] for up to SPLIT_MAX_COLS columns a launch (blockIdx.y = the column): a thread makes 16 bytes
//                   of the dense destination, stored as one 128-bit word where the destination is 16-byte aligned, and read as one where
//                   the rows are multiples of 16 bytes and aligned
// Every kernel returns at once when the error word is set (it is ~0 while there is no error).  k_split_flags, the one kernel that sets
// it, goes by the gate instead: a workgroup that starts after another has reported its row still reports its own, so the word names
// the FIRST negative key on every run.

static constexpr int SPLIT_TILE = 4 * FE_THREADS;          // rows of one tile: four rounds of a workgroup's 256
static constexpr int SPLIT_WAVES = FE_THREADS / 64;
static constexpr unsigned long long SPLIT_NO_ERROR = ~0ull;
static constexpr unsigned long long SPLIT_ERR_KEY = 1;     // the error word's kind (its high half); the low half is the row
static constexpr int SPLIT_KEY_POSITION = 0, SPLIT_KEY_I32 = 1, SPLIT_KEY_I64 = 2;
static constexpr int SPLIT_RANDOM = 0, SPLIT_TIME = 1;

// the 53-bit draw of (seed, key k, stream s): splitmix64's finalizer, all modulo 2^64
__device__ inline unsigned long long split_draw(unsigned long long seed, unsigned long long k, unsigned s) {
    unsigned long long x = seed + 0x9E3779B97F4A7C15ull * (2ull * k + s + 1ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x >> 11;
}

// a timestamp as an unsigned key of the same order
__device__ inline unsigned long long split_ts_key(long long ts) { return (unsigned long long)ts ^ 0x8000000000000000ull; }

// the side of row i: 0 = not sampled, 1 = training, 2 = test
__device__ inline unsigned split_side(const unsigned char* __restrict__ flags, const long long* __restrict__ ts, long long i, int mode, long long split_ts) {
    const unsigned f = flags[i];
    if (mode == SPLIT_TIME && f) return ts[i] <= split_ts ? 1u : 2u;
    return f;
}

__global__ void k_split_begin(const unsigned long long* __restrict__ err, unsigned* __restrict__ gate) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *gate = *err != SPLIT_NO_ERROR;
}

__global__ __launch_bounds__(FE_THREADS) void k_split_flags(const void* __restrict__ key, int key_kind, long long n, unsigned long long seed, unsigned long long t_sample,
                                                           unsigned long long t_train, int mode, unsigned char* __restrict__ flags,
                                                           unsigned long long* __restrict__ n_sampled, const unsigned* __restrict__ gate,
                                                           unsigned long long* __restrict__ err) {
    if (*gate) return;
    unsigned mine = 0;
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const long long k = key_kind == SPLIT_KEY_I32 ? (long long)((const int*)key)[i] : key_kind == SPLIT_KEY_I64 ? ((const long long*)key)[i] : i;
        unsigned f = 0;
        if (k < 0) atomicMin(err, SPLIT_ERR_KEY << 32 | (unsigned long long)i);
        else if (split_draw(seed, (unsigned long long)k, 0) < t_sample) {
            f = mode == SPLIT_TIME || split_draw(seed, (unsigned long long)k, 1) < t_train ? 1u : 2u;
            ++mine;
        }
        flags[i] = (unsigned char)f;
    }
    __shared__ unsigned total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(n_sampled, (unsigned long long)total);
}

// sel[0] = the digits picked so far (pass p: the top 8 p bits of the key, right-aligned), sel[1] = the rank among the keys that match them
__global__ __launch_bounds__(FE_THREADS) void k_split_hist(const unsigned char* __restrict__ flags, const long long* __restrict__ ts, long long n, int pass,
                                                          const unsigned long long* __restrict__ sel, unsigned* __restrict__ hist, const unsigned long long* __restrict__ err) {
    if (*err != SPLIT_NO_ERROR) return;
    __shared__ unsigned bins[256];
    bins[threadIdx.x] = 0;                                                  // (FE_THREADS == 256)
    __syncthreads();
    const unsigned long long prefix = sel[0];
    const int shift = 56 - 8 * pass, above = pass == 0 ? 63 : shift + 8;      // (pass 0 has no digits above it: every key matches)
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        if (!flags[i]) continue;
        const unsigned long long k = split_ts_key(ts[i]);
        if (pass == 0 || (k >> above) == prefix) atomicAdd(&bins[(unsigned)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned c = bins[threadIdx.x];
    if (c) atomicAdd(&hist[pass * 256 + threadIdx.x], c);
}

__global__ __launch_bounds__(FE_THREADS) void k_split_pick(int pass, double train, const unsigned long long* __restrict__ n_sampled, const unsigned* __restrict__ hist,
                                                          unsigned long long* __restrict__ sel, const unsigned long long* __restrict__ err) {
    if (*err != SPLIT_NO_ERROR) return;
    __shared__ unsigned sh[FE_THREADS];
    unsigned long long prefix = sel[0], rank = sel[1];
    if (pass == 0) {
        const double r = ceil(train * (double)*n_sampled);                  // one product, one ceil: 0 <= r <= n_sampled < 2^31
        const unsigned long long ru = (unsigned long long)r;
        prefix = 0;
        rank = (ru > 1 ? ru : 1) - 1;
    }
    const unsigned c = hist[pass * 256 + threadIdx.x];
    unsigned total;
    const unsigned e = fe_block_scan(c, sh, &total);
    if ((unsigned long long)e <= rank && rank < (unsigned long long)e + c) {   // one thread at most; none where no row is sampled
        sel[0] = prefix << 8 | (unsigned long long)threadIdx.x;
        sel[1] = rank - e;
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_split_count(const unsigned char* __restrict__ flags, const long long* __restrict__ ts, long long n, int n_tiles, int mode,
                                                           const unsigned long long* __restrict__ sel, unsigned* __restrict__ cnt, const unsigned long long* __restrict__ err) {
    if (*err != SPLIT_NO_ERROR) return;
    __shared__ unsigned both[2];
    const long long split_ts = (long long)split_ts_key((long long)sel[0]);
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (threadIdx.x < 2) both[threadIdx.x] = 0;
        __syncthreads();
        unsigned a = 0, b = 0;
        for (int k = 0; k < SPLIT_TILE / FE_THREADS; ++k) {
            const long long i = (long long)tile * SPLIT_TILE + k * FE_THREADS + threadIdx.x;
            const unsigned f = i < n ? split_side(flags, ts, i, mode, split_ts) : 0u;
            a += f == 1u; b += f == 2u;
        }
        if (a) atomicAdd(&both[0], a);
        if (b) atomicAdd(&both[1], b);
        __syncthreads();
        if (threadIdx.x == 0) { cnt[tile] = both[0]; cnt[n_tiles + tile] = both[1]; }
        __syncthreads();
    }
}

// off = cnt after the scan: off[tile] = the tile's first place among the training rows, off[n_tiles + tile] - off[n_tiles] among the test rows
__global__ __launch_bounds__(FE_THREADS) void k_split_write(const unsigned char* __restrict__ flags, const long long* __restrict__ ts, long long n, int n_tiles, int mode,
                                                           const unsigned long long* __restrict__ sel, const unsigned* __restrict__ off, int* __restrict__ index_train,
                                                           int* __restrict__ index_test, const unsigned long long* __restrict__ err) {
    if (*err != SPLIT_NO_ERROR) return;
    __shared__ unsigned waves[2][SPLIT_WAVES];
    const long long split_ts = (long long)split_ts_key((long long)sel[0]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned test0 = off[n_tiles];
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        unsigned at_train = off[tile], at_test = off[n_tiles + tile] - test0;
        for (int k = 0; k < SPLIT_TILE / FE_THREADS; ++k) {
            const long long i = (long long)tile * SPLIT_TILE + k * FE_THREADS + threadIdx.x;
            const unsigned f = i < n ? split_side(flags, ts, i, mode, split_ts) : 0u;
            const unsigned long long ma = __ballot(f == 1u), mb = __ballot(f == 2u);
            if (lane == 0) { waves[0][wave] = (unsigned)__popcll(ma); waves[1][wave] = (unsigned)__popcll(mb); }
            __syncthreads();
            unsigned before_a = 0, before_b = 0, all_a = 0, all_b = 0;
            for (int w = 0; w < SPLIT_WAVES; ++w) {
                const unsigned ca = waves[0][w], cb = waves[1][w];
                if (w < wave) { before_a += ca; before_b += cb; }
                all_a += ca; all_b += cb;
            }
            if (f == 1u) index_train[at_train + before_a + (unsigned)__popcll(ma & below)] = (int)i;      // < n_train: the scan's totals
            else if (f == 2u) index_test[at_test + before_b + (unsigned)__popcll(mb & below)] = (int)i;
            at_train += all_a; at_test += all_b;
            __syncthreads();
        }
    }
}

// words[0] is the error word; words[1 .. 4] = n_sampled, n_train, n_test, split_timestamp (0 in random mode and where no row is sampled)
__global__ void k_split_words(int n_tiles, int mode, const unsigned long long* __restrict__ n_sampled, const unsigned long long* __restrict__ sel,
                              const unsigned* __restrict__ off, long long* __restrict__ words) {
    if ((unsigned long long)words[0] != SPLIT_NO_ERROR || threadIdx.x || blockIdx.x) return;
    words[1] = (long long)*n_sampled;
    words[2] = (long long)off[n_tiles];
    words[3] = (long long)(off[2 * n_tiles] - off[n_tiles]);
    words[4] = mode == SPLIT_TIME && *n_sampled ? (long long)split_ts_key((long long)sel[0]) : 0ll;
}

static constexpr int SPLIT_MAX_COLS = 32;
struct SplitColSet { sprk_split_col col[SPLIT_MAX_COLS]; };

// Column blockIdx.y: the destination is n_index * row_bytes dense bytes, made in units of 16 (four words; the last unit may be short).
// An index outside [0, n_rows) leaves its destination row as it is.
__global__ __launch_bounds__(FE_THREADS) void k_take_rows(SplitColSet set, const int* __restrict__ index, long long n_index, long long n_rows) {
    const sprk_split_col c = set.col[blockIdx.y];
    const long long W = c.row_bytes / 4, words = n_index * W, units = (words + 3) / 4;
    const unsigned char* src = (const unsigned char*)c.src;
    unsigned* dst = (unsigned*)c.dst;
    const bool wide_dst = ((uintptr_t)c.dst & 15) == 0;
    const bool wide_src = (W & 3) == 0 && ((uintptr_t)c.src & 15) == 0 && (c.src_stride & 15) == 0;          // a unit lies within one row, 16-byte aligned
    for (long long u = (long long)blockIdx.x * FE_THREADS + threadIdx.x; u < units; u += (long long)gridDim.x * FE_THREADS) {
        const long long w0 = u * 4;
        long long j = W == 1 ? w0 : w0 / W, k = W == 1 ? 0 : w0 - j * W;
        const int count = words - w0 < 4 ? (int)(words - w0) : 4;
        unsigned v[4] = {0u, 0u, 0u, 0u};
        unsigned ok = 0;                                                    // bit e: word e comes from a row inside the source
        if (wide_src) {
            const long long r = index[j];
            if (r >= 0 && r < n_rows) {
                const uint4 q = *(const uint4*)(src + r * c.src_stride + k * 4);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                ok = 15u;
            }
        } else {
            for (int e = 0; e < count; ++e) {
                const long long r = index[j];
                if (r >= 0 && r < n_rows) { v[e] = *(const unsigned*)(src + r * c.src_stride + k * 4); ok |= 1u << e; }
                if (++k == W) { k = 0; ++j; }
            }
        }
        if (wide_dst && count == 4 && ok == 15u) *(uint4*)(dst + w0) = make_uint4(v[0], v[1], v[2], v[3]);
        else
            for (int e = 0; e < count; ++e)
                if (ok >> e & 1u) dst[w0 + e] = v[e];
    }
}
