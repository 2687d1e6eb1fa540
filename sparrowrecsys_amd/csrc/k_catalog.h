// k_catalog.h -- the reference's DataManager on the device: per-movie average rating as Java computes it (Movie.addRating, Movie.java:93-98),
// the rating-sorted and year-sorted lists of the whole catalogue and of every genre (getMovies / getMoviesByGenre, DataManager.java:253-283),
// candidate generation and the default similarity ranker (SimilarMovieProcess.java:39-83, :145-159).  The definition these kernels equal
// bit for bit is sparrowrecsys_amd/catalog.py catalog_host / similar_host; DESIGN.md section 5.9 has the rules.  Uses
// k_segments.h: the counts-only scan, the segment sort (behind the `ungrouped` word for the ratings, ungated for the lists) and
// fe_block_scan in k_cat_similar; and k_user_emb.h's UE_W_* control words.
//
// sprk_catalog_build, one stream, no host synchronisation (api_catalog.h launches them in this order):
//   k_cat_count       per rating: a non-finite rating raises the error word; a rating on a movie the table holds is counted, and a
//                     movie's second run of rows in the input raises `ungrouped` (as k_ue_count does for users)
//   k_fe_scan_*<false>  exclusive scan over movies of the counts: segment offsets
//   -- only when `ungrouped` is raised --
//   k_cat_scatter     per rating: (input row, rating) into its movie's segment at an atomic cursor, any order
//   k_fe_sort_short (gate = the word), k_fe_sort_long_chunks + k_fe_merge_pass (+ k_fe_long_copy): every segment by input row
//   -- always --
//   k_cat_avg_short   one lane per movie of fewer than CAT_WAVE_MIN ratings: the recurrence, ratings loaded a chunk ahead
//   k_cat_avg_wave    one wave per longer movie: 64 ratings per coalesced load, a chunk ahead; every lane runs the one chain on values
//                     read from the lanes' registers (v_readlane), so no load and no LDS access sits on the chain
//   k_cat_list_count, k_cat_list_scan: the sizes and offsets of the 2 (G + 1) lists
//   k_cat_list_scatter: per (list, member) the 64-bit key (average or year, inverted for descending) and the tie position
//   k_fe_sort_short, k_fe_sort_long_chunks + k_fe_merge_pass: the lists as 2 (G + 1) segments; (key, tie position) is a total order
//   k_cat_list_write  tie position -> movie id
// sprk_catalog_similar: k_cat_similar, one workgroup per query.
// Integer atomics only count; nothing depends on the order of arrival.

static constexpr int CAT_THREADS = 256;
static_assert(CAT_THREADS == FE_THREADS, "k_cat_similar calls fe_block_scan; api_catalog.h sizes the grids of CAT_THREADS kernels with fe_grid_capped");
static constexpr int CAT_WAVE_MIN = 128;           // a movie of this many ratings or more gets a wave of its own
static constexpr int CAT_CHUNK = 8;                // ratings per lane and pipeline stage of k_cat_avg_short
static constexpr int CAT_MAX_CAND = 4096;          // gathered list entries of one query: 12 bytes x 4096 of LDS at the most
static constexpr int CAT_MAX_GENRES = 32;
static constexpr int CAT_MAX_SEGS = CAT_MAX_GENRES + 2;
static constexpr unsigned long long CAT_ERR_RATING = 3, CAT_ERR_LISTS = 4;

// k_emb_rank.h's er_key: Double.compare order as an unsigned key (0.0 above -0.0, every NaN one greatest value), and its inverse
// (every NaN comes back as Java's Double.NaN)
__device__ inline unsigned long long cat_key(double s) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(s);
    if (s != s) return ~0ull;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double cat_unkey(unsigned long long k) {
    if (k == ~0ull) return __longlong_as_double(0x7ff8000000000000ll);
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ inline bool cat_finite(float r) { return ((unsigned)__float_as_int(r) & 0x7f800000u) != 0x7f800000u; }

// Movie.addRating: avg = (avg * n + score) / (n + 1), one double multiply, one add, one IEEE division, never fused or reassociated.
// (__dmul_rn / __dadd_rn are plain operators in this toolchain and a product feeding a sum would contract into an fma -- k_emb_rank.h's
// products are float32 and converted, which nothing fuses --: contraction is switched off for these two functions instead.)
__device__ inline double cat_step(double avg, unsigned n, float score) {
#pragma clang fp contract(off)
    const double product = avg * (double)n;
    const double sum = product + (double)score;
    return sum / (double)(n + 1u);
}

// calculateSimilarScore: every operation rounded on its own; 0 / 0 = NaN
__device__ inline double cat_score(int same, int n_genres_q, int n_genres_c, double avg_c) {
#pragma clang fp contract(off)
    const double gs = ((double)same / (double)(n_genres_q + n_genres_c)) / 2.0;
    const double rs = avg_c / 5.0;
    const double a = gs * 0.7, b = rs * 0.3;
    return a + b;
}

__global__ __launch_bounds__(CAT_THREADS) void k_cat_count(long long n, const int* __restrict__ movie, const float* __restrict__ rating, int n_movies,
                                                           const unsigned char* __restrict__ has, unsigned* __restrict__ len, unsigned* __restrict__ runs,
                                                           unsigned* __restrict__ first, unsigned* __restrict__ words, unsigned long long* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * CAT_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CAT_THREADS) {
        if (!cat_finite(rating[i])) { atomicMin(err, CAT_ERR_RATING << 32 | (unsigned long long)i); continue; }   // (the row takes no further part)
        const int m = movie[i];
        if (m < 0 || m >= n_movies || !has[m]) continue;                       // movieMap.get == null: skipped, no error
        atomicAdd(&len[m], 1u);
        if (i == 0 || movie[i - 1] != m) {
            first[m] = (unsigned)i;                                            // (read only when every movie has one run: one writer)
            if (atomicAdd(&runs[m], 1u)) words[UE_W_UNGROUPED] = 1u;
        }
    }
}

__global__ __launch_bounds__(CAT_THREADS) void k_cat_scatter(long long n, const int* __restrict__ movie, const float* __restrict__ rating, int n_movies,
                                                             const unsigned char* __restrict__ has, const unsigned* __restrict__ seg_off, unsigned* __restrict__ cursor,
                                                             long long* __restrict__ seg_key, int* __restrict__ seg_rating, const unsigned* __restrict__ words) {
    if (!words[UE_W_UNGROUPED]) return;
    for (long long i = (long long)blockIdx.x * CAT_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CAT_THREADS) {
        const float r = rating[i];
        const int m = movie[i];
        if (!cat_finite(r) || m < 0 || m >= n_movies || !has[m]) continue;     // k_cat_count's predicate
        const size_t pos = (size_t)seg_off[m] + atomicAdd(&cursor[m], 1u);     // < seg_off[m + 1]: the same rows were counted
        seg_key[pos] = i;
        seg_rating[pos] = __float_as_int(r);
    }
}

// a movie's ratings in input order: a segment of seg_rating, or, when the input is grouped by movie, the input column itself
__device__ inline const float* cat_ratings_of(bool ungrouped, const int* __restrict__ seg_rating, const float* __restrict__ rating, const unsigned* __restrict__ first,
                                              long long m, unsigned lo, unsigned len) {
    return ungrouped ? (const float*)seg_rating + lo : rating + (len ? first[m] : 0u);
}

// v[k] = src[at + k], clamped to the last rating (len > 0): no branch around a load
__device__ inline void cat_load_chunk(const float* __restrict__ src, unsigned at, unsigned len, float (&v)[CAT_CHUNK]) {
#pragma unroll
    for (int k = 0; k < CAT_CHUNK; ++k) v[k] = src[at + k < len ? at + k : len - 1];
}

// One lane per movie; every movie's count is written here.  The chunk after this one is in flight while this one's steps run.
__global__ __launch_bounds__(CAT_THREADS) void k_cat_avg_short(int n_movies, const unsigned* __restrict__ seg_off, const unsigned* __restrict__ first,
                                                               const int* __restrict__ seg_rating, const float* __restrict__ rating, const unsigned* __restrict__ words,
                                                               double* __restrict__ avg, int* __restrict__ count) {
    const bool ungrouped = words[UE_W_UNGROUPED] != 0;
    for (long long m = (long long)blockIdx.x * CAT_THREADS + threadIdx.x; m < n_movies; m += (long long)gridDim.x * CAT_THREADS) {
        const unsigned lo = seg_off[m], len = seg_off[m + 1] - lo;
        count[m] = (int)len;
        if (len >= (unsigned)CAT_WAVE_MIN) continue;                           // k_cat_avg_wave's
        double a = 0.0;
        if (len) {
            const float* __restrict__ src = cat_ratings_of(ungrouped, seg_rating, rating, first, m, lo, len);
            float cur[CAT_CHUNK], nxt[CAT_CHUNK] = {};
            cat_load_chunk(src, 0u, len, cur);
            for (unsigned k = 0; k < len; k += CAT_CHUNK) {
                if (k + CAT_CHUNK < len) cat_load_chunk(src, k + CAT_CHUNK, len, nxt);
#pragma unroll
                for (int j = 0; j < CAT_CHUNK; ++j)
                    if (k + j < len) a = cat_step(a, k + j, cur[j]);
#pragma unroll
                for (int j = 0; j < CAT_CHUNK; ++j) cur[j] = nxt[j];
            }
        }
        avg[m] = a;
    }
}

// One wave per movie of CAT_WAVE_MIN ratings or more.  Lane l holds rating base + l of the current 64 and loads that of the next 64
// before the steps start; step j takes its rating from lane j's register, a wave-uniform value, so all 64 lanes carry the same chain.
__global__ __launch_bounds__(CAT_THREADS) void k_cat_avg_wave(int n_movies, const unsigned* __restrict__ seg_off, const unsigned* __restrict__ first,
                                                              const int* __restrict__ seg_rating, const float* __restrict__ rating, const unsigned* __restrict__ words,
                                                              double* __restrict__ avg) {
    const bool ungrouped = words[UE_W_UNGROUPED] != 0;
    const unsigned lane = threadIdx.x & 63u;
    const long long wave = (long long)blockIdx.x * (CAT_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long n_waves = (long long)gridDim.x * (CAT_THREADS / 64);
    for (long long m = wave; m < n_movies; m += n_waves) {
        const unsigned lo = seg_off[m], len = seg_off[m + 1] - lo;
        if (len < (unsigned)CAT_WAVE_MIN) continue;                            // (the whole wave)
        const float* __restrict__ src = cat_ratings_of(ungrouped, seg_rating, rating, first, m, lo, len);
        double a = 0.0;
        float cur = src[lane];                                                 // len >= 128 > lane
        for (unsigned base = 0; base < len; base += 64u) {
            float nxt = 0.0f;
            if (base + 64u < len) nxt = src[base + 64u + lane < len ? base + 64u + lane : len - 1u];
            const unsigned left = len - base;
            if (left >= 64u) {
#pragma unroll
                for (int j = 0; j < 64; ++j) a = cat_step(a, base + (unsigned)j, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur), j)));
            } else {
                for (unsigned j = 0; j < left; ++j) a = cat_step(a, base + j, __shfl(cur, (int)j));
            }
            cur = nxt;
        }
        if (lane == 0) avg[m] = a;
    }
}

// The 2 (G + 1) lists: list g < G = genre g by rating, list G = the whole catalogue by rating, list G + 1 + g = genre g by year, list
// 2 G + 1 = the whole catalogue by year.  cnt[g] = the members of genre g, cnt[G] = the movies held.
__global__ __launch_bounds__(CAT_THREADS) void k_cat_list_count(int n_movies, const unsigned* __restrict__ mask, const unsigned char* __restrict__ has, int G, unsigned* __restrict__ cnt) {
    __shared__ unsigned s_cnt[CAT_MAX_GENRES + 1];
    if (threadIdx.x <= CAT_MAX_GENRES) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned gmask = G >= 32 ? ~0u : (1u << G) - 1u;
    for (long long m = (long long)blockIdx.x * CAT_THREADS + threadIdx.x; m < n_movies; m += (long long)gridDim.x * CAT_THREADS) {
        if (!has[m]) continue;
        atomicAdd(&s_cnt[G], 1u);
        for (unsigned bits = mask[m] & gmask; bits; bits &= bits - 1u) atomicAdd(&s_cnt[__ffs((int)bits) - 1], 1u);
    }
    __syncthreads();
    if ((int)threadIdx.x <= G && s_cnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
}

// one thread: the offsets, as the sort's segment table and as the output.  Lists that would not fit `capacity` raise the error word and
// every list is left empty, so nothing below leaves its array.
__global__ void k_cat_list_scan(int G, const unsigned* __restrict__ cnt, long long capacity, unsigned* __restrict__ seg_off, int* __restrict__ list_offsets,
                                unsigned long long* __restrict__ err) {
    if (blockIdx.x || threadIdx.x) return;
    const int L = 2 * (G + 1);
    unsigned long long total = 0;
    for (int l = 0; l < L; ++l) total += cnt[l % (G + 1)];
    const bool fits = total <= (unsigned long long)capacity;
    if (!fits) atomicMin(err, CAT_ERR_LISTS << 32);
    unsigned o = 0;
    for (int l = 0; l <= L; ++l) {
        seg_off[l] = o;
        list_offsets[l] = (int)o;
        if (fits && l < L) o += cnt[l % (G + 1)];
    }
}

__device__ inline void cat_list_put(int l, unsigned slot, long long key, int tie, const unsigned* __restrict__ seg_off, long long* __restrict__ lkey, int* __restrict__ lrow) {
    const size_t pos = (size_t)seg_off[l] + slot;
    if (pos < (size_t)seg_off[l + 1]) { lkey[pos] = key; lrow[pos] = tie; }   // (always, for a table whose positions are what they claim to be)
}

// Per movie held: its pair in the two whole-catalogue lists, at the slot its hash position names (a permutation of the movies held: no
// counter), and in the two lists of each of its genres, at an atomic cursor.  Ascending (key, tie position) is the list's order: the key
// is the inverted Double.compare key of the average, or minus the year.  inv_file / inv_hash: tie position -> movie.
__global__ __launch_bounds__(CAT_THREADS) void k_cat_list_scatter(int n_movies, const unsigned* __restrict__ mask, const unsigned char* __restrict__ has, const int* __restrict__ year,
                                                                  const int* __restrict__ file_pos, const int* __restrict__ hash_pos, const double* __restrict__ avg, int G,
                                                                  const unsigned* __restrict__ seg_off, unsigned* __restrict__ cursor, long long* __restrict__ lkey,
                                                                  int* __restrict__ lrow, int* __restrict__ inv_file, int* __restrict__ inv_hash) {
    const unsigned gmask = G >= 32 ? ~0u : (1u << G) - 1u;
    for (long long m = (long long)blockIdx.x * CAT_THREADS + threadIdx.x; m < n_movies; m += (long long)gridDim.x * CAT_THREADS) {
        if (!has[m]) continue;
        const int fp = file_pos[m], hp = hash_pos[m];
        if ((unsigned)fp < (unsigned)n_movies) inv_file[fp] = (int)m;
        if ((unsigned)hp < (unsigned)n_movies) inv_hash[hp] = (int)m;
        const long long ka = (long long)(~cat_key(avg[m]) ^ 0x8000000000000000ull), ky = -(long long)year[m];
        if (hp >= 0) {
            cat_list_put(G, (unsigned)hp, ka, hp, seg_off, lkey, lrow);
            cat_list_put(2 * G + 1, (unsigned)hp, ky, hp, seg_off, lkey, lrow);
        }
        for (unsigned bits = mask[m] & gmask; bits; bits &= bits - 1u) {
            const int g = __ffs((int)bits) - 1;
            cat_list_put(g, atomicAdd(&cursor[g], 1u), ka, fp, seg_off, lkey, lrow);
            cat_list_put(G + 1 + g, atomicAdd(&cursor[G + 1 + g], 1u), ky, fp, seg_off, lkey, lrow);
        }
    }
}

// blockIdx.y = the list; the entries of list_movies past the last list are written too (-1)
__global__ __launch_bounds__(CAT_THREADS) void k_cat_list_write(int G, int n_movies, const unsigned* __restrict__ seg_off, const int* __restrict__ lrow, const int* __restrict__ inv_file,
                                                                const int* __restrict__ inv_hash, int* __restrict__ list_movies, long long capacity) {
    const int l = blockIdx.y, L = 2 * (G + 1);
    const int* __restrict__ inv = (l % (G + 1) == G) ? inv_hash : inv_file;
    const long long lo = seg_off[l], hi = seg_off[l + 1];
    for (long long p = lo + (long long)blockIdx.x * CAT_THREADS + threadIdx.x; p < hi; p += (long long)gridDim.x * CAT_THREADS) {
        const int r = lrow[p];
        list_movies[p] = (unsigned)r < (unsigned)n_movies ? inv[r] : -1;
    }
    if (l == 0)
        for (long long p = (long long)seg_off[L] + (long long)blockIdx.x * CAT_THREADS + threadIdx.x; p < capacity; p += (long long)gridDim.x * CAT_THREADS) list_movies[p] = -1;
}

// ---- candidates and the default ranker: one workgroup per query ----
// Dynamic LDS: key [B] 64-bit, id [B] int (B = the power of two that holds the most entries a query can gather), then the scan's
// FE_THREADS words, the gathered segments' sources [CAT_MAX_SEGS] (64-bit) and starts [CAT_MAX_SEGS + 1], and two words.
__host__ __device__ inline size_t cat_similar_lds(int B) { return (size_t)B * 12 + FE_THREADS * 4 + CAT_MAX_SEGS * 8 + (CAT_MAX_SEGS + 1 + 3) * 4; }

// bitonic sort of id[0 .. P) ascending
__device__ inline void cat_sort_ids(int* id, int P) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += CAT_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const int a = id[i], b = id[x];
                    if ((b < a) == ((i & k) == 0)) { id[i] = b; id[x] = a; }
                }
            }
            __syncthreads();
        }
}

// mode 0 = candidateGenerator: the heads (top_n) of the rating lists of the query's genres; mode 1 = multipleRetrievalCandidates: those,
// and the heads (extra_n) of the whole catalogue's rating and year lists.  The union without the query, ascending by movie id.
// kind 0: the ids, padded with -1 up to out_stride, and their count (ids past out_stride are not written: the count tells).
// kind 1: calculateSimilarScore per candidate, sorted by (score descending in Double.compare order, id ascending); the first `size` ids
// and scores (padded with -1 / 0.0 up to `size`) and min(size, candidates).
__global__ __launch_bounds__(CAT_THREADS) void k_cat_similar(const int* __restrict__ query, int n_movies, const unsigned* __restrict__ mask, const unsigned char* __restrict__ has,
                                                             const unsigned char* __restrict__ n_genres, const double* __restrict__ avg, int G,
                                                             const int* __restrict__ list_offsets, const int* __restrict__ list_movies, long long list_entries,
                                                             int mode, int top_n, int extra_n, int kind, int size, int B,
                                                             int* __restrict__ out_ids, double* __restrict__ out_scores, int out_stride, int* __restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cat_lds[];
    unsigned long long* key = (unsigned long long*)cat_lds;
    int* id = (int*)(cat_lds + (size_t)B * 8);
    unsigned* sh = (unsigned*)(cat_lds + (size_t)B * 12);
    long long* seg_src = (long long*)(sh + FE_THREADS);
    int* seg_start = (int*)(seg_src + CAT_MAX_SEGS);
    int* hdr = seg_start + CAT_MAX_SEGS + 1;                                   // [0] = segments
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int q = query[b];
    int* oi = out_ids + b * (size_t)out_stride;
    double* os = kind ? out_scores + b * (size_t)out_stride : nullptr;
    const int W = kind ? size : out_stride;
    const bool held = q >= 0 && q < n_movies && has[q] != 0;
    if (!held) {                                                               // (the whole workgroup) getMovieById == null: no candidates
        for (int i = tid; i < W; i += CAT_THREADS) { oi[i] = -1; if (os) os[i] = 0.0; }
        if (tid == 0) out_count[b] = 0;
        return;
    }
    const unsigned gmask = G >= 32 ? ~0u : (1u << G) - 1u;
    const unsigned mq = mask[q] & gmask;
    if (tid == 0) {
        int n_seg = 0, total = 0;
        auto add = [&](int l, int head) {
            long long lo = list_offsets[l], hi = list_offsets[l + 1];
            lo = lo < 0 ? 0 : lo > list_entries ? list_entries : lo;
            hi = hi < lo ? lo : hi > list_entries ? list_entries : hi;
            long long c = hi - lo < head ? hi - lo : head;
            if (c > B - total) c = B - total;                                  // (never, for the B the host derives from G, top_n and extra_n)
            seg_src[n_seg] = lo;
            seg_start[n_seg++] = total;
            total += (int)c;
        };
        for (unsigned bits = mq; bits; bits &= bits - 1u) add(__ffs((int)bits) - 1, top_n);
        if (mode == 1) { add(G, extra_n); add(2 * G + 1, extra_n); }
        seg_start[n_seg] = total;
        hdr[0] = n_seg;
    }
    __syncthreads();
    const int n_seg = hdr[0], total = seg_start[n_seg];
    int P = 2;
    while (P < total) P <<= 1;
    for (int i = tid; i < P; i += CAT_THREADS) {
        int v = 0x7fffffff;
        if (i < total) {
            int s = 0;
            while (seg_start[s + 1] <= i) ++s;                                 // (empty segments are passed over)
            const int c = list_movies[seg_src[s] + (i - seg_start[s])];
            if ((unsigned)c < (unsigned)n_movies && c != q) v = c;             // candidateMap.remove(movie.getMovieId())
        }
        id[i] = v;
    }
    __syncthreads();
    cat_sort_ids(id, P);
    // duplicates out, survivors to the front, in place: a thread reads its stretch (and the element before it) into registers, the
    // scan's first barrier separates all reads from all writes
    const int E = P >= CAT_THREADS ? P / CAT_THREADS : 1;
    int v[CAT_MAX_CAND / CAT_THREADS];
    unsigned keep = 0, n_keep = 0;
#pragma unroll
    for (int e = 0; e < CAT_MAX_CAND / CAT_THREADS; ++e) {
        const int i = tid * E + e;
        v[e] = 0x7fffffff;
        if (e < E && i < P) {
            v[e] = id[i];
            const int prev = i ? id[i - 1] : -1;
            if (v[e] != 0x7fffffff && v[e] != prev) { keep |= 1u << e; ++n_keep; }
        }
    }
    unsigned n_cand;
    unsigned at = fe_block_scan(n_keep, sh, &n_cand);
#pragma unroll
    for (int e = 0; e < CAT_MAX_CAND / CAT_THREADS; ++e)
        if (keep >> e & 1u) id[at++] = v[e];
    __syncthreads();
    const int C = (int)n_cand;
    if (kind == 0) {
        for (int i = tid; i < W; i += CAT_THREADS) oi[i] = i < C ? id[i] : -1;
        if (tid == 0) out_count[b] = C;
        return;
    }
    int P2 = 2;
    while (P2 < C) P2 <<= 1;
    const int ngq = (int)n_genres[q];
    for (int i = tid; i < P2; i += CAT_THREADS) {
        if (i < C) {
            const int c = id[i];
            key[i] = cat_key(cat_score(__popc(mask[q] & mask[c]), ngq, (int)n_genres[c], avg[c]));         // NaN: the greatest key
        } else {
            key[i] = 0ull;                                                     // padding: below every real key (0 is no key), after every id
            id[i] = 0x7fffffff;
        }
    }
    __syncthreads();
    // k_emb_rank's network: "before" = (key greater) or (key equal and id smaller); ids ascend with the candidate position
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P2; i += CAT_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long ki = key[i], kl = key[l];
                    const int pi = id[i], pl = id[l];
                    const bool i_first = ki > kl || (ki == kl && pi < pl);
                    const bool up = (i & k) == 0;
                    if (up ? !i_first : i_first) { key[i] = kl; key[l] = ki; id[i] = pl; id[l] = pi; }
                }
            }
            __syncthreads();
        }
    const int n_out = size < C ? size : C;
    for (int i = tid; i < W; i += CAT_THREADS) {
        oi[i] = i < n_out ? id[i] : -1;
        os[i] = i < n_out ? cat_unkey(key[i]) : 0.0;
    }
    if (tid == 0) out_count[b] = n_out;
}
