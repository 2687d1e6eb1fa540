// k_item2vec.h -- item2vec on the device (the reference's offline/spark/embedding/Embedding.scala: processItemSequence, then Spark
// Word2Vec = skip-gram with hierarchical softmax): rating sequences from ratings, and the trainer.  The definitions these kernels equal
// bit for bit are sparrowrecsys_amd/item2vec.py sequences_host and skipgram_host; DESIGN.md section 5.11 has the rules.  Uses
// k_segments.h: the counts-only scan and the (ungated) segment sort; k_als.h: the row predicate.
//
// sprk_item_sequences, one stream, no host synchronisation (api_item2vec.h launches them in this order):
//   k_i2v_seq_count    per rating: validate (error word); a row with rating >= 3.5f counts for its user and its item
//   k_fe_scan_*<false> exclusive scan over users: the sequences' offsets
//   k_i2v_seq_scatter  per kept rating: (timestamp, input row) into its user's segment at an atomic cursor, any order
//   k_fe_sort_*        every segment by (timestamp, input row)
//   k_i2v_seq_emit     the offsets and the items in their order
// sprk_skipgram_fit:
//   k_i2v_mark         per sequence item: 1 if it is in the vocabulary
//   k_fe_scan_*<false> its exclusive scan: the global position of every kept item; the total must be the caller's n_words
//   k_i2v_corpus       per kept item: its word, the bounds of its sentence; counts the records of its word's row and its path's rows
//   k_fe_scan_*<false> over the 2 V rows (syn0's, then syn1's): the occurrence lists' offsets
//   k_i2v_records      per kept item: one record (centre << 32 | context) per centre that can reach it, into its word's list;
//                      one record (centre << 32 | depth) into the list of every node of its path
//   k_fe_sort_*        every list by its key: ascending (centre, context or depth), once -- the corpus does not change
//   k_i2v_init         init -> vectors, zeros -> syn1
//   -- per iteration, per round of R positions --
//   k_i2v_positions    one position per lane group: its emissions into the round's buffers E0 (per context) and E1 (per depth)
//   k_i2v_apply        one row per lane group: its records of this round, a contiguous run of its list (two binary searches), added in
//                      order; only the window mask varies per iteration, recomputed from the counter
//   -- at the end --
//   k_i2v_loss_pos, k_i2v_loss_chunks, k_i2v_loss_final
// No float atomics, no transcendental: every output is a function of the input alone.

static constexpr int I2V_THREADS = 128;            // k_i2v_positions / k_i2v_loss_pos: 40 KB of LDS a workgroup
static constexpr int I2V_MAX_CODE = 40;
static constexpr int I2V_MAX_D = 64;
static constexpr int I2V_MAX_WINDOW = 16;
static constexpr int I2V_TABLE = 1000;
static constexpr int I2V_LOSS_CHUNK = 1024;
static constexpr int I2V_APPLY_CHUNK = 16;         // records of a row k_i2v_apply has in flight
static constexpr unsigned long long I2V_ERR_MOVIE = 2, I2V_ERR_CORPUS = 4;

__global__ __launch_bounds__(FE_THREADS) void k_i2v_seq_count(long long n, const int* __restrict__ user, const int* __restrict__ movie, const float* __restrict__ rating,
                                                              int n_users, int n_items, unsigned* __restrict__ len_user, int* __restrict__ item_count,
                                                              unsigned long long* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const int u = user[i], m = movie[i];
        const float r = rating[i];
        const unsigned long long kind = als_row_kind(u, m, r, n_users, n_items);
        if (kind) { atomicMin(err, kind << 32 | (unsigned long long)i); continue; }
        if (r >= 3.5f) {
            atomicAdd(&len_user[u], 1u);
            atomicAdd(&item_count[m], 1);
        }
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_i2v_seq_scatter(long long n, const int* __restrict__ user, const int* __restrict__ movie, const float* __restrict__ rating,
                                                                const long long* __restrict__ timestamp, int n_users, int n_items, const unsigned* __restrict__ off,
                                                                unsigned* __restrict__ cursor, long long* __restrict__ key, int* __restrict__ val) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const int u = user[i];
        const float r = rating[i];
        if (als_row_kind(u, movie[i], r, n_users, n_items) || !(r >= 3.5f)) continue;      // k_i2v_seq_count's predicate
        const size_t p = (size_t)off[u] + atomicAdd(&cursor[u], 1u);                       // < off[u + 1]: the same rows were counted
        key[p] = timestamp[i];
        val[p] = (int)i;
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_i2v_seq_emit(long long n, int n_users, const unsigned* __restrict__ off, const int* __restrict__ val,
                                                             const int* __restrict__ movie, int* __restrict__ seq_offsets, int* __restrict__ seq_items) {
    const long long kept = off[n_users];                                                   // <= n
    const long long rows = n > (long long)n_users + 1 ? n : (long long)n_users + 1;
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < rows; i += (long long)gridDim.x * FE_THREADS) {
        if (i <= n_users) seq_offsets[i] = (int)off[i];
        if (i < kept && i < n) seq_items[i] = movie[val[i]];
    }
}

// ---- the trainer

__device__ inline unsigned long long i2v_mix(unsigned long long x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// the window shrink of position k in iteration it: item2vec.py shrink
__device__ inline int i2v_shrink(unsigned long long seed, int it, long long k, int window) {
    const unsigned long long s = seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)it + 1ull);
    return (int)((i2v_mix(i2v_mix(s) ^ (unsigned long long)k) >> 33) % (unsigned long long)window);
}
// the tables are the caller's: whatever they hold, an index made from them stays inside [0, 40] x [0, V)
__device__ inline int i2v_len(const int* __restrict__ code_len, int w) {
    const int L = code_len[w];
    return L < 0 ? 0 : L > I2V_MAX_CODE ? I2V_MAX_CODE : L;
}
__device__ inline int i2v_point(const int* __restrict__ points, int w, int d, int V) {
    const int p = points[(size_t)w * I2V_MAX_CODE + d];
    return p < 0 ? 0 : p >= V ? V - 1 : p;
}

__global__ __launch_bounds__(FE_THREADS) void k_i2v_mark(long long n, const int* __restrict__ seq_items, const int* __restrict__ lut, int n_items, unsigned* __restrict__ a,
                                                         unsigned long long* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const int m = seq_items[i];
        int v = -1;
        if (m < 0 || m >= n_items) atomicMin(err, I2V_ERR_MOVIE << 32 | (unsigned long long)i);
        else v = lut[m];
        a[i] = v >= 0 ? 1u : 0u;
    }
}

// the word and the sentence of kept item i, at position p = a[i]; false when the item is not kept.  Offsets that are not a partition
// of [0, n) give a sentence of the one word: every index derived from lo / hi stays inside [0, N).
__device__ inline bool i2v_place(long long i, long long n, int n_seq, const int* __restrict__ seq_off, const unsigned* __restrict__ a, int max_sentence,
                                 long long& p, long long& lo, long long& hi) {
    if (a[i + 1] == a[i]) return false;
    p = a[i];
    int s_lo = 0, s_hi = n_seq - 1;                                                        // the last sequence whose offset is <= i
    while (s_lo < s_hi) {
        const int mid = (s_lo + s_hi + 1) >> 1;
        if ((long long)seq_off[mid] <= i) s_lo = mid; else s_hi = mid - 1;
    }
    long long b = seq_off[s_lo], e = seq_off[s_lo + 1];
    b = b < 0 ? 0 : b > n ? n : b;
    e = e < 0 ? 0 : e > n ? n : e;
    long long fs = a[b], fe = a[e];
    if (!(fs <= p && p < fe)) { fs = p; fe = p + 1; }
    lo = fs + (p - fs) / max_sentence * max_sentence;
    hi = lo + max_sentence < fe ? lo + max_sentence : fe;
    return true;
}

__global__ __launch_bounds__(FE_THREADS) void k_i2v_corpus(long long n, int n_seq, const int* __restrict__ seq_off, const int* __restrict__ seq_items, const int* __restrict__ lut,
                                                           const unsigned* __restrict__ a, long long N, int max_sentence, int window, int V,
                                                           const int* __restrict__ code_len, const int* __restrict__ points, int* __restrict__ pos_word,
                                                           unsigned* __restrict__ pos_lo, unsigned* __restrict__ pos_hi, unsigned* __restrict__ cnt,
                                                           unsigned long long* __restrict__ err) {
    if ((long long)a[n] != N) {                                                            // (the whole grid: nothing below runs)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicMin(err, I2V_ERR_CORPUS << 32 | (unsigned long long)a[n]);
        return;
    }
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        long long p, lo, hi;
        if (!i2v_place(i, n, n_seq, seq_off, a, max_sentence, p, lo, hi)) continue;
        const int w = lut[seq_items[i]];                                                   // in [0, V): the item was marked
        const int wc = w < 0 ? 0 : w >= V ? V - 1 : w;
        pos_word[p] = wc;
        pos_lo[p] = (unsigned)lo;
        pos_hi[p] = (unsigned)hi;
        if (hi - lo < 2) continue;
        const long long c0 = lo > p - window ? lo : p - window, c1 = hi - 1 < p + window ? hi - 1 : p + window;
        atomicAdd(&cnt[wc], (unsigned)(c1 - c0));                                          // the centres that can reach p: [c0, c1] without p
        const int L = i2v_len(code_len, wc);
        for (int d = 0; d < L; ++d) atomicAdd(&cnt[V + i2v_point(points, wc, d, V)], 1u);
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_i2v_records(long long n, int n_seq, const int* __restrict__ seq_off, const int* __restrict__ seq_items, const int* __restrict__ lut,
                                                            const unsigned* __restrict__ a, long long N, int max_sentence, int window, int V,
                                                            const int* __restrict__ code_len, const int* __restrict__ points, const unsigned* __restrict__ off,
                                                            unsigned* __restrict__ cursor, long long* __restrict__ key, int* __restrict__ val) {
    if ((long long)a[n] != N) return;
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        long long p, lo, hi;
        if (!i2v_place(i, n, n_seq, seq_off, a, max_sentence, p, lo, hi)) continue;
        if (hi - lo < 2) continue;
        const int w = lut[seq_items[i]];
        const int wc = w < 0 ? 0 : w >= V ? V - 1 : w;
        const long long c0 = lo > p - window ? lo : p - window, c1 = hi - 1 < p + window ? hi - 1 : p + window;
        for (long long k = c0; k <= c1; ++k) {
            if (k == p) continue;
            const size_t at = (size_t)off[wc] + atomicAdd(&cursor[wc], 1u);                // < off[wc + 1]: k_i2v_corpus counted the same
            key[at] = k << 32 | p;
            val[at] = 0;
        }
        const int L = i2v_len(code_len, wc);
        for (int d = 0; d < L; ++d) {
            const int row = V + i2v_point(points, wc, d, V);
            const size_t at = (size_t)off[row] + atomicAdd(&cursor[row], 1u);
            key[at] = p << 32 | (long long)d;
            val[at] = 0;
        }
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_i2v_init(int V, int D, const float* __restrict__ init, int init_stride, float* __restrict__ vectors, int stride,
                                                         float* __restrict__ syn1) {
    const long long cells = (long long)V * D;
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < cells; i += (long long)gridDim.x * FE_THREADS) {
        const long long r = i / D;
        const int d = (int)(i % D);
        vectors[(size_t)r * stride + d] = init[(size_t)r * init_stride + d];
        syn1[i] = 0.0f;
    }
}

// the float32 dot in index order from 0.0f: lane i of the group holds product i; every lane of the group gets the sum
template <int G>
__device__ inline float i2v_dot(float p, int D) {
#pragma clang fp contract(off)
    float f = 0.0f;
    for (int i = 0; i < D; ++i) f = f + __shfl(p, i, G);
    return f;
}

// One position per group of G lanes, lane = dimension (G = 16 for D <= 16, else 64).  The centre's path rows of syn1 and the increments
// inc1 they collect stay in LDS, a lane's own words (no lane reads another's: the only traffic between lanes is the dot).
template <int G>
__global__ __launch_bounds__(I2V_THREADS) void k_i2v_positions(long long r0, long long r1, long long N, const unsigned* __restrict__ total, const int* __restrict__ pos_word,
                                                               const unsigned* __restrict__ pos_lo, const unsigned* __restrict__ pos_hi,
                                                               const int* __restrict__ code_len, const unsigned char* __restrict__ codes, const int* __restrict__ points,
                                                               int V, const float* __restrict__ syn0, int stride, const float* __restrict__ syn1, int D, int window,
                                                               int it, unsigned long long seed, float alpha, const float* __restrict__ exp_table,
                                                               float* __restrict__ E0, float* __restrict__ E1) {
#pragma clang fp contract(off)
    __shared__ float path[I2V_THREADS / G][2][I2V_MAX_CODE][G];
    if ((long long)*total != N) return;
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const long long k = r0 + (long long)blockIdx.x * (I2V_THREADS / G) + grp;
    if (k >= r1) return;                                                                    // (the whole group)
    const long long lo = pos_lo[k], hi = pos_hi[k];
    if (hi - lo < 2) return;                                                                // no context: emits nothing
    const bool live = gl < D;
    const int dim = live ? gl : 0;
    const int w = pos_word[k];
    const int L = i2v_len(code_len, w);
    float (*s1)[G] = path[grp][0];
    float (*inc)[G] = path[grp][1];
    for (int d = 0; d < L; ++d) {
        s1[d][gl] = syn1[(size_t)i2v_point(points, w, d, V) * D + dim];
        inc[d][gl] = 0.0f;
    }
    const int reach = window - i2v_shrink(seed, it, k, window);
    const long long c0 = lo > k - reach ? lo : k - reach, c1 = hi - 1 < k + reach ? hi - 1 : k + reach;
    const size_t slot = (size_t)(k - r0);
    for (long long c = c0; c <= c1; ++c) {
        if (c == k) continue;
        const float x = syn0[(size_t)pos_word[c] * stride + dim];
        float neu = 0.0f;
        for (int d = 0; d < L; ++d) {
            const float s = s1[d][gl] + inc[d][gl];
            const float prod = x * s;
            const float f = i2v_dot<G>(live ? prod : 0.0f, D);
            if (f > -6.0f && f < 6.0f) {
                const float scaled = (f + 6.0f) * 83.0f;                                    // 83 = Spark's 1000 / 6 / 2.0 with its integer division
                const int idx = (int)scaled;                                                // in [0, 996]
                const float label = 1.0f - (float)codes[(size_t)w * I2V_MAX_CODE + d];
                const float diff = label - exp_table[idx];
                const float g = diff * alpha;
                const float gs = g * s;
                neu = neu + gs;
                const float gx = g * x;
                inc[d][gl] = inc[d][gl] + gx;
            }
        }
        if (live) E0[(slot * (size_t)(2 * window + 1) + (size_t)(c - k + window)) * D + dim] = neu;
    }
    if (live)
        for (int d = 0; d < L; ++d) E1[(slot * I2V_MAX_CODE + d) * D + dim] = inc[d][gl];
}

__device__ inline size_t i2v_lower_bound(const long long* __restrict__ key, size_t lo, size_t hi, long long bound) {
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (key[mid] < bound) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One row of syn0 (rows [0, V)) or syn1 (rows [V, 2 V)) per group of G lanes: the row's records whose centre lies in [r0, r1), in the
// list's order; a record of syn0 counts when its centre's window of this iteration reaches the context.
template <int G>
__global__ __launch_bounds__(FE_THREADS) void k_i2v_apply(long long r0, long long r1, long long N, const unsigned* __restrict__ total, int V, const unsigned* __restrict__ off,
                                                          const long long* __restrict__ key, float* __restrict__ syn0, int stride, float* __restrict__ syn1, int D,
                                                          int window, int it, unsigned long long seed, int row_cap, const float* __restrict__ E0,
                                                          const float* __restrict__ E1) {
#pragma clang fp contract(off)
    if ((long long)*total != N) return;
    const long long row = ((long long)blockIdx.x * FE_THREADS + threadIdx.x) / G;
    const int gl = threadIdx.x % G;
    if (row >= 2ll * V) return;
    const bool live = gl < D;
    const int dim = live ? gl : 0;
    const size_t b0 = i2v_lower_bound(key, off[row], off[row + 1], r0 << 32);
    const size_t b1 = i2v_lower_bound(key, b0, off[row + 1], r1 << 32);
    float sum = 0.0f;
    unsigned cnt = 0;
    // I2V_APPLY_CHUNK records at a time: their keys, then their emissions, are loaded together, and only the adds wait for one another.
    // A record that does not count adds +0.0f: sum is never -0.0f (it starts at +0.0f, and round-to-nearest gives +0.0f for every exact
    // cancellation), so sum + (+0.0f) is sum, bit for bit.  Its emission slot may hold anything (nobody wrote it this round): it is
    // loaded -- the address is inside the buffer -- and dropped by a select, never multiplied.
    for (size_t j = b0; j < b1; j += I2V_APPLY_CHUNK) {
        long long kk[I2V_APPLY_CHUNK];
        float e[I2V_APPLY_CHUNK];
        bool on[I2V_APPLY_CHUNK];
#pragma unroll
        for (int u = 0; u < I2V_APPLY_CHUNK; ++u) kk[u] = key[j + u < b1 ? j + u : b1 - 1];
#pragma unroll
        for (int u = 0; u < I2V_APPLY_CHUNK; ++u) {
            const long long k = kk[u] >> 32, m = kk[u] & 0xffffffffll;
            const size_t slot = (size_t)(k - r0);
            on[u] = j + u < b1;
            if (row < V) {
                const long long dist = m > k ? m - k : k - m;
                on[u] = on[u] && dist <= window - i2v_shrink(seed, it, k, window);
                e[u] = E0[(slot * (size_t)(2 * window + 1) + (size_t)(m - k + window)) * D + dim];
            } else {
                e[u] = E1[(slot * I2V_MAX_CODE + (size_t)m) * D + dim];
            }
        }
#pragma unroll
        for (int u = 0; u < I2V_APPLY_CHUNK; ++u) {
            sum = sum + (on[u] ? e[u] : 0.0f);
            cnt += on[u] ? 1u : 0u;
        }
    }
    if (!cnt || !live) return;
    float* cell = row < V ? syn0 + (size_t)row * stride + dim : syn1 + (size_t)(row - V) * D + dim;
    float add = sum;
    if (cnt > (unsigned)row_cap) {
        const float scale = __fdiv_rn((float)row_cap, (float)cnt);
        add = sum * scale;
    }
    *cell = *cell + add;
}

// the loss terms of one position at the full window under the final model, added in doubles by ascending (context, depth)
template <int G>
__global__ __launch_bounds__(I2V_THREADS) void k_i2v_loss_pos(long long N, const unsigned* __restrict__ total, const int* __restrict__ pos_word, const unsigned* __restrict__ pos_lo,
                                                              const unsigned* __restrict__ pos_hi, const int* __restrict__ code_len, const unsigned char* __restrict__ codes,
                                                              const int* __restrict__ points, int V, const float* __restrict__ syn0, int stride,
                                                              const float* __restrict__ syn1, int D, int window, const double* __restrict__ loss_table,
                                                              double* __restrict__ pos_loss, unsigned* __restrict__ pos_terms) {
#pragma clang fp contract(off)
    __shared__ float path[I2V_THREADS / G][I2V_MAX_CODE][G];
    if ((long long)*total != N) return;
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const long long k = (long long)blockIdx.x * (I2V_THREADS / G) + grp;
    if (k >= N) return;
    const long long lo = pos_lo[k], hi = pos_hi[k];
    const bool live = gl < D;
    const int dim = live ? gl : 0;
    const int w = pos_word[k];
    const int L = i2v_len(code_len, w);
    float (*s1)[G] = path[grp];
    for (int d = 0; d < L; ++d) s1[d][gl] = syn1[(size_t)i2v_point(points, w, d, V) * D + dim];
    const long long c0 = lo > k - window ? lo : k - window, c1 = hi - 1 < k + window ? hi - 1 : k + window;
    double sum = 0.0;
    unsigned terms = 0;
    for (long long c = c0; c <= c1; ++c) {
        if (c == k) continue;
        const float x = syn0[(size_t)pos_word[c] * stride + dim];
        for (int d = 0; d < L; ++d) {
            const float prod = x * s1[d][gl];
            const float f = i2v_dot<G>(live ? prod : 0.0f, D);
            int idx = 0;                                                                    // f <= -6 or NaN
            if (f >= 6.0f) idx = I2V_TABLE - 1;
            else if (f > -6.0f) { const float scaled = (f + 6.0f) * 83.0f; idx = (int)scaled; }
            sum = sum + loss_table[(size_t)codes[(size_t)w * I2V_MAX_CODE + d] % 2u * I2V_TABLE + idx];
            ++terms;
        }
    }
    if (gl == 0) { pos_loss[k] = sum; pos_terms[k] = terms; }
}

__global__ __launch_bounds__(FE_THREADS) void k_i2v_loss_chunks(long long N, const unsigned* __restrict__ total, const double* __restrict__ pos_loss,
                                                                const unsigned* __restrict__ pos_terms, double* __restrict__ chunk_loss,
                                                                unsigned long long* __restrict__ chunk_terms) {
#pragma clang fp contract(off)
    if ((long long)*total != N) return;
    const long long chunks = (N + I2V_LOSS_CHUNK - 1) / I2V_LOSS_CHUNK;
    for (long long c = (long long)blockIdx.x * FE_THREADS + threadIdx.x; c < chunks; c += (long long)gridDim.x * FE_THREADS) {
        const long long b = c * I2V_LOSS_CHUNK, e = b + I2V_LOSS_CHUNK < N ? b + I2V_LOSS_CHUNK : N;
        double sum = 0.0;
        unsigned long long terms = 0;
        for (long long k = b; k < e; ++k) { sum = sum + pos_loss[k]; terms += pos_terms[k]; }
        chunk_loss[c] = sum;
        chunk_terms[c] = terms;
    }
}

__global__ void k_i2v_loss_final(long long N, const unsigned* __restrict__ total, const double* __restrict__ chunk_loss, const unsigned long long* __restrict__ chunk_terms,
                                 double* __restrict__ loss) {
#pragma clang fp contract(off)
    if ((long long)*total != N) return;
    const long long chunks = (N + I2V_LOSS_CHUNK - 1) / I2V_LOSS_CHUNK;
    double sum = 0.0;
    unsigned long long terms = 0;
    for (long long c = 0; c < chunks; ++c) { sum = sum + chunk_loss[c]; terms += chunk_terms[c]; }
    *loss = terms ? __ddiv_rn(sum, (double)terms) : 0.0;
}

// ---- the graph route: transitions between adjacent items of a sequence, and random walks over them (item2vec.py transitions_host,
// walks_host).  The transitions are kept EXPANDED: one entry per adjacent pair in its `prev` item's segment, sorted by `next`, so
// row_total[prev] is the segment's length and "the first next whose cumulative pair_count exceeds t" is the segment's entry t.

// true when items[i], items[i + 1] are adjacent in one sequence
__device__ inline bool i2v_pair(long long i, long long n, int n_seq, const int* __restrict__ seq_off) {
    if (i + 1 >= n) return false;
    int s_lo = 0, s_hi = n_seq - 1;                                                        // the last sequence whose offset is <= i
    while (s_lo < s_hi) {
        const int mid = (s_lo + s_hi + 1) >> 1;
        if ((long long)seq_off[mid] <= i) s_lo = mid; else s_hi = mid - 1;
    }
    return i + 1 < (long long)seq_off[s_lo + 1];
}

__global__ __launch_bounds__(FE_THREADS) void k_i2v_pair_count(long long n, int n_seq, const int* __restrict__ seq_off, const int* __restrict__ items, int n_items,
                                                               unsigned* __restrict__ len, unsigned long long* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const int m = items[i];
        if (m < 0 || m >= n_items) { atomicMin(err, I2V_ERR_MOVIE << 32 | (unsigned long long)i); continue; }
        if (!i2v_pair(i, n, n_seq, seq_off)) continue;
        const int nx = items[i + 1];
        if (nx < 0 || nx >= n_items) continue;                                             // (reported by its own thread)
        atomicAdd(&len[m], 1u);
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_i2v_pair_scatter(long long n, int n_seq, const int* __restrict__ seq_off, const int* __restrict__ items, int n_items,
                                                                 const unsigned* __restrict__ off, unsigned* __restrict__ cursor, long long* __restrict__ key,
                                                                 int* __restrict__ val) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const int m = items[i];
        if (m < 0 || m >= n_items || !i2v_pair(i, n, n_seq, seq_off)) continue;            // k_i2v_pair_count's predicate
        const int nx = items[i + 1];
        if (nx < 0 || nx >= n_items) continue;
        const size_t p = (size_t)off[m] + atomicAdd(&cursor[m], 1u);
        key[p] = nx;
        val[p] = (int)i;                                                                   // equal `next` by place in the input: the sort's keys are distinct
    }
}

// item2vec.py walk_word
__device__ inline unsigned long long i2v_walk_word(unsigned long long seed, long long walk, int step) {
    const unsigned long long s = seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)walk + 1ull);
    return i2v_mix(i2v_mix(s) ^ (unsigned long long)step);
}

// one walk per thread into its sample_length slots of `padded`; wlen[walk] = its length
__global__ __launch_bounds__(FE_THREADS) void k_i2v_walk(long long sample_count, int sample_length, unsigned long long seed, int n_items, const unsigned* __restrict__ off,
                                                         const long long* __restrict__ key, int* __restrict__ padded, unsigned* __restrict__ wlen) {
    const unsigned total = off[n_items];
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < sample_count; i += (long long)gridDim.x * FE_THREADS) {
        if (!total) { wlen[i] = 0u; continue; }
        const unsigned t0 = (unsigned)__umul64hi(i2v_walk_word(seed, i, 0), (unsigned long long)total);      // < total
        int lo = 0, hi = n_items - 1;                                                      // the last item whose offset is <= t0: its segment holds t0
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= t0) lo = mid; else hi = mid - 1;
        }
        int cur = lo;
        unsigned len = 0;
        padded[(size_t)i * sample_length + len++] = cur;
        for (int s = 1; s < sample_length; ++s) {
            const unsigned b = off[cur], rt = off[cur + 1] - b;
            if (!rt) break;                                                                // no successor: the walk ends
            const unsigned t = (unsigned)__umul64hi(i2v_walk_word(seed, i, s), (unsigned long long)rt);      // < rt
            cur = (int)key[(size_t)b + t];
            padded[(size_t)i * sample_length + len++] = cur;
        }
        wlen[i] = len;
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_i2v_walk_emit(long long sample_count, int sample_length, const unsigned* __restrict__ woff, const int* __restrict__ padded,
                                                              int* __restrict__ walk_offsets, int* __restrict__ walk_items) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i <= sample_count; i += (long long)gridDim.x * FE_THREADS) {
        const unsigned b = woff[i];
        walk_offsets[i] = (int)b;
        if (i == sample_count) continue;
        const unsigned len = woff[i + 1] - b;                                              // <= sample_length
        for (unsigned s = 0; s < len; ++s) walk_items[(size_t)b + s] = padded[(size_t)i * sample_length + s];
    }
}
