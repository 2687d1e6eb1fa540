// k_feature_eng.h -- ratings -> training samples and the feature store's rows, on the device (FeatureEngForRecModel.scala:21-130: label,
// movie aggregates, the previous-100-ratings window of every user).  The definition these kernels equal bit for bit is
// sparrowrecsys_amd/featureeng.py samples_host; DESIGN.md section 5.7 has the rules.  Uses k_segments.h: FE_THREADS, the scan with
// its `kept` half (the only user of it) and the segment sort.
//
// Stages, one stream, no host synchronisation (api_feature_eng.h launches them in this order):
//   k_fe_hist       per rating: validate (error word), count the user's ratings, add the movie's n / S / Q      (integer atomics)
//   k_fe_scan_*<true>  (k_segments.h) exclusive scans over users of len and of kept = max(0, len - 2): segment and sample offsets
//   k_fe_scatter    per rating: (timestamp, input row) into its user's segment, any order (the sort key is total)
//   k_fe_sort_short, k_fe_sort_long_chunks + k_fe_merge_pass (+ k_fe_long_copy)  (k_segments.h) every user's segment by (timestamp, input row)
//   k_fe_movie_stats per movie: the four float32 of the store's movie row
//   k_fe_window     per sorted position: the window's count / S / Q, last positives, 32 genre counters, top five; writes the sample
//   k_fe_store      per user and per movie: the store's rows and `has` bytes
// All sums are integer sums: the result is a function of the input alone.

static constexpr int FE_WINDOW = 100;             // rowsBetween(-100, -1)
static constexpr int FE_POSITIVE_R2 = 7;          // label = rating >= 3.5
static constexpr unsigned long long FE_ERR_USER = 1, FE_ERR_MOVIE = 2, FE_ERR_RATING = 3;

// 2 * rating as an integer in [0, 20], or -1 for a rating off the half-star scale (NaN included)
__device__ inline int fe_r2(float r) {
    const float t = r * 2.0f;
    if (!(t >= 0.0f && t <= 20.0f)) return -1;
    const int k = (int)t;
    return (float)k == t ? k : -1;
}

// round-half-to-even of 50 S / n: the average rating in hundredths (S = the sum of 2 * rating)
__host__ __device__ inline unsigned fe_avg_h(unsigned long long n, unsigned long long S) {
    if (n == 0) return 0;
    const unsigned long long a = 50ull * S, q = a / n, r = a % n;
    return (unsigned)(q + ((2 * r > n || (2 * r == n && (q & 1))) ? 1 : 0));
}

// round-half-to-even of 100 sqrt(N / (4 d)), N = n Q - S^2, d = n (n - 1): the sample standard deviation in hundredths, decided in
// integers of type W (64 bits for a window of n <= 100, 128 for a movie's count up to 2^31).  h <= 708 (two ratings, 0 and 10).
template <class W> __host__ __device__ inline unsigned fe_sd_h(unsigned long long n, unsigned long long S, unsigned long long Q) {
    if (n < 2) return 0;
    const W N = (W)n * (W)Q - (W)S * (W)S, d = (W)n * (W)(n - 1), R = N * (W)10000;
    unsigned long long h = 0;
    for (unsigned long long bit = 512; bit; bit >>= 1) {           // floor: the greatest h with (2 h)^2 d <= 10^4 N
        const unsigned long long c = h | bit;
        if ((W)(4 * c * c) * d <= R) h = c;
    }
    const W t = (W)((2 * h + 1) * (2 * h + 1)) * d;
    if (t < R || (t == R && (h & 1))) ++h;
    return (unsigned)h;
}

__device__ inline float fe_hundredths(unsigned h) { return (float)((double)h / 100.0); }

__global__ __launch_bounds__(FE_THREADS) void k_fe_hist(long long n, const int* __restrict__ user, const int* __restrict__ movie, const float* __restrict__ rating,
                                                        int n_users, int n_movies, unsigned* __restrict__ len, unsigned* __restrict__ mv_cnt,
                                                        unsigned long long* __restrict__ mv_S, unsigned long long* __restrict__ mv_Q,
                                                        unsigned long long* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const int u = user[i], m = movie[i], r2 = fe_r2(rating[i]);
        const unsigned long long kind = (u < 0 || u >= n_users) ? FE_ERR_USER : (m < 0 || m >= n_movies) ? FE_ERR_MOVIE : r2 < 0 ? FE_ERR_RATING : 0;
        if (kind) { atomicMin(err, kind << 32 | (unsigned long long)i); continue; }      // (the row takes no further part: every later index stays in range)
        atomicAdd(&len[u], 1u);
        atomicAdd(&mv_cnt[m], 1u);
        atomicAdd(&mv_S[m], (unsigned long long)r2);
        atomicAdd(&mv_Q[m], (unsigned long long)(r2 * r2));
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_fe_scatter(long long n, const int* __restrict__ user, const int* __restrict__ movie, const float* __restrict__ rating,
                                                           const long long* __restrict__ ts, int n_users, int n_movies, const unsigned* __restrict__ seg_off,
                                                           unsigned* __restrict__ cursor, long long* __restrict__ seg_ts, int* __restrict__ seg_row, int* __restrict__ seg_user) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const int u = user[i], m = movie[i];
        if (u < 0 || u >= n_users || m < 0 || m >= n_movies || fe_r2(rating[i]) < 0) continue;      // k_fe_hist's predicate
        const size_t pos = (size_t)seg_off[u] + atomicAdd(&cursor[u], 1u);                             // < seg_off[u + 1]: the same rows were counted
        seg_ts[pos] = ts[i];
        seg_row[pos] = (int)i;
        seg_user[pos] = u;
    }
}

// mv_dense[m] = {releaseYear, movieRatingCount, movieAvgRating, movieRatingStddev} as float32 bits
__global__ __launch_bounds__(FE_THREADS) void k_fe_movie_stats(int n_movies, const int* __restrict__ mv_year, const unsigned* __restrict__ mv_cnt,
                                                               const unsigned long long* __restrict__ mv_S, const unsigned long long* __restrict__ mv_Q, float* __restrict__ mv_dense) {
    const int m = blockIdx.x * FE_THREADS + threadIdx.x;
    if (m >= n_movies) return;
    const unsigned long long n = mv_cnt[m], S = mv_S[m], Q = mv_Q[m];
    float* o = mv_dense + (size_t)m * 4;
    o[0] = (float)mv_year[m];
    o[1] = (float)(unsigned)n;
    o[2] = fe_hundredths(fe_avg_h(n, S));
    o[3] = fe_hundredths(fe_sd_h<unsigned __int128>(n, S, Q));
}

// bit g of b (8 bits) -> byte g of the result = 1
__device__ inline unsigned long long fe_spread8(unsigned b) {
    const unsigned long long x = ((unsigned long long)b * 0x0101010101010101ull) & 0x8040201008040201ull;
    return ((x + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}

// What a window is read from: entry i of the walk gives 2 * rating, and for a positive rating its movie and the movie's genre mask.
// Here the workgroup's LDS image (k_fe_window); k_store_update.h has the other one, a user's ring and its new ratings.
struct FeLdsWindow {
    const int* movie_;
    const unsigned* mask_;
    const unsigned char* r2_;
    __device__ unsigned r2(long long i) const { return r2_[i]; }
    __device__ int movie(long long i) const { return movie_[i]; }
    __device__ unsigned mask(long long i) const { return mask_[i]; }
};

// One window, walked backwards over the entries last .. first of `w` (most recent first, which is the order of userRatedMovie1..):
// S and Q of 2 * rating, the first H positive movies to hist[0 .. H) (0 where there are fewer), and top[0 .. 5) = the five greatest keys
// count << 5 | (31 - dictionary id) among the genres with count > 0 (count desc, dictionary id asc; 0 = none).  The 32 genre counters
// (<= 100 each) are bytes of four 64-bit registers.
template <class Window>
__device__ inline void fe_window_fold(const Window w, long long last, long long first, int H, int* __restrict__ hist, unsigned* S_out, unsigned* Q_out, unsigned* top) {
    unsigned S = 0, Q = 0;
    int n_pos = 0;
    unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (long long i = last; i >= first; --i) {
        const unsigned r2 = w.r2(i);
        S += r2; Q += r2 * r2;
        if (r2 >= FE_POSITIVE_R2) {
            if (n_pos < H) hist[n_pos] = w.movie(i);
            ++n_pos;
            const unsigned g = w.mask(i);
            c0 += fe_spread8(g & 255u); c1 += fe_spread8((g >> 8) & 255u); c2 += fe_spread8((g >> 16) & 255u); c3 += fe_spread8(g >> 24);
        }
    }
    for (int k = n_pos; k < H; ++k) hist[k] = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) top[k] = 0;
#pragma unroll
    for (int g = 0; g < 32; ++g) {
        const unsigned long long cw = g < 8 ? c0 : g < 16 ? c1 : g < 24 ? c2 : c3;
        const unsigned c = (unsigned)(cw >> ((g & 7) * 8)) & 255u;
        unsigned key = c ? (c << 5 | (unsigned)(31 - g)) : 0u;
#pragma unroll
        for (int k = 0; k < 5; ++k) {                                          // kept sorted by insertion
            const unsigned hi = top[k] > key ? top[k] : key;
            key = top[k] > key ? key : top[k];
            top[k] = hi;
        }
    }
    *S_out = S; *Q_out = Q;
}

// userGenre of a key of fe_window_fold's top five: a genre outside the vocabulary holds its place as -1
__device__ inline int fe_top_genre(unsigned key, int n_vocab) {
    const int id = 31 - (int)(key & 31u);
    return (key && id < n_vocab) ? id : -1;
}

// One thread per sorted position.  The workgroup's FE_THREADS positions and the FE_WINDOW before them sit in LDS (movie, genre mask,
// 2 * rating); a thread folds its window with fe_window_fold.
__global__ __launch_bounds__(FE_THREADS) void k_fe_window(const unsigned* __restrict__ seg_off, const unsigned* __restrict__ kept_off, int n_users,
                                                          const long long* __restrict__ seg_ts, const int* __restrict__ seg_row, const int* __restrict__ seg_user,
                                                          const int* __restrict__ movie, const float* __restrict__ rating,
                                                          const int* __restrict__ mv_genre3, const unsigned* __restrict__ mv_mask, const float* __restrict__ mv_dense,
                                                          unsigned* __restrict__ mv_flag, int n_vocab, int H,
                                                          int* __restrict__ out_user, int* __restrict__ out_movie, float* __restrict__ out_rating, long long* __restrict__ out_ts,
                                                          int* __restrict__ out_label, int* __restrict__ out_src, int* __restrict__ out_genres, int* __restrict__ out_hist,
                                                          float* __restrict__ out_dense) {
    __shared__ int s_movie[FE_THREADS + FE_WINDOW];
    __shared__ unsigned s_mask[FE_THREADS + FE_WINDOW];
    __shared__ unsigned char s_r2[FE_THREADS + FE_WINDOW];
    const long long total = seg_off[n_users];
    const long long b0 = (long long)blockIdx.x * FE_THREADS;
    if (b0 >= total) return;                                                   // (the whole workgroup)
    const long long lo = b0 - FE_WINDOW;
    for (int i = threadIdx.x; i < FE_THREADS + FE_WINDOW; i += FE_THREADS) {
        const long long q = lo + i;
        if (q >= 0 && q < total) {
            const int row = seg_row[q], m = movie[row];
            s_movie[i] = m;
            s_mask[i] = mv_mask[m];
            s_r2[i] = (unsigned char)fe_r2(rating[row]);
        }
    }
    __syncthreads();
    const long long pos = b0 + threadIdx.x;
    if (pos >= total) return;
    const int u = seg_user[pos];
    const long long start = seg_off[u], p = pos - start;
    if (p < 2) return;                                                         // userRatingCount <= 1: dropped
    const size_t j = (size_t)kept_off[u] + (size_t)(p - 2);
    const int me = (int)(pos - lo);
    const int first = (int)((pos - FE_WINDOW > start ? pos - FE_WINDOW : start) - lo);
    unsigned S = 0, Q = 0;
    unsigned top[5];
    fe_window_fold(FeLdsWindow{s_movie, s_mask, s_r2}, (long long)me - 1, (long long)first, H, out_hist + j * (size_t)H, &S, &Q, top);
    const int row = seg_row[pos], m = s_movie[me];
    const unsigned r2 = s_r2[me];
    const int count = me - first;
    out_user[j] = u;
    out_movie[j] = m;
    out_rating[j] = rating[row];
    out_ts[j] = seg_ts[pos];
    out_label[j] = r2 >= FE_POSITIVE_R2 ? 1 : 0;
    out_src[j] = row;
    int* og = out_genres + j * 8;
    for (int k = 0; k < 3; ++k) og[k] = mv_genre3[(size_t)m * 3 + k];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        og[3 + k] = fe_top_genre(top[k], n_vocab);
    }
    float* od = out_dense + j * 7;
    const float* md = mv_dense + (size_t)m * 4;
    for (int k = 0; k < 4; ++k) od[k] = md[k];
    od[4] = (float)count;
    od[5] = fe_hundredths(fe_avg_h((unsigned long long)count, S));
    od[6] = fe_hundredths(fe_sd_h<unsigned long long>((unsigned long long)count, S, Q));
    mv_flag[m] = 1u;                                                           // (every writer stores the same word)
}

// The store (featurestore.py's layout).  User row = the user's last kept sample: history | userGenre1..5 | count avg stddev | zeros.
// Movie row = movieGenre1..3 | year count avg stddev | 0 of any kept sample that names the movie: these columns depend on the movie
// alone, so the latest such sample's are every such sample's.  An id without a kept sample: the NA defaults and has = 0.
__global__ __launch_bounds__(FE_THREADS) void k_fe_store(int n_users, int n_movies, int H, int user_pitch, const unsigned* __restrict__ kept_off,
                                                         const int* __restrict__ out_genres, const int* __restrict__ out_hist, const float* __restrict__ out_dense,
                                                         const int* __restrict__ mv_genre3, const float* __restrict__ mv_dense, const unsigned* __restrict__ mv_flag,
                                                         int* __restrict__ user_rows, unsigned char* __restrict__ user_has, int* __restrict__ movie_rows,
                                                         unsigned char* __restrict__ movie_has) {
    const long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x;
    if (i < n_users) {
        int* row = user_rows + (size_t)i * user_pitch;
        const unsigned k0 = kept_off[i], k1 = kept_off[i + 1];
        const bool has = k1 > k0;
        const size_t j = has ? (size_t)k1 - 1 : 0;
        for (int k = 0; k < H; ++k) row[k] = has ? out_hist[j * (size_t)H + k] : 0;
        for (int k = 0; k < 5; ++k) row[H + k] = has ? out_genres[j * 8 + 3 + k] : -1;
        for (int k = 0; k < 3; ++k) row[H + 5 + k] = has ? __float_as_int(out_dense[j * 7 + 4 + k]) : 0;
        for (int k = H + 8; k < user_pitch; ++k) row[k] = 0;
        user_has[i] = has ? 1 : 0;
    }
    if (i < n_movies) {
        int* row = movie_rows + (size_t)i * 8;
        const bool has = mv_flag[i] != 0;
        for (int k = 0; k < 3; ++k) row[k] = has ? mv_genre3[(size_t)i * 3 + k] : -1;
        for (int k = 0; k < 4; ++k) row[3 + k] = has ? __float_as_int(mv_dense[(size_t)i * 4 + k]) : 0;
        row[7] = 0;
        movie_has[i] = has ? 1 : 0;
    }
}
