// k_store_update.h -- new ratings applied to an existing feature store, on the device: after the call the store's four tables are the
// tables sprk_feature_eng writes from ALL ratings applied so far (DESIGN.md section 5.14 has the contract and why a small state is
// enough).  The definition these kernels equal byte for byte is sparrowrecsys_amd/featureeng.py update_host.  Uses k_segments.h (the scan
// and the segment sort) and k_feature_eng.h (fe_r2, fe_avg_h, fe_sd_h, fe_window_fold: the window is folded by the code k_fe_window runs).
//
// The state, next to the tables: per user the count of ratings applied, the latest timestamp applied and a ring of the last FE_WINDOW
// ratings (movie, 2 * rating) at slot position % FE_WINDOW; per movie n / S / Q over all ratings and the flag "a kept sample names it".
//
// Stages, one stream, no host synchronisation (api_store_update.h launches them in this order):
//   k_su_check      per new rating: id ranges, the half-star scale, timestamp >= the user's latest; writes the error word ALONE
//   k_su_count      per new rating: its user's new ratings
//   k_fe_scan_*<false>  (k_segments.h) segment offsets of the new ratings per user
//   k_su_scatter    per new rating: (timestamp, row in the batch) into its user's segment
//   k_fe_sort_*     (k_segments.h) every user's new ratings by (timestamp, row in the batch)
//   k_su_positions  per sorted new position: the movie's n / S / Q (integer atomics), touched, and flagged at a user position >= 2
//   k_su_users      per user with new ratings: the window before the new last position, from the OLD ring and the sorted new ratings -> the user row
//   k_su_ring       per user with new ratings: the last min(k, FE_WINDOW) new ratings into the ring, the count, the latest timestamp
//   k_su_movies     per touched movie: its row from n / S / Q and the movie table, or the NA defaults while it is not flagged
// Every kernel after k_su_check returns at once when the error word is set: a failed update changes neither state nor tables.  (The
// scan and the sort run regardless, on a workspace that then holds zero counts.)  All sums are integer sums.

static constexpr unsigned long long FE_ERR_OLDER = 4;
static constexpr unsigned long long SU_NO_ERROR = ~0ull;

__global__ __launch_bounds__(FE_THREADS) void k_su_check(long long n, const int* __restrict__ user, const int* __restrict__ movie, const float* __restrict__ rating,
                                                         const long long* __restrict__ ts, int n_users, int n_movies, const long long* __restrict__ last_ts,
                                                         unsigned long long* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const int u = user[i], m = movie[i];
        const unsigned long long kind = (u < 0 || u >= n_users) ? FE_ERR_USER : (m < 0 || m >= n_movies) ? FE_ERR_MOVIE : fe_r2(rating[i]) < 0 ? FE_ERR_RATING
                                        : ts[i] < last_ts[u] ? FE_ERR_OLDER : 0;
        if (kind) atomicMin(err, kind << 32 | (unsigned long long)i);
    }
}

__global__ __launch_bounds__(FE_THREADS) void k_su_count(long long n, const int* __restrict__ user, unsigned* __restrict__ len, const unsigned long long* __restrict__ err) {
    if (*err != SU_NO_ERROR) return;
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) atomicAdd(&len[user[i]], 1u);
}

__global__ __launch_bounds__(FE_THREADS) void k_su_scatter(long long n, const int* __restrict__ user, const long long* __restrict__ ts, const unsigned* __restrict__ seg_off,
                                                           unsigned* __restrict__ cursor, long long* __restrict__ seg_ts, int* __restrict__ seg_row, int* __restrict__ seg_user,
                                                           const unsigned long long* __restrict__ err) {
    if (*err != SU_NO_ERROR) return;
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const int u = user[i];
        const size_t pos = (size_t)seg_off[u] + atomicAdd(&cursor[u], 1u);                             // < seg_off[u + 1]: k_su_count counted the same rows
        seg_ts[pos] = ts[i];
        seg_row[pos] = (int)i;
        seg_user[pos] = u;
    }
}

// sorted new position q of user u is the user's position u_cnt[u] + (q - seg_off[u]) among all ratings applied
__global__ __launch_bounds__(FE_THREADS) void k_su_positions(long long n, const unsigned* __restrict__ seg_off, const int* __restrict__ seg_row, const int* __restrict__ seg_user,
                                                             const int* __restrict__ movie, const float* __restrict__ rating, const unsigned* __restrict__ u_cnt,
                                                             unsigned* __restrict__ mv_cnt, unsigned long long* __restrict__ mv_S, unsigned long long* __restrict__ mv_Q,
                                                             unsigned char* __restrict__ mv_flag, unsigned char* __restrict__ mv_touched, const unsigned long long* __restrict__ err) {
    if (*err != SU_NO_ERROR) return;
    for (long long q = (long long)blockIdx.x * FE_THREADS + threadIdx.x; q < n; q += (long long)gridDim.x * FE_THREADS) {
        const int u = seg_user[q], row = seg_row[q], m = movie[row];
        const unsigned r2 = (unsigned)fe_r2(rating[row]);
        atomicAdd(&mv_cnt[m], 1u);
        atomicAdd(&mv_S[m], (unsigned long long)r2);
        atomicAdd(&mv_Q[m], (unsigned long long)(r2 * r2));
        mv_touched[m] = 1;                                                     // (every writer stores the same byte)
        if ((unsigned long long)u_cnt[u] + (unsigned long long)(q - seg_off[u]) >= 2) mv_flag[m] = 1;
    }
}

// A user's ratings by position: below `old` the ring (the state before this update), from `old` on the sorted new ratings.
struct SuWindow {
    const int* ring_movie;                 // the user's FE_WINDOW slots
    const unsigned char* ring_r2;
    const int* new_row;                    // the user's sorted new ratings: rows of the batch
    const int* batch_movie;                // the batch's columns
    const float* batch_rating;
    const unsigned* mv_mask;
    long long old;
    __device__ unsigned r2(long long i) const { return i < old ? ring_r2[i % FE_WINDOW] : (unsigned)fe_r2(batch_rating[new_row[i - old]]); }
    __device__ int movie(long long i) const { return i < old ? ring_movie[i % FE_WINDOW] : batch_movie[new_row[i - old]]; }
    __device__ unsigned mask(long long i) const { return mv_mask[movie(i)]; }
};

// One thread per user; a user without new ratings is passed over.  The user row is the user's last kept sample: the window
// [P - FE_WINDOW, P - 1] before the last position P = old + k - 1, kept iff P >= 2.  Its positions below `old` are >= old - FE_WINDOW + k - 1 >=
// old - FE_WINDOW: the ring holds them.  (First version: the <= 100 entries are read from global memory by one thread.)
__global__ __launch_bounds__(FE_THREADS) void k_su_users(int n_users, const unsigned* __restrict__ seg_off, const int* __restrict__ seg_row, const int* __restrict__ movie,
                                                         const float* __restrict__ rating, const unsigned* __restrict__ mv_mask, const unsigned* __restrict__ u_cnt,
                                                         const int* __restrict__ ring_movie, const unsigned char* __restrict__ ring_r2, int n_vocab, int H, int user_pitch,
                                                         int* __restrict__ user_rows, unsigned char* __restrict__ user_has, const unsigned long long* __restrict__ err) {
    if (*err != SU_NO_ERROR) return;
    for (long long u = (long long)blockIdx.x * FE_THREADS + threadIdx.x; u < n_users; u += (long long)gridDim.x * FE_THREADS) {
        const unsigned base = seg_off[u], k = seg_off[u + 1] - base;
        if (k == 0) continue;
        const long long old = u_cnt[u], P = old + k - 1;
        if (P < 2) continue;                                                   // still no kept sample: the row keeps its NA defaults
        const long long first = P > FE_WINDOW ? P - FE_WINDOW : 0;
        const SuWindow w{ring_movie + (size_t)u * FE_WINDOW, ring_r2 + (size_t)u * FE_WINDOW, seg_row + base, movie, rating, mv_mask, old};
        int* row = user_rows + (size_t)u * user_pitch;
        unsigned S, Q, top[5];
        fe_window_fold(w, P - 1, first, H, row, &S, &Q, top);
        const unsigned long long count = (unsigned long long)(P - first);
#pragma unroll
        for (int g = 0; g < 5; ++g) row[H + g] = fe_top_genre(top[g], n_vocab);
        row[H + 5] = __float_as_int((float)(int)count);
        row[H + 6] = __float_as_int(fe_hundredths(fe_avg_h(count, S)));
        row[H + 7] = __float_as_int(fe_hundredths(fe_sd_h<unsigned long long>(count, S, Q)));
        for (int g = H + 8; g < user_pitch; ++g) row[g] = 0;
        user_has[u] = 1;
    }
}

// A launch of its own AFTER k_su_users, which reads the slots this one overwrites.
__global__ __launch_bounds__(FE_THREADS) void k_su_ring(int n_users, const unsigned* __restrict__ seg_off, const long long* __restrict__ seg_ts, const int* __restrict__ seg_row,
                                                        const int* __restrict__ movie, const float* __restrict__ rating, unsigned* __restrict__ u_cnt, long long* __restrict__ u_last_ts,
                                                        int* __restrict__ ring_movie, unsigned char* __restrict__ ring_r2, const unsigned long long* __restrict__ err) {
    if (*err != SU_NO_ERROR) return;
    for (long long u = (long long)blockIdx.x * FE_THREADS + threadIdx.x; u < n_users; u += (long long)gridDim.x * FE_THREADS) {
        const unsigned base = seg_off[u], k = seg_off[u + 1] - base;
        if (k == 0) continue;
        const long long old = u_cnt[u];
        int* rm = ring_movie + (size_t)u * FE_WINDOW;
        unsigned char* rr = ring_r2 + (size_t)u * FE_WINDOW;
        for (unsigned j = k > (unsigned)FE_WINDOW ? k - FE_WINDOW : 0u; j < k; ++j) {
            const int row = seg_row[base + j];
            const int slot = (int)((old + j) % FE_WINDOW);
            rm[slot] = movie[row];
            rr[slot] = (unsigned char)fe_r2(rating[row]);
        }
        u_cnt[u] = (unsigned)(old + k);
        u_last_ts[u] = seg_ts[base + k - 1];                                   // the greatest key of the sorted segment
    }
}

// k_fe_movie_stats' arithmetic and k_fe_store's movie row, for the movies this batch names
__global__ __launch_bounds__(FE_THREADS) void k_su_movies(int n_movies, const unsigned char* __restrict__ mv_touched, const int* __restrict__ mv_year, const int* __restrict__ mv_genre3,
                                                          const unsigned* __restrict__ mv_cnt, const unsigned long long* __restrict__ mv_S, const unsigned long long* __restrict__ mv_Q,
                                                          const unsigned char* __restrict__ mv_flag, int* __restrict__ movie_rows, unsigned char* __restrict__ movie_has,
                                                          const unsigned long long* __restrict__ err) {
    if (*err != SU_NO_ERROR) return;
    for (long long m = (long long)blockIdx.x * FE_THREADS + threadIdx.x; m < n_movies; m += (long long)gridDim.x * FE_THREADS) {
        if (!mv_touched[m]) continue;
        int* row = movie_rows + (size_t)m * 8;
        const bool has = mv_flag[m] != 0;
        const unsigned long long n = mv_cnt[m], S = mv_S[m], Q = mv_Q[m];
        for (int k = 0; k < 3; ++k) row[k] = has ? mv_genre3[(size_t)m * 3 + k] : -1;
        row[3] = has ? __float_as_int((float)mv_year[m]) : 0;
        row[4] = has ? __float_as_int((float)(unsigned)n) : 0;
        row[5] = has ? __float_as_int(fe_hundredths(fe_avg_h(n, S))) : 0;
        row[6] = has ? __float_as_int(fe_hundredths(fe_sd_h<unsigned __int128>(n, S, Q))) : 0;
        row[7] = 0;
        movie_has[m] = has ? 1 : 0;
    }
}
