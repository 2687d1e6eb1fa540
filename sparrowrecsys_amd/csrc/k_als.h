// k_als.h -- ALS collaborative filtering on the device (the reference's offline/spark/model/CollaborativeFiltering.scala: Spark ALS,
// explicit feedback, no non-negativity): factors from ratings, and scores from factors.  The definition these kernels equal bit for bit
// is sparrowrecsys_amd/als.py als_host; DESIGN.md section 5.10 has the rules.  Uses k_segments.h: the counts-only scan and the
// (ungated) segment sort, once per side.
//
// Stages, one stream, no host synchronisation (api_als.h launches them in this order):
//   k_als_count       per rating: validate (error word), count the user's and the movie's ratings
//   k_fe_scan_*<false>  exclusive scans of the two sets of counts: segment offsets
//   k_als_scatter     per rating: into its MOVIE's segment as (user << 32 | input row, rating bits) and into its USER's segment as
//                     (movie << 32 | input row, rating bits), at atomic cursors, any order
//   k_fe_sort_short + k_fe_sort_long_chunks + k_fe_merge_pass (+ k_fe_long_copy)  each segment by its key, once for all sweeps
//   k_als_init        per row: counts, has, init_user -> user_factors (a non-finite value: error word), zeros -> item_factors
//   -- 2 x iters times --
//   k_als_begin       one thread: the work counter back to 0; `stop` = the error word is set (so an error of an earlier stage ends the
//                     sweeps, and a row that fails in a sweep does not hide another of the same sweep: the word is a function of the input)
//   k_als_half_sweep  per (destination row, accumulator): the normal equations; then per row: Cholesky and the two triangular solves
// No float or double atomics and nothing split along a row's ratings: the result is a function of the input alone.

static constexpr int ALS_THREADS = 256;
static_assert(ALS_THREADS == FE_THREADS, "api_als.h sizes the grids of ALS_THREADS kernels with fe_grid_capped");
static constexpr int ALS_G = 16;                   // lanes per destination row: four rows a wave
static constexpr int ALS_CHUNK = 16;               // ratings per lane group and pipeline stage
static constexpr int ALS_MAX_RANK = 16;
static constexpr int ALS_SLOTS = ALS_MAX_RANK + 1; // doubles staged per rating: the factor row, then the rating
static constexpr int ALS_MAX_ACC = ALS_MAX_RANK * (ALS_MAX_RANK + 1) / 2 + ALS_MAX_RANK;     // 152
static constexpr unsigned long long ALS_ERR_USER = 1, ALS_ERR_MOVIE = 2, ALS_ERR_RATING = 3, ALS_ERR_USER_SOLVE = 5, ALS_ERR_MOVIE_SOLVE = 6, ALS_ERR_INIT = 7;
enum { ALS_W_LONG_USER = 0, ALS_W_LONG_MOVIE = 1, ALS_W_NEXT_ROW = 2, ALS_W_STOP = 3 };     // the workspace's control words

__device__ inline bool als_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ inline unsigned long long als_row_kind(int u, int m, float r, int n_users, int n_items) {
    return (u < 0 || u >= n_users) ? ALS_ERR_USER : (m < 0 || m >= n_items) ? ALS_ERR_MOVIE : !als_finite(r) ? ALS_ERR_RATING : 0ull;
}

__global__ __launch_bounds__(ALS_THREADS) void k_als_count(long long n, const int* __restrict__ user, const int* __restrict__ movie, const float* __restrict__ rating,
                                                           int n_users, int n_items, unsigned* __restrict__ len_user, unsigned* __restrict__ len_movie,
                                                           unsigned long long* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * ALS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * ALS_THREADS) {
        const int u = user[i], m = movie[i];
        const unsigned long long kind = als_row_kind(u, m, rating[i], n_users, n_items);
        if (kind) { atomicMin(err, kind << 32 | (unsigned long long)i); continue; }       // (the row takes no further part: every later index stays in range)
        atomicAdd(&len_user[u], 1u);
        atomicAdd(&len_movie[m], 1u);
    }
}

__global__ __launch_bounds__(ALS_THREADS) void k_als_scatter(long long n, const int* __restrict__ user, const int* __restrict__ movie, const float* __restrict__ rating,
                                                             int n_users, int n_items, const unsigned* __restrict__ off_user, const unsigned* __restrict__ off_movie,
                                                             unsigned* __restrict__ cur_user, unsigned* __restrict__ cur_movie, long long* __restrict__ key_user,
                                                             int* __restrict__ val_user, long long* __restrict__ key_movie, int* __restrict__ val_movie) {
    for (long long i = (long long)blockIdx.x * ALS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * ALS_THREADS) {
        const int u = user[i], m = movie[i];
        const float r = rating[i];
        if (als_row_kind(u, m, r, n_users, n_items)) continue;                            // k_als_count's predicate
        const size_t pu = (size_t)off_user[u] + atomicAdd(&cur_user[u], 1u);               // < off_user[u + 1]: the same rows were counted
        const size_t pm = (size_t)off_movie[m] + atomicAdd(&cur_movie[m], 1u);
        key_user[pu] = (long long)m << 32 | i;                                             // i < 2^31 - 1
        val_user[pu] = __float_as_int(r);
        key_movie[pm] = (long long)u << 32 | i;
        val_movie[pm] = __float_as_int(r);
    }
}

// every output row but the factors the sweeps write: counts, has, the initial user factors, zero item factors
__global__ __launch_bounds__(ALS_THREADS) void k_als_init(int n_users, int n_items, int rank, const unsigned* __restrict__ off_user, const unsigned* __restrict__ off_movie,
                                                          const float* __restrict__ init_user, int init_stride, float* __restrict__ user_factors, int user_stride,
                                                          float* __restrict__ item_factors, int item_stride, unsigned char* __restrict__ user_has,
                                                          unsigned char* __restrict__ item_has, int* __restrict__ user_count, int* __restrict__ item_count,
                                                          unsigned long long* __restrict__ err) {
    const long long rows = n_users > n_items ? n_users : n_items;
    for (long long i = (long long)blockIdx.x * ALS_THREADS + threadIdx.x; i < rows; i += (long long)gridDim.x * ALS_THREADS) {
        if (i < n_users) {
            const unsigned c = off_user[i + 1] - off_user[i];
            user_count[i] = (int)c;
            user_has[i] = c ? 1 : 0;
            bool finite = true;
            for (int d = 0; d < rank; ++d) {
                const float x = init_user[(size_t)i * init_stride + d];
                finite = finite && als_finite(x);
                user_factors[(size_t)i * user_stride + d] = x;
            }
            if (!finite) atomicMin(err, ALS_ERR_INIT << 32 | (unsigned long long)i);
        }
        if (i < n_items) {
            const unsigned c = off_movie[i + 1] - off_movie[i];
            item_count[i] = (int)c;
            item_has[i] = c ? 1 : 0;
            for (int d = 0; d < rank; ++d) item_factors[(size_t)i * item_stride + d] = 0.0f;
        }
    }
}

__global__ void k_als_begin(unsigned* __restrict__ words, const unsigned long long* __restrict__ err) {
    words[ALS_W_NEXT_ROW] = 0u;
    words[ALS_W_STOP] = *err != ~0ull ? 1u : 0u;
}

// dpptrf + dpptrs on one packed system in LDS, one lane: A = the packed upper triangle (entry (i, j), i <= j, at j (j + 1) / 2 + i), overwritten
// by U; b overwritten by the solution.  The operation order is the definition's (als.py cholesky_solve_host): every product and every
// difference rounded on its own (no contraction), correctly rounded division and square root.  -> false when some d is not > 0.
__device__ inline bool als_cholesky_solve(double* A, double* b, int rank) {
#pragma clang fp contract(off)
    for (int j = 0; j < rank; ++j) {
        double* cj = A + j * (j + 1) / 2;
        for (int i = 0; i < j; ++i) {
            const double* ci = A + i * (i + 1) / 2;
            double s = cj[i];
            for (int p = 0; p < i; ++p) {
                const double prod = ci[p] * cj[p];
                s = s - prod;
            }
            cj[i] = __ddiv_rn(s, ci[i]);
        }
        double t = 0.0;
        for (int p = 0; p < j; ++p) {
            const double sq = cj[p] * cj[p];
            t = t + sq;
        }
        const double d = cj[j] - t;
        if (!(d > 0.0)) return false;
        cj[j] = __dsqrt_rn(d);
    }
    for (int j = 0; j < rank; ++j) {                                           // U^T z = b
        const double* cj = A + j * (j + 1) / 2;
        double t = b[j];
        for (int i = 0; i < j; ++i) {
            const double prod = cj[i] * b[i];
            t = t - prod;
        }
        b[j] = __ddiv_rn(t, cj[j]);
    }
    for (int j = rank - 1; j >= 0; --j) {                                      // U y = z; dpptrs's skip is kept: without it a -0.0 above would become +0.0
        const double* cj = A + j * (j + 1) / 2;
        if (b[j] != 0.0) {
            const double yj = __ddiv_rn(b[j], cj[j]);
            b[j] = yj;
            for (int i = j - 1; i >= 0; --i) {
                const double prod = yj * cj[i];
                b[i] = b[i] - prod;
            }
        }
    }
    return true;
}

// One half-sweep: destination row d (a movie, then a user) solves for its factor from the factor rows `src` of the other side.
//
// Shape.  ALS_G = 16 lanes walk one row's ratings, four rows a wave; the row's T = rank (rank + 1) / 2 + rank accumulators (the packed
// triangle, then atb) are dealt round-robin over the 16 lanes, NCH = ceil(T / 16) independent chains per lane: 2 up to rank 6, 5 up to
// rank 10, 10 up to rank 16.  Rows are handed out through an integer counter, four at a time per wave, so a wave behind a long row holds
// up no other.  Per chunk of ALS_CHUNK ratings a lane holds the other side's ids and the ratings of the chunk after the next and its
// dimension of the factor rows of the next chunk in flight (loads only, nothing waits) while this chunk is accumulated: the 16 lanes
// stage the widened factor row and the rating of every rating of the chunk in LDS (17 doubles), and every chain then does
// acc = fma(slot[pi], slot[pj], acc), with (pi, pj) = (i, j) for a triangle entry and (i, the rating's slot) for atb.
// Why fma gives the definition's bits although the definition rounds the product first: both factors are float32 values widened to
// double (24-bit significands, exponents within float32's), so the product has at most 48 significant bits and an exponent far inside
// binary64's range -- it is EXACT, the rounding of the product changes nothing, and fma(x, y, acc) == acc + (x * y) bit for bit.
// The definition's two skips (x[j] == 0 in dspr, rating == 0 in daxpy) are dropped: for finite factors the product is then +-0.0, and
// acc + (+-0.0) is acc bit for bit because acc is never -0.0 (it starts at +0.0 and round-to-nearest gives +0.0 for every exact
// cancellation).  A rating slot past the row's end is staged as zeros for the same reason.  Chains past T accumulate rating^2 and are
// never read.
// After the walk the accumulators meet in LDS and one lane per row adds n * reg to the diagonal and runs als_cholesky_solve.
template <int NCH>
__global__ __launch_bounds__(ALS_THREADS) void k_als_half_sweep(int n_dst, int rank, double reg, const unsigned* __restrict__ seg_off, const long long* __restrict__ seg_key,
                                                                const int* __restrict__ seg_val, const float* __restrict__ src, int src_stride,
                                                                float* __restrict__ dst, int dst_stride, unsigned long long fail_kind,
                                                                unsigned* __restrict__ words, unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)                                                 // n * reg, then the sum: the one fused operation here is the explicit fma below
    constexpr int ROWS = 64 / ALS_G, WAVES = ALS_THREADS / 64;
    __shared__ double stage[WAVES][ROWS][ALS_CHUNK * ALS_SLOTS];
    static_assert(NCH * ALS_G <= ALS_CHUNK * ALS_SLOTS && ALS_MAX_ACC <= 10 * ALS_G, "the accumulators meet in the staging area");
    if (words[ALS_W_STOP]) return;                                             // an earlier stage or sweep reported an error: the outputs hold no result
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane / ALS_G, gl = lane % ALS_G;
    const int tri = rank * (rank + 1) / 2, T = tri + rank;
    double* my_stage = stage[wave][grp];
    double* my_system = my_stage;                                             // the row's T accumulators meet where its ratings were staged: T <= NCH * 16 <= 160 < 16 * 17
    int pi[NCH], pj[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int a = gl + ALS_G * c;
        int i = ALS_MAX_RANK, j = ALS_MAX_RANK;                                // a chain past T: rating * rating, never read
        if (a < tri) {
            j = 0;
            while ((j + 1) * (j + 2) / 2 <= a) ++j;
            i = a - j * (j + 1) / 2;
        } else if (a < T) {
            i = a - tri;
        }
        pi[c] = i; pj[c] = j;
    }
    for (;;) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&words[ALS_W_NEXT_ROW], (unsigned)ROWS);
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        if (base >= (unsigned)n_dst) break;                                    // (the whole wave)
        const unsigned d = base + (unsigned)grp;
        const bool live = d < (unsigned)n_dst;                                 // (a wave's last draw can pass the end)
        unsigned lo = 0, len = 0;
        if (live) { lo = seg_off[d]; len = seg_off[d + 1] - lo; }
        double acc[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = 0.0;
        int oid[ALS_CHUNK];                                                    // the other side's ids and the ratings, two chunks ahead; -1 past the end
        float rt[ALS_CHUNK];
        float xv[ALS_CHUNK], rv[ALS_CHUNK];                                    // this lane's dimension of the factor rows and the ratings, one chunk ahead
        auto load_keys = [&](unsigned t) {
#pragma unroll
            for (int k = 0; k < ALS_CHUNK; ++k) {
                const bool in = t + k < len;                                   // (len < 2^31: no wrap)
                oid[k] = in ? (int)(seg_key[(size_t)lo + t + k] >> 32) : -1;
                rt[k] = in ? __int_as_float(seg_val[(size_t)lo + t + k]) : 0.0f;
            }
        };
        auto load_rows = [&]() {
#pragma unroll
            for (int k = 0; k < ALS_CHUNK; ++k) {
                xv[k] = (oid[k] >= 0 && gl < rank) ? src[(size_t)oid[k] * src_stride + gl] : 0.0f;
                rv[k] = rt[k];
            }
        };
        load_keys(0u);
        load_rows();
        load_keys((unsigned)ALS_CHUNK);
        for (unsigned t = 0; __any(t < len); t += ALS_CHUNK) {
#pragma unroll
            for (int k = 0; k < ALS_CHUNK; ++k) {
                my_stage[k * ALS_SLOTS + gl] = (double)xv[k];
                if (gl == 0) my_stage[k * ALS_SLOTS + ALS_MAX_RANK] = (double)rv[k];
            }
            load_rows();
            load_keys(t + 2u * ALS_CHUNK);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < ALS_CHUNK; ++k) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[c] = __builtin_fma(my_stage[k * ALS_SLOTS + pi[c]], my_stage[k * ALS_SLOTS + pj[c]], acc[c]);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) my_system[gl + ALS_G * c] = acc[c];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (live && gl == 0) {
            bool ok = len > 0;
            if (ok) {
                const double lam = (double)len * reg;
                for (int j = 0; j < rank; ++j) my_system[j * (j + 1) / 2 + j] = my_system[j * (j + 1) / 2 + j] + lam;
                ok = als_cholesky_solve(my_system, my_system + tri, rank);
                if (!ok) atomicMin(err, fail_kind << 32 | (unsigned long long)d);
            }
            for (int i = 0; i < rank; ++i) dst[(size_t)d * dst_stride + i] = ok ? (float)my_system[tri + i] : 0.0f;   // a row without ratings: zeros
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// ALSModel's score: the float32 dot in index order, every product and every sum rounded on its own; NaN (Spark's cold start) when either
// id is outside its table or has no factor
__device__ inline float als_dot(const float* __restrict__ u, const float* __restrict__ v, int rank) {
#pragma clang fp contract(off)
    float acc = 0.0f;
    for (int d = 0; d < rank; ++d) {
        const float prod = u[d] * v[d];
        acc = acc + prod;
    }
    return acc;
}

__global__ __launch_bounds__(ALS_THREADS) void k_als_predict(long long n, const int* __restrict__ user, const int* __restrict__ item, const float* __restrict__ user_factors,
                                                             int user_stride, const unsigned char* __restrict__ user_has, const float* __restrict__ item_factors,
                                                             int item_stride, const unsigned char* __restrict__ item_has, int n_users, int n_items, int rank,
                                                             float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * ALS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * ALS_THREADS) {
        const int u = user[i], m = item[i];
        float s = __uint_as_float(0x7fc00000u);
        if (u >= 0 && u < n_users && m >= 0 && m < n_items && user_has[u] && item_has[m])
            s = als_dot(user_factors + (size_t)u * user_stride, item_factors + (size_t)m * item_stride, rank);
        out[i] = s;
    }
}
