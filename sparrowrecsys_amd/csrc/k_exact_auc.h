// k_exact_auc.h -- the exact areas under the ROC and the PR curve over every distinct score (Spark's BinaryClassificationMetrics, as
// offline/spark/evaluate/Evaluator.scala of the reference calls it), from float32 scores and labels that lie in device memory.
// sparrowrecsys_amd/metrics.py exact_auc_host is the DEFINITION; these kernels give its bits: every count is an
// integer, the ROC numerator a 64-bit integer sum, and the PR sum is added in the definition's order -- runs of EA_PR_RUN consecutive
// groups, each from +0.0 in group order, then the run sums from +0.0 in run order.  No floating-point atomic anywhere; the double
// arithmetic is written with plain operators under `#pragma clang fp contract(off)` (every operation rounded on its own; `/` is hipcc's
// correctly rounded sequence), as in k_catalog.h and k_train.h.
// Included by sparrow_metrics.hip inside the unit's private namespace, after k_segments.h (FE_THREADS, the scan and the segment sort).
//   k_ea_count     per row: validate (error word), the 32-bit key, count the key's bin
//   (seg_scan)     counts -> bin offsets
//   k_ea_gate      the sort's gate word: 1 when the error word is clean
//   k_ea_scatter   per row: (key << 1 | positive, row) to the bin's segment at an atomic cursor
//   k_ea_sort_short, then the long segments' chunked sort and merge passes (k_segments.h): every bin that holds more than one score, by
//                  (key, positive, row) -- the sort keys are distinct, as the merge by rank needs them.  A bin of one score keeps its
//                  arrival order, which no count can see
//   k_ea_flags     per sorted place: group start, positive -> two arrays that (seg_scan) turns into running counts
//   k_ea_groups    per group end: (threshold, tp, fp) to the compact table
//   k_ea_roc       per group: neg_g (2 tp_{g-1} + pos_g), a 64-bit integer sum (wave, workgroup, one integer atomic)
//   k_ea_pr_runs   one wave per run of EA_PR_RUN groups: the terms, added in group order
//   k_ea_finish    one wave: the run sums in run order, the two divisions, the result
// Every kernel returns at once when the error word is set (EA_CLEAN = no error), so a failed call changes no output.
//
// The key: a finite float32 s, -0.0 taken as +0.0, with bits u -> u ^ 0x7fffffff when s >= 0, u when s < 0.  Ascending keys are
// descending scores: the largest finite float32 has key 0x00800000, +0.0 has 0x7fffffff, the most negative finite 0xff7fffff.

static constexpr int EA_PR_RUN = 1024;                 // metrics.PR_RUN: part of the definition
static constexpr unsigned long long EA_CLEAN = ~0ull;
static constexpr unsigned long long EA_ERR_SCORE = 1, EA_ERR_LABEL = 2;
enum { EA_W_LONG = 0, EA_W_GATE = 1, EA_W_ROC = 2 /* and 3: one uint64 */, EA_W_COUNT = 4 };

// sprk_exact_auc_result (include/sparrow_hip.h)
struct EaResult { long long n, n_pos, n_groups; unsigned long long roc_numerator; double pr_sum, area_under_roc, area_under_pr; };

__device__ __forceinline__ unsigned ea_key(float s) {
    const unsigned u = __float_as_uint(s);
    if (s == 0.0f) return 0x7fffffffu;                                    // both zeros
    return (u & 0x80000000u) ? u : u ^ 0x7fffffffu;
}
__device__ __forceinline__ float ea_score(unsigned key) { return __uint_as_float((key & 0x80000000u) ? key : key ^ 0x7fffffffu); }
__device__ __forceinline__ bool ea_finite(float s) { return (__float_as_uint(s) & 0x7f800000u) != 0x7f800000u; }

// positive iff label > 0.5 (Spark's BinaryLabelCounter); *finite = false for a float label that is NaN or infinite
__device__ __forceinline__ bool ea_positive(const unsigned char* __restrict__ labels, long long stride, int storage, long long i, bool* finite) {
    const unsigned char* p = labels + i * stride;
    *finite = true;
    switch (storage) {
        case SPRK_COL_F32: { const float v = *reinterpret_cast<const float*>(p); *finite = ea_finite(v); return v > 0.5f; }
        case SPRK_COL_I32: return *reinterpret_cast<const int*>(p) > 0;
        case SPRK_COL_I64: return *reinterpret_cast<const long long*>(p) > 0;
        default: return *p != 0;                                          // SPRK_COL_U8, SPRK_COL_BOOL
    }
}

// one counter per lane, or -- all live lanes on one counter, as with tied scores -- one add of the lane count: -> the counter's value
// before this lane's add (lanes of a shared add get consecutive values)
__device__ __forceinline__ unsigned ea_bump(unsigned* __restrict__ counters, unsigned bin) {
    const unsigned long long live = __ballot(1);
    const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)bin);
    if (__ballot(bin == first) == live) {
        const int leader = __ffsll((long long)live) - 1;
        unsigned base = 0;
        if ((int)__lane_id() == leader) base = atomicAdd(&counters[bin], (unsigned)__popcll(live));
        base = (unsigned)__shfl((int)base, leader, 64);
        return base + (unsigned)__popcll(live & ((1ull << __lane_id()) - 1ull));
    }
    return atomicAdd(&counters[bin], 1u);
}

__global__ __launch_bounds__(FE_THREADS) void k_ea_count(long long n, const float* __restrict__ scores, const unsigned char* __restrict__ labels, int storage, long long stride,
                                                         int shift, unsigned* __restrict__ bin_off, unsigned long long* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const float s = scores[i];
        bool label_finite;
        (void)ea_positive(labels, stride, storage, i, &label_finite);
        if (!ea_finite(s)) { atomicMin(err, EA_ERR_SCORE << 32 | (unsigned long long)i); continue; }
        if (!label_finite) { atomicMin(err, EA_ERR_LABEL << 32 | (unsigned long long)i); continue; }
        (void)ea_bump(bin_off, ea_key(s) >> shift);
    }
}

__global__ void k_ea_gate(unsigned* __restrict__ words, const unsigned long long* __restrict__ err) {
    if (threadIdx.x == 0 && blockIdx.x == 0) words[EA_W_GATE] = *err == EA_CLEAN ? 1u : 0u;
}

__global__ __launch_bounds__(FE_THREADS) void k_ea_scatter(long long n, const float* __restrict__ scores, const unsigned char* __restrict__ labels, int storage, long long stride,
                                                           int shift, const unsigned* __restrict__ bin_off, unsigned* __restrict__ cursor, long long* __restrict__ seg_key,
                                                           int* __restrict__ seg_row, const unsigned long long* __restrict__ err) {
    if (*err != EA_CLEAN) return;
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const unsigned key = ea_key(scores[i]);
        bool label_finite;
        const bool positive = ea_positive(labels, stride, storage, i, &label_finite);
        const unsigned bin = key >> shift;
        const unsigned at = bin_off[bin] + ea_bump(cursor, bin);             // < bin_off[bin + 1] <= n: k_ea_count counted this row
        seg_key[at] = (long long)(((unsigned long long)key << 1) | (positive ? 1ull : 0ull));
        seg_row[at] = (int)i;
    }
}

// k_fe_sort_short (k_segments.h) with one more way out: a bin whose rows all have ONE score needs no order -- the counts of a group do
// not depend on the order inside it -- and is left as it was scattered.  Scores rounded to three digits put tens of thousands of
// equal keys into a bin at 2^24 rows; without this they all take the chunked sort and the merge passes (docs/exact_auc_results.md).
// The workgroup reads the bin 256 keys at a time until two differ; bins longer than EA_TIE_SCAN_MAX go to the long list unread.
// Dynamic LDS: cap x 12 bytes, as k_fe_sort_short.  gate: zero when the error word is set: the whole workgroup returns.
static constexpr unsigned EA_TIE_SCAN_MAX = 1u << 18;
__global__ __launch_bounds__(FE_THREADS) void k_ea_sort_short(int n_bins, int cap, const unsigned* __restrict__ seg_off, long long* __restrict__ seg_key, int* __restrict__ seg_row,
                                                              int* __restrict__ long_list, unsigned* __restrict__ n_long, const unsigned* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ea_lds[];
    if (!*gate) return;
    long long* sts = (long long*)ea_lds;
    int* srow = (int*)(ea_lds + (size_t)cap * 8);
    for (int u = blockIdx.x; u < n_bins; u += gridDim.x) {
        const unsigned base = seg_off[u], len = seg_off[u + 1] - base;
        if (len < 2) continue;
        if (len <= EA_TIE_SCAN_MAX) {
            const long long first = seg_key[base] >> 1;
            int mixed = 0;
            for (unsigned i0 = 0; i0 < len && !mixed; i0 += FE_THREADS) {     // (mixed is the workgroup's: every thread leaves together)
                const unsigned i = i0 + threadIdx.x;
                mixed = __syncthreads_or(i < len && (seg_key[base + i] >> 1) != first);
            }
            if (!mixed) continue;
        }
        if (len <= (unsigned)cap) fe_sort_lds(seg_key + base, seg_row + base, (int)len, sts, srow);
        else if (threadIdx.x == 0) long_list[atomicAdd(n_long, 1u)] = u;        // at most n / (cap + 1) bins: the list holds n / 64 + 1
    }
}

// places 0 .. n (n + 1 of them: the scans' totals land in the last): start[i] = 1 where a group begins, pos[i] = 1 for a positive
__global__ __launch_bounds__(FE_THREADS) void k_ea_flags(long long n, const long long* __restrict__ seg_key, unsigned* __restrict__ start, unsigned* __restrict__ pos,
                                                         const unsigned long long* __restrict__ err) {
    if (*err != EA_CLEAN) return;
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i <= n; i += (long long)gridDim.x * FE_THREADS) {
        unsigned s = 0, p = 0;
        if (i < n) {
            const long long k = seg_key[i];
            s = (i == 0 || (seg_key[i - 1] >> 1) != (k >> 1)) ? 1u : 0u;
            p = (unsigned)(k & 1);
        }
        start[i] = s;
        pos[i] = p;
    }
}

// start / pos after their exclusive scans: start[i + 1] = the groups that begin in places 0 .. i, pos[i + 1] = the positives there.
// The last place of group g (0-based) writes the table's row g: the threshold, tp and fp (cumulative).  thr / tp_out / fp_out: the
// caller's arrays, each may be null.
__global__ __launch_bounds__(FE_THREADS) void k_ea_groups(long long n, const long long* __restrict__ seg_key, const unsigned* __restrict__ start, const unsigned* __restrict__ pos,
                                                          unsigned* __restrict__ g_tp, unsigned* __restrict__ g_fp, float* __restrict__ thr, unsigned* __restrict__ tp_out,
                                                          unsigned* __restrict__ fp_out, const unsigned long long* __restrict__ err) {
    if (*err != EA_CLEAN) return;
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FE_THREADS) {
        const long long k = seg_key[i];
        if (i + 1 < n && (seg_key[i + 1] >> 1) == (k >> 1)) continue;
        const unsigned g = start[i + 1] - 1u;                                 // < n
        const unsigned tp = pos[i + 1], fp = (unsigned)(i + 1) - tp;
        g_tp[g] = tp;
        g_fp[g] = fp;
        if (thr) thr[g] = ea_score((unsigned)((unsigned long long)k >> 1));
        if (tp_out) tp_out[g] = tp;
        if (fp_out) fp_out[g] = fp;
    }
}

// roc_numerator = the sum over groups of neg_g (2 tp_{g-1} + pos_g): at most 2 P N < 2^62
__global__ __launch_bounds__(FE_THREADS) void k_ea_roc(const unsigned* __restrict__ n_groups, const unsigned* __restrict__ g_tp, const unsigned* __restrict__ g_fp,
                                                       unsigned long long* __restrict__ roc, const unsigned long long* __restrict__ err) {
    __shared__ unsigned long long sh[FE_THREADS / 64];
    if (*err != EA_CLEAN) return;
    const long long G = *n_groups;
    unsigned long long acc = 0;
    for (long long g = (long long)blockIdx.x * FE_THREADS + threadIdx.x; g < G; g += (long long)gridDim.x * FE_THREADS) {
        const unsigned long long tp = g_tp[g], fp = g_fp[g], tp0 = g ? g_tp[g - 1] : 0u, fp0 = g ? g_fp[g - 1] : 0u;
        acc += (fp - fp0) * (2ull * tp0 + (tp - tp0));
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < FE_THREADS / 64; ++w) t += sh[w];
        if (t) atomicAdd(roc, t);
    }
}

// term_g = float64(pos_g) (prec_g + prec_{g-1}), prec_g = float64(tp_g) / float64(tp_g + fp_g), prec_{-1} := prec_0; +0.0 past the last group
__device__ __forceinline__ double ea_pr_term(long long g, long long G, const unsigned* __restrict__ g_tp, const unsigned* __restrict__ g_fp) {
#pragma clang fp contract(off)
    if (g >= G) return 0.0;
    const unsigned tp = g_tp[g], fp = g_fp[g];
    const double prec = (double)tp / (double)((unsigned long long)tp + fp);
    double prev = prec;
    unsigned tp0 = 0;
    if (g > 0) {
        tp0 = g_tp[g - 1];
        prev = (double)tp0 / (double)((unsigned long long)tp0 + g_fp[g - 1]);
    }
    return (double)(tp - tp0) * (prec + prev);
}

// v of lanes 0 .. 63 added to acc in lane order: every lane computes the same sum
__device__ __forceinline__ double ea_add_lanes(double acc, double v) {
#pragma clang fp contract(off)
    for (int k = 0; k < 64; ++k) acc = acc + __shfl(v, k, 64);
    return acc;
}

// one wave per run (run r to wave r mod the launch's waves): 64 terms at a time, added in group order from +0.0
__global__ __launch_bounds__(FE_THREADS) void k_ea_pr_runs(const unsigned* __restrict__ n_groups, const unsigned* __restrict__ g_tp, const unsigned* __restrict__ g_fp,
                                                           double* __restrict__ run_sum, const unsigned long long* __restrict__ err) {
    if (*err != EA_CLEAN) return;
    const long long G = *n_groups, runs = (G + EA_PR_RUN - 1) / EA_PR_RUN;
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (FE_THREADS / 64);
    for (long long r = (long long)blockIdx.x * (FE_THREADS / 64) + (threadIdx.x >> 6); r < runs; r += waves) {
        double acc = 0.0;
        for (int c = 0; c < EA_PR_RUN; c += 64) {
            const long long g0 = r * EA_PR_RUN + c;
            if (g0 >= G) break;                                               // (wave-uniform: only +0.0 would follow)
            acc = ea_add_lanes(acc, ea_pr_term(g0 + lane, G, g_tp, g_fp));
        }
        if (lane == 0) run_sum[r] = acc;
    }
}

// one wave: the run sums in run order from +0.0, then the result.  start_total / pos_total: the last elements of the two scans.
__global__ __launch_bounds__(64) void k_ea_finish(long long n, const unsigned* __restrict__ start_total, const unsigned* __restrict__ pos_total, const double* __restrict__ run_sum,
                                                  const unsigned long long* __restrict__ roc, EaResult* __restrict__ result, const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    if (*err != EA_CLEAN) return;
    const long long G = *start_total, runs = (G + EA_PR_RUN - 1) / EA_PR_RUN;
    const int lane = threadIdx.x;
    double acc = 0.0;
    for (long long r0 = 0; r0 < runs; r0 += 64) acc = ea_add_lanes(acc, r0 + lane < runs ? run_sum[r0 + lane] : 0.0);
    if (lane != 0) return;
    const unsigned long long P = *pos_total, N = (unsigned long long)n - P, num = *roc;
    EaResult res;
    res.n = n;
    res.n_pos = (long long)P;
    res.n_groups = G;
    res.roc_numerator = num;
    res.pr_sum = acc;
    res.area_under_roc = N == 0 ? 1.0 : (P == 0 ? 0.0 : (double)num / (double)(2ull * P * N));
    res.area_under_pr = P == 0 ? 0.0 : acc / (double)(2ull * P);
    *result = res;
}
