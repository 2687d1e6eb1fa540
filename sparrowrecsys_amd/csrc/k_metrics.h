// k_metrics.h -- `model.evaluate`'s accumulators in device memory (DeepFM.py:117-126: binary cross-entropy, accuracy at 0.5 and the two
// 200-threshold Keras AUCs): one update folds n float32 scores and their labels into a caller-owned state without a score or a label
// leaving the device.  sparrowrecsys_amd/metrics.py stays the definition of every number; everything that is a count has its bits.
// Included inside the kernels' namespace by sparrow_metrics.hip, the library's unit for these kernels and their C ABI.
//
// The state, as 8-byte words (include/sparrow_hip.h documents it: Python reads it back):
//   [0] T   [1] n   [2] n_correct   [3] loss_sum (double)   pos[T + 1]   neg[T + 1]   th[T] (double)   partial[MT_MAX_GRID] (double)
// Per sample, with p = (double)score and y = (double)label:
//   bucket    = the number of thresholds t in th[0..T) with !(p <= t): 0 .. T, NaN in T.  th is metrics._confusion's table, and
//               tp[i] = sum of pos[b] over b > i, fp[i] likewise over neg.  No threshold is a float32, so the index guess
//               (int)(p (T - 1)) + 1 is corrected against the double table (a copy in LDS) before it counts.
//   n_correct += ((p > 0.5 ? 1.0 : 0.0) == y)
//   loss_sum  += -(y log(pc) + (1 - y) log(1 - pc)), pc = p clipped to [1e-7, 1 - 1e-7] (a NaN stays a NaN, as np.clip keeps it)
//
// k_metrics_update: a capped grid of 256-thread workgroups walks slices of MT_SLICE samples (slice s to workgroup s mod grid); a lane
// reads four consecutive scores as one 16-byte load where the array allows it, the labels with their own byte stride.  Counts go to
// ONE workgroup histogram of 32-bit counters in LDS (a wave whose 64 lanes hold one bucket -- all-equal scores -- adds its lane
// count once); every nonzero counter is flushed once per workgroup with a 64-bit integer atomic, so the counts do not depend on the
// order of arrival.  The host hands a launch at most MT_LAUNCH_MAX samples, which keeps a workgroup's counters below 2^21.  The loss
// takes NO floating-point atomic: a lane sums its samples in index order, the wave and the workgroup in a fixed tree, and the
// workgroup stores ONE double into partial[blockIdx.x]; k_metrics_finish (one workgroup, next on the stream) adds partial[0 .. G) in
// index order to the running sum.  The loss word after an update is a function of (the word before, the inputs, n) alone.
// Both kernels take T from word 0 of the state, ON THE DEVICE (the host never reads the state), and check it against the size the
// caller gave before they touch anything else; the launch's LDS is therefore sized for MT_MAX_T (16 KB), whatever T turns out to be.

extern __shared__ __attribute__((aligned(16))) unsigned char mt_smem[];

#define MT_THREADS 256
#define MT_SLICE 4096                                  // samples of one slice: 4 per lane, 4 rounds
#define MT_MAX_GRID 1024                               // workgroups of one launch = doubles of the partial array
#define MT_LAUNCH_MAX (1ll << 31)                      // samples of one launch: at most 2^21 per workgroup
#define MT_MAX_T 1024                                  // SPRK_METRICS_MAX_THRESHOLDS

__host__ __device__ __forceinline__ size_t mt_state_words(int T) { return 4 + 2 * ((size_t)T + 1) + (size_t)T + MT_MAX_GRID; }
__host__ __device__ __forceinline__ size_t mt_lds_bytes(int T) { return 8 * (size_t)T + 4 * 2 * ((size_t)T + 1) + 8 + 8 * (MT_THREADS / 64); }

// zero the counters and write the threshold table: th[0] = 0 - 1e-7, th[i] = i / (T - 1), th[T - 1] = 1 + 1e-7 (IEEE double
// division of two exact integers: the bits of Python's (i + 1) / (num_thresholds - 1))
static __global__ __launch_bounds__(MT_THREADS) void k_metrics_reset(unsigned long long* __restrict__ state, int T) {
    const size_t words = mt_state_words(T);
    double* th = reinterpret_cast<double*>(state + 4 + 2 * ((size_t)T + 1));
    for (size_t w = threadIdx.x; w < words; w += MT_THREADS) {
        const size_t i = w - (4 + 2 * ((size_t)T + 1));                  // (wraps below the table: not < T then)
        if (w == 0) state[w] = (unsigned long long)T;
        else if (i < (size_t)T) th[i] = i == 0 ? 0.0 - 1e-7 : (i == (size_t)T - 1 ? 1.0 + 1e-7 : (double)(long long)i / (double)(T - 1));
        else state[w] = 0ull;
    }
}

__device__ __forceinline__ double mt_label(const unsigned char* __restrict__ labels, long long stride, int storage, long long i) {
    const unsigned char* p = labels + i * stride;
    switch (storage) {
        case SPRK_COL_F32: return (double)*reinterpret_cast<const float*>(p);
        case SPRK_COL_I32: return (double)*reinterpret_cast<const int*>(p);
        case SPRK_COL_I64: return (double)*reinterpret_cast<const long long*>(p);
        case SPRK_COL_U8: return (double)*p;
        default: return *p ? 1.0 : 0.0;                                   // SPRK_COL_BOOL
    }
}

// T as reset wrote it into the state this launch was given `words` 8-byte words of; 0 (the launch does nothing) for a state that was
// never reset or is shorter than its own T needs: nothing outside the caller's `words` is ever touched
__device__ __forceinline__ int mt_state_T(const unsigned long long* __restrict__ state, unsigned long long words) {
    const unsigned long long T = state[0];
    return T >= 2 && T <= MT_MAX_T && mt_state_words((int)T) <= words ? (int)T : 0;
}

static __global__ __launch_bounds__(MT_THREADS) void k_metrics_update(unsigned long long* __restrict__ state, unsigned long long words,
                                                               const float* __restrict__ scores, int vec4, const unsigned char* __restrict__ labels,
                                                               int storage, long long stride, long long n) {
    const int T = mt_state_T(state, words);
    if (T == 0) return;
    double* s_th = reinterpret_cast<double*>(mt_smem);                       // [T]
    unsigned* s_hist = reinterpret_cast<unsigned*>(s_th + T);             // pos[T + 1], neg[T + 1]
    unsigned* s_correct = s_hist + 2 * (T + 1);                           // (+ one pad word)
    double* s_loss = reinterpret_cast<double*>(s_correct + 2);            // [waves]
    const int tid = threadIdx.x;
    const double* th = reinterpret_cast<const double*>(state + 4 + 2 * ((size_t)T + 1));
    for (int i = tid; i < T; i += MT_THREADS) s_th[i] = th[i];
    for (int i = tid; i < 2 * (T + 1) + 2; i += MT_THREADS) s_hist[i] = 0u;
    __syncthreads();
    const double scale = (double)(T - 1);
    double loss = 0.0;
    unsigned correct = 0;
    const long long slices = (n + MT_SLICE - 1) / MT_SLICE;
    for (long long s = blockIdx.x; s < slices; s += gridDim.x) {
        for (int r = 0; r < MT_SLICE / (4 * MT_THREADS); ++r) {
            const long long i0 = s * MT_SLICE + ((long long)r * MT_THREADS + tid) * 4;
            if (i0 >= n) break;
            const int m = n - i0 < 4 ? (int)(n - i0) : 4;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (vec4 && m == 4) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(scores + i0);
                v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
            } else {
                for (int k = 0; k < m; ++k) v[k] = scores[i0 + k];
            }
            for (int k = 0; k < m; ++k) {
                const double p = (double)v[k];
                const double y = mt_label(labels, stride, storage, i0 + k);
                // bucket: a guess from p (T - 1), then the table decides
                int b = T;
                if (p == p) {
                    double x = p * scale;
                    x = x < 0.0 ? 0.0 : (x > (double)(T - 1) ? (double)(T - 1) : x);
                    b = (int)x + 1;
                    while (b < T && !(p <= s_th[b])) ++b;
                    while (b > 0 && p <= s_th[b - 1]) --b;
                }
                const int slot = (y != 0.0 ? 0 : T + 1) + b;
                // all-equal scores: the wave's lanes hold one slot, one of them adds the lane count
                const unsigned long long live = __ballot(1);
                const int first = __builtin_amdgcn_readfirstlane(slot);
                if (__ballot(slot == first) == live) {
                    if (__lane_id() == (unsigned)__ffsll((long long)live) - 1u) atomicAdd(&s_hist[slot], (unsigned)__popcll(live));
                } else {
                    atomicAdd(&s_hist[slot], 1u);
                }
                correct += ((p > 0.5 ? 1.0 : 0.0) == y) ? 1u : 0u;
                const double pc = p < 1e-7 ? 1e-7 : (p > 1.0 - 1e-7 ? 1.0 - 1e-7 : p);       // (NaN stays)
                if (y == 1.0) loss += -log(pc);                           // -(1 log(pc) + 0 log(1 - pc)): the same bits, one log
                else if (y == 0.0) loss += -log(1.0 - pc);
                else loss += -(y * log(pc) + (1.0 - y) * log(1.0 - pc));
            }
        }
    }
    // the loss: lanes -> wave (fixed tree) -> workgroup (wave order) -> partial[blockIdx.x]
    for (int off = 32; off > 0; off >>= 1) {
        loss += __shfl_down(loss, off, 64);
        correct += __shfl_down(correct, off, 64);
    }
    if ((tid & 63) == 0) {
        s_loss[tid >> 6] = loss;
        if (correct) atomicAdd(s_correct, correct);
    }
    __syncthreads();
    if (tid == 0) {
        double t = s_loss[0];
        for (int w = 1; w < MT_THREADS / 64; ++w) t += s_loss[w];
        reinterpret_cast<double*>(state)[4 + 2 * ((size_t)T + 1) + (size_t)T + blockIdx.x] = t;
        if (*s_correct) atomicAdd(state + 2, (unsigned long long)*s_correct);
    }
    for (int i = tid; i < 2 * (T + 1); i += MT_THREADS) {
        const unsigned c = s_hist[i];
        if (c) atomicAdd(state + 4 + i, (unsigned long long)c);
    }
}

// partial[0 .. G) in index order, then onto the running sum; n += the launch's samples
static __global__ __launch_bounds__(MT_THREADS) void k_metrics_finish(unsigned long long* __restrict__ state, unsigned long long words, int G, long long n) {
    const int T = mt_state_T(state, words);
    if (T == 0) return;
    double* s_part = reinterpret_cast<double*>(mt_smem);                     // [G]
    const double* part = reinterpret_cast<const double*>(state) + 4 + 2 * ((size_t)T + 1) + (size_t)T;
    for (int i = threadIdx.x; i < G; i += MT_THREADS) s_part[i] = part[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < G; ++i) t += s_part[i];
        reinterpret_cast<double*>(state)[3] += t;
        state[1] += (unsigned long long)n;
    }
}
