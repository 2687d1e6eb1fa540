// k_train.h -- Adam training of the graphs "embedding rows + numerics -> Dense/ReLU stack -> one sigmoid" (NeuralCF arch 1, EmbeddingMLP):
// the device side of sparrowrecsys_amd/trainer.py, whose train_host is the DEFINITION of every bit computed here.
//   k_tr_check       ids in their vocabularies, numerics and labels finite: the error word (kind << 32 | row, the least wins)
//   k_tr_count / k_tr_scatter   the schedule: one segment per batch, an entry per (sample, id column) with id >= 0, keyed
//                    (column's first row + id) << 32 | position in the batch; k_segments.h sorts every segment
//   k_tr_invmap      (id column, dimension) -> input row of the first Dense kernel
//   k_tr_step        one workgroup per tile of samples: forward, sigmoid_def, backward; p, dx and the tile's partial dW / db
//   k_tr_dense_adam  per Dense parameter: the tiles' partials added in tile order, then Adam
//   k_tr_table_adam  per (table row, dimension): the row's run in the batch's sorted entries added tile by tile, then Adam (g = 0 for a row
//                    the batch did not touch: Keras' Adam moves every row on every step)
// FP32 VALU by construction: every product and sum is rounded on its own.  This toolchain's __fmul_rn / __fadd_rn are the plain operators
// and its __fsqrt_rn is the approximate instruction, so -- as in k_catalog.h and k_item2vec.h -- the arithmetic is written with operators
// under `#pragma clang fp contract(off)`, and sqrtf and `/` are the correctly rounded sequences (hipcc's default).
// No float atomics; every kernel of a step returns at once when the error word is set, so a failed check changes no parameter.

static constexpr int TR_THREADS = 256;
static constexpr int TR_MAX_COLS = SPRK_TRAIN_MAX_COLS, TR_MAX_LAYERS = SPRK_TRAIN_MAX_LAYERS, TR_MAX_X = SPRK_TRAIN_MAX_X, TR_MAX_WIDTH = SPRK_TRAIN_MAX_WIDTH;
static constexpr unsigned long long TR_ERR_ID = 1, TR_ERR_NUMERIC = 2, TR_ERR_LABEL = 3, TR_CLEAN = ~0ull;

struct TrainDims {                           // a kernel argument, by value (about 1.5 KB)
    int n_cols, n_dense, emb_dim, n_x, n_layers;
    int vocab[TR_MAX_COLS], genre[TR_MAX_COLS];
    long long tab_off[TR_MAX_COLS];          // the column's table in the parameter vector (floats)
    long long row_base[TR_MAX_COLS + 1];     // its first row among all tables' rows
    int width[TR_MAX_LAYERS + 1], fan[TR_MAX_LAYERS + 1];          // the hidden layers, then the head (width 1)
    long long ker_off[TR_MAX_LAYERS + 1], bias_off[TR_MAX_LAYERS + 1];
    long long n_table, n_params;             // floats of all tables (= the first Dense parameter), of everything
    short xcol[TR_MAX_X], xsub[TR_MAX_X];
};

__device__ inline bool tr_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// A value in a 32-bit register of its own (dyn_split.h lone_scalar(), which this unit does not include): hipcc packs `h1 * l2` and `l1 * h2` of
// tr_sigmoid into one v_pk_mul_f32 whose low result takes the HIGH dword of a VGPR src1, the form build() refuses.  A pair built from a
// value that went through this statement has it as the low dword.
__device__ __forceinline__ float tr_lone(float x) {
    asm("" : "+v"(x));
    return x;
}

// trainer.sigmoid_def, operation for operation
__device__ inline float tr_sigmoid(float z) {
#pragma clang fp contract(off)
    const float t = fminf(fmaxf(-z, -87.0f), 87.0f);
    const float n = (t * 1.44269504088896341f + 12582912.0f) - 12582912.0f;
    const float r = (t - n * 0.693359375f) - n * -2.12194440e-4f;
    float q = 1.9875691500e-4f;
    q = q * r + 1.3981999507e-3f;
    q = q * r + 8.3334519073e-3f;
    q = q * r + 4.1665795894e-2f;
    q = q * r + 1.6666665459e-1f;
    q = q * r + 5.0000001201e-1f;
    const float u = (q * r) * r + r;
    const float scale = __uint_as_float((unsigned)((int)n + 127) << 23);
    const float a = 1.0f + scale, b = scale * u;
    const float aa = a - 1.0f;
    const float al = (1.0f - (a - aa)) + (scale - aa);                       // 1 + scale = a + al, exactly
    const float dh = a + b;
    const float bb = dh - a;
    const float dl = ((a - (dh - bb)) + (b - bb)) + al;                      // the denominator = dh + dl
    const float p0 = 1.0f / dh;
    float p = p0;
    if (fabsf(n) <= 100.0f) {                                                // the residual 1 - (dh + dl) p0, its product split exactly (Dekker)
        const float x = dh * p0;
        const float c1 = dh * 4097.0f, c2 = p0 * 4097.0f;
        const float h1 = c1 - (c1 - dh), h2 = c2 - (c2 - p0);
        const float l1 = dh - h1, l2 = tr_lone(p0 - h2);
        const float y = ((h1 * h2 - x) + h1 * l2 + l1 * h2) + l1 * l2;
        const float rr = ((1.0f - x) - y) - dl * p0;
        p = p0 + p0 * rr;
    }
    return z < -87.0f ? 0.0f : p;
}

// trainer.adam_step on one element
__device__ inline void tr_adam(float g, float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, float alpha, float c1, float c2, float eps) {
#pragma clang fp contract(off)
    const float m1 = *m + (g - *m) * c1;
    const float v1 = *v + (g * g - *v) * c2;
    *m = m1;
    *v = v1;
    *w = *w - (alpha * m1) / (sqrtf(v1) + eps);
}

__global__ __launch_bounds__(TR_THREADS) void k_tr_check(long long n, const int* __restrict__ ids, const float* __restrict__ dense, const float* __restrict__ labels,
                                                         TrainDims dm, unsigned long long* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * TR_THREADS) {
        unsigned long long kind = tr_finite(labels[i]) ? 0 : TR_ERR_LABEL;
        for (int f = 0; f < dm.n_dense; ++f)
            if (!tr_finite(dense[i * dm.n_dense + f])) kind = TR_ERR_NUMERIC;
        for (int c = 0; c < dm.n_cols; ++c) {
            const int id = ids[i * dm.n_cols + c];
            if (id < (dm.genre[c] ? -1 : 0) || id >= dm.vocab[c]) kind = TR_ERR_ID;
        }
        if (kind) atomicMin(err, kind << 32 | (unsigned long long)i);
    }
}

// entries per batch: off[b] += 1 per (position, column) with id >= 0
__global__ __launch_bounds__(TR_THREADS) void k_tr_count(long long n, int batch, const int* __restrict__ ids, const int* __restrict__ order, int n_cols,
                                                         unsigned* __restrict__ off) {
    const long long total = n * n_cols;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TR_THREADS) {
        const long long i = e / n_cols;
        const int c = (int)(e - i * n_cols);
        const long long r = order ? order[i] : i;
        if (ids[r * n_cols + c] >= 0) atomicAdd(&off[i / batch], 1u);
    }
}

// the entries, at an atomic cursor inside their batch's segment (the sort orders them: the result does not depend on the arrival)
__global__ __launch_bounds__(TR_THREADS) void k_tr_scatter(long long n, int batch, const int* __restrict__ ids, const int* __restrict__ order, TrainDims dm,
                                                           const unsigned* __restrict__ off, unsigned* __restrict__ cursor, long long* __restrict__ key,
                                                           int* __restrict__ val, const unsigned long long* __restrict__ err) {
    if (*err != TR_CLEAN) return;                                            // (an id outside its table would key another table's row)
    const long long total = n * dm.n_cols;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TR_THREADS) {
        const long long i = e / dm.n_cols;
        const int c = (int)(e - i * dm.n_cols);
        const long long r = order ? order[i] : i;
        const int id = ids[r * dm.n_cols + c];
        if (id < 0) continue;
        const long long b = i / batch;
        const unsigned slot = off[b] + atomicAdd(&cursor[b], 1u);           // < off[b + 1]: k_tr_count counted this entry
        key[slot] = (dm.row_base[c] + id) << 32 | (i - b * batch);
        val[slot] = c;
    }
}

__global__ __launch_bounds__(TR_THREADS) void k_tr_invmap(TrainDims dm, int* __restrict__ inv) {
    const int cd = dm.n_cols * dm.emb_dim;
    for (int e = threadIdx.x; e < cd; e += TR_THREADS) inv[e] = -1;
    __syncthreads();
    for (int k = threadIdx.x; k < dm.n_x; k += TR_THREADS)
        if (dm.xcol[k] >= 0) inv[dm.xcol[k] * dm.emb_dim + dm.xsub[k]] = k;
}

// One tile of one batch.  Dynamic LDS, floats: x [tile][n_x], a_l [tile][width_l] per hidden layer, two gradient buffers [tile][wide].
// first = the batch's first position, nb = its rows; p_out / dx are indexed by the position in the batch; partial = [tiles][n_params - n_table].
__global__ __launch_bounds__(TR_THREADS) void k_tr_step(TrainDims dm, const int* __restrict__ ids, const float* __restrict__ dense, const float* __restrict__ labels,
                                                        const int* __restrict__ order, long long first, int nb, int tile, int wide, const float* __restrict__ params,
                                                        float* __restrict__ p_out, float* __restrict__ dx, float* __restrict__ partial,
                                                        const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float tr_lds[];
    if (*err != TR_CLEAN) return;
    const int t0 = blockIdx.x * tile;
    const int cnt = nb - t0 < tile ? nb - t0 : tile;                        // >= 1: the grid is ceil(nb / tile)
    const int L = dm.n_layers, n_x = dm.n_x;
    float* act[TR_MAX_LAYERS + 1];
    act[0] = tr_lds;
    {
        float* at = tr_lds + (size_t)tile * n_x;
        for (int l = 0; l < L; ++l) { act[l + 1] = at; at += (size_t)tile * dm.width[l]; }
    }
    float* g0 = tr_lds + (size_t)tile * n_x;
    for (int l = 0; l < L; ++l) g0 += (size_t)tile * dm.width[l];
    float* g1 = g0 + (size_t)tile * wide;

    for (int e = threadIdx.x; e < cnt * n_x; e += TR_THREADS) {
        const int i = e / n_x, k = e - i * n_x;
        const long long pos = first + t0 + i;
        const long long r = order ? order[pos] : pos;
        const int c = dm.xcol[k], s = dm.xsub[k];
        float x;
        if (c < 0) x = dense[r * dm.n_dense + s];
        else {
            const int id = ids[r * dm.n_cols + c];
            x = id >= 0 ? params[dm.tab_off[c] + (long long)id * dm.emb_dim + s] : 0.0f;
        }
        act[0][e] = x;
    }
    __syncthreads();

    for (int l = 0; l < L; ++l) {
        const int fan = dm.fan[l], H = dm.width[l];
        const float* __restrict__ W = params + dm.ker_off[l];
        const float* __restrict__ bias = params + dm.bias_off[l];
        const float* in = act[l];
        float* out = act[l + 1];
        for (int e = threadIdx.x; e < cnt * H; e += TR_THREADS) {
            const int i = e / H, j = e - i * H;
            float z = 0.0f;
            for (int k = 0; k < fan; ++k) z = z + in[i * fan + k] * W[k * H + j];
            z = z + bias[j];
            out[e] = z > 0.0f ? z : 0.0f;
        }
        __syncthreads();
    }
    {
        const int fan = dm.fan[L];
        const float* __restrict__ W = params + dm.ker_off[L];
        const float bh = params[dm.bias_off[L]];
        const float* in = act[L];
        const float fn = (float)nb;
        for (int i = threadIdx.x; i < cnt; i += TR_THREADS) {
            float z = 0.0f;
            for (int k = 0; k < fan; ++k) z = z + in[i * fan + k] * W[k];
            z = z + bh;
            const float p = tr_sigmoid(z);
            const long long pos = first + t0 + i;
            p_out[t0 + i] = p;
            g0[i] = (p - labels[order ? order[pos] : pos]) / fn;
        }
        __syncthreads();
    }

    const long long ndp = dm.n_params - dm.n_table;
    float* __restrict__ mine = partial + (long long)blockIdx.x * ndp;
    float* dz = g0;
    float* nx = g1;
    for (int l = L; l >= 0; --l) {
        const int fan = dm.fan[l], H = dm.width[l];
        const float* __restrict__ W = params + dm.ker_off[l];
        const float* a = act[l];
        for (int e = threadIdx.x; e < fan * H; e += TR_THREADS) {
            const int k = e / H, j = e - k * H;
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + a[i * fan + k] * dz[i * H + j];
            mine[dm.ker_off[l] - dm.n_table + e] = s;
        }
        for (int j = threadIdx.x; j < H; j += TR_THREADS) {
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + dz[i * H + j];
            mine[dm.bias_off[l] - dm.n_table + j] = s;
        }
        for (int e = threadIdx.x; e < cnt * fan; e += TR_THREADS) {
            const int i = e / fan, k = e - i * fan;
            float s = 0.0f;
            for (int j = 0; j < H; ++j) s = s + W[k * H + j] * dz[i * H + j];
            nx[e] = (l == 0 || a[e] > 0.0f) ? s : 0.0f;
        }
        __syncthreads();
        float* t = dz; dz = nx; nx = t;
    }
    for (int e = threadIdx.x; e < cnt * n_x; e += TR_THREADS) dx[(long long)t0 * n_x + e] = dz[e];
}

__global__ __launch_bounds__(TR_THREADS) void k_tr_dense_adam(TrainDims dm, int tiles, const float* __restrict__ partial, float* __restrict__ params, float* __restrict__ m,
                                                              float* __restrict__ v, const float* __restrict__ alphas, long long step, float c1, float c2, float eps,
                                                              const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    if (*err != TR_CLEAN) return;
    const long long ndp = dm.n_params - dm.n_table;
    const float alpha = alphas[step];
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < ndp; e += (long long)gridDim.x * TR_THREADS) {
        float g = 0.0f;
        int t = 0;
        for (; t + 8 <= tiles; t += 8) {                                     // eight loads in flight, added in tile order
            float q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = partial[(long long)(t + u) * ndp + e];
#pragma unroll
            for (int u = 0; u < 8; ++u) g = g + q[u];
        }
        for (; t < tiles; ++t) g = g + partial[(long long)t * ndp + e];
        tr_adam(g, params + dm.n_table + e, m + dm.n_table + e, v + dm.n_table + e, alpha, c1, c2, eps);
    }
}

// seg = [lo, hi) of the batch's entries, sorted by (row, position)
__global__ __launch_bounds__(TR_THREADS) void k_tr_table_adam(TrainDims dm, int tile, const unsigned* __restrict__ off, long long b, const long long* __restrict__ key,
                                                              const int* __restrict__ inv, const float* __restrict__ dx, float* __restrict__ params,
                                                              float* __restrict__ m, float* __restrict__ v, const float* __restrict__ alphas, long long step, float c1,
                                                              float c2, float eps, const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    if (*err != TR_CLEAN) return;
    const long long seg_lo = off[b], seg_hi = off[b + 1];
    const float alpha = alphas[step];
    const int D = dm.emb_dim;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < dm.n_table; e += (long long)gridDim.x * TR_THREADS) {
        const long long row = e / D;
        const int d = (int)(e - row * D);
        int c = 0;
        while (c + 1 < dm.n_cols && row >= dm.row_base[c + 1]) ++c;
        const int k = inv[c * D + d];
        long long lo = seg_lo, hi = seg_hi;
        const long long want = row << 32;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (key[mid] < want) lo = mid + 1; else hi = mid;
        }
        float g = 0.0f, s = 0.0f;
        int cur = -1;
        if (k >= 0)
            for (; lo < seg_hi; ++lo) {
                const long long kk = key[lo];
                if ((kk >> 32) != row) break;
                const int pos = (int)(kk & 0xffffffffll);
                const int t = pos / tile;
                if (t != cur) {
                    if (cur >= 0) g = g + s;
                    s = 0.0f;
                    cur = t;
                }
                s = s + dx[(long long)pos * dm.n_x + k];
            }
        if (cur >= 0) g = g + s;
        tr_adam(g, params + e, m + e, v + e, alpha, c1, c2, eps);
    }
}
