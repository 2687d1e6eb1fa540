// k_train_tower.h -- Adam training of the two-tower NeuralCF (arch 2: a Dense/ReLU tower over the movie row, one over the user row, their dot, one Dense
// unit and a sigmoid), and the towers' output vectors for whole tables: the device side of sparrowrecsys_amd/trainer_tower.py, whose train_host and
// tower_rows_host are the DEFINITION of every bit computed here.  The schedule is k_train.h's: k_tr_check, k_tr_count,
// k_tr_scatter and the k_segments.h sort give, per batch, one sorted run of positions per (column, id).  Per step:
//   k_tw_step        one workgroup per tile of samples: both towers forward side by side, the dot, sigmoid_def, backward; p, per position dx [2 emb_dim]
//                    (movie row's gradient, then user row's) and the tile's partial sums of every Dense parameter
//   k_tf_dense_adam  (k_train_fm.h) per Dense parameter: the tiles' partials added in tile order, then Adam
//   k_tw_table_adam  per (table row, dimension): the row's run added tile by tile, then Adam (g = 0 for a row the batch did not touch); k_tr_table_adam
//                    for two columns whose input rows are their own elements, storing through tf_adam
//   k_tw_rows        every row of one table through its tower, by the forward's own statements: the item or user vectors
// Arithmetic as in k_train.h: FP32 VALU, operators under `#pragma clang fp contract(off)`, tr_sigmoid and tr_adam (through tf_adam: a NaN that reaches
// p, a parameter, m or v is stored as 0x7fc00000 -- a dot can overflow, and 0 * inf follows); no float atomics; every kernel of a step returns at once
// when the error word is set.  The LDS carves and every per-layer offset come in TowerDims, so no kernel indexes an array of its own by a layer.

static constexpr int TW_MAX_LAYERS = SPRK_TRAIN_TOWER_MAX_LAYERS, TW_MAX_WIDTH = SPRK_TRAIN_TOWER_MAX_WIDTH, TW_MAX_DIM = SPRK_TRAIN_TOWER_MAX_DIM;

struct TowerDims {                           // a kernel argument, by value
    int emb_dim, n_layers, wide;             // wide = 2 x the widest hidden layer: a gradient buffer holds both towers' side by side
    int vocab[2];                            // movieId, userId
    int width[TW_MAX_LAYERS], fan[TW_MAX_LAYERS];
    long long tab_off[2];                    // the side's table in the parameter vector (floats)
    long long ker_off[2][TW_MAX_LAYERS], bias_off[2][TW_MAX_LAYERS];        // [0] the item tower, [1] the user tower
    long long head_ker, head_bias;
    long long n_table, n_params;             // floats of both tables (= the first Dense parameter), of everything
    // the carves of k_tw_step's LDS for the launch's tile, in floats from its start, each a multiple of 4
    int lds_act[2][TW_MAX_LAYERS], lds_dot, lds_dl, lds_g0, lds_g1;
};

// One tile of one batch.  Dynamic LDS, floats: x [tile][2 D] (movie row, user row), per tower and layer a [tile][width], dot [tile], dlogit [tile], two
// gradient buffers [2][tile][widest layer].  first = the batch's first position, nb = its rows; p_out / dx are indexed by the position in the batch;
// partial = [tiles][n_params - n_table].  A layer's item and user units share one loop; each unit's own k loop fixes its rounding.
__global__ __launch_bounds__(TR_THREADS) void k_tw_step(TowerDims dm, const int* __restrict__ ids, const float* __restrict__ labels, const int* __restrict__ order,
                                                        long long first, int nb, int tile, const float* __restrict__ params, float* __restrict__ p_out,
                                                        float* __restrict__ dx, float* __restrict__ partial, const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float tw_lds[];
    if (*err != TR_CLEAN) return;
    const int t0 = blockIdx.x * tile;
    const int cnt = nb - t0 < tile ? nb - t0 : tile;                        // >= 1: the grid is ceil(nb / tile)
    const int D = dm.emb_dim, D2 = 2 * D, L = dm.n_layers, HL = dm.width[L - 1];
    float* x = tw_lds;
    float* dot = tw_lds + dm.lds_dot;
    float* dl = tw_lds + dm.lds_dl;

    for (int e = threadIdx.x; e < cnt * D2; e += TR_THREADS) {
        const int i = e / D2, k = e - i * D2;
        const int s = k >= D ? 1 : 0;
        const long long pos = first + t0 + i;
        const long long r = order ? order[pos] : pos;
        const int id = ids[r * 2 + s];
        x[e] = params[dm.tab_off[s] + (long long)id * D + (k - s * D)];
    }
    __syncthreads();

    for (int l = 0; l < L; ++l) {
        const int fan = dm.fan[l], H = dm.width[l], half = cnt * H;
        const int stride = l ? fan : D2;
        for (int e = threadIdx.x; e < 2 * half; e += TR_THREADS) {
            const int s = e >= half ? 1 : 0;
            const int r = e - s * half;
            const int i = r / H, j = r - i * H;
            const float* in = l ? tw_lds + dm.lds_act[s][l - 1] : x + s * D;
            const float* __restrict__ W = params + dm.ker_off[s][l];
            float z = 0.0f;
            for (int k = 0; k < fan; ++k) z = z + in[i * stride + k] * W[k * H + j];
            z = z + params[dm.bias_off[s][l] + j];
            tw_lds[dm.lds_act[s][l] + r] = z > 0.0f ? z : 0.0f;
        }
        __syncthreads();
    }
    const float* it = tw_lds + dm.lds_act[0][L - 1];
    const float* us = tw_lds + dm.lds_act[1][L - 1];
    const float hk = params[dm.head_ker], bh = params[dm.head_bias];
    {
        const float fn = (float)nb;
        for (int i = threadIdx.x; i < cnt; i += TR_THREADS) {
            const long long pos = first + t0 + i;
            float s = 0.0f;
            for (int d = 0; d < HL; ++d) s = s + it[i * HL + d] * us[i * HL + d];
            dot[i] = s;
            float z = 0.0f;
            z = z + s * hk;
            z = z + bh;
            const float p = tf_canon(z != z ? z : tr_sigmoid(z));
            p_out[t0 + i] = p;
            dl[i] = (p - labels[order ? order[pos] : pos]) / fn;
        }
        __syncthreads();
    }

    const long long nt = dm.n_table;
    float* __restrict__ mine = partial + (long long)blockIdx.x * (dm.n_params - nt);
    float* dz = tw_lds + dm.lds_g0;                                          // [2][cnt][H]: the item tower's, then the user tower's
    float* nx = tw_lds + dm.lds_g1;
    {   // the head: its two gradients, and each tower's last gradient -- ddot times the OTHER tower's output -- under its own ReLU mask
        if (threadIdx.x == 0) {
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + dot[i] * dl[i];
            mine[dm.head_ker - nt] = s;
        }
        if (threadIdx.x == TR_THREADS / 2) {
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + dl[i];
            mine[dm.head_bias - nt] = s;
        }
        const int half = cnt * HL;
        for (int e = threadIdx.x; e < 2 * half; e += TR_THREADS) {
            const int s = e >= half ? 1 : 0;
            const int r = e - s * half;
            const int i = r / HL;
            float dd = 0.0f;
            dd = dd + hk * dl[i];
            const float own = s ? us[r] : it[r], other = s ? it[r] : us[r];
            dz[e] = own > 0.0f ? dd * other : 0.0f;
        }
        __syncthreads();
    }
    for (int l = L - 1; l >= 0; --l) {
        const int fan = dm.fan[l], H = dm.width[l], half = cnt * H;
        const int stride = l ? fan : D2;
        for (int e = threadIdx.x; e < 2 * fan * H; e += TR_THREADS) {
            const int s = e >= fan * H ? 1 : 0;
            const int r = e - s * fan * H;
            const int k = r / H, j = r - k * H;
            const float* a = l ? tw_lds + dm.lds_act[s][l - 1] : x + s * D;
            const float* g = dz + s * half;
            float sum = 0.0f;
            for (int i = 0; i < cnt; ++i) sum = sum + a[i * stride + k] * g[i * H + j];
            mine[dm.ker_off[s][l] - nt + r] = sum;
        }
        for (int e = threadIdx.x; e < 2 * H; e += TR_THREADS) {
            const int s = e >= H ? 1 : 0;
            const int j = e - s * H;
            const float* g = dz + s * half;
            float sum = 0.0f;
            for (int i = 0; i < cnt; ++i) sum = sum + g[i * H + j];
            mine[dm.bias_off[s][l] - nt + j] = sum;
        }
        const int below = cnt * fan;
        for (int e = threadIdx.x; e < 2 * below; e += TR_THREADS) {
            const int s = e >= below ? 1 : 0;
            const int r = e - s * below;
            const int i = r / fan, k = r - i * fan;
            const float* __restrict__ W = params + dm.ker_off[s][l];
            const float* g = dz + s * half;
            float sum = 0.0f;
            for (int j = 0; j < H; ++j) sum = sum + W[k * H + j] * g[i * H + j];
            if (l) nx[e] = tw_lds[dm.lds_act[s][l - 1] + r] > 0.0f ? sum : 0.0f;
            else dx[(long long)(t0 + i) * D2 + s * D + k] = sum;
        }
        __syncthreads();
        float* t = dz; dz = nx; nx = t;
    }
}

// [off[b], off[b + 1]) = the batch's entries, sorted by (row, position); element e is (row, dimension) of the movie table, then of the user table;
// dx = [position][2 emb_dim]
__global__ __launch_bounds__(TR_THREADS) void k_tw_table_adam(TowerDims dm, int tile, const unsigned* __restrict__ off, long long b, const long long* __restrict__ key,
                                                              const float* __restrict__ dx, float* __restrict__ params, float* __restrict__ m, float* __restrict__ v,
                                                              const float* __restrict__ alphas, long long step, float c1, float c2, float eps,
                                                              const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    if (*err != TR_CLEAN) return;
    const long long seg_lo = off[b], seg_hi = off[b + 1];
    const float alpha = alphas[step];
    const int D = dm.emb_dim;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < dm.n_table; e += (long long)gridDim.x * TR_THREADS) {
        const long long row = e / D;
        const int d = (int)(e - row * D);
        const int k = (row >= dm.vocab[0] ? D : 0) + d;
        long long lo = seg_lo, hi = seg_hi;
        const long long want = row << 32;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (key[mid] < want) lo = mid + 1; else hi = mid;
        }
        float g = 0.0f, s = 0.0f;
        int cur = -1;
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
            s = s + dx[(long long)pos * (2 * D) + k];
        }
        if (cur >= 0) g = g + s;
        tf_adam(g, params + e, m + e, v + e, alpha, c1, c2, eps);
    }
}

// The tower vectors of a whole table: tiles of `tile` rows, a grid-stride loop over them.  Dynamic LDS, floats: two buffers of `buf` floats (>= tile x the
// widest of emb_dim and the hidden layers, a multiple of 4); the last layer is written to out[row x stride + j] and nothing else of out is touched.
__global__ __launch_bounds__(TR_THREADS) void k_tw_rows(TowerDims dm, int side, int tile, int buf, int n_tiles, const float* __restrict__ params,
                                                        float* __restrict__ out, long long stride) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float tw_rows_lds[];
    const int D = dm.emb_dim, L = dm.n_layers, V = dm.vocab[side];
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const long long r0 = (long long)t * tile;
        const int cnt = V - r0 < tile ? (int)(V - r0) : tile;
        float* in = tw_rows_lds;
        float* nx = tw_rows_lds + buf;
        for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) in[e] = params[dm.tab_off[side] + r0 * D + e];
        __syncthreads();
        for (int l = 0; l < L; ++l) {
            const int fan = dm.fan[l], H = dm.width[l];
            const float* __restrict__ W = params + dm.ker_off[side][l];
            for (int e = threadIdx.x; e < cnt * H; e += TR_THREADS) {
                const int i = e / H, j = e - i * H;
                float z = 0.0f;
                for (int k = 0; k < fan; ++k) z = z + in[i * fan + k] * W[k * H + j];
                z = z + params[dm.bias_off[side][l] + j];
                z = z > 0.0f ? z : 0.0f;
                if (l == L - 1) out[(r0 + i) * stride + j] = z;
                else nx[e] = z;
            }
            __syncthreads();
            float* q = in; in = nx; nx = q;
        }
    }
}
