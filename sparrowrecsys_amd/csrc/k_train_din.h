// k_train_din.h -- Adam training of DIN (an attention unit shared over the history slots, PReLU with trained alpha, weighted sum pooling, one movie
// table read through hist_len + 1 id columns): the device side of sparrowrecsys_amd/trainer_din.py, whose train_host is the DEFINITION of every bit
// computed here.  The schedule is k_train.h's with one generalisation: k_tr_check and k_tr_count as they are, and
//   k_td_scatter     an entry per (position, column) with id >= 0, keyed (table's first row + id) << 32 | (position in the batch x 16 + column): the
//                    columns of one table share a run, and the k_segments.h sort fixes the (sample, column) order inside it
// Per step, three launches:
//   k_td_step        one workgroup per tile of samples: gather, attention over the T slots, pooling, tail, sigmoid_def, backward; p, per (position,
//                    column) the emb_dim-wide row gradient, and the tile's partial sums of every parameter that is no table
//   k_tr_dense_adam  (k_train.h, as it is) per such parameter: the tiles' partials added in tile order, then Adam
//   k_td_table_adam  per (table row, dimension): the row's run added tile by tile, then Adam (g = 0 for a row the batch did not touch)
// Arithmetic as in k_train.h: FP32 VALU, operators under `#pragma clang fp contract(off)`, tr_sigmoid and tr_adam; no float atomics; every kernel
// returns at once when the error word is set.  att0/kernel, att0/bias, att_prelu/alpha and att1/kernel are staged in LDS once per workgroup: a
// workgroup reads them tile x T times forward and again backward.

static constexpr int TD_MAX_COLS = SPRK_TRAIN_DIN_MAX_COLS, TD_MAX_LAYERS = SPRK_TRAIN_DIN_MAX_LAYERS, TD_MAX_X = SPRK_TRAIN_DIN_MAX_X;
static constexpr int TD_MAX_WIDTH = SPRK_TRAIN_DIN_MAX_WIDTH, TD_MAX_EMB = SPRK_TRAIN_DIN_MAX_EMB;
static constexpr int TD_SRC_NUMERIC = -1, TD_SRC_POOLED = -2;
static_assert(TD_MAX_COLS == 16, "a schedule key holds position x 16 + column");

struct DinDims {                             // a kernel argument, by value (about 2 KB)
    int n_cols, n_dense, emb_dim, hist, att, n_x, n_layers, n_tables;
    int wide;                                // the widest gradient buffer: a tail layer, hist x att, 4 x hist x emb_dim
    int table[TD_MAX_COLS];                  // column -> table
    long long tab_off[TD_MAX_COLS + 1];      // table -> its first float in the parameter vector; [n_tables] = n_table
    long long row_base[TD_MAX_COLS + 1];     // table -> its first row among all tables' rows: the schedule's keys
    long long att0_ker, att0_bias, att_alpha, att1_ker, att1_bias;
    int width[TD_MAX_LAYERS + 1], fan[TD_MAX_LAYERS + 1];           // the tail's layers, then the head (width 1)
    long long ker_off[TD_MAX_LAYERS + 1], bias_off[TD_MAX_LAYERS + 1], alpha_off[TD_MAX_LAYERS];
    long long n_table, n_params;             // floats of all tables (= the first parameter that is none), of everything
    short xsrc[TD_MAX_X], xsub[TD_MAX_X];    // fc0's input rows: an id column outside the history, TD_SRC_NUMERIC or TD_SRC_POOLED; the element
    short prow[TD_MAX_EMB], crow[TD_MAX_EMB];                       // dimension -> fc0's input row of the pooled vector, of the candidate
};

// trainer_din.prelu and prelu_back
__device__ __forceinline__ float td_prelu(float z, float alpha) {
#pragma clang fp contract(off)
    return z > 0.0f ? z : (z < 0.0f ? alpha * z : 0.0f);
}
__device__ __forceinline__ float td_prelu_dz(float z, float alpha, float dy) {
#pragma clang fp contract(off)
    return z > 0.0f ? dy : (z < 0.0f ? alpha * dy : 0.0f);
}
__device__ __forceinline__ float td_prelu_dalpha(float z, float dy) {
#pragma clang fp contract(off)
    return z < 0.0f ? dy * z : 0.0f;
}

__global__ __launch_bounds__(TR_THREADS) void k_td_scatter(long long n, int batch, const int* __restrict__ ids, const int* __restrict__ order, DinDims dm,
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
        key[slot] = (dm.row_base[dm.table[c]] + id) << 32 | ((i - b * batch) * TD_MAX_COLS + c);          // batch <= 2^28: 32 bits hold it
        val[slot] = c;
    }
}

// One tile of one batch.  Dynamic LDS, floats: W0 [4 D][H], b0 [H], alpha [T][H], w1 [H] once; then per sample of the tile hc [T + 1][D] (the
// candidate's row, then the slots'), zu [T][H] (the attention's pre-activations), sv [T], dl [T], x0 [n_x], dx0 [n_x], per tail layer z [width]
// and y [width], two gradient buffers [wide].  first = the batch's first position, nb = its rows; p_out / drow are indexed by the position in the
// batch; drow = [position][column][D]; partial = [tiles][n_params - n_table].
__global__ __launch_bounds__(TR_THREADS) void k_td_step(DinDims dm, const int* __restrict__ ids, const float* __restrict__ dense, const float* __restrict__ labels,
                                                        const int* __restrict__ order, long long first, int nb, int tile, const float* __restrict__ params,
                                                        float* __restrict__ p_out, float* __restrict__ drow, float* __restrict__ partial,
                                                        const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float td_lds[];
    if (*err != TR_CLEAN) return;
    const int t0 = blockIdx.x * tile;
    const int cnt = nb - t0 < tile ? nb - t0 : tile;                        // >= 1: the grid is ceil(nb / tile)
    const int L = dm.n_layers, T = dm.hist, D = dm.emb_dim, H = dm.att, NX = dm.n_x, C = dm.n_cols, F = dm.n_dense;
    const int RD = (T + 1) * D, TH = T * H, A4 = 4 * D, TA = T * A4;
    float* W0 = td_lds;
    float* b0 = W0 + A4 * H;
    float* al = b0 + H;
    float* w1 = al + TH;
    float* hc = w1 + H;
    float* zu = hc + (size_t)tile * RD;
    float* sv = zu + (size_t)tile * TH;
    float* dl = sv + (size_t)tile * T;
    float* x0 = dl + (size_t)tile * T;
    float* dx0 = x0 + (size_t)tile * NX;
    float* zl[TD_MAX_LAYERS];
    float* yl[TD_MAX_LAYERS];
    float* at = dx0 + (size_t)tile * NX;
    for (int l = 0; l < L; ++l) {
        zl[l] = at; at += (size_t)tile * dm.width[l];
        yl[l] = at; at += (size_t)tile * dm.width[l];
    }
    float* g0 = at;
    float* g1 = g0 + (size_t)tile * dm.wide;

    // ---- gather the T + 1 movie rows; stage the attention unit's weights
    for (int e = threadIdx.x; e < cnt * RD; e += TR_THREADS) {
        const int i = e / RD, r = e - i * RD;
        const int col = r / D, d = r - col * D;
        const long long pos = first + t0 + i;
        const long long row = order ? order[pos] : pos;
        const int id = ids[row * C + col];
        hc[e] = id >= 0 ? params[dm.tab_off[0] + (long long)id * D + d] : 0.0f;
    }
    for (int e = threadIdx.x; e < A4 * H; e += TR_THREADS) W0[e] = params[dm.att0_ker + e];
    for (int e = threadIdx.x; e < TH; e += TR_THREADS) al[e] = params[dm.att_alpha + e];
    for (int e = threadIdx.x; e < H; e += TR_THREADS) { b0[e] = params[dm.att0_bias + e]; w1[e] = params[dm.att1_ker + e]; }
    __syncthreads();

    // ---- a = [h - c | h | c | h c] into g0 [cnt][T][4 D]
    for (int e = threadIdx.x; e < cnt * TA; e += TR_THREADS) {
        const int i = e / TA, r = e - i * TA;
        const int t = r / A4, k = r - t * A4;
        const int blk = k / D, d = k - blk * D;
        const float h = hc[i * RD + (1 + t) * D + d], c = hc[i * RD + d];
        g0[e] = blk == 0 ? h - c : blk == 1 ? h : blk == 2 ? c : h * c;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * TH; e += TR_THREADS) {
        const int q = e / H, j = e - q * H;
        const float* in = g0 + (size_t)q * A4;
        float z = 0.0f;
        for (int k = 0; k < A4; ++k) z = z + in[k] * W0[k * H + j];
        zu[e] = z + b0[j];
    }
    __syncthreads();
    {
        const float b1 = params[dm.att1_bias];
        for (int q = threadIdx.x; q < cnt * T; q += TR_THREADS) {
            const int t = q % T;
            float z = 0.0f;
            for (int j = 0; j < H; ++j) z = z + td_prelu(zu[q * H + j], al[t * H + j]) * w1[j];
            z = z + b1;
            sv[q] = z != z ? z : tr_sigmoid(z);
        }
    }
    __syncthreads();

    // ---- fc0's input: table rows, numerics, the pooled vector ((+0 + h_0 s_0) + h_1 s_1) + ...
    for (int e = threadIdx.x; e < cnt * NX; e += TR_THREADS) {
        const int i = e / NX, k = e - i * NX;
        const int src = dm.xsrc[k], sub = dm.xsub[k];
        const long long pos = first + t0 + i;
        const long long row = order ? order[pos] : pos;
        float x;
        if (src == TD_SRC_NUMERIC) x = dense[row * F + sub];
        else if (src == TD_SRC_POOLED) {
            x = 0.0f;
            for (int t = 0; t < T; ++t) x = x + hc[i * RD + (1 + t) * D + sub] * sv[i * T + t];
        } else if (src == 0) x = hc[i * RD + sub];
        else {
            const int id = ids[row * C + src];
            x = id >= 0 ? params[dm.tab_off[dm.table[src]] + (long long)id * D + sub] : 0.0f;
        }
        x0[e] = x;
    }
    __syncthreads();

    // ---- the tail and the head
    for (int l = 0; l < L; ++l) {
        const int fan = dm.fan[l], Hl = dm.width[l];
        const float* __restrict__ W = params + dm.ker_off[l];
        const float* __restrict__ bias = params + dm.bias_off[l];
        const float* __restrict__ alpha = params + dm.alpha_off[l];
        const float* in = l ? yl[l - 1] : x0;
        for (int e = threadIdx.x; e < cnt * Hl; e += TR_THREADS) {
            const int i = e / Hl, j = e - i * Hl;
            float z = 0.0f;
            for (int k = 0; k < fan; ++k) z = z + in[i * fan + k] * W[k * Hl + j];
            z = z + bias[j];
            zl[l][e] = z;
            yl[l][e] = td_prelu(z, alpha[j]);
        }
        __syncthreads();
    }
    {
        const int fan = dm.fan[L];
        const float* __restrict__ W = params + dm.ker_off[L];
        const float bh = params[dm.bias_off[L]];
        const float* in = yl[L - 1];
        const float fn = (float)nb;
        for (int i = threadIdx.x; i < cnt; i += TR_THREADS) {
            float z = 0.0f;
            for (int k = 0; k < fan; ++k) z = z + in[i * fan + k] * W[k];
            z = z + bh;
            const float p = z != z ? z : tr_sigmoid(z);
            const long long pos = first + t0 + i;
            p_out[t0 + i] = p;
            g0[i] = (p - labels[order ? order[pos] : pos]) / fn;
        }
        __syncthreads();
    }

    // ---- backward through the head and the tail: dz of layer l in `dz`; the layer's input gradient goes to `nx` (to dx0 for fc0), where the
    // ---- PReLU in front of it turns dy into dz in place while its alpha's partial sum is taken
    const long long nt = dm.n_table;
    float* __restrict__ mine = partial + (long long)blockIdx.x * (dm.n_params - nt);
    float* dz = g0;
    float* nx = g1;
    for (int l = L; l >= 0; --l) {
        const int fan = dm.fan[l], Hl = dm.width[l];
        const float* __restrict__ W = params + dm.ker_off[l];
        const float* a = l ? yl[l - 1] : x0;
        float* out = l ? nx : dx0;
        for (int e = threadIdx.x; e < fan * Hl; e += TR_THREADS) {
            const int k = e / Hl, j = e - k * Hl;
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + a[i * fan + k] * dz[i * Hl + j];
            mine[dm.ker_off[l] - nt + e] = s;
        }
        for (int j = threadIdx.x; j < Hl; j += TR_THREADS) {
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + dz[i * Hl + j];
            mine[dm.bias_off[l] - nt + j] = s;
        }
        for (int e = threadIdx.x; e < cnt * fan; e += TR_THREADS) {
            const int i = e / fan, k = e - i * fan;
            float s = 0.0f;
            for (int j = 0; j < Hl; ++j) s = s + W[k * Hl + j] * dz[i * Hl + j];
            out[e] = s;
        }
        __syncthreads();
        if (l) {
            const float* z = zl[l - 1];
            const float* __restrict__ alpha = params + dm.alpha_off[l - 1];
            for (int j = threadIdx.x; j < fan; j += TR_THREADS) {
                const float aj = alpha[j];
                float s = 0.0f;
                for (int i = 0; i < cnt; ++i) {
                    const float zz = z[i * fan + j], dy = nx[i * fan + j];
                    s = s + td_prelu_dalpha(zz, dy);
                    nx[i * fan + j] = td_prelu_dz(zz, aj, dy);
                }
                mine[dm.alpha_off[l - 1] - nt + j] = s;
            }
            __syncthreads();
            float* t = dz; dz = nx; nx = t;
        }
    }

    // ---- the attention sigmoid: ds_t = sum_d dpooled_d h_td; its logit's gradient (ds_t s_t)(1 - s_t)
    for (int q = threadIdx.x; q < cnt * T; q += TR_THREADS) {
        const int i = q / T, t = q - i * T;
        float ds = 0.0f;
        for (int d = 0; d < D; ++d) ds = ds + dx0[i * NX + dm.prow[d]] * hc[i * RD + (1 + t) * D + d];
        const float s = sv[q];
        dl[q] = (ds * s) * (1.0f - s);
    }
    __syncthreads();
    // att1's partials over the (sample, slot) pairs; du into g0 [cnt][T][H] with att_prelu/alpha[t]'s partial over the samples
    const int pairs = cnt * T;
    for (int j = threadIdx.x; j < H + 1; j += TR_THREADS) {
        float s = 0.0f;
        if (j < H) {
            for (int q = 0; q < pairs; ++q) s = s + td_prelu(zu[q * H + j], al[(q % T) * H + j]) * dl[q];
            mine[dm.att1_ker - nt + j] = s;
        } else {
            for (int q = 0; q < pairs; ++q) s = s + dl[q];
            mine[dm.att1_bias - nt] = s;
        }
    }
    for (int e = threadIdx.x; e < TH; e += TR_THREADS) {
        const int t = e / H, j = e - t * H;
        const float aj = al[e], wj = w1[j];
        float s = 0.0f;
        for (int i = 0; i < cnt; ++i) {
            const int q = i * T + t;
            const float u = zu[q * H + j];
            float dy = 0.0f;
            dy = dy + wj * dl[q];
            s = s + td_prelu_dalpha(u, dy);
            g0[q * H + j] = td_prelu_dz(u, aj, dy);
        }
        mine[dm.att_alpha - nt + e] = s;
    }
    __syncthreads();
    // att0's partials (a recomputed from the gathered rows) and dA = _back(att0/kernel, du) into g1 [cnt][T][4 D]
    for (int e = threadIdx.x; e < A4 * H; e += TR_THREADS) {
        const int k = e / H, j = e - k * H;
        const int blk = k / D, d = k - blk * D;
        float s = 0.0f;
        for (int q = 0; q < pairs; ++q) {
            const int i = q / T, t = q - i * T;
            const float h = hc[i * RD + (1 + t) * D + d], c = hc[i * RD + d];
            const float a = blk == 0 ? h - c : blk == 1 ? h : blk == 2 ? c : h * c;
            s = s + a * g0[q * H + j];
        }
        mine[dm.att0_ker - nt + e] = s;
    }
    for (int j = threadIdx.x; j < H; j += TR_THREADS) {
        float s = 0.0f;
        for (int q = 0; q < pairs; ++q) s = s + g0[q * H + j];
        mine[dm.att0_bias - nt + j] = s;
    }
    for (int e = threadIdx.x; e < cnt * TA; e += TR_THREADS) {
        const int q = e / A4, k = e - q * A4;
        float s = 0.0f;
        for (int j = 0; j < H; ++j) s = s + W0[k * H + j] * g0[q * H + j];
        g1[e] = s;
    }
    __syncthreads();

    // ---- the gradient that reaches each gathered row, per (position, column)
    for (int e = threadIdx.x; e < cnt * RD; e += TR_THREADS) {
        const int i = e / RD, r = e - i * RD;
        const int col = r / D, d = r - col * D;
        float x;
        if (col) {
            const int q = i * T + (col - 1);
            const float* dA = g1 + (size_t)q * A4;
            x = ((dx0[i * NX + dm.prow[d]] * sv[q] + dA[d]) + dA[D + d]) + dA[3 * D + d] * hc[i * RD + d];
        } else {
            x = dx0[i * NX + dm.crow[d]];
            for (int t = 0; t < T; ++t) {
                const float* dA = g1 + (size_t)(i * T + t) * A4;
                x = ((x - dA[d]) + dA[2 * D + d]) + dA[3 * D + d] * hc[i * RD + (1 + t) * D + d];
            }
        }
        drow[((long long)(t0 + i) * C + col) * D + d] = x;
    }
    for (int e = threadIdx.x; e < cnt * NX; e += TR_THREADS) {
        const int i = e / NX, k = e - i * NX;
        const int src = dm.xsrc[k];
        if (src > T) drow[((long long)(t0 + i) * C + src) * D + dm.xsub[k]] = dx0[e];
    }
}

// [off[b], off[b + 1]) = the batch's entries, sorted by (row among all tables' rows, position, column)
__global__ __launch_bounds__(TR_THREADS) void k_td_table_adam(DinDims dm, int tile, const unsigned* __restrict__ off, long long b, const long long* __restrict__ key,
                                                              const float* __restrict__ drow, float* __restrict__ params, float* __restrict__ m,
                                                              float* __restrict__ v, const float* __restrict__ alphas, long long step, float c1, float c2, float eps,
                                                              const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    if (*err != TR_CLEAN) return;
    const long long seg_lo = off[b], seg_hi = off[b + 1];
    const float alpha = alphas[step];
    const int D = dm.emb_dim, C = dm.n_cols;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < dm.n_table; e += (long long)gridDim.x * TR_THREADS) {
        int t = 0;
        while (t + 1 < dm.n_tables && e >= dm.tab_off[t + 1]) ++t;
        const long long local = e - dm.tab_off[t];
        const long long row = dm.row_base[t] + local / D;
        const int d = (int)(local % D);
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
            const unsigned pc = (unsigned)(kk & 0xffffffffll);
            const int pos = (int)(pc >> 4), col = (int)(pc & 15u);
            const int tl = pos / tile;
            if (tl != cur) {
                if (cur >= 0) g = g + s;
                s = 0.0f;
                cur = tl;
            }
            s = s + drow[((long long)pos * C + col) * D + d];
        }
        if (cur >= 0) g = g + s;
        tr_adam(g, params + e, m + e, v + e, alpha, c1, c2, eps);
    }
}
