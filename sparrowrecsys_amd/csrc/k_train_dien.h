// k_train_dien.h -- Adam training of DIEN (a Keras GRU over the history slots that consumes the embedding's zero mask, a sigmoid attention gate per
// slot, the reference's AUGRU, a PReLU tail): the device side of sparrowrecsys_amd/trainer_dien.py, whose train_host is the DEFINITION of every bit
// computed here.  The schedule is k_train_din.h's (k_tr_check, the count, the scatter keyed by table row and (position,
// column), the segment sort): the movie table is read through hist + 1 columns here too.  k_te_count and k_te_scatter are k_tr_count and
// k_td_scatter less the masked slots, whose entries of row 0 would carry +0.  Per step, three launches:
//   k_te_step        one workgroup per tile of samples: gather, the GRU, the gate and the AUGRU forward with every per-slot activation the walk back
//                    reads kept in LDS, the tail, sigmoid_def; backward through the tail, the AUGRU from the last slot down, the gate, the masked
//                    GRU from the last slot down; p, per (position, column) the emb_dim-wide row gradient, and the tile's partial sums of every
//                    parameter that is no table, the (sample, slot) pairs sample-major
//   k_tr_dense_adam  (k_train.h, as it is)
//   k_td_table_adam  (k_train_din.h, as it is)
// Arithmetic as in k_train.h: FP32 VALU, operators under `#pragma clang fp contract(off)`, tr_sigmoid and tr_adam; no float atomics; every kernel
// returns at once when the error word is set.  The GRU's two kernels and bias and the AUGRU's nine kernels and six biases (15 D D + 12 D floats)
// are staged in LDS once per workgroup where emb_dim <= TE_STAGE_EMB; wider models, the gate's and the tail's weights are read from L2.

static constexpr int TE_STAGE_EMB = 16;

struct DienDims {                            // a kernel argument, by value (about 2 KB)
    int n_cols, n_dense, emb_dim, hist, att, n_x, n_layers, n_tables;
    int wide;                                // the widest tail layer: the two gradient buffers of the tail
    int staged;                              // the recurrent weights sit in LDS
    int table[TD_MAX_COLS];                  // column -> table
    long long tab_off[TD_MAX_COLS + 1];      // table -> its first float in the parameter vector; [n_tables] = n_table
    long long gru, att0_ker, att0_bias, att1_ker, att1_bias, aug, h0;       // gru: kernel, recurrent kernel, bias; aug: per gate r, z, h its five arrays
    int width[TD_MAX_LAYERS + 1], fan[TD_MAX_LAYERS + 1];           // the tail's layers, then the head (width 1)
    long long ker_off[TD_MAX_LAYERS + 1], bias_off[TD_MAX_LAYERS + 1], alpha_off[TD_MAX_LAYERS];
    long long n_table, n_params;             // floats of all tables (= the first parameter that is none), of everything
    short xsrc[TD_MAX_X], xsub[TD_MAX_X];    // fc0's input rows: an id column outside the history, TD_SRC_NUMERIC or TD_SRC_POOLED (the AUGRU's state)
    short prow[TD_MAX_EMB], crow[TD_MAX_EMB];                       // dimension -> fc0's input row of the AUGRU's state, of the candidate
};

// sigmoid_def as the trainers' kernels call it, and trainer_dien.tanh_def: (s + s) - 1 with s = sigmoid_def(z + z)
__device__ __forceinline__ float te_sigmoid(float z) { return z != z ? z : tr_sigmoid(z); }
__device__ __forceinline__ float te_tanh(float z) {
#pragma clang fp contract(off)
    const float s = te_sigmoid(z + z);
    return (s + s) - 1.0f;
}

// k_tr_count and k_td_scatter without the masked slots: a history column's id 0 carries +0 in every element, and a sum from +0 is the same
// bits without it, so it gets no entry.  (With them, every batch's run of row 0 is a fifth of its history entries long and one thread of
// k_td_table_adam walks it per dimension: two thirds of a step in docs/train_dien_results.md's first measurement.)
__device__ __forceinline__ bool te_entry(int id, int c, int hist) { return id >= 0 && !(id == 0 && c >= 1 && c <= hist); }

__global__ __launch_bounds__(TR_THREADS) void k_te_count(long long n, int batch, const int* __restrict__ ids, const int* __restrict__ order, int n_cols, int hist,
                                                         unsigned* __restrict__ off) {
    const long long total = n * n_cols;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TR_THREADS) {
        const long long i = e / n_cols;
        const int c = (int)(e - i * n_cols);
        const long long r = order ? order[i] : i;
        if (te_entry(ids[r * n_cols + c], c, hist)) atomicAdd(&off[i / batch], 1u);
    }
}

__global__ __launch_bounds__(TR_THREADS) void k_te_scatter(long long n, int batch, const int* __restrict__ ids, const int* __restrict__ order, DinDims dm,
                                                           const unsigned* __restrict__ off, unsigned* __restrict__ cursor, long long* __restrict__ key,
                                                           int* __restrict__ val, const unsigned long long* __restrict__ err) {
    if (*err != TR_CLEAN) return;                                            // (an id outside its table would key another table's row)
    const long long total = n * dm.n_cols;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TR_THREADS) {
        const long long i = e / dm.n_cols;
        const int c = (int)(e - i * dm.n_cols);
        const long long r = order ? order[i] : i;
        const int id = ids[r * dm.n_cols + c];
        if (!te_entry(id, c, dm.hist)) continue;
        const long long b = i / batch;
        const unsigned slot = off[b] + atomicAdd(&cursor[b], 1u);           // < off[b + 1]: k_te_count counted this entry
        key[slot] = (dm.row_base[dm.table[c]] + id) << 32 | ((i - b * batch) * TD_MAX_COLS + c);          // batch <= 2^28: 32 bits hold it
        val[slot] = c;
    }
}

// One tile of one batch.  Dynamic LDS, floats: the staged weights once; then the arrays of trainer_dien.lds_bytes, each [tile][...].  first = the
// batch's first position, nb = its rows; p_out / drow are indexed by the position in the batch; drow = [position][column][D]; partial =
// [tiles][n_params - n_table].
__global__ __launch_bounds__(TR_THREADS) void k_te_step(DienDims dm, const int* __restrict__ ids, const float* __restrict__ dense, const float* __restrict__ labels,
                                                        const int* __restrict__ order, long long first, int nb, int tile, const float* __restrict__ params,
                                                        float* __restrict__ p_out, float* __restrict__ drow, float* __restrict__ partial,
                                                        const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float te_lds[];
    if (*err != TR_CLEAN) return;
    const int t0 = blockIdx.x * tile;
    const int cnt = nb - t0 < tile ? nb - t0 : tile;                        // >= 1: the grid is ceil(nb / tile)
    const int L = dm.n_layers, T = dm.hist, D = dm.emb_dim, H = dm.att, NX = dm.n_x, C = dm.n_cols, F = dm.n_dense;
    const int RD = (T + 1) * D, TD_ = T * D, TH = T * H, D3 = 3 * D, T3 = T * D3, DD = D * D;
    const int n_gru = 2 * D * D3 + 2 * D3, n_gate = 3 * DD + 2 * D;
    float* at = te_lds;
    float* stage = at;
    if (dm.staged) at += n_gru + 3 * n_gate;
    float* hc = at;  at += (size_t)tile * RD;                                // the candidate's row, then the slots'
    float* hp = at;  at += (size_t)tile * TD_;                               // the GRU: the state before the slot, z, r, hh, mh_h, the output g
    float* gz = at;  at += (size_t)tile * TD_;
    float* gr = at;  at += (size_t)tile * TD_;
    float* ghh = at; at += (size_t)tile * TD_;
    float* gmh = at; at += (size_t)tile * TD_;
    float* gg = at;  at += (size_t)tile * TD_;
    float* ya = at;  at += (size_t)tile * TH;                                // the gate: y, a
    float* av = at;  at += (size_t)tile * T;
    float* hsp = at; at += (size_t)tile * TD_;                               // the AUGRU: the state before the slot, r_t, z_t, hc_t, the three pre
    float* rt = at;  at += (size_t)tile * TD_;
    float* zt = at;  at += (size_t)tile * TD_;
    float* hct = at; at += (size_t)tile * TD_;
    float* pre = at; at += (size_t)tile * T3;
    float* do3 = at; at += (size_t)tile * T3;                                // the walk back: do and dpre of the gates r, z, h; then the GRU's dmx and dmh
    float* dp3 = at; at += (size_t)tile * T3;
    float* dq = at;  at += (size_t)tile * TD_;
    float* dg = at;  at += (size_t)tile * TD_;
    float* dl = at;  at += (size_t)tile * T;
    float* de = at;  at += (size_t)tile * TH;
    float* vv = at;  at += (size_t)tile * 8 * D;                             // eight vectors of D per sample
    float* x0 = at;  at += (size_t)tile * NX;
    float* dx0 = at; at += (size_t)tile * NX;
    float* zl[TD_MAX_LAYERS];
    float* yl[TD_MAX_LAYERS];
    for (int l = 0; l < L; ++l) {
        zl[l] = at; at += (size_t)tile * dm.width[l];
        yl[l] = at; at += (size_t)tile * dm.width[l];
    }
    float* g0 = at;
    float* g1 = g0 + (size_t)tile * dm.wide;
    const int V = 8 * D;                                                     // vv's stride per sample

    // ---- gather the T + 1 movie rows; stage the recurrent weights
    for (int e = threadIdx.x; e < cnt * RD; e += TR_THREADS) {
        const int i = e / RD, r = e - i * RD;
        const int col = r / D, d = r - col * D;
        const long long pos = first + t0 + i;
        const long long row = order ? order[pos] : pos;
        const int id = ids[row * C + col];
        hc[e] = id >= 0 ? params[dm.tab_off[0] + (long long)id * D + d] : 0.0f;
    }
    if (dm.staged) {
        for (int e = threadIdx.x; e < n_gru; e += TR_THREADS) stage[e] = params[dm.gru + e];
        for (int e = threadIdx.x; e < 3 * n_gate; e += TR_THREADS) stage[n_gru + e] = params[dm.aug + e];
    }
    const float* Wg = dm.staged ? stage : params + dm.gru;                   // gru/kernel [D][3 D], gru_rec/kernel [D][3 D], gru/bias [2][3 D]
    const float* Wa = dm.staged ? stage + n_gru : params + dm.aug;           // per gate: in kernel [D][D], in bias, hid kernel, out kernel, out bias
    const float* Wk = Wg;
    const float* Uk = Wg + D * D3;
    const float* bk = Wg + 2 * D * D3;
    const float* __restrict__ W0 = params + dm.att0_ker;
    const float* __restrict__ b0 = params + dm.att0_bias;
    const float* __restrict__ w1 = params + dm.att1_ker;
    for (int e = threadIdx.x; e < cnt * 2 * D; e += TR_THREADS) {            // the GRU's state (vv[0]) and held output (vv[1]) from +0
        const int i = e / (2 * D), r = e - i * 2 * D;
        vv[i * V + r] = 0.0f;
    }
    __syncthreads();

    // ---- the GRU: mx in vv[2..4], mh in vv[5..7]
    for (int t = 0; t < T; ++t) {
        for (int e = threadIdx.x; e < cnt * 2 * D3; e += TR_THREADS) {
            const int i = e / (2 * D3), j = e - i * 2 * D3;
            float z = 0.0f;
            if (j < D3) {
                const float* x = hc + i * RD + (1 + t) * D;
                for (int k = 0; k < D; ++k) z = z + x[k] * Wk[k * D3 + j];
                z = z + bk[j];
            } else {
                const float* h = vv + i * V;
                for (int k = 0; k < D; ++k) z = z + h[k] * Uk[k * D3 + (j - D3)];
                z = z + bk[j];                                               // bias row 1 follows row 0
            }
            vv[i * V + 2 * D + j] = z;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {
            const int i = e / D, d = e - i * D;
            const float* mx = vv + i * V + 2 * D;
            const float* mh = mx + D3;
            const float h = vv[i * V + d];
            const float z = te_sigmoid(mx[d] + mh[d]);
            const float r = te_sigmoid(mx[D + d] + mh[D + d]);
            const float hh = te_tanh(mx[2 * D + d] + r * mh[2 * D + d]);
            const float hn = z * h + (1.0f - z) * hh;
            const int q = (i * T + t) * D + d;
            hp[q] = h; gz[q] = z; gr[q] = r; ghh[q] = hh; gmh[q] = mh[2 * D + d];
            const long long pos = first + t0 + i;
            if (ids[(order ? order[pos] : pos) * C + 1 + t] != 0) { vv[i * V + d] = hn; vv[i * V + D + d] = hn; }
            gg[q] = vv[i * V + D + d];                                       // a masked slot repeats the output before it
        }
        __syncthreads();
    }

    // ---- the attention gate
    for (int e = threadIdx.x; e < cnt * TH; e += TR_THREADS) {
        const int q = e / H, j = e - q * H;
        const int i = q / T;
        float z = 0.0f;
        for (int k = 0; k < D; ++k) z = z + (gg[q * D + k] * hc[i * RD + k]) * W0[k * H + j];
        ya[e] = te_sigmoid(z + b0[j]);
    }
    __syncthreads();
    {
        const float b1 = params[dm.att1_bias];
        for (int q = threadIdx.x; q < cnt * T; q += TR_THREADS) {
            float z = 0.0f;
            for (int j = 0; j < H; ++j) z = z + ya[q * H + j] * w1[j];
            av[q] = te_sigmoid(z + b1);
        }
    }
    for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {                // the AUGRU's state (vv[0]) from augru/h0
        const int i = e / D, d = e - i * D;
        vv[i * V + d] = params[dm.h0 + d];
    }
    __syncthreads();

    // ---- the AUGRU
    for (int t = 0; t < T; ++t) {
        for (int e = threadIdx.x; e < cnt * 2 * D; e += TR_THREADS) {        // pre of the gates r and z
            const int i = e / (2 * D), r = e - i * 2 * D;
            const int k3 = r / D, j = r - k3 * D;
            const float* Wq = Wa + k3 * n_gate;
            const float* g = gg + (i * T + t) * D;
            const float* hs = vv + i * V;
            float a = 0.0f, b = 0.0f;
            for (int k = 0; k < D; ++k) a = a + g[k] * Wq[k * D + j];
            a = a + Wq[DD + j];
            for (int k = 0; k < D; ++k) b = b + hs[k] * Wq[DD + D + k * D + j];
            pre[((i * T + t) * 3 + k3) * D + j] = a + b;
            if (k3 == 0) hsp[(i * T + t) * D + j] = hs[j];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * 2 * D; e += TR_THREADS) {
            const int i = e / (2 * D), r = e - i * 2 * D;
            const int k3 = r / D, j = r - k3 * D;
            const float* Wq = Wa + k3 * n_gate;
            const float* pr = pre + ((i * T + t) * 3 + k3) * D;
            float z = 0.0f;
            for (int k = 0; k < D; ++k) z = z + pr[k] * Wq[2 * DD + D + k * D + j];
            z = z + Wq[3 * DD + D + j];
            (k3 ? zt : rt)[(i * T + t) * D + j] = te_sigmoid(z);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {            // pre of the gate h: hid = hs z_t
            const int i = e / D, j = e - i * D;
            const float* Wq = Wa + 2 * n_gate;
            const float* g = gg + (i * T + t) * D;
            const float* hs = vv + i * V;
            const float* z = zt + (i * T + t) * D;
            float a = 0.0f, b = 0.0f;
            for (int k = 0; k < D; ++k) a = a + g[k] * Wq[k * D + j];
            a = a + Wq[DD + j];
            for (int k = 0; k < D; ++k) b = b + (hs[k] * z[k]) * Wq[DD + D + k * D + j];
            pre[((i * T + t) * 3 + 2) * D + j] = a + b;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {
            const int i = e / D, j = e - i * D;
            const float* Wq = Wa + 2 * n_gate;
            const float* pr = pre + ((i * T + t) * 3 + 2) * D;
            float z = 0.0f;
            for (int k = 0; k < D; ++k) z = z + pr[k] * Wq[2 * DD + D + k * D + j];
            z = z + Wq[3 * DD + D + j];
            const float h = te_tanh(z);
            const int q = (i * T + t) * D + j;
            hct[q] = h;
            const float u = av[i * T + t] * rt[q];
            const float hs = vv[i * V + j];
            vv[i * V + j] = (1.0f - u) * hs + u * h;
        }
        __syncthreads();
    }

    // ---- fc0's input: table rows, numerics, the AUGRU's last state
    for (int e = threadIdx.x; e < cnt * NX; e += TR_THREADS) {
        const int i = e / NX, k = e - i * NX;
        const int src = dm.xsrc[k], sub = dm.xsub[k];
        const long long pos = first + t0 + i;
        const long long row = order ? order[pos] : pos;
        float x;
        if (src == TD_SRC_NUMERIC) x = dense[row * F + sub];
        else if (src == TD_SRC_POOLED) x = vv[i * V + sub];
        else if (src == 0) x = hc[i * RD + sub];
        else {
            const int id = ids[row * C + src];
            x = id >= 0 ? params[dm.tab_off[dm.table[src]] + (long long)id * D + sub] : 0.0f;
        }
        x0[e] = x;
    }
    __syncthreads();

    // ---- the tail and the head (k_td_step's)
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
            const float p = te_sigmoid(z);
            const long long pos = first + t0 + i;
            p_out[t0 + i] = p;
            g0[i] = (p - labels[order ? order[pos] : pos]) / fn;
        }
        __syncthreads();
    }

    // ---- backward through the head and the tail (k_td_step's)
    const long long nt = dm.n_table;
    float* __restrict__ mine = partial + (long long)blockIdx.x * (dm.n_params - nt);
    {
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
    }

    // ---- the AUGRU from the last slot down: dhs in vv[0], du in vv[1], dhz in vv[2]; da_t into dl
    for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {
        const int i = e / D, d = e - i * D;
        vv[i * V + d] = dx0[i * NX + dm.prow[d]];
    }
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {
            const int i = e / D, d = e - i * D;
            const int q = (i * T + t) * D + d;
            const float dhs = vv[i * V + d], h = hct[q];
            const float u = av[i * T + t] * rt[q];
            vv[i * V + D + d] = dhs * (h - hsp[q]);
            const float dhc = dhs * u;
            do3[((i * T + t) * 3 + 2) * D + d] = dhc * (1.0f - h * h);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {            // dpre_h = _back(out_h/kernel, do_h)
            const int i = e / D, k = e - i * D;
            const float* Wo = Wa + 2 * n_gate + 2 * DD + D;
            const float* dz = do3 + ((i * T + t) * 3 + 2) * D;
            float s = 0.0f;
            for (int j = 0; j < D; ++j) s = s + Wo[k * D + j] * dz[j];
            dp3[((i * T + t) * 3 + 2) * D + k] = s;
        }
        for (int i = threadIdx.x; i < cnt; i += TR_THREADS) {                // da_t = sum_d du_d r_td
            const float* du = vv + i * V + D;
            const float* r = rt + (i * T + t) * D;
            float s = 0.0f;
            for (int d = 0; d < D; ++d) s = s + du[d] * r[d];
            dl[i * T + t] = s;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {            // dhz = _back(hid_h/kernel, dpre_h); do_z, do_r
            const int i = e / D, k = e - i * D;
            const int q = (i * T + t) * D + k;
            const float* Wh = Wa + 2 * n_gate + DD + D;
            const float* dz = dp3 + ((i * T + t) * 3 + 2) * D;
            float s = 0.0f;
            for (int j = 0; j < D; ++j) s = s + Wh[k * D + j] * dz[j];
            vv[i * V + 2 * D + k] = s;
            const float z = zt[q], r = rt[q];
            const float dzt = s * hsp[q];
            do3[((i * T + t) * 3 + 1) * D + k] = (dzt * z) * (1.0f - z);
            const float dr = vv[i * V + D + k] * av[i * T + t];
            do3[((i * T + t) * 3 + 0) * D + k] = (dr * r) * (1.0f - r);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * 2 * D; e += TR_THREADS) {        // dpre_r, dpre_z
            const int i = e / (2 * D), r = e - i * 2 * D;
            const int k3 = r / D, k = r - k3 * D;
            const float* Wo = Wa + k3 * n_gate + 2 * DD + D;
            const float* dz = do3 + ((i * T + t) * 3 + k3) * D;
            float s = 0.0f;
            for (int j = 0; j < D; ++j) s = s + Wo[k * D + j] * dz[j];
            dp3[((i * T + t) * 3 + k3) * D + k] = s;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {            // the state before the slot receives
            const int i = e / D, k = e - i * D;
            const int q = (i * T + t) * D + k;
            const float* Wr = Wa + DD + D;
            const float* Wz = Wa + n_gate + DD + D;
            const float* dr = dp3 + ((i * T + t) * 3 + 0) * D;
            const float* dz = dp3 + ((i * T + t) * 3 + 1) * D;
            float a = 0.0f, b = 0.0f;
            for (int j = 0; j < D; ++j) a = a + Wr[k * D + j] * dr[j];
            for (int j = 0; j < D; ++j) b = b + Wz[k * D + j] * dz[j];
            const float u = av[i * T + t] * rt[q];
            vv[i * V + k] = ((vv[i * V + k] * (1.0f - u) + a) + b) + vv[i * V + 2 * D + k] * zt[q];
        }
        __syncthreads();
    }

    // ---- the gate: dl, de, dq; dg
    for (int q = threadIdx.x; q < cnt * T; q += TR_THREADS) {
        const float a = av[q];
        dl[q] = (dl[q] * a) * (1.0f - a);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * TH; e += TR_THREADS) {
        const int q = e / H, j = e - q * H;
        const float y = ya[e];
        float dy = 0.0f;
        dy = dy + w1[j] * dl[q];
        de[e] = (dy * y) * (1.0f - y);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * TD_; e += TR_THREADS) {
        const int q = e / D, k = e - q * D;
        float s = 0.0f;
        for (int j = 0; j < H; ++j) s = s + W0[k * H + j] * de[q * H + j];
        dq[e] = s;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * TD_; e += TR_THREADS) {
        const int q = e / D, k = e - q * D;
        const int i = q / T;
        float x = dq[e] * hc[i * RD + k];
        for (int k3 = 0; k3 < 3; ++k3) {
            const float* Wi = Wa + k3 * n_gate;
            const float* dz = dp3 + (q * 3 + k3) * D;
            float s = 0.0f;
            for (int j = 0; j < D; ++j) s = s + Wi[k * D + j] * dz[j];
            x = x + s;
        }
        dg[e] = x;
    }
    // ---- the partial sums of the gate, the AUGRU and augru/h0 over the tile's (sample, slot) pairs, sample-major
    const int pairs = cnt * T;
    for (int e = threadIdx.x; e < D * H; e += TR_THREADS) {
        const int k = e / H, j = e - k * H;
        float s = 0.0f;
        for (int q = 0; q < pairs; ++q) s = s + (gg[q * D + k] * hc[(q / T) * RD + k]) * de[q * H + j];
        mine[dm.att0_ker - nt + e] = s;
    }
    for (int j = threadIdx.x; j < 2 * H + 1; j += TR_THREADS) {
        float s = 0.0f;
        if (j < H) {
            for (int q = 0; q < pairs; ++q) s = s + de[q * H + j];
            mine[dm.att0_bias - nt + j] = s;
        } else if (j < 2 * H) {
            for (int q = 0; q < pairs; ++q) s = s + ya[q * H + (j - H)] * dl[q];
            mine[dm.att1_ker - nt + (j - H)] = s;
        } else {
            for (int q = 0; q < pairs; ++q) s = s + dl[q];
            mine[dm.att1_bias - nt] = s;
        }
    }
    for (int e = threadIdx.x; e < 3 * n_gate; e += TR_THREADS) {
        const int k3 = e / n_gate, r = e - k3 * n_gate;
        float s = 0.0f;
        if (r < DD) {                                                        // in kernel: g x dpre
            const int k = r / D, j = r - k * D;
            for (int q = 0; q < pairs; ++q) s = s + gg[q * D + k] * dp3[(q * 3 + k3) * D + j];
        } else if (r < DD + D) {                                             // in bias
            const int j = r - DD;
            for (int q = 0; q < pairs; ++q) s = s + dp3[(q * 3 + k3) * D + j];
        } else if (r < 2 * DD + D) {                                         // hid kernel: hs (r, z) or hs z_t (h) x dpre
            const int k = (r - DD - D) / D, j = (r - DD - D) - k * D;
            if (k3 < 2) for (int q = 0; q < pairs; ++q) s = s + hsp[q * D + k] * dp3[(q * 3 + k3) * D + j];
            else for (int q = 0; q < pairs; ++q) s = s + (hsp[q * D + k] * zt[q * D + k]) * dp3[(q * 3 + k3) * D + j];
        } else if (r < 3 * DD + D) {                                         // out kernel: pre x do
            const int k = (r - 2 * DD - D) / D, j = (r - 2 * DD - D) - k * D;
            for (int q = 0; q < pairs; ++q) s = s + pre[(q * 3 + k3) * D + k] * do3[(q * 3 + k3) * D + j];
        } else {                                                             // out bias
            const int j = r - 3 * DD - D;
            for (int q = 0; q < pairs; ++q) s = s + do3[(q * 3 + k3) * D + j];
        }
        mine[dm.aug - nt + e] = s;
    }
    for (int d = threadIdx.x; d < D; d += TR_THREADS) {
        float s = 0.0f;
        for (int i = 0; i < cnt; ++i) s = s + vv[i * V + d];
        mine[dm.h0 - nt + d] = s;
    }
    __syncthreads();

    // ---- the masked GRU from the last slot down: dh in vv[4], do in vv[5], dhn z in vv[6]; dmx into do3, dmh into dp3, each [pair][3 D]
    for (int e = threadIdx.x; e < cnt * 2 * D; e += TR_THREADS) {
        const int i = e / (2 * D), r = e - i * 2 * D;
        vv[i * V + 4 * D + r] = 0.0f;
    }
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {
            const int i = e / D, d = e - i * D;
            const int q = (i * T + t) * D + d;
            const long long pos = first + t0 + i;
            const bool on = ids[(order ? order[pos] : pos) * C + 1 + t] != 0;
            const float dout = vv[i * V + 5 * D + d] + dg[q];
            float* dmx = do3 + (i * T + t) * D3;
            float* dmh = dp3 + (i * T + t) * D3;
            if (on) {
                const float h = hp[q], z = gz[q], r = gr[q], hh = ghh[q];
                const float dhn = vv[i * V + 4 * D + d] + dout;
                const float dzg = dhn * (h - hh), dhh = dhn * (1.0f - z);
                const float dph = dhh * (1.0f - hh * hh);
                const float drr = dph * gmh[q];
                const float dpz = (dzg * z) * (1.0f - z), dpr = (drr * r) * (1.0f - r);
                dmx[d] = dpz; dmx[D + d] = dpr; dmx[2 * D + d] = dph;
                dmh[d] = dpz; dmh[D + d] = dpr; dmh[2 * D + d] = dph * r;
                vv[i * V + 6 * D + d] = dhn * z;
                vv[i * V + 5 * D + d] = 0.0f;
            } else {
                dmx[d] = 0.0f; dmx[D + d] = 0.0f; dmx[2 * D + d] = 0.0f;
                dmh[d] = 0.0f; dmh[D + d] = 0.0f; dmh[2 * D + d] = 0.0f;
                vv[i * V + 5 * D + d] = dout;
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {
            const int i = e / D, k = e - i * D;
            const long long pos = first + t0 + i;
            const bool on = ids[(order ? order[pos] : pos) * C + 1 + t] != 0;
            float a = 0.0f;
            if (on) {
                const float* dmx = do3 + (i * T + t) * D3;
                const float* dmh = dp3 + (i * T + t) * D3;
                float b = 0.0f;
                for (int j = 0; j < D3; ++j) a = a + Wk[k * D3 + j] * dmx[j];
                for (int j = 0; j < D3; ++j) b = b + Uk[k * D3 + j] * dmh[j];
                vv[i * V + 4 * D + k] = vv[i * V + 6 * D + k] + b;
            }
            drow[((long long)(t0 + i) * C + 1 + t) * D + k] = a;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < 2 * D * D3 + 2 * D3; e += TR_THREADS) {
        float s = 0.0f;
        if (e < D * D3) {                                                    // gru/kernel: x x dmx
            const int k = e / D3, j = e - k * D3;
            for (int q = 0; q < pairs; ++q) s = s + hc[(q / T) * RD + (1 + q % T) * D + k] * do3[q * D3 + j];
        } else if (e < 2 * D * D3) {                                         // gru_rec/kernel: the state before the slot x dmh
            const int k = (e - D * D3) / D3, j = (e - D * D3) - k * D3;
            for (int q = 0; q < pairs; ++q) s = s + hp[q * D + k] * dp3[q * D3 + j];
        } else if (e < 2 * D * D3 + D3) {
            const int j = e - 2 * D * D3;
            for (int q = 0; q < pairs; ++q) s = s + do3[q * D3 + j];
        } else {
            const int j = e - 2 * D * D3 - D3;
            for (int q = 0; q < pairs; ++q) s = s + dp3[q * D3 + j];
        }
        mine[dm.gru - nt + e] = s;
    }

    // ---- the candidate's row and the columns behind the history
    for (int e = threadIdx.x; e < cnt * D; e += TR_THREADS) {
        const int i = e / D, d = e - i * D;
        float x = dx0[i * NX + dm.crow[d]];
        for (int t = 0; t < T; ++t) x = x + dq[(i * T + t) * D + d] * gg[(i * T + t) * D + d];
        drow[((long long)(t0 + i) * C) * D + d] = x;
    }
    for (int e = threadIdx.x; e < cnt * NX; e += TR_THREADS) {
        const int i = e / NX, k = e - i * NX;
        const int src = dm.xsrc[k];
        if (src > T) drow[((long long)(t0 + i) * C + src) * D + dm.xsub[k]] = dx0[e];
    }
}
