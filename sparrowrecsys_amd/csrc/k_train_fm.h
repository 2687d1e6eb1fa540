// k_train_fm.h -- Adam training of DeepFM_v2 (first order + sum-of-squares FM cross over per-field Dense projections + a deep stack, one sigmoid):
// the device side of sparrowrecsys_amd/trainer_fm.py, whose train_host is the DEFINITION of every bit computed here.
// The schedule is k_train.h's: k_tr_check, k_tr_count, k_tr_scatter and the k_segments.h sort give, per batch, one sorted run of positions per
// (field, id); that run serves the emb/ row of width emb_dim AND the fo_cat/kernel row of width 1.  Per step:
//   k_tf_step        one workgroup per tile of samples: forward, sigmoid_def, backward; p, per position de (the groups' table-row gradients) and
//                    d_first, and the tile's partial sums of every parameter that is no table
//   k_tf_dense_adam  per such parameter: the tiles' partials added in tile order, then Adam
//   k_tf_table_adam  per element of emb/* and fo_cat/kernel: the row's run added tile by tile, then Adam (g = 0 for a row the batch did not touch
//                    and for the table of a field outside `order`)
// Arithmetic as in k_train.h: FP32 VALU, operators under `#pragma clang fp contract(off)`, tr_sigmoid and tr_adam; no float atomics; every kernel
// returns at once when the error word is set.  A NaN that reaches p, a parameter, m or v is stored as 0x7fc00000 (trainer_fm.py says why).

static constexpr int TF_MAX_FIELDS = SPRK_TRAIN_FM_MAX_FIELDS, TF_MAX_LAYERS = SPRK_TRAIN_FM_MAX_LAYERS, TF_MAX_GROUPS = SPRK_TRAIN_FM_MAX_FIELDS + 1;
static constexpr int TF_MAX_PROJ = SPRK_TRAIN_FM_MAX_PROJ, TF_MAX_FLAT = SPRK_TRAIN_FM_MAX_FLAT, TF_MAX_WIDTH = SPRK_TRAIN_FM_MAX_WIDTH, TF_MAX_IN = SPRK_TRAIN_FM_MAX_IN;

struct FmDims {                              // a kernel argument, by value
    int n_fields, n_dense, emb_dim, proj, groups, n_layers;
    int n_in;                                // one sample's inputs: (groups - 1) x emb_dim table-row elements in group order, then the numerics
    int flat, cat, wide;                     // groups x proj; 1 + proj + the last hidden width; the widest gradient buffer
    int vocab[TF_MAX_FIELDS], fo_off[TF_MAX_FIELDS];
    int fo_rank[TF_MAX_FIELDS];              // the fields in ascending fo_off order
    int grp_field[TF_MAX_FIELDS], field_grp[TF_MAX_FIELDS];         // group -> field; field -> group or -1
    long long tab_off[TF_MAX_FIELDS];        // the field's emb/ table in the parameter vector (floats)
    long long row_base[TF_MAX_FIELDS + 1];   // its first row among all tables' rows: the schedule's keys
    long long fo_ker, fo_bias, fonum_ker, fonum_bias;
    long long proj_ker[TF_MAX_GROUPS], proj_bias[TF_MAX_GROUPS];
    int width[TF_MAX_LAYERS + 1], fan[TF_MAX_LAYERS + 1];           // the deep layers, then the head (width 1, fan = cat)
    long long ker_off[TF_MAX_LAYERS + 1], bias_off[TF_MAX_LAYERS + 1];
    long long n_emb, n_table, n_params;      // floats of the emb/ tables; + fo_cat/kernel (= the first Dense parameter); of everything
};

__device__ __forceinline__ float tf_canon(float x) { return x != x ? __uint_as_float(0x7fc00000u) : x; }

__device__ inline void tf_adam(float g, float* w, float* m, float* v, float alpha, float c1, float c2, float eps) {
    tr_adam(g, w, m, v, alpha, c1, c2, eps);
    *w = tf_canon(*w);
    *m = tf_canon(*m);
    *v = tf_canon(*v);
}

// One tile of one batch.  Dynamic LDS, floats, per sample of the tile: x [n_in], v [flat], s [proj], c = [first, fm, last activation] [cat], the other
// activations, d_fm [proj], d_first [1], two gradient buffers [wide].  first = the batch's first position, nb = its rows; p_out / de / dfirst are
// indexed by the position in the batch; partial = [tiles][n_params - n_table].
__global__ __launch_bounds__(TR_THREADS) void k_tf_step(FmDims dm, const int* __restrict__ ids, const float* __restrict__ dense, const float* __restrict__ labels,
                                                        const int* __restrict__ order, long long first, int nb, int tile, const float* __restrict__ params,
                                                        float* __restrict__ p_out, float* __restrict__ de, float* __restrict__ dfirst, float* __restrict__ partial,
                                                        const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float tf_lds[];
    if (*err != TR_CLEAN) return;
    const int t0 = blockIdx.x * tile;
    const int cnt = nb - t0 < tile ? nb - t0 : tile;                        // >= 1: the grid is ceil(nb / tile)
    const int L = dm.n_layers, G = dm.groups, P = dm.proj, D = dm.emb_dim, F = dm.n_dense, NI = dm.n_in, FL = dm.flat, CW = dm.cat;
    const int ED = (G - 1) * D;
    float* x = tf_lds;
    float* v = x + (size_t)tile * NI;
    float* S = v + (size_t)tile * FL;
    float* c = S + (size_t)tile * P;
    float* aptr[TF_MAX_LAYERS + 1];                                          // aptr[l] = the input of deep layer l, aptr[L] = the last activation (inside c)
    int astr[TF_MAX_LAYERS + 1];
    aptr[0] = v; astr[0] = FL;
    float* at = c + (size_t)tile * CW;
    for (int l = 0; l + 1 < L; ++l) { aptr[l + 1] = at; astr[l + 1] = dm.width[l]; at += (size_t)tile * dm.width[l]; }
    aptr[L] = c + 1 + P; astr[L] = CW;
    float* dfm = at;
    float* dfst = dfm + (size_t)tile * P;
    float* g0 = dfst + tile;
    float* g1 = g0 + (size_t)tile * dm.wide;

    for (int e = threadIdx.x; e < cnt * NI; e += TR_THREADS) {
        const int i = e / NI, k = e - i * NI;
        const long long pos = first + t0 + i;
        const long long r = order ? order[pos] : pos;
        float xv;
        if (k >= ED) xv = dense[r * F + (k - ED)];
        else {
            const int g = k / D, d = k - g * D, f = dm.grp_field[g];
            const int id = ids[r * dm.n_fields + f];
            xv = id >= 0 ? params[dm.tab_off[f] + (long long)id * D + d] : 0.0f;
        }
        x[e] = xv;
    }
    __syncthreads();

    // first order and the projections
    for (int i = threadIdx.x; i < cnt; i += TR_THREADS) {
        const long long pos = first + t0 + i;
        const long long r = order ? order[pos] : pos;
        float a = 0.0f;
        for (int q = 0; q < dm.n_fields; ++q) {
            const int f = dm.fo_rank[q];
            const int id = ids[r * dm.n_fields + f];
            if (id >= 0) a = a + params[dm.fo_ker + dm.fo_off[f] + id];
        }
        a = a + params[dm.fo_bias];
        float z = 0.0f;
        for (int k = 0; k < F; ++k) z = z + x[i * NI + ED + k] * params[dm.fonum_ker + k];
        z = z + params[dm.fonum_bias];
        c[i * CW] = a + z;
    }
    for (int e = threadIdx.x; e < cnt * FL; e += TR_THREADS) {
        const int i = e / FL, r = e - i * FL;
        const int g = r / P, j = r - g * P;
        const int fan = g < G - 1 ? D : F;
        const float* __restrict__ W = params + dm.proj_ker[g];
        const float* in = x + i * NI + g * D;
        float z = 0.0f;
        for (int k = 0; k < fan; ++k) z = z + in[k] * W[k * P + j];
        v[e] = z + params[dm.proj_bias[g] + j];
    }
    __syncthreads();

    // the FM cross, and the deep stack (its first layer reads v as well)
    for (int e = threadIdx.x; e < cnt * P; e += TR_THREADS) {
        const int i = e / P, j = e - i * P;
        float s = 0.0f, q = 0.0f;
        for (int g = 0; g < G; ++g) {
            const float vv = v[i * FL + g * P + j];
            s = s + vv;
            q = q + vv * vv;
        }
        S[e] = s;
        c[i * CW + 1 + j] = s * s - q;
    }
    for (int l = 0; l < L; ++l) {
        const int fan = dm.fan[l], H = dm.width[l], si = astr[l], so = astr[l + 1];
        const float* __restrict__ W = params + dm.ker_off[l];
        const float* __restrict__ bias = params + dm.bias_off[l];
        const float* in = aptr[l];
        float* out = aptr[l + 1];
        for (int e = threadIdx.x; e < cnt * H; e += TR_THREADS) {
            const int i = e / H, j = e - i * H;
            float z = 0.0f;
            for (int k = 0; k < fan; ++k) z = z + in[i * si + k] * W[k * H + j];
            z = z + bias[j];
            out[i * so + j] = z > 0.0f ? z : 0.0f;
        }
        __syncthreads();
    }
    {
        const float* __restrict__ W = params + dm.ker_off[L];
        const float bh = params[dm.bias_off[L]];
        const float fn = (float)nb;
        for (int i = threadIdx.x; i < cnt; i += TR_THREADS) {
            float z = 0.0f;
            for (int k = 0; k < CW; ++k) z = z + c[i * CW + k] * W[k];
            z = z + bh;
            const float p = z != z ? z : tr_sigmoid(z);
            const long long pos = first + t0 + i;
            p_out[t0 + i] = tf_canon(p);
            g0[i] = (p - labels[order ? order[pos] : pos]) / fn;
        }
        __syncthreads();
    }

    const long long nt = dm.n_table;
    float* __restrict__ mine = partial + (long long)blockIdx.x * (dm.n_params - nt);
    {   // the head: its gradients, d_first, d_fm and the last activation's gradient under its ReLU mask
        const float* __restrict__ W = params + dm.ker_off[L];
        const int HL = dm.width[L - 1];
        for (int k = threadIdx.x; k < CW; k += TR_THREADS) {
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + c[i * CW + k] * g0[i];
            mine[dm.ker_off[L] - nt + k] = s;
        }
        if (threadIdx.x == 0) {
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + g0[i];
            mine[dm.bias_off[L] - nt] = s;
        }
        for (int e = threadIdx.x; e < cnt * CW; e += TR_THREADS) {
            const int i = e / CW, k = e - i * CW;
            float s = 0.0f;
            s = s + W[k] * g0[i];
            if (k == 0) { dfst[i] = s; dfirst[t0 + i] = s; }
            else if (k <= P) dfm[i * P + (k - 1)] = s;
            else g1[i * HL + (k - 1 - P)] = c[e] > 0.0f ? s : 0.0f;
        }
        __syncthreads();
    }
    float* dz = g1;
    float* nx = g0;
    for (int l = L - 1; l >= 0; --l) {
        const int fan = dm.fan[l], H = dm.width[l], sa = astr[l];
        const float* __restrict__ W = params + dm.ker_off[l];
        const float* a = aptr[l];
        for (int e = threadIdx.x; e < fan * H; e += TR_THREADS) {
            const int k = e / H, j = e - k * H;
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + a[i * sa + k] * dz[i * H + j];
            mine[dm.ker_off[l] - nt + e] = s;
        }
        for (int j = threadIdx.x; j < H; j += TR_THREADS) {
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + dz[i * H + j];
            mine[dm.bias_off[l] - nt + j] = s;
        }
        for (int e = threadIdx.x; e < cnt * fan; e += TR_THREADS) {
            const int i = e / fan, k = e - i * fan;
            float s = 0.0f;
            for (int j = 0; j < H; ++j) s = s + W[k * H + j] * dz[i * H + j];
            nx[e] = (l == 0 || a[i * sa + k] > 0.0f) ? s : 0.0f;
        }
        __syncthreads();
        float* t = dz; dz = nx; nx = t;
    }
    // dz = d_flat [cnt][flat]; dv in its place: d_flat + d_fm (2 (s - v))
    for (int e = threadIdx.x; e < cnt * FL; e += TR_THREADS) {
        const int i = e / FL, r = e - i * FL;
        const int j = r % P;
        dz[e] = dz[e] + dfm[i * P + j] * (2.0f * (S[i * P + j] - v[e]));
    }
    __syncthreads();
    for (int g = 0; g < G; ++g) {
        const int fan = g < G - 1 ? D : F;
        for (int e = threadIdx.x; e < fan * P; e += TR_THREADS) {
            const int k = e / P, j = e - k * P;
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + x[i * NI + g * D + k] * dz[i * FL + g * P + j];
            mine[dm.proj_ker[g] - nt + e] = s;
        }
        for (int j = threadIdx.x; j < P; j += TR_THREADS) {
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + dz[i * FL + g * P + j];
            mine[dm.proj_bias[g] - nt + j] = s;
        }
    }
    for (int e = threadIdx.x; e < cnt * ED; e += TR_THREADS) {
        const int i = e / ED, r = e - i * ED;
        const int g = r / D, d = r - g * D;
        const float* __restrict__ W = params + dm.proj_ker[g];
        float s = 0.0f;
        for (int j = 0; j < P; ++j) s = s + W[d * P + j] * dz[i * FL + g * P + j];
        de[(long long)(t0 + i) * ED + r] = s;
    }
    for (int k = threadIdx.x; k < F + 1; k += TR_THREADS) {
        float s = 0.0f;
        if (k < F) {
            for (int i = 0; i < cnt; ++i) s = s + x[i * NI + ED + k] * dfst[i];
            mine[dm.fonum_ker - nt + k] = s;
        } else {
            for (int i = 0; i < cnt; ++i) s = s + dfst[i];
            mine[dm.fo_bias - nt] = s;
            mine[dm.fonum_bias - nt] = s;
        }
    }
}

__global__ __launch_bounds__(TR_THREADS) void k_tf_dense_adam(long long n_table, long long ndp, int tiles, const float* __restrict__ partial, float* __restrict__ params,
                                                              float* __restrict__ m, float* __restrict__ v, const float* __restrict__ alphas, long long step, float c1,
                                                              float c2, float eps, const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    if (*err != TR_CLEAN) return;
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
        tf_adam(g, params + n_table + e, m + n_table + e, v + n_table + e, alpha, c1, c2, eps);
    }
}

// [off[b], off[b + 1]) = the batch's entries, sorted by (row, position); element e < n_emb is (row, dimension) of an emb/ table, beyond it a row of fo_cat/kernel
__global__ __launch_bounds__(TR_THREADS) void k_tf_table_adam(FmDims dm, int tile, const unsigned* __restrict__ off, long long b, const long long* __restrict__ key,
                                                              const float* __restrict__ de, const float* __restrict__ dfirst, float* __restrict__ params,
                                                              float* __restrict__ m, float* __restrict__ v, const float* __restrict__ alphas, long long step, float c1,
                                                              float c2, float eps, const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    if (*err != TR_CLEAN) return;
    const long long seg_lo = off[b], seg_hi = off[b + 1];
    const float alpha = alphas[step];
    const int D = dm.emb_dim, ED = (dm.groups - 1) * D;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < dm.n_table; e += (long long)gridDim.x * TR_THREADS) {
        long long row;                       // among all tables' rows
        const float* src;                    // the per-position gradient this element adds up, or nullptr: g = 0
        int stride;
        if (e < dm.n_emb) {
            row = e / D;
            const int d = (int)(e - row * D);
            int f = 0;
            while (f + 1 < dm.n_fields && row >= dm.row_base[f + 1]) ++f;
            const int g = dm.field_grp[f];
            src = g >= 0 ? de + g * D + d : nullptr;
            stride = ED;
        } else {
            const int r = (int)(e - dm.n_emb);
            int f = 0;
            for (int q = 0; q < dm.n_fields; ++q)
                if (r >= dm.fo_off[q] && r < dm.fo_off[q] + dm.vocab[q]) f = q;
            row = dm.row_base[f] + (r - dm.fo_off[f]);
            src = dfirst;
            stride = 1;
        }
        float g = 0.0f, s = 0.0f;
        int cur = -1;
        if (src) {
            long long lo = seg_lo, hi = seg_hi;
            const long long want = row << 32;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (key[mid] < want) lo = mid + 1; else hi = mid;
            }
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
                s = s + src[(long long)pos * stride];
            }
        }
        if (cur >= 0) g = g + s;
        tf_adam(g, params + e, m + e, v + e, alpha, c1, c2, eps);
    }
}
