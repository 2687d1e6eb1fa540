// k_train_pair.h -- Adam training of the pair-dot DeepFM (first-order weights that are rows of the head's kernel + P explicit dots of FM table rows + a
// deep stack over deep-only tables, one sigmoid): the device side of sparrowrecsys_amd/trainer_pair.py, whose train_host is the DEFINITION of every bit
// computed here.  The schedule is k_train.h's: k_tr_check, k_tr_count, k_tr_scatter and the k_segments.h sort give, per batch,
// one sorted run of positions per (field, id); that run serves the emb/ row, the deep_emb/ row (a deep key, tables not shared) and the head/kernel row of
// width 1.  Per step:
//   k_tp_step        one workgroup per tile of samples: forward, sigmoid_def, backward; p, per position de (every field's FM-row gradient), dd (the
//                    deep tables' row gradients, tables not shared) and dfirst, and the tile's partial sums of every parameter that is no table row
//   k_tp_dense_adam  per such parameter: the tiles' partials added in tile order, then Adam (k_tf_dense_adam over a parameter stretch with a hole:
//                    head/kernel's first-order rows lie between head/bias and head/kernel's Dense tail)
//   k_tp_table_adam  per element of emb/*, deep_emb/* and head/kernel's first-order rows: the row's run added tile by tile, then Adam (g = 0 for a row
//                    the batch did not touch)
// Arithmetic as in k_train.h: FP32 VALU, operators under `#pragma clang fp contract(off)`, tr_sigmoid and tr_adam (through tf_adam: a NaN that reaches
// p, a parameter, m or v is stored as 0x7fc00000); no float atomics; every kernel returns at once when the error word is set.

static constexpr int TP_MAX_FIELDS = SPRK_TRAIN_PAIR_MAX_FIELDS, TP_MAX_PAIRS = SPRK_TRAIN_PAIR_MAX_PAIRS, TP_MAX_LAYERS = SPRK_TRAIN_PAIR_MAX_LAYERS;
static constexpr int TP_MAX_WIDTH = SPRK_TRAIN_PAIR_MAX_WIDTH, TP_MAX_X = SPRK_TRAIN_PAIR_MAX_X, TP_MAX_DIM = SPRK_TRAIN_PAIR_MAX_DIM;

struct PairDims {                            // a kernel argument, by value (about 2.6 KB)
    int n_fields, n_dense, emb_dim, n_pairs, n_deep, shared, n_x, n_layers;
    int wide;                                // the widest gradient buffer: the deep input or a hidden layer
    int fo_total;                            // head/kernel's first-order rows
    int vocab[TP_MAX_FIELDS], fo_off[TP_MAX_FIELDS];
    int fo_rank[TP_MAX_FIELDS];              // the fields in ascending fo_off order
    int deep_col[TP_MAX_FIELDS], field_slot[TP_MAX_FIELDS];         // deep table -> field; field -> deep table or -1
    int width[TP_MAX_LAYERS], fan[TP_MAX_LAYERS];
    long long tab_off[TP_MAX_FIELDS];        // the field's emb/ table in the parameter vector (floats)
    long long dtab_off[TP_MAX_FIELDS];       // deep table j: deep_emb/, or the field's emb/ table when shared
    long long row_base[TP_MAX_FIELDS + 1];   // the field's first row among all fields' rows: the schedule's keys
    long long ker_off[TP_MAX_LAYERS], bias_off[TP_MAX_LAYERS];
    long long head_bias, head_ker;           // head/kernel's row 0; its Dense tail [n_pairs + last width] starts at head_ker + fo_total
    long long n_emb, n_tab;                  // floats of the emb/ tables; + the deep_emb/ tables (= the first Dense parameter)
    long long nd1, ndp;                      // Dense floats before head/kernel (deep layers, head/bias); + head/kernel's tail: a tile's partial sums
    long long n_params;
    signed char pair_a[TP_MAX_PAIRS], pair_b[TP_MAX_PAIRS];
    signed char xsrc[TP_MAX_X];              // per deep input row: its deep table, -1 = a numeric
    short xsub[TP_MAX_X];                    // the element of the table row, or the numeric
    short xinv[TP_MAX_FIELDS * TP_MAX_DIM];  // [deep table][element] -> the deep input row
};

// One tile of one batch.  Dynamic LDS, floats, per sample of the tile: ef [fields][emb_dim] (the FM rows), x [n_x], the activations, dots [pairs],
// td [pairs] (the dots' gradients), two gradient buffers [wide].  first = the batch's first position, nb = its rows; p_out / de / dd / dfirst are indexed
// by the position in the batch; partial = [tiles][ndp].
__global__ __launch_bounds__(TR_THREADS) void k_tp_step(PairDims dm, const int* __restrict__ ids, const float* __restrict__ dense, const float* __restrict__ labels,
                                                        const int* __restrict__ order, long long first, int nb, int tile, const float* __restrict__ params,
                                                        float* __restrict__ p_out, float* __restrict__ de, float* __restrict__ dd, float* __restrict__ dfirst,
                                                        float* __restrict__ partial, const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float tp_lds[];
    if (*err != TR_CLEAN) return;
    const int t0 = blockIdx.x * tile;
    const int cnt = nb - t0 < tile ? nb - t0 : tile;                        // >= 1: the grid is ceil(nb / tile)
    const int NF = dm.n_fields, D = dm.emb_dim, FD = NF * D, NX = dm.n_x, P = dm.n_pairs, L = dm.n_layers, ND = dm.n_deep, F = dm.n_dense;
    const int HL = dm.width[L - 1], CW = P + HL;
    float* ef = tp_lds;
    float* act[TP_MAX_LAYERS + 1];                                           // act[l] = the input of deep layer l, act[L] = the last activation
    act[0] = ef + (size_t)tile * FD;
    float* at = act[0] + (size_t)tile * NX;
    for (int l = 0; l < L; ++l) { act[l + 1] = at; at += (size_t)tile * dm.width[l]; }
    float* dots = at;
    float* td = dots + (size_t)tile * P;
    float* g0 = td + (size_t)tile * P;
    float* g1 = g0 + (size_t)tile * dm.wide;

    for (int e = threadIdx.x; e < cnt * FD; e += TR_THREADS) {
        const int i = e / FD, r = e - i * FD;
        const int f = r / D, d = r - f * D;
        const long long pos = first + t0 + i;
        const long long row = order ? order[pos] : pos;
        const int id = ids[row * NF + f];
        ef[e] = id >= 0 ? params[dm.tab_off[f] + (long long)id * D + d] : 0.0f;
    }
    for (int e = threadIdx.x; e < cnt * NX; e += TR_THREADS) {
        const int i = e / NX, k = e - i * NX;
        const long long pos = first + t0 + i;
        const long long row = order ? order[pos] : pos;
        const int j = dm.xsrc[k], s = dm.xsub[k];
        float xv;
        if (j < 0) xv = dense[row * F + s];
        else {
            const int id = ids[row * NF + dm.deep_col[j]];
            xv = id >= 0 ? params[dm.dtab_off[j] + (long long)id * D + s] : 0.0f;
        }
        act[0][e] = xv;
    }
    __syncthreads();

    // the pair dots, and the deep stack
    for (int e = threadIdx.x; e < cnt * P; e += TR_THREADS) {
        const int i = e / P, q = e - i * P;
        const float* ea = ef + i * FD + dm.pair_a[q] * D;
        const float* eb = ef + i * FD + dm.pair_b[q] * D;
        float s = 0.0f;
        for (int d = 0; d < D; ++d) s = s + ea[d] * eb[d];
        dots[e] = s;
    }
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
    const float* aL = act[L];
    const float* __restrict__ Wt = params + dm.head_ker + dm.fo_total;      // head/kernel's Dense tail: the pairs' rows, then the last activation's
    {
        const float bh = params[dm.head_bias];
        const float fn = (float)nb;
        for (int i = threadIdx.x; i < cnt; i += TR_THREADS) {
            const long long pos = first + t0 + i;
            const long long row = order ? order[pos] : pos;
            float z = 0.0f;
            for (int q = 0; q < NF; ++q) {
                const int f = dm.fo_rank[q];
                const int id = ids[row * NF + f];
                if (id >= 0) z = z + params[dm.head_ker + dm.fo_off[f] + id];
            }
            for (int q = 0; q < P; ++q) z = z + dots[i * P + q] * Wt[q];
            for (int j = 0; j < HL; ++j) z = z + aL[i * HL + j] * Wt[P + j];
            z = z + bh;
            const float p = z != z ? z : tr_sigmoid(z);
            p_out[t0 + i] = tf_canon(p);
            const float dl = (tf_canon(p) - labels[row]) / fn;
            g0[i] = dl;
            dfirst[t0 + i] = dl;
        }
        __syncthreads();
    }

    float* __restrict__ mine = partial + (long long)blockIdx.x * dm.ndp;
    {   // the head: its Dense tail's gradients and its bias's, the dots' gradients t and the last activation's gradient under its ReLU mask
        for (int k = threadIdx.x; k < CW; k += TR_THREADS) {
            float s = 0.0f;
            if (k < P)
                for (int i = 0; i < cnt; ++i) s = s + dots[i * P + k] * g0[i];
            else
                for (int i = 0; i < cnt; ++i) s = s + aL[i * HL + (k - P)] * g0[i];
            mine[dm.nd1 + k] = s;
        }
        if (threadIdx.x == 0) {
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + g0[i];
            mine[dm.head_bias - dm.n_tab] = s;
        }
        for (int e = threadIdx.x; e < cnt * CW; e += TR_THREADS) {
            const int i = e / CW, k = e - i * CW;
            float s = 0.0f;
            s = s + Wt[k] * g0[i];
            if (k < P) td[i * P + k] = s;
            else g1[i * HL + (k - P)] = aL[i * HL + (k - P)] > 0.0f ? s : 0.0f;
        }
        __syncthreads();
    }
    float* dz = g1;
    float* nx = g0;
    for (int l = L - 1; l >= 0; --l) {
        const int fan = dm.fan[l], H = dm.width[l];
        const float* __restrict__ W = params + dm.ker_off[l];
        const float* a = act[l];
        for (int e = threadIdx.x; e < fan * H; e += TR_THREADS) {
            const int k = e / H, j = e - k * H;
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + a[i * fan + k] * dz[i * H + j];
            mine[dm.ker_off[l] - dm.n_tab + e] = s;
        }
        for (int j = threadIdx.x; j < H; j += TR_THREADS) {
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + dz[i * H + j];
            mine[dm.bias_off[l] - dm.n_tab + j] = s;
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
    // dz = the deep input's gradient [cnt][n_x].  A field's FM-row gradient: from +0, the pairs in pair order -- as a: t e_b, then as b: t e_a --, then
    // (shared tables) the deep input's gradient of that key.
    for (int e = threadIdx.x; e < cnt * FD; e += TR_THREADS) {
        const int i = e / FD, r = e - i * FD;
        const int f = r / D, d = r - f * D;
        const float* row = ef + i * FD + d;
        float s = 0.0f;
        for (int q = 0; q < P; ++q) {
            const int a = dm.pair_a[q], b = dm.pair_b[q];
            const float t = td[i * P + q];
            if (a == f) s = s + t * row[b * D];
            if (b == f) s = s + t * row[a * D];
        }
        const int j = dm.field_slot[f];
        if (dm.shared && j >= 0) s = s + dz[i * NX + dm.xinv[j * D + d]];
        de[(long long)(t0 + i) * FD + r] = s;
    }
    if (!dm.shared) {
        const int DD = ND * D;
        for (int e = threadIdx.x; e < cnt * DD; e += TR_THREADS) {
            const int i = e / DD, r = e - i * DD;
            dd[(long long)(t0 + i) * DD + r] = dz[i * NX + dm.xinv[r]];
        }
    }
}

// partial = [tiles][ndp]; element e < nd1 is parameter n_tab + e, beyond it parameter n_tab + gap + e: head/kernel's first-order rows lie between
__global__ __launch_bounds__(TR_THREADS) void k_tp_dense_adam(long long n_tab, long long nd1, long long gap, long long ndp, int tiles, const float* __restrict__ partial,
                                                              float* __restrict__ params, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ alphas,
                                                              long long step, float c1, float c2, float eps, const unsigned long long* __restrict__ err) {
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
        const long long at = n_tab + e + (e < nd1 ? 0 : gap);
        tf_adam(g, params + at, m + at, v + at, alpha, c1, c2, eps);
    }
}

// [off[b], off[b + 1]) = the batch's entries, sorted by (row, position); element e < n_emb is (row, dimension) of an emb/ table, e < n_tab of a deep_emb/
// table, beyond it a first-order row of head/kernel
__global__ __launch_bounds__(TR_THREADS) void k_tp_table_adam(PairDims dm, int tile, const unsigned* __restrict__ off, long long b, const long long* __restrict__ key,
                                                              const float* __restrict__ de, const float* __restrict__ dd, const float* __restrict__ dfirst,
                                                              float* __restrict__ params, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ alphas,
                                                              long long step, float c1, float c2, float eps, const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    if (*err != TR_CLEAN) return;
    const long long seg_lo = off[b], seg_hi = off[b + 1];
    const float alpha = alphas[step];
    const int D = dm.emb_dim;
    const long long total = dm.n_tab + dm.fo_total;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TR_THREADS) {
        long long row, at;                   // among all fields' rows; in the parameter vector
        const float* src;                    // the per-position gradient this element adds up
        int stride;
        if (e < dm.n_emb) {
            row = e / D;
            const int d = (int)(e - row * D);
            int f = 0;
            while (f + 1 < dm.n_fields && row >= dm.row_base[f + 1]) ++f;
            src = de + f * D + d;
            stride = dm.n_fields * D;
            at = e;
        } else if (e < dm.n_tab) {
            int j = 0;
            while (j + 1 < dm.n_deep && e >= dm.dtab_off[j + 1]) ++j;
            const long long local = e - dm.dtab_off[j];
            const long long lr = local / D;
            const int d = (int)(local - lr * D);
            row = dm.row_base[dm.deep_col[j]] + lr;
            src = dd + j * D + d;
            stride = dm.n_deep * D;
            at = e;
        } else {
            const int r = (int)(e - dm.n_tab);
            int f = 0;
            for (int q = 0; q < dm.n_fields; ++q)
                if (r >= dm.fo_off[q] && r < dm.fo_off[q] + dm.vocab[q]) f = q;
            row = dm.row_base[f] + (r - dm.fo_off[f]);
            src = dfirst;
            stride = 1;
            at = dm.head_ker + r;
        }
        float g = 0.0f, s = 0.0f;
        int cur = -1;
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
        if (cur >= 0) g = g + s;
        tf_adam(g, params + at, m + at, v + at, alpha, c1, c2, eps);
    }
}
