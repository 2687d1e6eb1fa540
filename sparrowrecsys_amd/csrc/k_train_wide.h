// k_train_wide.h -- Adam training of Wide&Deep: EmbeddingMLP's graph (k_train.h) plus a wide term in the head whose parameter row is chosen by a hash
// of two id columns: the device side of sparrowrecsys_amd/trainer_wide.py, whose train_host is the DEFINITION of every bit computed here (DESIGN.md
// section 5.20).  From k_train.h, unchanged: k_tr_check, k_tr_invmap, k_tr_dense_adam, k_tr_table_adam (the ten deep tables), tr_sigmoid, tr_adam.
//   k_trw_buckets     once per fit: bucket[row] = FingerprintCat64(0xDECAFCAFFE, a, b) mod buckets (the 64-bit modulo is paid here, not per step)
//   k_trw_count / k_trw_scatter   k_tr_count / k_tr_scatter with the tableless column's entry replaced by the cross row's: one per sample, keyed
//                     (deep rows + bucket) << 32 | position in the batch, so the one segment sort orders both
//   k_trw_step        k_tr_step with the wide term in the head; per position also dc [cw]: dl (indicator form) or dl * head/kernel[H + d]; the
//                     sample's cross row is marked in a bitmap (an integer atomicOr) that the host clears before every step
//   k_trw_cross_adam  per (cross row, dimension): the row's run in the batch's sorted entries added tile by tile, then Adam (g = +0 for a row the
//                     batch did not hash to: its bit is clear and nothing is searched -- of 10 M rows a batch of 4096 marks at most 4096, and
//                     twelve dependent loads per element were nine tenths of the step, docs/train_wide_results.md)
// The TrainDims of a wide model (api_train_wide.h): n_cols counts the tableless last column (ids' stride, k_tr_check's range) while the tables,
// row_base and n_table cover the columns before it; the head's bias comes BEFORE its kernel; fan[n_layers] is the deep fan H and n_params ends
// the Dense parameters (the cross_dim extra rows of head/kernel included): the cross rows -- cross_buckets x cw floats -- follow at n_params.
// cw = max(1, cross_dim).  FP32 VALU, `#pragma clang fp contract(off)`, no float atomics, as k_train.h.

static constexpr int TRW_MAX_CROSS_DIM = SPRK_TRAIN_WIDE_MAX_CROSS_DIM;

// the chain of k_tile_forward.h's cross_bucket and oracle.farmhash64.cross_hashed, restated: this unit uses nothing of the engine's
__device__ inline unsigned long long trw_mix(unsigned long long v) { return v ^ (v >> 47); }
__device__ inline unsigned long long trw_cat64(unsigned long long fp1, unsigned long long fp2) {
    const unsigned long long mul = 0xc6a4a7935bd1e995ull;
    unsigned long long r = fp1 ^ mul;
    r ^= trw_mix(fp2 * mul) * mul;
    r *= mul;
    r = trw_mix(r) * mul;
    return trw_mix(r);
}

__global__ __launch_bounds__(TR_THREADS) void k_trw_buckets(long long n, const int* __restrict__ ids, int n_cols, int ca, int cb, unsigned long long buckets,
                                                            int* __restrict__ bucket, const unsigned long long* __restrict__ err) {
    if (*err != TR_CLEAN) return;                                            // (a bucket is only ever hashed from ids inside their vocabularies)
    for (long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * TR_THREADS) {
        unsigned long long h = 0xDECAFCAFFEull;
        h = trw_cat64(h, (unsigned long long)(long long)ids[i * n_cols + ca]);
        h = trw_cat64(h, (unsigned long long)(long long)ids[i * n_cols + cb]);
        bucket[i] = (int)(h % buckets);
    }
}

// entries per batch: off[b] += 1 per (position, deep column) with id >= 0, and 1 per position for the cross row (column cb's turn)
__global__ __launch_bounds__(TR_THREADS) void k_trw_count(long long n, int batch, const int* __restrict__ ids, const int* __restrict__ order, int n_cols, int cb,
                                                          unsigned* __restrict__ off) {
    const long long total = n * n_cols;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TR_THREADS) {
        const long long i = e / n_cols;
        const int c = (int)(e - i * n_cols);
        const long long r = order ? order[i] : i;
        if (c == cb || ids[r * n_cols + c] >= 0) atomicAdd(&off[i / batch], 1u);
    }
}

__global__ __launch_bounds__(TR_THREADS) void k_trw_scatter(long long n, int batch, const int* __restrict__ ids, const int* __restrict__ order, TrainDims dm, int cb,
                                                            const int* __restrict__ bucket, const unsigned* __restrict__ off, unsigned* __restrict__ cursor,
                                                            long long* __restrict__ key, int* __restrict__ val, const unsigned long long* __restrict__ err) {
    if (*err != TR_CLEAN) return;
    const long long total = n * dm.n_cols;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TR_THREADS) {
        const long long i = e / dm.n_cols;
        const int c = (int)(e - i * dm.n_cols);
        const long long r = order ? order[i] : i;
        long long row;
        if (c == cb) row = dm.row_base[dm.n_cols] + bucket[r];              // the cross rows come after every deep table's
        else {
            const int id = ids[r * dm.n_cols + c];
            if (id < 0) continue;
            row = dm.row_base[c] + id;
        }
        const long long b = i / batch;
        const unsigned slot = off[b] + atomicAdd(&cursor[b], 1u);           // < off[b + 1]: k_trw_count counted this entry
        key[slot] = row << 32 | (i - b * batch);
        val[slot] = c;
    }
}

// One tile of one batch: k_tr_step's LDS (x, the activations, two gradient buffers), then e [tile][cross_dim] in the embedding form.
// dx [position][n_x] and dc [position][cw] are indexed by the position in the batch; partial = [tiles][n_params - n_table].
__global__ __launch_bounds__(TR_THREADS) void k_trw_step(TrainDims dm, int cross_dim, const int* __restrict__ bucket, const int* __restrict__ ids,
                                                         const float* __restrict__ dense, const float* __restrict__ labels, const int* __restrict__ order, long long first,
                                                         int nb, int tile, int wide, const float* __restrict__ params, float* __restrict__ p_out, float* __restrict__ dx,
                                                         float* __restrict__ dc, unsigned* __restrict__ touched, float* __restrict__ partial,
                                                         const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float trw_lds[];
    if (*err != TR_CLEAN) return;
    const int t0 = blockIdx.x * tile;
    const int cnt = nb - t0 < tile ? nb - t0 : tile;                        // >= 1: the grid is ceil(nb / tile)
    const int L = dm.n_layers, n_x = dm.n_x;
    float* act[TR_MAX_LAYERS + 1];
    act[0] = trw_lds;
    float* g0 = trw_lds + (size_t)tile * n_x;
    for (int l = 0; l < L; ++l) { act[l + 1] = g0; g0 += (size_t)tile * dm.width[l]; }
    float* g1 = g0 + (size_t)tile * wide;
    float* ce = g1 + (size_t)tile * wide;
    const float* __restrict__ cross = params + dm.n_params;

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
    for (int e = threadIdx.x; e < cnt * cross_dim; e += TR_THREADS) {
        const int i = e / cross_dim, d = e - i * cross_dim;
        const long long pos = first + t0 + i;
        ce[e] = cross[(long long)bucket[order ? order[pos] : pos] * cross_dim + d];
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
    const int cw = cross_dim > 0 ? cross_dim : 1;
    {
        const int fan = dm.fan[L];
        const float* __restrict__ W = params + dm.ker_off[L];
        const float bh = params[dm.bias_off[L]];
        const float* in = act[L];
        const float fn = (float)nb;
        for (int i = threadIdx.x; i < cnt; i += TR_THREADS) {
            const long long pos = first + t0 + i;
            const long long r = order ? order[pos] : pos;
            float z = 0.0f;
            for (int k = 0; k < fan; ++k) z = z + in[i * fan + k] * W[k];
            if (cross_dim > 0)
                for (int d = 0; d < cross_dim; ++d) z = z + ce[i * cross_dim + d] * W[fan + d];
            else
                z = z + cross[bucket[r]];                                    // the indicator's one row: its product with 1 is exact
            z = z + bh;
            const float p = tr_sigmoid(z);
            p_out[t0 + i] = p;
            const float dl = (p - labels[r]) / fn;
            g0[i] = dl;
            atomicOr(&touched[bucket[r] >> 5], 1u << (bucket[r] & 31));
            if (cross_dim > 0)
                for (int d = 0; d < cross_dim; ++d) dc[(long long)(t0 + i) * cw + d] = dl * W[fan + d];
            else
                dc[t0 + i] = dl;
        }
        __syncthreads();
    }

    const long long ndp = dm.n_params - dm.n_table;
    float* __restrict__ mine = partial + (long long)blockIdx.x * ndp;
    for (int d = threadIdx.x; d < cross_dim; d += TR_THREADS) {             // head/kernel[H + d]: e's column against dl
        float s = 0.0f;
        for (int i = 0; i < cnt; ++i) s = s + ce[i * cross_dim + d] * g0[i];
        mine[dm.ker_off[L] - dm.n_table + dm.fan[L] + d] = s;
    }
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

// The batch's cross entries are the last nb of its segment [off[b], off[b + 1]): one per sample, keyed above every deep row.
__global__ __launch_bounds__(TR_THREADS) void k_trw_cross_adam(long long row0, long long n_cross, int cw, int tile, const unsigned* __restrict__ off, long long b, int nb,
                                                               const long long* __restrict__ key, const unsigned* __restrict__ touched, const float* __restrict__ dc,
                                                               float* __restrict__ params, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ alphas, long long step, float c1,
                                                               float c2, float eps, const unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
    if (*err != TR_CLEAN) return;
    const long long seg_hi = off[b + 1], seg_lo = seg_hi - nb;
    const float alpha = alphas[step];
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < n_cross; e += (long long)gridDim.x * TR_THREADS) {
        const long long row = e / cw;
        const int d = (int)(e - row * cw);
        long long lo = seg_hi, hi = seg_hi;
        if (touched[row >> 5] >> (row & 31) & 1u) lo = seg_lo;
        const long long want = (row0 + row) << 32;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (key[mid] < want) lo = mid + 1; else hi = mid;
        }
        float g = 0.0f, s = 0.0f;
        int cur = -1;
        for (; lo < seg_hi; ++lo) {
            const long long kk = key[lo];
            if ((kk >> 32) != row0 + row) break;
            const int pos = (int)(kk & 0xffffffffll);
            const int t = pos / tile;
            if (t != cur) {
                if (cur >= 0) g = g + s;
                s = 0.0f;
                cur = t;
            }
            s = s + dc[(long long)pos * cw + d];
        }
        if (cur >= 0) g = g + s;
        tr_adam(g, params + e, m + e, v + e, alpha, c1, c2, eps);
    }
}
