// api_item2vec.h -- C ABI: sprk_item_sequences (ratings -> per-user item sequences and item counts), sprk_item_walks (sequences -> random
// walks over their transition graph) and sprk_skipgram_fit (sequences or walks + the host's vocabulary tables -> item vectors), k_item2vec.h.  From host_segments.h: the carver and the workspace check, the grids,
// seg_scan and seg_sort.  Every argument is checked before any device call; the calls enqueue their kernels on the caller's stream and
// return: no synchronisation, no memory of their own.
namespace {
struct SeqWorkspace {
    unsigned* off;                 // [n_users + 1]  len, then its exclusive scan                       [zeroed]
    unsigned* cursor;              // [n_users]                                                         [zeroed]
    unsigned* words;               // [4]            word 0: the long segments                          [zeroed]
    size_t zeroed_bytes;
    unsigned* tops;                // [n_tiles]
    int* long_list;                // [n / 64 + 1]
    long long* key;                // [n]            timestamp
    long long* tmp_key;            // [n]
    int* val;                      // [n]            input row
    int* tmp_val;                  // [n]
    int tiles;
    size_t bytes;
};
inline bool seq_sizes_ok(int64_t n, int32_t n_users, int32_t n_items) {
    return n >= 0 && n < 0x7fffffffll && n_users >= 0 && n_users < 0x7fffffff && n_items >= 0 && n_items < 0x7fffffff;
}
SeqWorkspace seq_carve(void* base, int64_t n, int32_t n_users) {
    SeqWorkspace w;
    Carver c{base};
    const size_t nu = (size_t)n_users, nr = (size_t)n;
    w.off = c.take<unsigned>(nu + 1);
    w.cursor = c.take<unsigned>(nu);
    w.words = c.take<unsigned>(4);
    w.zeroed_bytes = c.at;
    w.tiles = seg_scan_tiles(nu);
    w.tops = c.take<unsigned>((size_t)w.tiles);
    w.long_list = c.take<int>(nr / 64 + 1);
    w.key = c.take<long long>(nr);
    w.tmp_key = c.take<long long>(nr);
    w.val = c.take<int>(nr);
    w.tmp_val = c.take<int>(nr);
    w.bytes = c.at;
    return w;
}

struct SkipWorkspace {
    unsigned* a;                   // [n + 1]        kept flags, then their exclusive scan: positions   [zeroed]
    unsigned* off;                 // [2 V + 1]      records per row, then their exclusive scan          [zeroed]
    unsigned* cursor;              // [2 V]                                                             [zeroed]
    unsigned* words;               // [4]            word 0: the long segments                          [zeroed]
    int* pos_word;                 // [N]                                                               [zeroed]
    unsigned* pos_lo;              // [N]                                                               [zeroed]
    unsigned* pos_hi;              // [N]                                                               [zeroed]
    size_t zeroed_bytes;
    unsigned* tops;                // [n_tiles]      (the larger scan's)
    int* long_list;                // [T / 64 + 1]
    long long* key;                // [T]            T = N (2 window + 40): room for every record
    long long* tmp_key;            // [T]
    int* val;                      // [T]
    int* tmp_val;                  // [T]
    float* E0;                     // [R' (2 window + 1) D]   R' = min(round, max(N, 1))
    float* E1;                     // [R' 40 D]
    double* pos_loss;              // [N]
    unsigned* pos_terms;           // [N]
    double* chunk_loss;            // [ceil(N / 1024)]
    unsigned long long* chunk_terms;
    int tiles_a, tiles_off;
    long long records, round;
    size_t bytes;
};
inline bool skip_sizes_ok(int64_t n, int32_t n_seq, int32_t V, int64_t N, int32_t D, int32_t window, int32_t round) {
    return n >= 0 && n < 0x7fffffffll && n_seq >= 0 && n_seq < 0x7fffffff && V >= 0 && V < 0x3fffffff && N >= 0 && N <= n && D >= 1 && D <= I2V_MAX_D &&
           window >= 1 && window <= I2V_MAX_WINDOW && round >= 1 && N * (2ll * window + I2V_MAX_CODE) < 0x7fffffffll && (n == 0 || n_seq > 0) && (V > 0 || N == 0);
}
SkipWorkspace skip_carve(void* base, int64_t n, int32_t V, int64_t N, int32_t D, int32_t window, int32_t round) {
    SkipWorkspace w;
    Carver c{base};
    const size_t nn = (size_t)n, nv = (size_t)V, np = (size_t)N;
    w.records = N * (2ll * window + I2V_MAX_CODE);
    w.round = round < (N > 1 ? N : 1) ? round : (N > 1 ? N : 1);
    const size_t nt = (size_t)w.records, nr = (size_t)w.round;
    w.a = c.take<unsigned>(nn + 1);
    w.off = c.take<unsigned>(2 * nv + 1);
    w.cursor = c.take<unsigned>(2 * nv);
    w.words = c.take<unsigned>(4);
    w.pos_word = c.take<int>(np);
    w.pos_lo = c.take<unsigned>(np);
    w.pos_hi = c.take<unsigned>(np);
    w.zeroed_bytes = c.at;
    w.tiles_a = seg_scan_tiles(nn);
    w.tiles_off = seg_scan_tiles(2 * nv);
    w.tops = c.take<unsigned>((size_t)(w.tiles_a > w.tiles_off ? w.tiles_a : w.tiles_off));
    w.long_list = c.take<int>(nt / 64 + 1);
    w.key = c.take<long long>(nt);
    w.tmp_key = c.take<long long>(nt);
    w.val = c.take<int>(nt);
    w.tmp_val = c.take<int>(nt);
    w.E0 = c.take<float>(nr * (size_t)(2 * window + 1) * (size_t)D);
    w.E1 = c.take<float>(nr * (size_t)I2V_MAX_CODE * (size_t)D);
    w.pos_loss = c.take<double>(np);
    w.pos_terms = c.take<unsigned>(np);
    w.chunk_loss = c.take<double>(np / I2V_LOSS_CHUNK + 1);
    w.chunk_terms = c.take<unsigned long long>(np / I2V_LOSS_CHUNK + 1);
    w.bytes = c.at;
    return w;
}

struct WalkWorkspace {
    unsigned* off;                 // [n_items + 1]  pairs per `prev`, then their exclusive scan        [zeroed]
    unsigned* cursor;              // [n_items]                                                         [zeroed]
    unsigned* words;               // [4]            word 0: the long segments                          [zeroed]
    unsigned* wlen;                // [sample_count + 1]  walk lengths, then their exclusive scan       [zeroed]
    size_t zeroed_bytes;
    unsigned* tops;                // [n_tiles]      (the larger scan's)
    int* long_list;                // [n / 64 + 1]
    long long* key;                // [n]            next
    long long* tmp_key;            // [n]
    int* val;                      // [n]            place in the input
    int* tmp_val;                  // [n]
    int* padded;                   // [sample_count sample_length]
    int tiles_off, tiles_walk;
    size_t bytes;
};
inline bool walk_sizes_ok(int64_t n, int32_t n_seq, int32_t n_items, int64_t sample_count, int32_t sample_length) {
    return n >= 0 && n < 0x7fffffffll && n_seq >= 0 && n_seq < 0x7fffffff && n_items >= 0 && n_items < 0x7fffffff && sample_count >= 0 && sample_length >= 1 &&
           sample_count < 0x7fffffffll && sample_count * sample_length < 0x7fffffffll && (n == 0 || n_seq > 0);
}
WalkWorkspace walk_carve(void* base, int64_t n, int32_t n_items, int64_t sample_count, int32_t sample_length) {
    WalkWorkspace w;
    Carver c{base};
    const size_t nn = (size_t)n, ni = (size_t)n_items, ns = (size_t)sample_count;
    w.off = c.take<unsigned>(ni + 1);
    w.cursor = c.take<unsigned>(ni);
    w.words = c.take<unsigned>(4);
    w.wlen = c.take<unsigned>(ns + 1);
    w.zeroed_bytes = c.at;
    w.tiles_off = seg_scan_tiles(ni);
    w.tiles_walk = seg_scan_tiles(ns);
    w.tops = c.take<unsigned>((size_t)(w.tiles_off > w.tiles_walk ? w.tiles_off : w.tiles_walk));
    w.long_list = c.take<int>(nn / 64 + 1);
    w.key = c.take<long long>(nn);
    w.tmp_key = c.take<long long>(nn);
    w.val = c.take<int>(nn);
    w.tmp_val = c.take<int>(nn);
    w.padded = c.take<int>(ns * (size_t)sample_length);
    w.bytes = c.at;
    return w;
}
}  // namespace

extern "C" {

size_t sprk_item_walks_workspace_bytes(int64_t n_seq_items, int32_t n_seq, int32_t n_items, int64_t sample_count, int32_t sample_length) {
    if (!walk_sizes_ok(n_seq_items, n_seq, n_items, sample_count, sample_length)) return 0;
    return walk_carve(nullptr, n_seq_items, n_items, sample_count, sample_length).bytes;
}

int sprk_item_walks(const int32_t* seq_offsets, const int32_t* seq_items, int64_t n_seq_items, int32_t n_seq, int32_t n_items,
                    int64_t sample_count, int32_t sample_length, uint64_t seed, int32_t* walk_offsets, int32_t* walk_items,
                    uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_item_walks");
    if (!walk_sizes_ok(n_seq_items, n_seq, n_items, sample_count, sample_length))
        return fail(SPRK_EINVAL, "item_walks: bad sizes (need 0 <= n_seq_items < 2^31 - 1, n_seq > 0 unless empty, 0 <= n_items < 2^31 - 1, sample_length >= 1, "
                                 "0 <= sample_count sample_length < 2^31 - 1)");
    if (!error_key) return fail(SPRK_EINVAL, "item_walks: NULL error word");
    if ((uintptr_t)error_key & 7) return fail(SPRK_EINVAL, "item_walks: misaligned error word");
    if (!seq_offsets || !walk_offsets) return fail(SPRK_EINVAL, "item_walks: NULL offsets");
    if (n_seq_items > 0 && !seq_items) return fail(SPRK_EINVAL, "item_walks: NULL seq_items");
    if (sample_count > 0 && !walk_items) return fail(SPRK_EINVAL, "item_walks: NULL walk_items");
    if (((uintptr_t)seq_offsets & 3) || ((uintptr_t)seq_items & 3) || ((uintptr_t)walk_offsets & 3) || ((uintptr_t)walk_items & 3))
        return fail(SPRK_EINVAL, "item_walks: misaligned column");
    const WalkWorkspace w = walk_carve(workspace, n_seq_items, n_items, sample_count, sample_length);
    SPRK_TRY(check_workspace("item_walks", "sprk_item_walks_workspace_bytes", workspace, workspace_bytes, w.bytes));
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_seq_items;
    unsigned long long* err = (unsigned long long*)error_key;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_i2v_pair_count, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, (int)n_seq, seq_offsets, seq_items, (int)n_items, w.off, err);
        HIP_TRY(hipGetLastError());
    }
    SPRK_TRY(seg_scan(w.off, (long long)n_items + 1, w.tops, w.tiles_off, FeScanKept<false>{}, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_i2v_pair_scatter, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, (int)n_seq, seq_offsets, seq_items, (int)n_items, (const unsigned*)w.off,
                           w.cursor, w.key, w.val);
        HIP_TRY(hipGetLastError());
        SPRK_TRY(seg_sort(cap, n, n_items, w.off, w.key, w.val, w.tmp_key, w.tmp_val, w.long_list, w.words, nullptr, st));
    }
    if (sample_count > 0) {
        hipLaunchKernelGGL(k_i2v_walk, dim3(fe_grid_capped(sample_count)), dim3(FE_THREADS), 0, st, (long long)sample_count, (int)sample_length, (unsigned long long)seed,
                           (int)n_items, (const unsigned*)w.off, (const long long*)w.key, w.padded, w.wlen);
        HIP_TRY(hipGetLastError());
    }
    SPRK_TRY(seg_scan(w.wlen, (long long)sample_count + 1, w.tops, w.tiles_walk, FeScanKept<false>{}, st));
    hipLaunchKernelGGL(k_i2v_walk_emit, dim3(fe_grid_capped(sample_count + 1)), dim3(FE_THREADS), 0, st, (long long)sample_count, (int)sample_length, (const unsigned*)w.wlen,
                       (const int*)w.padded, walk_offsets, walk_items);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}


size_t sprk_item_sequences_workspace_bytes(int64_t n_ratings, int32_t n_users, int32_t n_items) {
    if (!seq_sizes_ok(n_ratings, n_users, n_items)) return 0;
    return seq_carve(nullptr, n_ratings, n_users).bytes;
}

int sprk_item_sequences(const int32_t* user_id, const int32_t* movie_id, const float* rating, const int64_t* timestamp, int64_t n_ratings,
                        int32_t n_users, int32_t n_items, int32_t* seq_offsets, int32_t* seq_items, int32_t* item_count,
                        uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_item_sequences");
    if (!seq_sizes_ok(n_ratings, n_users, n_items))
        return fail(SPRK_EINVAL, "item_sequences: bad sizes (need 0 <= n_ratings < 2^31 - 1, 0 <= n_users < 2^31 - 1, 0 <= n_items < 2^31 - 1)");
    if (!error_key) return fail(SPRK_EINVAL, "item_sequences: NULL error word");
    if ((uintptr_t)error_key & 7) return fail(SPRK_EINVAL, "item_sequences: misaligned error word");
    if (n_ratings > 0 && (!user_id || !movie_id || !rating || !timestamp || !seq_items)) return fail(SPRK_EINVAL, "item_sequences: NULL rating column or seq_items");
    if (!seq_offsets) return fail(SPRK_EINVAL, "item_sequences: NULL seq_offsets");
    if (n_items > 0 && !item_count) return fail(SPRK_EINVAL, "item_sequences: NULL item_count");
    if (((uintptr_t)user_id & 3) || ((uintptr_t)movie_id & 3) || ((uintptr_t)rating & 3) || ((uintptr_t)timestamp & 7) || ((uintptr_t)seq_offsets & 3) ||
        ((uintptr_t)seq_items & 3) || ((uintptr_t)item_count & 3))
        return fail(SPRK_EINVAL, "item_sequences: misaligned column");
    const SeqWorkspace w = seq_carve(workspace, n_ratings, n_users);
    SPRK_TRY(check_workspace("item_sequences", "sprk_item_sequences_workspace_bytes", workspace, workspace_bytes, w.bytes));
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_ratings;
    unsigned long long* err = (unsigned long long*)error_key;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    if (n_items > 0) HIP_TRY(hipMemsetAsync(item_count, 0, (size_t)n_items * sizeof(int32_t), st));
    if (n > 0) {
        hipLaunchKernelGGL(k_i2v_seq_count, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, user_id, movie_id, rating, (int)n_users, (int)n_items, w.off, item_count, err);
        HIP_TRY(hipGetLastError());
    }
    SPRK_TRY(seg_scan(w.off, (long long)n_users + 1, w.tops, w.tiles, FeScanKept<false>{}, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_i2v_seq_scatter, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, user_id, movie_id, rating, (const long long*)timestamp, (int)n_users,
                           (int)n_items, (const unsigned*)w.off, w.cursor, w.key, w.val);
        HIP_TRY(hipGetLastError());
        SPRK_TRY(seg_sort(cap, n, n_users, w.off, w.key, w.val, w.tmp_key, w.tmp_val, w.long_list, w.words, nullptr, st));
    }
    const long long rows = n > (long long)n_users + 1 ? n : (long long)n_users + 1;
    hipLaunchKernelGGL(k_i2v_seq_emit, dim3(fe_grid_capped(rows)), dim3(FE_THREADS), 0, st, n, (int)n_users, (const unsigned*)w.off, (const int*)w.val, movie_id, seq_offsets, seq_items);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

size_t sprk_skipgram_workspace_bytes(int64_t n_seq_items, int32_t n_seq, int32_t vocab_size, int64_t n_words, int32_t D, int32_t window, int32_t round) {
    if (!skip_sizes_ok(n_seq_items, n_seq, vocab_size, n_words, D, window, round)) return 0;
    return skip_carve(nullptr, n_seq_items, vocab_size, n_words, D, window, round).bytes;
}

int sprk_skipgram_fit(const int32_t* seq_offsets, const int32_t* seq_items, int64_t n_seq_items, int32_t n_seq,
                      const int32_t* item_vocab, int32_t n_items, int32_t vocab_size, int64_t n_words,
                      const int32_t* code_len, const uint8_t* codes, const int32_t* points,
                      const float* init, int32_t init_stride, const float* exp_table, const double* loss_table,
                      int32_t D, int32_t window, int32_t iters, double lr, int32_t round, int32_t row_cap, uint64_t seed, int32_t max_sentence,
                      float* vectors, int32_t stride, float* syn1, double* loss,
                      uint64_t* error_key, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_skipgram_fit");
    if (D < 1 || D > I2V_MAX_D) return fail(SPRK_EINVAL, "skipgram_fit: D = %d outside [1, %d]", D, I2V_MAX_D);
    if (window < 1 || window > I2V_MAX_WINDOW) return fail(SPRK_EINVAL, "skipgram_fit: window = %d outside [1, %d]", window, I2V_MAX_WINDOW);
    if (round < 1 || row_cap < 1 || max_sentence < 1) return fail(SPRK_EINVAL, "skipgram_fit: round = %d, row_cap = %d, max_sentence = %d must be >= 1", round, row_cap, max_sentence);
    if (iters < 0) return fail(SPRK_EINVAL, "skipgram_fit: iters = %d is negative", iters);
    if (!(lr > 0.0) || lr > 1.7976931348623157e308) return fail(SPRK_EINVAL, "skipgram_fit: lr must be finite and > 0");
    if (n_items < 0 || n_items >= 0x7fffffff) return fail(SPRK_EINVAL, "skipgram_fit: n_items outside [0, 2^31 - 1)");
    if (!skip_sizes_ok(n_seq_items, n_seq, vocab_size, n_words, D, window, round))
        return fail(SPRK_EINVAL, "skipgram_fit: bad sizes (need 0 <= n_words <= n_seq_items < 2^31 - 1, n_seq > 0 and vocab_size > 0 unless empty, "
                                 "n_words (2 window + 40) < 2^31 - 1)");
    if (stride < D || init_stride < D) return fail(SPRK_EINVAL, "skipgram_fit: stride = %d, init_stride = %d, a row holds D = %d floats", stride, init_stride, D);
    if (!error_key || !loss) return fail(SPRK_EINVAL, "skipgram_fit: NULL error word or loss");
    if (((uintptr_t)error_key & 7) || ((uintptr_t)loss & 7)) return fail(SPRK_EINVAL, "skipgram_fit: misaligned error word or loss");
    if (!seq_offsets) return fail(SPRK_EINVAL, "skipgram_fit: NULL seq_offsets");
    if (n_seq_items > 0 && (!seq_items || !item_vocab)) return fail(SPRK_EINVAL, "skipgram_fit: NULL seq_items or item_vocab");
    if (vocab_size > 0 && (!code_len || !codes || !points || !init || !vectors || !syn1)) return fail(SPRK_EINVAL, "skipgram_fit: NULL vocabulary table");
    if (!exp_table || !loss_table) return fail(SPRK_EINVAL, "skipgram_fit: NULL exp_table or loss_table");
    if (((uintptr_t)seq_offsets & 3) || ((uintptr_t)seq_items & 3) || ((uintptr_t)item_vocab & 3) || ((uintptr_t)code_len & 3) || ((uintptr_t)points & 3) ||
        ((uintptr_t)init & 3) || ((uintptr_t)exp_table & 3) || ((uintptr_t)loss_table & 7) || ((uintptr_t)vectors & 3) || ((uintptr_t)syn1 & 3))
        return fail(SPRK_EINVAL, "skipgram_fit: misaligned column");
    const SkipWorkspace w = skip_carve(workspace, n_seq_items, vocab_size, n_words, D, window, round);
    SPRK_TRY(check_workspace("skipgram_fit", "sprk_skipgram_workspace_bytes", workspace, workspace_bytes, w.bytes));
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_seq_items, N = n_words;
    const int V = vocab_size;
    unsigned long long* err = (unsigned long long*)error_key;
    const unsigned* total = w.a + n;

    HIP_TRY(hipMemsetAsync(workspace, 0, w.zeroed_bytes, st));
    HIP_TRY(hipMemsetAsync(loss, 0, sizeof(double), st));
    if (V > 0) {
        hipLaunchKernelGGL(k_i2v_init, dim3(fe_grid_capped((long long)V * D)), dim3(FE_THREADS), 0, st, V, (int)D, init, (int)init_stride, vectors, (int)stride, syn1);
        HIP_TRY(hipGetLastError());
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_i2v_mark, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, seq_items, item_vocab, (int)n_items, w.a, err);
        HIP_TRY(hipGetLastError());
    }
    SPRK_TRY(seg_scan(w.a, n + 1, w.tops, w.tiles_a, FeScanKept<false>{}, st));
    if (n == 0 || V == 0) return SPRK_OK;                                    // (N == 0 was checked for V == 0; n == 0 gives N == 0)
    hipLaunchKernelGGL(k_i2v_corpus, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, (int)n_seq, seq_offsets, seq_items, item_vocab, (const unsigned*)w.a, N,
                       (int)max_sentence, (int)window, V, code_len, points, w.pos_word, w.pos_lo, w.pos_hi, w.off, err);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_scan(w.off, 2ll * V + 1, w.tops, w.tiles_off, FeScanKept<false>{}, st));
    if (N == 0) return SPRK_OK;
    hipLaunchKernelGGL(k_i2v_records, dim3(fe_grid_capped(n)), dim3(FE_THREADS), 0, st, n, (int)n_seq, seq_offsets, seq_items, item_vocab, (const unsigned*)w.a, N,
                       (int)max_sentence, (int)window, V, code_len, points, (const unsigned*)w.off, w.cursor, w.key, w.val);
    HIP_TRY(hipGetLastError());
    SPRK_TRY(seg_sort(cap, w.records, 2 * V, w.off, w.key, w.val, w.tmp_key, w.tmp_val, w.long_list, w.words, nullptr, st));

    const bool wide = D > 16;
    const int per_block = I2V_THREADS / (wide ? 64 : 16);                     // positions a workgroup of k_i2v_positions holds
    const long long apply_threads = 2ll * V * (wide ? 64 : 16);
    const unsigned apply_grid = (unsigned)((apply_threads + FE_THREADS - 1) / FE_THREADS);
    for (int it = 0; it < iters; ++it)
        for (long long r0 = 0; r0 < N; r0 += w.round) {
            const long long r1 = r0 + w.round < N ? r0 + w.round : N;
            const double done = (double)((long long)it * N + r0);
            const double a1 = lr * (1.0 - done / (double)(N * (long long)iters + 1)), a2 = lr * 1e-4;
            const float alpha = (float)(a1 > a2 ? a1 : a2);
            const unsigned pg = (unsigned)((r1 - r0 + per_block - 1) / per_block);
            if (wide) {
                hipLaunchKernelGGL(k_i2v_positions<64>, dim3(pg), dim3(I2V_THREADS), 0, st, r0, r1, N, total, (const int*)w.pos_word, (const unsigned*)w.pos_lo,
                                   (const unsigned*)w.pos_hi, code_len, codes, points, V, (const float*)vectors, (int)stride, (const float*)syn1, (int)D, (int)window, it,
                                   (unsigned long long)seed, alpha, exp_table, w.E0, w.E1);
                hipLaunchKernelGGL(k_i2v_apply<64>, dim3(apply_grid), dim3(FE_THREADS), 0, st, r0, r1, N, total, V, (const unsigned*)w.off, (const long long*)w.key, vectors,
                                   (int)stride, syn1, (int)D, (int)window, it, (unsigned long long)seed, (int)row_cap, (const float*)w.E0, (const float*)w.E1);
            } else {
                hipLaunchKernelGGL(k_i2v_positions<16>, dim3(pg), dim3(I2V_THREADS), 0, st, r0, r1, N, total, (const int*)w.pos_word, (const unsigned*)w.pos_lo,
                                   (const unsigned*)w.pos_hi, code_len, codes, points, V, (const float*)vectors, (int)stride, (const float*)syn1, (int)D, (int)window, it,
                                   (unsigned long long)seed, alpha, exp_table, w.E0, w.E1);
                hipLaunchKernelGGL(k_i2v_apply<16>, dim3(apply_grid), dim3(FE_THREADS), 0, st, r0, r1, N, total, V, (const unsigned*)w.off, (const long long*)w.key, vectors,
                                   (int)stride, syn1, (int)D, (int)window, it, (unsigned long long)seed, (int)row_cap, (const float*)w.E0, (const float*)w.E1);
            }
            HIP_TRY(hipGetLastError());
        }
    const unsigned lg = (unsigned)((N + per_block - 1) / per_block);
    if (wide)
        hipLaunchKernelGGL(k_i2v_loss_pos<64>, dim3(lg), dim3(I2V_THREADS), 0, st, N, total, (const int*)w.pos_word, (const unsigned*)w.pos_lo, (const unsigned*)w.pos_hi, code_len,
                           codes, points, V, (const float*)vectors, (int)stride, (const float*)syn1, (int)D, (int)window, loss_table, w.pos_loss, w.pos_terms);
    else
        hipLaunchKernelGGL(k_i2v_loss_pos<16>, dim3(lg), dim3(I2V_THREADS), 0, st, N, total, (const int*)w.pos_word, (const unsigned*)w.pos_lo, (const unsigned*)w.pos_hi, code_len,
                           codes, points, V, (const float*)vectors, (int)stride, (const float*)syn1, (int)D, (int)window, loss_table, w.pos_loss, w.pos_terms);
    hipLaunchKernelGGL(k_i2v_loss_chunks, dim3(fe_grid_capped((N + I2V_LOSS_CHUNK - 1) / I2V_LOSS_CHUNK)), dim3(FE_THREADS), 0, st, N, total, (const double*)w.pos_loss,
                       (const unsigned*)w.pos_terms, w.chunk_loss, w.chunk_terms);
    hipLaunchKernelGGL(k_i2v_loss_final, dim3(1), dim3(1), 0, st, N, total, (const double*)w.chunk_loss, (const unsigned long long*)w.chunk_terms, loss);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
