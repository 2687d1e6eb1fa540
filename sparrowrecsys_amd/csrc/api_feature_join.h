// api_feature_join.h -- C ABI: sprk_join_features ((userId, movieId) pairs x the feature store's two tables -> packed ids / dense,
// k_feature_join.h) and sprk_rank_scores (scores -> candidate positions best first, k_rank_scores.h).  Part of sparrow_hip.hip;
// included there behind api_pack_columns.h.  Both calls validate every argument before any device call, launch on the caller's stream
// and return: no synchronisation, no memory of their own.
extern "C" {

int sprk_join_features(const int32_t* user_rows, const uint8_t* user_has, int32_t n_users, int32_t user_pitch,
                       const int32_t* movie_rows, const uint8_t* movie_has, int32_t n_movies, int32_t movie_pitch,
                       const int32_t* user_ids, const int32_t* movie_ids, int32_t Q, int32_t C, int32_t shared_candidates,
                       const sprk_join_col* id_cols, int32_t n_id, const sprk_join_col* dense_cols, int32_t n_dense,
                       int32_t* ids_out, float* dense_out, uint64_t* range_key, void* stream) {
    RoctxRange roctx_range_("sprk_join_features");
    // every check before any device call
    if (Q < 0 || C < 0 || n_id < 0 || n_dense < 0) return fail(SPRK_EINVAL, "join_features: negative Q / C / column count");
    if (n_id + (int64_t)n_dense > SPRK_PACK_MAX_COLS)
        return fail(SPRK_EINVAL, "join_features joins at most %d columns (%lld given)", SPRK_PACK_MAX_COLS, (long long)n_id + n_dense);
    if (shared_candidates != 0 && shared_candidates != 1) return fail(SPRK_EINVAL, "join_features: shared_candidates must be 0 or 1");
    if (n_users < 0 || n_movies < 0 || user_pitch < 4 || movie_pitch < 4 || (user_pitch & 3) || (movie_pitch & 3) || user_pitch > 65536 || movie_pitch > 65536)
        return fail(SPRK_EINVAL, "join_features: bad table geometry (row pitches are multiples of 4 dwords in [4, 65536])");
    if (!user_rows || !user_has || !movie_rows || !movie_has) return fail(SPRK_EINVAL, "join_features: NULL table / has flags");
    if (!user_ids || !movie_ids) return fail(SPRK_EINVAL, "join_features: NULL user_ids / movie_ids");
    if ((n_id > 0 && (!id_cols || !ids_out)) || (n_dense > 0 && (!dense_cols || !dense_out))) return fail(SPRK_EINVAL, "join_features: NULL column list / output");
    if (!range_key) return fail(SPRK_EINVAL, "join_features: NULL range key word");
    if (((uintptr_t)user_rows & 15) || ((uintptr_t)movie_rows & 15) || ((uintptr_t)ids_out & 15) || ((uintptr_t)dense_out & 15))
        return fail(SPRK_EINVAL, "join_features: the tables and the outputs must start on a 16-byte boundary");
    if (((uintptr_t)user_ids & 3) || ((uintptr_t)movie_ids & 3) || ((uintptr_t)range_key & 7)) return fail(SPRK_EINVAL, "join_features: misaligned ids / key word");
    if ((int64_t)Q * (int64_t)C > 0x7FFFFFFFll) return fail(SPRK_EINVAL, "join_features: Q * C = %lld rows beyond 2^31 - 1", (long long)Q * C);
    JoinDev D;
    memset(&D, 0, sizeof(D));
    const int n_cols = n_id + n_dense;
    int sort_key[SPRK_PACK_MAX_COLS], col_vocab[SPRK_PACK_MAX_COLS], rule_of[SPRK_PACK_MAX_COLS], walk[SPRK_PACK_MAX_COLS];
    for (int j = 0; j < n_cols; ++j) {
        const sprk_join_col& c = j < n_id ? id_cols[j] : dense_cols[j - n_id];
        const char* mat = j < n_id ? "id" : "dense";
        const int k = j < n_id ? j : j - n_id;
        if (c.source < SPRK_JOIN_PAIR_USER || c.source > SPRK_JOIN_MOVIE_ROW) return fail(SPRK_EINVAL, "join_features: %s column %d has unknown source %d", mat, k, c.source);
        if (j < n_id ? (c.rule != SPRK_RULE_IDENTITY && c.rule != SPRK_RULE_GENRE) : c.rule != SPRK_RULE_DENSE)
            return fail(SPRK_EINVAL, "join_features: %s column %d has rule %d (id columns: identity or genre, dense columns: dense)", mat, k, c.rule);
        const bool pair = c.source == SPRK_JOIN_PAIR_USER || c.source == SPRK_JOIN_PAIR_MOVIE;
        if (pair && c.rule != SPRK_RULE_IDENTITY) return fail(SPRK_EINVAL, "join_features: %s column %d: the pair's own ids are identity columns", mat, k);
        if (!pair) {
            const int pitch = c.source == SPRK_JOIN_USER_ROW ? user_pitch : movie_pitch;
            if (c.offset < 0 || c.offset >= pitch) return fail(SPRK_EINVAL, "join_features: %s column %d reads dword %d of a row of %d", mat, k, c.offset, pitch);
        }
        if (c.rule != SPRK_RULE_DENSE && c.vocab < 1) return fail(SPRK_EINVAL, "join_features: %s column %d has vocab %d", mat, k, c.vocab);
        sort_key[j] = c.source * 65536 + (pair ? 0 : c.offset);       // (offsets are below 65536: the pitch limit)
        col_vocab[j] = c.vocab; rule_of[j] = c.rule;
        walk[j] = j;
    }
    if (Q == 0 || C == 0 || n_cols == 0) return SPRK_OK;
    // the kernel walks the columns by (source, offset): neighbours in a row share a 16-byte granule
    for (int a = 1; a < n_cols; ++a) {                                    // (insertion sort: stable, at most 128 entries)
        const int w = walk[a];
        int b = a;
        while (b > 0 && sort_key[walk[b - 1]] > sort_key[w]) { walk[b] = walk[b - 1]; --b; }
        walk[b] = w;
    }
    for (int k = 0; k < n_cols; ++k) {
        const int j = walk[k];
        D.desc[k] = ((unsigned)j << 24) | ((unsigned)(sort_key[j] >> 16) << 20) | ((unsigned)rule_of[j] << 16) | (unsigned)(sort_key[j] & 0xFFFF);
        D.vocab[k] = col_vocab[j];
    }
    D.n_id = n_id; D.n_dense = n_dense;
    D.rows = (unsigned)((int64_t)Q * C); D.C = (unsigned)C; D.shared = shared_candidates;
    D.n_users = n_users; D.n_movies = n_movies; D.user_pitch = user_pitch; D.movie_pitch = movie_pitch;
    D.user_rows = user_rows; D.movie_rows = movie_rows; D.user_has = user_has; D.movie_has = movie_has;
    D.user_ids = user_ids; D.movie_ids = movie_ids;
    const unsigned grid = (unsigned)(((size_t)D.rows + FJ_TILE - 1) / FJ_TILE);
    hipLaunchKernelGGL(k_feature_join, dim3(grid), dim3(FJ_TILE), PK_OUT_BYTES, (hipStream_t)stream, D, (int*)ids_out, dense_out, (unsigned long long*)range_key);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

int sprk_rank_scores(const float* scores, int32_t Q, int32_t C, int32_t* order, void* stream) {
    RoctxRange roctx_range_("sprk_rank_scores");
    if (Q < 0) return fail(SPRK_EINVAL, "rank_scores: negative Q");
    if (C < 1 || C > RS_MAX_SORT) return fail(SPRK_EINVAL, "rank_scores: C = %d outside [1, %d]", C, RS_MAX_SORT);
    if (!scores || !order) return fail(SPRK_EINVAL, "rank_scores: NULL scores / order");
    if (((uintptr_t)scores & 3) || ((uintptr_t)order & 3)) return fail(SPRK_EINVAL, "rank_scores: misaligned scores / order");
    if (Q == 0) return SPRK_OK;
    int P = 2;
    while (P < C) P <<= 1;
    hipLaunchKernelGGL(k_rank_scores, dim3((unsigned)Q), dim3(RS_THREADS), (size_t)P * sizeof(unsigned long long), (hipStream_t)stream, scores, C, P, order);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
