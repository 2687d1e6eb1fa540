// api_lsh.h -- C ABI: sprk_lsh_hash / sprk_lsh_build (+ sprk_lsh_build_workspace_bytes) / sprk_lsh_query, embedding LSH on the device
// (k_lsh.h).  From host_segments.h: the carver and the workspace check, the grids, seg_sort -- every hash table is one segment of n
// (bucket, row) keys.  Every argument is checked before any device call; the calls enqueue their kernels on the caller's stream and
// return: no synchronisation, no memory of their own.
namespace {
// pairs of the query kernel's LDS buffer: LSH_CHUNK, or SPRK_LSH_CHUNK = a power of two in [64, LSH_CHUNK], read at each call (tests: a
// buffer that fills and is cut many times at a few hundred candidates)
int lsh_chunk_len() {
    if (const char* e = getenv("SPRK_LSH_CHUNK")) {
        const int v = atoi(e);
        if (v >= 64 && v <= LSH_CHUNK && (v & (v - 1)) == 0) return v;
    }
    return LSH_CHUNK;
}
// The workspace of sprk_lsh_build, carved in this order; every part starts on a 16-byte boundary.
struct LshWorkspace {
    unsigned* off;                 // [2]   {0, n}: the one segment of a table
    unsigned* n_long;              // [T]   seg_sort's count of long segments, a word per table
    int* long_list;                // [T]   a place per table
    long long* tmp_key;            // [n]   the merge passes' other side, shared by the tables (they are sorted one after another)
    int* tmp_val;                  // [n]
    size_t bytes;
};
inline bool lsh_sizes_ok(int64_t n, int32_t T) { return n >= 0 && n < 0x7fffffffll && T >= 1 && T <= LSH_MAX_T; }
LshWorkspace lsh_carve(void* base, int64_t n, int32_t T) {
    LshWorkspace w;
    Carver c{base};
    w.off = c.take<unsigned>(2);
    w.n_long = c.take<unsigned>((size_t)T);
    w.long_list = c.take<int>((size_t)T);
    w.tmp_key = c.take<long long>((size_t)n);
    w.tmp_val = c.take<int>((size_t)n);
    w.bytes = c.at;
    return w;
}
inline bool lsh_length_ok(double bucket_length) { return bucket_length > 0.0 && bucket_length <= 1.7976931348623157e308; }
// the checks sprk_lsh_hash and sprk_lsh_query share: the table, the vectors, the bucket length
int lsh_check_table(const char* call, const float* emb, int64_t n, int32_t D, int32_t stride, const double* vectors, int32_t T, double bucket_length) {
    if (!lsh_sizes_ok(n, T)) return fail(SPRK_EINVAL, "%s: bad sizes (need 0 <= n < 2^31 - 1, 1 <= T <= %d)", call, LSH_MAX_T);
    if (D < 1 || D > LSH_MAX_D) return fail(SPRK_EINVAL, "%s: D = %d outside [1, %d]", call, D, LSH_MAX_D);
    if (stride < D) return fail(SPRK_EINVAL, "%s: stride = %d, a row holds D = %d floats", call, stride, D);
    if (!lsh_length_ok(bucket_length)) return fail(SPRK_EINVAL, "%s: bucket_length = %g must be finite and > 0", call, bucket_length);
    if (!vectors) return fail(SPRK_EINVAL, "%s: NULL vectors", call);
    if (n > 0 && !emb) return fail(SPRK_EINVAL, "%s: NULL table", call);
    if (((uintptr_t)emb & 3) || ((uintptr_t)vectors & 7)) return fail(SPRK_EINVAL, "%s: misaligned table or vectors", call);
    return SPRK_OK;
}
}  // namespace

extern "C" {

int sprk_lsh_hash(const float* emb, const uint8_t* has, int64_t n, int32_t D, int32_t stride, const double* vectors, int32_t T,
                  double bucket_length, int64_t* buckets, void* stream) {
    RoctxRange roctx_range_("sprk_lsh_hash");
    // every check before any device call
    SPRK_TRY(lsh_check_table("lsh_hash", emb, n, D, stride, vectors, T, bucket_length));
    if (n > 0 && !buckets) return fail(SPRK_EINVAL, "lsh_hash: NULL buckets");
    if ((uintptr_t)buckets & 7) return fail(SPRK_EINVAL, "lsh_hash: misaligned buckets");
    if (n == 0) return SPRK_OK;
    const size_t vec_bytes = (size_t)T * D * 8;
    const int stage = vec_bytes <= LSH_HASH_STAGE_BYTES;
    hipLaunchKernelGGL(k_lsh_hash, dim3(fe_grid_capped((long long)n * T)), dim3(FE_THREADS), stage ? vec_bytes : 0, (hipStream_t)stream, emb, has, (long long)n, (int)D,
                       (int)stride, vectors, (int)T, bucket_length, stage, (long long*)buckets);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

size_t sprk_lsh_build_workspace_bytes(int64_t n, int32_t T) {
    if (!lsh_sizes_ok(n, T)) return 0;
    return lsh_carve(nullptr, n, T).bytes;
}

int sprk_lsh_build(const int64_t* buckets, int64_t n, int32_t T, int64_t* idx_bucket, int32_t* idx_row, void* workspace, size_t workspace_bytes, void* stream) {
    RoctxRange roctx_range_("sprk_lsh_build");
    // every check before any device call
    if (!lsh_sizes_ok(n, T)) return fail(SPRK_EINVAL, "lsh_build: bad sizes (need 0 <= n < 2^31 - 1, 1 <= T <= %d)", LSH_MAX_T);
    if (n > 0 && (!buckets || !idx_bucket || !idx_row)) return fail(SPRK_EINVAL, "lsh_build: NULL buckets or index");
    if (((uintptr_t)buckets & 7) || ((uintptr_t)idx_bucket & 7) || ((uintptr_t)idx_row & 3)) return fail(SPRK_EINVAL, "lsh_build: misaligned buckets or index");
    const LshWorkspace w = lsh_carve(workspace, n, T);
    SPRK_TRY(check_workspace("lsh_build", "sprk_lsh_build_workspace_bytes", workspace, workspace_bytes, w.bytes));
    if (n == 0) return SPRK_OK;
    const int cap = fe_sort_cap();
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lsh_index_init, dim3(fe_grid_capped((long long)n * T)), dim3(FE_THREADS), 0, st, (const long long*)buckets, (long long)n, (int)T, (long long*)idx_bucket,
                       idx_row, w.off, w.n_long);
    HIP_TRY(hipGetLastError());
    for (int t = 0; t < T; ++t)
        SPRK_TRY(seg_sort(cap, n, 1, w.off, (long long*)idx_bucket + (size_t)t * n, idx_row + (size_t)t * n, w.tmp_key, w.tmp_val, w.long_list + t, w.n_long + t, nullptr, st));
    return SPRK_OK;
}

int sprk_lsh_query(const float* emb, const uint8_t* has, int64_t n, int32_t D, int32_t stride, const double* vectors, int32_t T,
                   double bucket_length, const int64_t* buckets, const int64_t* idx_bucket, const int32_t* idx_row,
                   const float* queries, const uint8_t* query_has, int32_t Q, int32_t query_stride, int32_t K,
                   double* dist, int32_t* rows, int32_t* count, void* stream) {
    RoctxRange roctx_range_("sprk_lsh_query");
    // every check before any device call
    SPRK_TRY(lsh_check_table("lsh_query", emb, n, D, stride, vectors, T, bucket_length));
    const int chunk = lsh_chunk_len();
    if (Q < 0) return fail(SPRK_EINVAL, "lsh_query: Q = %d", Q);
    if (query_stride < D) return fail(SPRK_EINVAL, "lsh_query: query_stride = %d, a row holds D = %d floats", query_stride, D);
    if (K < 1 || K > LSH_MAX_K || K >= chunk) return fail(SPRK_EINVAL, "lsh_query: K = %d outside [1, min(%d, chunk - 1 = %d)]", K, LSH_MAX_K, chunk - 1);
    if (n > 0 && (!buckets || !idx_bucket || !idx_row)) return fail(SPRK_EINVAL, "lsh_query: NULL buckets or index");
    if (Q > 0 && (!queries || !dist || !rows || !count)) return fail(SPRK_EINVAL, "lsh_query: NULL queries / dist / rows / count");
    if (((uintptr_t)buckets & 7) || ((uintptr_t)idx_bucket & 7) || ((uintptr_t)idx_row & 3) || ((uintptr_t)queries & 3) || ((uintptr_t)dist & 7) || ((uintptr_t)rows & 3) ||
        ((uintptr_t)count & 3))
        return fail(SPRK_EINVAL, "lsh_query: misaligned buckets, index, queries or output");
    if (Q == 0) return SPRK_OK;
    const size_t vec_bytes = (size_t)T * D * 8;
    const int stage = vec_bytes <= LSH_QUERY_STAGE_BYTES;
    const size_t lds = (size_t)chunk * 12 + (stage ? vec_bytes : 0) + 3 * LSH_MAX_T * 8 + (size_t)D * 4;       // <= 61 824 bytes
    const unsigned g = (unsigned)Q < fe_max_grid() ? (unsigned)Q : fe_max_grid();
    hipLaunchKernelGGL(k_lsh_query, dim3(g), dim3(LSH_THREADS), lds, (hipStream_t)stream, emb, has, (long long)n, (int)D, (int)stride, vectors, (int)T, bucket_length, stage,
                       (const long long*)buckets, (const long long*)idx_bucket, idx_row, queries, query_has, (int)Q, (int)query_stride, (int)K, chunk, dist, rows, count);
    HIP_TRY(hipGetLastError());
    return SPRK_OK;
}

}  // extern "C"
