// k_feature_join.h -- (userId, movieId) pairs -> the packed ids [rows][n_id] int32 / dense [rows][n_dense] float32 arrays ON THE DEVICE,
// joined from the two tables of the feature store (sparrowrecsys_amd/featurestore.py): the device counterpart of the reference's
// `uf:<userId>` / `mf:<movieId>` feature maps (FeatureEngForRecModel.scala:127-174,208-259, read by RecForYouProcess.java:46-52 and
// DataManager.loadMovieFeatures).  The tables hold what schema.pack_ids / pack_dense produce for every column, so the join converts
// nothing: it gathers, applies the READING model's vocabulary (genre outside [0, vocab) -> -1) and reports identity values outside
// [0, vocab) the way k_pack_columns.h does.  Included inside the kernels' namespace, behind k_pack_columns.h (pk_report is that file's).
//
// Output row q * C + c pairs user_ids[q] with movie_ids[q][c] (or movie_ids[c]: one candidate list shared by every query); the pair
// form is C = 1.  One workgroup of 256 threads joins a tile of 256 consecutive output rows.  The column descriptors are a kernel
// argument: the column loop, the source switch and every descriptor read are wave-uniform.  The host hands the columns over sorted by
// (source, offset) as well: the loop walks them in that order and keeps the current 16-byte granule of the lane's user row and of its
// movie row in registers, so every granule a model reads is loaded once per group of 32 output columns, with one 16-byte load per
// lane; in the cross form all lanes of a query load the same user-row address (one request).  A user or movie id outside its table,
// or with has == 0, reads the default row (identity 0, genre -1, dense 0.0) without touching the table.  The converted values of up
// to 32 columns are assembled in LDS; a matrix of at most 32 columns leaves as one contiguous span of 16-byte stores, a wider one as
// coalesced 128-byte row runs (k_pack_columns.h's two forms).
// Bandwidth-bound: per output row about user_pitch * 4 + 32 bytes in (served by L2 in the cross form), (n_id + n_dense) * 4 bytes out.

#define FJ_TILE 256
enum { FJ_PAIR_USER = 0, FJ_PAIR_MOVIE, FJ_USER_ROW, FJ_MOVIE_ROW };   // = SPRK_JOIN_*

struct JoinDev {
    int n_id, n_dense;
    unsigned rows, C;                              // rows = Q * C
    int shared;                                    // movie_ids is one [C] list
    int n_users, n_movies, user_pitch, movie_pitch;
    const int* user_rows;
    const int* movie_rows;
    const unsigned char* user_has;
    const unsigned char* movie_has;
    const int* user_ids;
    const int* movie_ids;
    // the columns in WALK order (sorted by source, then offset), ONE DWORD per column and array, indexed by the loop counter: every
    // scalar descriptor load then has a dword-aligned base (a scalar load ignores the low two bits of its base, and byte-sized descriptor
    // arrays indexed by a loaded column number let the compiler form a base of kernarg + 2 c)
    unsigned desc[PK_MAX_COLS];                    // column << 24 | source << 20 | rule << 16 | dword offset in the source row
    int vocab[PK_MAX_COLS];
};
static_assert(sizeof(JoinDev) + 24 <= 4096, "JoinDev travels as a kernel argument");

static __global__ __launch_bounds__(FJ_TILE) void k_feature_join(const JoinDev D, int* __restrict__ ids, float* __restrict__ dense,
                                                                 unsigned long long* __restrict__ range_key) {
    unsigned* tile = reinterpret_cast<unsigned*>(smem);                                         // [FJ_TILE][ldw]
    const unsigned row0 = blockIdx.x * FJ_TILE;
    const unsigned nrows = D.rows - row0 < FJ_TILE ? D.rows - row0 : FJ_TILE;
    const unsigned r = threadIdx.x, row = row0 + r;
    const bool active = r < nrows;
    int uid = 0, mid = 0;
    const int* urow = nullptr;                     // nullptr = the default row
    const int* mrow = nullptr;
    if (active) {
        const unsigned q = row / D.C;
        uid = D.user_ids[q];
        mid = D.movie_ids[D.shared ? (size_t)(row - q * D.C) : (size_t)row];
        if ((unsigned)uid < (unsigned)D.n_users && D.user_has[uid]) urow = D.user_rows + (size_t)uid * (size_t)D.user_pitch;
        if ((unsigned)mid < (unsigned)D.n_movies && D.movie_has[mid]) mrow = D.movie_rows + (size_t)mid * (size_t)D.movie_pitch;
    }
    const int n_cols = D.n_id + D.n_dense;
    for (int mat = 0; mat < 2; ++mat) {
        const int n = mat ? D.n_dense : D.n_id, cbase = mat ? D.n_id : 0;
        unsigned* out = mat ? reinterpret_cast<unsigned*>(dense) : reinterpret_cast<unsigned*>(ids);
        const bool single = n <= PK_GROUP;
        const int ldw = single ? n : PK_LDW;
        for (int g0 = 0; g0 < n; g0 += PK_GROUP) {
            const int gw = n - g0 < PK_GROUP ? n - g0 : PK_GROUP;
            const int c_lo = cbase + g0, c_hi = c_lo + gw;
            int cur_src = -1, cur_g = -1;          // the granule held in `v` (wave-uniform)
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            for (int k = 0; k < n_cols; ++k) {
                const unsigned d = D.desc[k];
                const int c = (int)(d >> 24);
                if (c < c_lo || c >= c_hi) continue;
                const int src = (int)(d >> 20) & 15, rule = (int)(d >> 16) & 15, off = (int)(d & 0xFFFFu), vocab = D.vocab[k];
                unsigned bits;
                bool present = true;
                if (src == FJ_PAIR_USER) bits = (unsigned)uid;
                else if (src == FJ_PAIR_MOVIE) bits = (unsigned)mid;
                else {
                    const int* base = src == FJ_USER_ROW ? urow : mrow;
                    const int g = off >> 2;
                    if (src != cur_src || g != cur_g) {
                        cur_src = src; cur_g = g;
                        if (base) v = *reinterpret_cast<const uint4*>(base + 4 * g);
                    }
                    const int e = off & 3;
                    bits = e == 0 ? v.x : (e == 1 ? v.y : (e == 2 ? v.z : v.w));
                    present = base != nullptr;
                }
                if (!present) bits = rule == 1 ? ~0u : 0u;                     // the default row: identity 0, genre -1, dense 0.0
                else if (rule == 1) { if (bits >= (unsigned)vocab) bits = ~0u; }
                else if (rule == 0) { if (active && bits >= (unsigned)vocab) pk_report(range_key, 0, c, row); }
                if (active) tile[r * ldw + (c - c_lo)] = bits;
            }
            __syncthreads();
            if (single) {
                // the tile is one contiguous span of the output: 16-byte stores (the span starts on a multiple of 1024 bytes)
                const unsigned dwords = nrows * (unsigned)n;
                unsigned* dst = out + (size_t)row0 * n;
                for (unsigned o = threadIdx.x * 4; o < dwords; o += FJ_TILE * 4) {
                    if (o + 4 <= dwords) *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(tile + o);
                    else for (unsigned kk = o; kk < dwords; ++kk) dst[kk] = tile[kk];
                }
            } else {
                for (unsigned o = threadIdx.x; o < nrows * (unsigned)gw; o += FJ_TILE) {
                    const unsigned rr = o / (unsigned)gw, cc = o - rr * (unsigned)gw;
                    out[(size_t)(row0 + rr) * n + g0 + cc] = tile[rr * PK_LDW + cc];
                }
            }
            __syncthreads();
        }
    }
}
