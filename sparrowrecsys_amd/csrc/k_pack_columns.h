// k_pack_columns.h -- a dict of feature columns -> the packed ids [rows][n_id] int32 / dense [rows][n_dense] float32 arrays ON THE
// DEVICE: the device twin of sprk_pack_columns (api_pack_columns.h; same rules, same bits), i.e. of schema.pack_ids / pack_dense,
// which restate the reference's Keras inputs + feature columns (DeepFM.py:30-76).  Included inside the kernels' namespace, behind
// k_csv_pack.h: the genre perfect hash, the two decimal parsers (through their reader types) and the newline passes are that file's.
//
// One workgroup of 256 threads packs a tile of 256 consecutive rows.  The column descriptors are a kernel argument (wave-uniform:
// the column loop, the storage switch and every descriptor read are scalar).  Per output column:
//   numeric storage   one element per lane, coalesced along the column (any byte stride: a strided view of a [B, 50] matrix)
//   S<w> / U<w>       rows are not 4-byte aligned (S11): the tile's contiguous span is staged into LDS (16-byte loads; U: one code
//                     point per lane, narrowed to a byte, anything above 127 -> 0xFF, which matches no genre and no digit), every
//                     lane then reads its own field from LDS.  A span beyond PK_STR_CAP bytes, or a strided column, is read in place.
//   text block        field (c, i) is line c * rows + i of the block; nl[] (k_csv_count -> scan -> k_csv_mark over the whole block)
//                     gives its bounds, the tile's 256 fields of one column are one contiguous piece: staged like the S span
// The converted values of up to 32 columns are assembled in LDS; when the matrix has at most 32 columns the tile IS a contiguous
// span of the output and leaves with 16-byte stores, otherwise every row's 128-byte run leaves as coalesced dwords.
// Nothing is guessed: a value outside the convertible cases sets the DECLINE key, an identity id outside [0, vocab) the RANGE key
// (both atomicMin over (column << 32 | row): column order wins over row order, as in pack_ids); the host reads the two after the launch.
// Bandwidth-bound on a few MB per call; the host -> device copy in front of it is the larger part of the call (profiles/r07).

#define PK_MAX_COLS 128                        // = SPRK_PACK_MAX_COLS
#define PK_TILE 256
#define PK_GROUP 32                            // output columns assembled in LDS at a time
#define PK_LDW 33                              // LDS row pitch (dwords) of a 32-column group: odd, conflict-free per lane
#define PK_OUT_BYTES (PK_TILE * PK_LDW * 4)
#define PK_STR_CAP 16384                       // bytes of one column's tile staged in LDS
enum { PK_BOOL = 0, PK_I8, PK_I16, PK_I32, PK_I64, PK_U8, PK_U16, PK_U32, PK_F32, PK_F64, PK_BYTES, PK_UCS4, PK_TEXT };   // = SPRK_COL_*

struct PackDev {
    int n_id, n_dense;
    unsigned rows, n_nl;
    const unsigned char* ptr[PK_MAX_COLS];     // id columns first, then the dense ones
    int stride[PK_MAX_COLS];
    int vocab[PK_MAX_COLS];
    unsigned short width[PK_MAX_COLS];         // S / U: element width; text: index of the column in the block
    unsigned char storage[PK_MAX_COLS], rule[PK_MAX_COLS];
    const unsigned char* text;
    size_t text_len;
    const unsigned long long* nl;
    unsigned long long g_mul;                  // the genre perfect hash of k_csv_pack.h
    unsigned long long gt_lo[32], gt_hi[32];
    signed char gt_len[32], gt_idx[32];
};
static_assert(sizeof(PackDev) + 24 <= 4096, "PackDev travels as a kernel argument");

// UCS4 element read in place: every code point as one byte (above 127 -> 0xFF)
struct PkRdGlobalU {
    typedef size_t pos_t;
    const unsigned* __restrict__ t;
    size_t len;
    __device__ __forceinline__ unsigned operator[](size_t i) const { const unsigned c = t[i]; return c > 127u ? 0xFFu : c; }
    __device__ __forceinline__ unsigned long long win(size_t i) const {
        unsigned long long w = 0;
        for (int k = 0; k < 8 && i + k < len; ++k) w |= (unsigned long long)(*this)[i + k] << (8 * k);
        return w;
    }
};

// keys[0] = first range error, keys[1] = first declined value: (column << 32) | row, ~0 = none
__device__ __forceinline__ void pk_report(unsigned long long* keys, int which, int c, unsigned row) {
    atomicMin(keys + which, ((unsigned long long)(unsigned)c << 32) | row);
}

// the string field [a, b) of column c -> the output's 32 bits
template <class R, class P>
__device__ __forceinline__ unsigned pk_from_string(const PackDev& D, const unsigned long long* g_tab, const signed char* g_len, const R& rd, P a, P b,
                                                   int c, unsigned row, unsigned long long* keys) {
    const int rule = D.rule[c];
    if (rule == 1) {                                               // genre vocabulary (exact match) or -1
        const unsigned gn = (unsigned)(b - a);
        int val = -1;
        if (gn >= 1 && gn <= 16) {
            unsigned long long w0 = rd.win(a), w1 = 0;
            if (gn < 8) w0 &= ~0ull >> (64 - 8 * gn);
            if (gn > 8) { w1 = rd.win(a + 8); if (gn < 16) w1 &= ~0ull >> (64 - 8 * (gn - 8)); }
            const unsigned sl = csv_genre_slot(w0, w1, gn, D.g_mul);
            if (g_len[sl] == (int)gn && g_tab[2 * sl] == w0 && g_tab[2 * sl + 1] == w1) val = g_len[32 + sl];
        }
        if (val >= D.vocab[c]) val = -1;
        return (unsigned)val;
    }
    double v = 0.0;
    int st = 1;                                                    // 0 = value, 1 = empty, 2 = not on the exact path
    if (a != b) {
        if ((unsigned)(b - a) <= 8 && csv_number_short(rd, a, b, v)) st = 0;
        else st = csv_number(rd, a, b, v);
    }
    if (st == 2) { pk_report(keys, 1, c, row); return 0u; }
    if (rule == 2) return __float_as_uint((float)v);
    if (!(v >= -9.2233720368547758e18 && v < 9.2233720368547758e18)) { pk_report(keys, 1, c, row); return 0u; }
    const long long iv = (long long)v;                             // int(float(v)) of the Python packer; empty -> 0
    if (iv < 0 || iv >= D.vocab[c]) pk_report(keys, 0, c, row);
    return (unsigned)(int)iv;
}

// an integer / a float element of column c -> the output's 32 bits
__device__ __forceinline__ unsigned pk_from_int(const PackDev& D, long long iv, bool is_bool, int c, unsigned row, unsigned long long* keys) {
    const int rule = D.rule[c];
    if (rule == 2) return __float_as_uint((float)iv);              // ONE rounding (numpy's astype(float32)), not by way of double
    if (rule == 1) {
        if (is_bool) { pk_report(keys, 1, c, row); return 0u; }
        return (iv < 0 || iv >= D.vocab[c]) ? ~0u : (unsigned)iv;
    }
    if (iv < 0 || iv >= D.vocab[c]) pk_report(keys, 0, c, row);
    return (unsigned)(int)iv;
}
__device__ __forceinline__ unsigned pk_from_float(const PackDev& D, double v, int c, unsigned row, unsigned long long* keys) {
    const int rule = D.rule[c];
    if (v != v) v = 0.0;                                           // NaN = missing
    if (rule == 2) return __float_as_uint((float)v);
    if (rule == 1 || !(v >= -9.2233720368547758e18 && v < 9.2233720368547758e18)) { pk_report(keys, 1, c, row); return 0u; }
    const long long iv = (long long)v;
    if (iv < 0 || iv >= D.vocab[c]) pk_report(keys, 0, c, row);
    return (unsigned)(int)iv;
}

// bytes [g0, g1) of `src` -> LDS at str + (g0 & 15) (16-byte loads for the granules that lie inside the span, bytes at its two ends:
// nothing outside [g0, g1) is read); returns that offset.  Workgroup-uniform arguments; the caller puts the barriers around it.
__device__ __forceinline__ unsigned pk_stage_bytes(const unsigned char* __restrict__ src, size_t g0, size_t g1, unsigned char* str) {
    const size_t A0 = (size_t)src + g0, A1 = (size_t)src + g1, base = A0 & ~(size_t)15;
    for (size_t o = (size_t)threadIdx.x * 16; base + o < A1; o += PK_TILE * 16) {
        const size_t q = base + o;
        if (q >= A0 && q + 16 <= A1) {
            *reinterpret_cast<uint4*>(str + o) = *reinterpret_cast<const uint4*>(q);
        } else {
            for (int k = 0; k < 16; ++k)
                if (q + k >= A0 && q + k < A1) str[o + k] = *reinterpret_cast<const unsigned char*>(q + k);
        }
    }
    return (unsigned)(A0 - base);
}

template <bool STR>
__global__ __launch_bounds__(PK_TILE) void k_pack_columns(const PackDev D, int* __restrict__ ids, float* __restrict__ dense,
                                                          unsigned long long* __restrict__ keys) {
    unsigned* tile = reinterpret_cast<unsigned*>(smem);                                         // [PK_TILE][ldw]
    unsigned char* str = reinterpret_cast<unsigned char*>(smem) + PK_OUT_BYTES;                 // STR: PK_STR_CAP + CSV_LDS_SLACK, then the genre table
    const unsigned long long* g_tab = reinterpret_cast<const unsigned long long*>(str + PK_STR_CAP + CSV_LDS_SLACK);
    const signed char* g_len = reinterpret_cast<const signed char*>(g_tab + 64);
    if constexpr (STR) {
        if (threadIdx.x < 32) {
            unsigned long long* g = const_cast<unsigned long long*>(g_tab);
            g[2 * threadIdx.x] = D.gt_lo[threadIdx.x];
            g[2 * threadIdx.x + 1] = D.gt_hi[threadIdx.x];
            signed char* gl = reinterpret_cast<signed char*>(g + 64);
            gl[threadIdx.x] = D.gt_len[threadIdx.x];
            gl[32 + threadIdx.x] = D.gt_idx[threadIdx.x];
        }
        __syncthreads();
    }
    const unsigned row0 = blockIdx.x * PK_TILE;
    const unsigned nrows = D.rows - row0 < PK_TILE ? D.rows - row0 : PK_TILE;
    const unsigned r = threadIdx.x, row = row0 + r;
    const bool active = r < nrows;
    for (int mat = 0; mat < 2; ++mat) {
        const int n = mat ? D.n_dense : D.n_id, cbase = mat ? D.n_id : 0;
        unsigned* out = mat ? reinterpret_cast<unsigned*>(dense) : reinterpret_cast<unsigned*>(ids);
        const bool single = n <= PK_GROUP;
        const int ldw = single ? n : PK_LDW;
        for (int g0 = 0; g0 < n; g0 += PK_GROUP) {
            const int gw = n - g0 < PK_GROUP ? n - g0 : PK_GROUP;
            for (int j = 0; j < gw; ++j) {
                const int c = cbase + g0 + j;
                const int storage = D.storage[c];
                const int stride = D.stride[c];
                const unsigned char* base = D.ptr[c];
                unsigned bits = 0;
                if (storage < PK_BYTES) {
                    if (active) {
                        const unsigned char* p = base + (long long)row * stride;
                        switch (storage) {
                        case PK_BOOL: bits = pk_from_int(D, *p != 0, true, c, row, keys); break;
                        case PK_I8: bits = pk_from_int(D, *reinterpret_cast<const signed char*>(p), false, c, row, keys); break;
                        case PK_I16: bits = pk_from_int(D, *reinterpret_cast<const short*>(p), false, c, row, keys); break;
                        case PK_I32: bits = pk_from_int(D, *reinterpret_cast<const int*>(p), false, c, row, keys); break;
                        case PK_I64: bits = pk_from_int(D, *reinterpret_cast<const long long*>(p), false, c, row, keys); break;
                        case PK_U8: bits = pk_from_int(D, *p, false, c, row, keys); break;
                        case PK_U16: bits = pk_from_int(D, *reinterpret_cast<const unsigned short*>(p), false, c, row, keys); break;
                        case PK_U32: bits = pk_from_int(D, *reinterpret_cast<const unsigned*>(p), false, c, row, keys); break;
                        case PK_F32: bits = pk_from_float(D, (double)*reinterpret_cast<const float*>(p), c, row, keys); break;
                        default: bits = pk_from_float(D, *reinterpret_cast<const double*>(p), c, row, keys); break;
                        }
                    }
                } else if constexpr (STR) {
                    const unsigned w = D.width[c];
                    if (storage == PK_TEXT) {
                        // lines [l0, l0 + nrows) of the block: one contiguous piece
                        const size_t l0 = (size_t)w * D.rows + row0;
                        const size_t t0 = l0 == 0 ? 0 : (size_t)D.nl[l0 - 1] + 1;
                        const size_t t1 = (size_t)D.nl[l0 + nrows - 1];
                        size_t lo = 0, hi = 0;
                        if (active) {
                            lo = l0 + r == 0 ? 0 : (size_t)D.nl[l0 + r - 1] + 1;
                            hi = (size_t)D.nl[l0 + r];
                        }
                        if (t1 - t0 <= PK_STR_CAP) {
                            __syncthreads();                               // (the previous column's readers)
                            const unsigned off = pk_stage_bytes(D.text, t0, t1, str);
                            __syncthreads();
                            if (active) {
                                const CsvRdLds rd{str};
                                bits = pk_from_string(D, g_tab, g_len, rd, off + (unsigned)(lo - t0), off + (unsigned)(hi - t0), c, row, keys);
                            }
                        } else if (active) {
                            const CsvRdGlobal rd{D.text, D.text_len};
                            bits = pk_from_string(D, g_tab, g_len, rd, lo, hi, c, row, keys);
                        }
                    } else {
                        const unsigned eb = storage == PK_UCS4 ? 4u * w : w;       // element bytes
                        if ((unsigned)stride == eb && nrows * w <= PK_STR_CAP) {
                            __syncthreads();
                            unsigned off = 0;
                            if (storage == PK_BYTES) {
                                off = pk_stage_bytes(base, (size_t)row0 * w, (size_t)(row0 + nrows) * w, str);
                            } else {
                                const unsigned* cp = reinterpret_cast<const unsigned*>(base) + (size_t)row0 * w;
                                for (unsigned k = threadIdx.x; k < nrows * w; k += PK_TILE) { const unsigned u = cp[k]; str[k] = (unsigned char)(u > 127u ? 0xFFu : u); }
                            }
                            __syncthreads();
                            if (active) {
                                const CsvRdLds rd{str};
                                unsigned a = off + r * w, b = a + w;
                                while (b > a && rd[b - 1] == 0) --b;      // numpy strips the trailing NULs; an embedded NUL stays
                                bits = pk_from_string(D, g_tab, g_len, rd, a, b, c, row, keys);
                            }
                        } else if (active) {
                            const unsigned char* p = base + (long long)row * stride;
                            if (storage == PK_BYTES) {
                                const CsvRdGlobal rd{p, w};
                                size_t b = w;
                                while (b > 0 && rd[b - 1] == 0) --b;
                                bits = pk_from_string(D, g_tab, g_len, rd, (size_t)0, b, c, row, keys);
                            } else {
                                const PkRdGlobalU rd{reinterpret_cast<const unsigned*>(p), w};
                                size_t b = w;
                                while (b > 0 && rd[b - 1] == 0) --b;
                                bits = pk_from_string(D, g_tab, g_len, rd, (size_t)0, b, c, row, keys);
                            }
                        }
                    }
                }
                if (active) tile[r * ldw + j] = bits;
            }
            __syncthreads();
            if (single) {
                // the tile is one contiguous span of the output: 16-byte stores (the span starts on a multiple of 1024 bytes)
                const unsigned dwords = nrows * (unsigned)n;
                unsigned* dst = out + (size_t)row0 * n;
                for (unsigned o = threadIdx.x * 4; o < dwords; o += PK_TILE * 4) {
                    if (o + 4 <= dwords) *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(tile + o);
                    else for (unsigned k = o; k < dwords; ++k) dst[k] = tile[k];
                }
            } else {
                for (unsigned o = threadIdx.x; o < nrows * (unsigned)gw; o += PK_TILE) {
                    const unsigned rr = o / (unsigned)gw, cc = o - rr * (unsigned)gw;
                    out[(size_t)(row0 + rr) * n + g0 + cc] = tile[rr * PK_LDW + cc];
                }
            }
            __syncthreads();
        }
    }
}
