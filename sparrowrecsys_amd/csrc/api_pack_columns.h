// api_pack_columns.h -- C ABI: a dict of feature columns -> packed ids / dense, on host threads (sprk_pack_columns) and on the device
// (sprk_pack_columns_device: k_pack_columns.h), sprk_pack_last_route.  Part of sparrow_hip.hip; included there behind api_ingest.h
// (kGenreVocab, DevScratch, genre_hash_table, scan_u32 are that file's).  The rule of both: convert the listed cases with the Python packer's bits or
// DECLINE the batch (SPRK_EKIND) -- include/sparrow_hip.h states the cases.
namespace {
thread_local int g_pack_route = -1;

const int kPkElemBytes[10] = {1, 1, 2, 4, 8, 1, 2, 4, 4, 8};       // SPRK_COL_BOOL .. SPRK_COL_F64
const unsigned long long kPkNone = ~0ull;
inline unsigned long long pk_key(int c, uint32_t row) { return ((unsigned long long)(unsigned)c << 32) | row; }

// [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)? -> strtod's value; anything else, or a result of +-inf, is declined
bool pk_parse_decimal(const char* s, size_t n, double* v) {
    auto dig = [&](size_t i) { return i < n && s[i] >= '0' && s[i] <= '9'; };
    size_t i = 0;
    if (i < n && (s[i] == '+' || s[i] == '-')) ++i;
    size_t n_int = 0, n_frac = 0;
    while (dig(i)) { ++i; ++n_int; }
    if (i < n && s[i] == '.') { ++i; while (dig(i)) { ++i; ++n_frac; } }
    if (n_int + n_frac == 0) return false;
    if (i < n && (s[i] == 'e' || s[i] == 'E')) {
        ++i;
        if (i < n && (s[i] == '+' || s[i] == '-')) ++i;
        if (!dig(i)) return false;
        while (dig(i)) ++i;
    }
    if (i != n) return false;
    char buf[64];
    std::string big;
    const char* z = buf;
    if (n < sizeof(buf)) { memcpy(buf, s, n); buf[n] = 0; }
    else { big.assign(s, n); z = big.c_str(); }
    const double d = strtod(z, nullptr);
    if (d - d != 0.0) return false;                              // +-inf ("1e400"): Python decides
    *v = d;
    return true;
}
inline bool pk_in_int64(double v) { return v >= -9.2233720368547758e18 && v < 9.2233720368547758e18; }

// what one chunk of rows found: the smallest key of a range error and of a declined value (column order wins over row order)
struct PkFound { unsigned long long range = kPkNone, decline = kPkNone; long long range_value = 0; };

// One string field -> the output's 32 bits.  false = declined.
inline bool pk_host_string(const sprk_pack_col& col, const char* s, size_t n, uint32_t* bits, long long* iv_out, bool* bad_range) {
    if (col.rule == SPRK_RULE_GENRE) {
        int32_t v = -1;
        for (int g = 0; g < 19; ++g)
            if (n == strlen(kGenreVocab[g]) && memcmp(s, kGenreVocab[g], n) == 0) { v = g; break; }
        if (v >= col.vocab) v = -1;
        *bits = (uint32_t)v;
        return true;
    }
    double d = 0.0;
    if (n != 0 && !pk_parse_decimal(s, n, &d)) return false;
    if (col.rule == SPRK_RULE_DENSE) { const float f = (float)d; memcpy(bits, &f, 4); return true; }
    if (!pk_in_int64(d)) return false;
    const long long iv = (long long)d;                           // int(float(v)) of the Python packer
    if (iv < 0 || iv >= col.vocab) { *bad_range = true; *iv_out = iv; }
    *bits = (uint32_t)(int32_t)iv;
    return true;
}
inline bool pk_host_int(const sprk_pack_col& col, long long iv, bool is_bool, uint32_t* bits, long long* iv_out, bool* bad_range) {
    if (col.rule == SPRK_RULE_DENSE) { const float f = (float)iv; memcpy(bits, &f, 4); return true; }   // one rounding, as astype(float32)
    if (col.rule == SPRK_RULE_GENRE) {
        if (is_bool) return false;
        *bits = (iv < 0 || iv >= col.vocab) ? ~0u : (uint32_t)iv;
        return true;
    }
    if (iv < 0 || iv >= col.vocab) { *bad_range = true; *iv_out = iv; }
    *bits = (uint32_t)(int32_t)iv;
    return true;
}
inline bool pk_host_float(const sprk_pack_col& col, double v, uint32_t* bits, long long* iv_out, bool* bad_range) {
    if (v != v) v = 0.0;
    if (col.rule == SPRK_RULE_DENSE) { const float f = (float)v; memcpy(bits, &f, 4); return true; }
    if (col.rule == SPRK_RULE_GENRE || !pk_in_int64(v)) return false;
    const long long iv = (long long)v;
    if (iv < 0 || iv >= col.vocab) { *bad_range = true; *iv_out = iv; }
    *bits = (uint32_t)(int32_t)iv;
    return true;
}
template <class T> inline T pk_load(const unsigned char* p) { T v; memcpy(&v, p, sizeof(T)); return v; }

// The element at `p` of a numeric / fixed-width column (w = its width), or the text field [p, p + n).
inline bool pk_host_elem(const sprk_pack_col& col, const unsigned char* p, size_t n, std::string& tmp, uint32_t* bits, long long* iv, bool* bad) {
    switch (col.storage) {
    case SPRK_COL_BOOL: return pk_host_int(col, *p != 0, true, bits, iv, bad);
    case SPRK_COL_I8: return pk_host_int(col, pk_load<int8_t>(p), false, bits, iv, bad);
    case SPRK_COL_I16: return pk_host_int(col, pk_load<int16_t>(p), false, bits, iv, bad);
    case SPRK_COL_I32: return pk_host_int(col, pk_load<int32_t>(p), false, bits, iv, bad);
    case SPRK_COL_I64: return pk_host_int(col, pk_load<int64_t>(p), false, bits, iv, bad);
    case SPRK_COL_U8: return pk_host_int(col, *p, false, bits, iv, bad);
    case SPRK_COL_U16: return pk_host_int(col, pk_load<uint16_t>(p), false, bits, iv, bad);
    case SPRK_COL_U32: return pk_host_int(col, pk_load<uint32_t>(p), false, bits, iv, bad);
    case SPRK_COL_F32: return pk_host_float(col, (double)pk_load<float>(p), bits, iv, bad);
    case SPRK_COL_F64: return pk_host_float(col, pk_load<double>(p), bits, iv, bad);
    case SPRK_COL_BYTES: {
        size_t m = (size_t)col.width;
        while (m > 0 && p[m - 1] == 0) --m;                      // numpy strips the trailing NULs; an embedded NUL stays
        return pk_host_string(col, (const char*)p, m, bits, iv, bad);
    }
    case SPRK_COL_UCS4: {
        size_t m = (size_t)col.width;
        while (m > 0 && pk_load<uint32_t>(p + 4 * (m - 1)) == 0) --m;
        tmp.resize(m);
        for (size_t k = 0; k < m; ++k) { const uint32_t u = pk_load<uint32_t>(p + 4 * k); tmp[k] = (char)(u > 127u ? 0xFFu : u); }   // above 127: no genre, no digit
        return pk_host_string(col, tmp.data(), m, bits, iv, bad);
    }
    default: return pk_host_string(col, (const char*)p, n, bits, iv, bad);
    }
}

// rows [r0, r1) of one output column -> out[row * ld + j]; nl = the text block's newline offsets
void pk_host_column(const sprk_pack_col& col, int key_col, const char* text, const uint64_t* nl, int64_t rows, int64_t r0, int64_t r1,
                    uint32_t* out, size_t ld, PkFound& found) {
    std::string tmp;
    const unsigned char* base = (const unsigned char*)col.data;
    for (int64_t r = r0; r < r1; ++r) {
        uint32_t bits = 0;
        long long iv = 0;
        bool bad = false, ok;
        if (col.storage == SPRK_COL_TEXT) {
            const size_t line = (size_t)col.width * (size_t)rows + (size_t)r;
            const size_t lo = line == 0 ? 0 : (size_t)nl[line - 1] + 1, hi = (size_t)nl[line];
            ok = pk_host_elem(col, (const unsigned char*)text + lo, hi - lo, tmp, &bits, &iv, &bad);
        } else {
            ok = pk_host_elem(col, base + r * col.stride, 0, tmp, &bits, &iv, &bad);
        }
        if (!ok) { const unsigned long long k = pk_key(key_col, (uint32_t)r); if (k < found.decline) found.decline = k; }
        else if (bad) { const unsigned long long k = pk_key(key_col, (uint32_t)r); if (k < found.range) { found.range = k; found.range_value = iv; } }
        out[(size_t)r * ld] = bits;
    }
}

int pk_validate(const char* who, const sprk_pack_col* id_cols, int32_t n_id, const sprk_pack_col* dense_cols, int32_t n_dense, const char* text,
                int32_t rows, const void* ids_out, const void* dense_out, bool device, int* n_text_out) {
    if (n_id < 0 || n_dense < 0 || rows < 0) return fail(SPRK_EINVAL, "%s: negative column count / rows", who);
    if ((n_id > 0 && (!id_cols || !ids_out)) || (n_dense > 0 && (!dense_cols || !dense_out))) return fail(SPRK_EINVAL, "%s: NULL column list / output", who);
    int max_text = -1;
    for (int j = 0; j < n_id + n_dense; ++j) {
        const sprk_pack_col& c = j < n_id ? id_cols[j] : dense_cols[j - n_id];
        const char* nm = c.name ? c.name : "?";
        if (!c.name) return fail(SPRK_EINVAL, "%s: column %d has no name", who, j);
        if (c.storage < SPRK_COL_BOOL || c.storage > SPRK_COL_TEXT) return fail(SPRK_EINVAL, "%s: column %s has unknown storage kind %d", who, nm, c.storage);
        if (j < n_id ? (c.rule != SPRK_RULE_IDENTITY && c.rule != SPRK_RULE_GENRE) : c.rule != SPRK_RULE_DENSE)
            return fail(SPRK_EINVAL, "%s: column %s has rule %d (id columns: identity or genre, dense columns: dense)", who, nm, c.rule);
        if (c.storage == SPRK_COL_TEXT) {
            if (c.width < 0 || c.width >= SPRK_PACK_MAX_COLS) return fail(SPRK_EINVAL, "%s: column %s: text column index %d", who, nm, c.width);
            if (!text) return fail(SPRK_EINVAL, "%s: column %s reads the text block, which is NULL", who, nm);
            if (c.on_device) return fail(SPRK_EINVAL, "%s: column %s: the text block is host memory", who, nm);
            if (c.width > max_text) max_text = c.width;
            continue;
        }
        if (!c.data) return fail(SPRK_EINVAL, "%s: column %s has no data", who, nm);
        if ((c.storage == SPRK_COL_BYTES || c.storage == SPRK_COL_UCS4) && (c.width < 1 || c.width > 65535))
            return fail(SPRK_EINVAL, "%s: column %s has width %d (1 .. 65535)", who, nm, c.width);
        if (c.on_device) {
            if (!device) return fail(SPRK_EINVAL, "%s: column %s is device memory (use sprk_pack_columns_device)", who, nm);
            const int64_t al = c.storage == SPRK_COL_BYTES ? 1 : (c.storage == SPRK_COL_UCS4 ? 4 : kPkElemBytes[c.storage]);
            if (((uintptr_t)c.data % al) || (c.stride % al)) return fail(SPRK_EINVAL, "%s: device column %s is not aligned to its element", who, nm);
            if (c.stride >= ((int64_t)1 << 31) || c.stride < -((int64_t)1 << 31)) return fail(SPRK_EINVAL, "%s: device column %s: stride beyond 2^31", who, nm);
        }
    }
    *n_text_out = max_text + 1;
    return SPRK_OK;
}

// offsets of the block's newlines; false (declined) unless there are exactly n_text * rows of them and the last byte is one
bool pk_newlines(const char* text, size_t len, size_t expect, std::vector<uint64_t>& nl) {
    nl.resize(expect);
    size_t k = 0;
    for (size_t i = 0; i < len; ++i)
        if (text[i] == '\n') { if (k == expect) return false; nl[k++] = i; }
    return k == expect && (expect == 0 ? len == 0 : text[len - 1] == '\n');
}

int pk_threads(int32_t n_threads, int64_t rows) {
    int T = n_threads < 1 ? 1 : (n_threads > 256 ? 256 : n_threads);
    if (rows < 16384) T = 1;                                     // (not worth a thread start)
    else if ((int64_t)T > rows / 8192) T = (int)(rows / 8192);
    return T;
}
template <class F> void pk_parallel(int T, int64_t rows, F body) {
    if (T <= 1) { body(0, (int64_t)0, rows); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back([&, t]() { body(t, rows * t / T, rows * (t + 1) / T); });
    for (auto& x : th) x.join();
}

int pk_decline(const sprk_pack_col* id_cols, int32_t n_id, const sprk_pack_col* dense_cols, unsigned long long key, const char* twin) {
    const int c = (int)(key >> 32);
    const sprk_pack_col& col = c < n_id ? id_cols[c] : dense_cols[c - n_id];
    g_pack_route = 0;
    return fail(SPRK_EKIND, "%s row %u holds a value the %s packer does not convert (declined: the next route decides)", col.name, (unsigned)(key & 0xFFFFFFFFu), twin);
}
int pk_range(const sprk_pack_col& col, long long value) {
    return fail(SPRK_ERANGE, "%s id %lld outside [0, %d) (reference: assert_less_than_num_buckets)", col.name, value, col.vocab);
}
}  // namespace

extern "C" {

int sprk_pack_columns(const sprk_pack_col* id_cols, int32_t n_id, const sprk_pack_col* dense_cols, int32_t n_dense, const char* text, size_t text_len,
                      int32_t rows, int32_t n_threads, int32_t* ids_out, float* dense_out) {
    g_pack_route = -1;
    int n_text = 0;
    SPRK_TRY(pk_validate("pack_columns", id_cols, n_id, dense_cols, n_dense, text, rows, ids_out, dense_out, false, &n_text));
    std::vector<uint64_t> nl;
    if (n_text && !pk_newlines(text, text_len, (size_t)n_text * (size_t)rows, nl)) {
        g_pack_route = 0;
        return fail(SPRK_EKIND, "the text block does not hold %d x %d newline-terminated fields (declined: the next route decides)", n_text, rows);
    }
    const int T = pk_threads(n_threads, rows);
    std::vector<PkFound> found(T);
    pk_parallel(T, rows, [&](int t, int64_t r0, int64_t r1) {
        for (int j = 0; j < n_id; ++j) pk_host_column(id_cols[j], j, text, nl.data(), rows, r0, r1, (uint32_t*)ids_out + j, (size_t)n_id, found[t]);
        for (int j = 0; j < n_dense; ++j) pk_host_column(dense_cols[j], n_id + j, text, nl.data(), rows, r0, r1, (uint32_t*)dense_out + j, (size_t)n_dense, found[t]);
    });
    PkFound all;
    for (const PkFound& f : found) {
        if (f.decline < all.decline) all.decline = f.decline;
        if (f.range < all.range) { all.range = f.range; all.range_value = f.range_value; }
    }
    if (all.decline != kPkNone) return pk_decline(id_cols, n_id, dense_cols, all.decline, "host");
    g_pack_route = 1;
    if (all.range != kPkNone) return pk_range(id_cols[all.range >> 32], all.range_value);
    return SPRK_OK;
}

}  // extern "C"

namespace {
// the calling thread's staging pair: a pinned host buffer and its device twin (plus the newline scratch behind it), kept and grown
struct PkStaging {
    void* host = nullptr;
    size_t host_cap = 0;
    DevScratch dev;
    int ensure_host(size_t bytes) {
        if (bytes <= host_cap) return SPRK_OK;
        if (host) (void)hipHostFree(host);
        host = nullptr; host_cap = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        if (hipHostMalloc(&host, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); host = nullptr; return fail(SPRK_EHIP, "pinned staging buffer of %zu bytes for the column packer", want); }
        host_cap = want;
        return SPRK_OK;
    }
};
thread_local PkStaging g_pack_staging;
inline size_t pk_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
}  // namespace

extern "C" {

int sprk_pack_columns_device(const sprk_pack_col* id_cols, int32_t n_id, const sprk_pack_col* dense_cols, int32_t n_dense, const char* text,
                             size_t text_len, int32_t rows, int32_t n_threads, int32_t* ids_dev, float* dense_dev, void* stream) {
    RoctxRange roctx_range_("sprk_pack_columns_device");
    g_pack_route = -1;
    int n_text = 0;
    SPRK_TRY(pk_validate("pack_columns_device", id_cols, n_id, dense_cols, n_dense, text, rows, ids_dev, dense_dev, true, &n_text));
    const int n_cols = n_id + n_dense;
    if (n_cols > SPRK_PACK_MAX_COLS) return fail(SPRK_EINVAL, "pack_columns_device packs at most %d columns (%d given)", SPRK_PACK_MAX_COLS, n_cols);
    if (((uintptr_t)ids_dev & 15) || ((uintptr_t)dense_dev & 15)) return fail(SPRK_EINVAL, "pack_columns_device: the outputs must start on a 16-byte boundary");
    if (rows == 0 || n_cols == 0) { g_pack_route = 2; return SPRK_OK; }
    auto column = [&](int j) -> const sprk_pack_col& { return j < n_id ? id_cols[j] : dense_cols[j - n_id]; };
    // the text block's newline count is checked on the host, before anything is launched: k_csv_mark writes one offset per newline
    const size_t n_nl = (size_t)n_text * (size_t)rows;
    if (n_text) {
        size_t k = 0;
        for (const char* p = text; (p = (const char*)memchr(p, '\n', (size_t)(text + text_len - p))) != nullptr; ++p) ++k;
        if (k != n_nl || text[text_len - 1] != '\n' || text_len >= ((size_t)1 << 32)) {
            g_pack_route = 0;
            return fail(SPRK_EKIND, "the text block does not hold %d x %d newline-terminated fields (declined: the next route decides)", n_text, rows);
        }
    }
    // layout of the staged bytes: 256 bytes of keys, every host column compacted (16-byte aligned, 16 spare bytes), the text block
    std::vector<size_t> off(n_cols, 0);
    size_t at = 256;
    bool any_str = n_text > 0;
    for (int j = 0; j < n_cols; ++j) {
        const sprk_pack_col& c = column(j);
        if (c.storage == SPRK_COL_BYTES || c.storage == SPRK_COL_UCS4) any_str = true;
        if (c.storage == SPRK_COL_TEXT || c.on_device) continue;
        int dup = -1;                                            // one source feeding several outputs is staged once
        for (int i = 0; i < j && dup < 0; ++i) {
            const sprk_pack_col& o = column(i);
            if (!o.on_device && o.storage == c.storage && o.data == c.data && o.stride == c.stride && o.width == c.width) dup = i;
        }
        if (dup >= 0) { off[j] = off[dup]; continue; }
        const size_t eb = c.storage == SPRK_COL_BYTES ? (size_t)c.width : (c.storage == SPRK_COL_UCS4 ? 4 * (size_t)c.width : (size_t)kPkElemBytes[c.storage]);
        off[j] = at;
        at = pk_up(at + eb * (size_t)rows + 16, 16);
    }
    const size_t off_text = at;
    if (n_text) at = pk_up(at + text_len + 16, 16);
    const size_t staged = at;
    // device-only scratch behind the staged bytes: the newline passes' counters and nl[]
    const size_t n_chunks = n_text ? (text_len + CSV_CHUNK - 1) / CSV_CHUNK : 0;
    const size_t sums_a = (n_chunks + SCAN_TILE - 1) / SCAN_TILE;
    const size_t off_counts = pk_up(staged, 256);
    const size_t off_nl = pk_up(off_counts + (n_chunks + sums_a + 64) * sizeof(unsigned), 256);
    const size_t total = off_nl + (n_nl + 1) * sizeof(unsigned long long);
    PkStaging& S = g_pack_staging;
    SPRK_TRY(S.ensure_host(staged));
    SPRK_TRY(S.dev.ensure(total));
    unsigned char* hb = (unsigned char*)S.host;
    unsigned char* db = (unsigned char*)S.dev.p;
    memset(hb, 0, 256);
    memset(hb, 0xFF, 16);                                         // keys[0] = range, keys[1] = decline: none yet
    // compaction, rows in chunks per thread and in blocks of 4096 inside a chunk: the columns of one [B, T] matrix share its cache lines
    const int T = pk_threads(n_threads, rows);
    pk_parallel(T, rows, [&](int, int64_t r0, int64_t r1) {
        for (int64_t b0 = r0; b0 < r1; b0 += 4096) {
            const int64_t b1 = b0 + 4096 < r1 ? b0 + 4096 : r1;
            for (int j = 0; j < n_cols; ++j) {
                const sprk_pack_col& c = column(j);
                if (c.storage == SPRK_COL_TEXT || c.on_device) continue;
                bool first = true;
                for (int i = 0; i < j && first; ++i) first = !(off[i] == off[j] && column(i).storage != SPRK_COL_TEXT && !column(i).on_device);
                if (!first) continue;
                const size_t eb = c.storage == SPRK_COL_BYTES ? (size_t)c.width : (c.storage == SPRK_COL_UCS4 ? 4 * (size_t)c.width : (size_t)kPkElemBytes[c.storage]);
                const unsigned char* src = (const unsigned char*)c.data;
                unsigned char* dst = hb + off[j];
                if (c.stride == (int64_t)eb) { memcpy(dst + (size_t)b0 * eb, src + b0 * c.stride, (size_t)(b1 - b0) * eb); continue; }
                switch (eb) {
                case 8: for (int64_t r = b0; r < b1; ++r) memcpy(dst + (size_t)r * 8, src + r * c.stride, 8); break;
                case 4: for (int64_t r = b0; r < b1; ++r) memcpy(dst + (size_t)r * 4, src + r * c.stride, 4); break;
                case 2: for (int64_t r = b0; r < b1; ++r) memcpy(dst + (size_t)r * 2, src + r * c.stride, 2); break;
                case 1: for (int64_t r = b0; r < b1; ++r) dst[r] = src[r * c.stride]; break;
                default: for (int64_t r = b0; r < b1; ++r) memcpy(dst + (size_t)r * eb, src + r * c.stride, eb); break;
                }
            }
        }
    });
    if (n_text) memcpy(hb + off_text, text, text_len);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(db, hb, staged, hipMemcpyHostToDevice, st));
    PackDev D;
    memset(&D, 0, sizeof(D));
    D.n_id = n_id; D.n_dense = n_dense; D.rows = (unsigned)rows; D.n_nl = (unsigned)n_nl;
    for (int j = 0; j < n_cols; ++j) {
        const sprk_pack_col& c = column(j);
        D.storage[j] = (unsigned char)c.storage; D.rule[j] = (unsigned char)c.rule; D.vocab[j] = c.vocab; D.width[j] = (unsigned short)c.width;
        if (c.storage == SPRK_COL_TEXT) continue;
        if (c.on_device) { D.ptr[j] = (const unsigned char*)c.data; D.stride[j] = (int)c.stride; continue; }
        D.ptr[j] = db + off[j];
        D.stride[j] = c.storage == SPRK_COL_BYTES ? c.width : (c.storage == SPRK_COL_UCS4 ? 4 * c.width : kPkElemBytes[c.storage]);
    }
    unsigned long long* keys = (unsigned long long*)db;
    if (n_text) {
        const unsigned char* tdev = db + off_text;
        unsigned* counts = (unsigned*)(db + off_counts);
        unsigned* sums = counts + n_chunks;
        unsigned long long* nl = (unsigned long long*)(db + off_nl);
        hipLaunchKernelGGL(k_csv_count, dim3((unsigned)n_chunks), dim3(256), 0, st, tdev, text_len, counts);
        scan_u32(counts, counts, n_chunks, sums, (unsigned*)(db + 64), st);
        hipLaunchKernelGGL(k_csv_mark, dim3((unsigned)n_chunks), dim3(256), 0, st, tdev, text_len, (const unsigned*)counts, nl);
        D.text = tdev; D.text_len = text_len; D.nl = nl;
    }
    if (any_str && !genre_hash_table(&D.g_mul, D.gt_lo, D.gt_hi, D.gt_len, D.gt_idx)) return fail(SPRK_EINVAL, "no perfect hash for the genre vocabulary");
    const unsigned grid = (unsigned)(((size_t)rows + PK_TILE - 1) / PK_TILE);
    if (any_str)
        hipLaunchKernelGGL(k_pack_columns<true>, dim3(grid), dim3(PK_TILE), PK_OUT_BYTES + PK_STR_CAP + CSV_LDS_SLACK + CSV_LDS_GENRE, st, D, (int*)ids_dev, dense_dev, keys);
    else
        hipLaunchKernelGGL(k_pack_columns<false>, dim3(grid), dim3(PK_TILE), PK_OUT_BYTES, st, D, (int*)ids_dev, dense_dev, keys);
    HIP_TRY(hipGetLastError());
    unsigned long long h_keys[2] = {kPkNone, kPkNone};
    HIP_TRY(hipMemcpyAsync(h_keys, keys, sizeof(h_keys), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_keys[1] != kPkNone) return pk_decline(id_cols, n_id, dense_cols, h_keys[1], "device");
    g_pack_route = 2;
    if (h_keys[0] != kPkNone) {
        // the message carries the full 64-bit value: the element goes through the host twin's converter (same bits wherever the device converts)
        const int c = (int)(h_keys[0] >> 32);
        const uint32_t row = (uint32_t)(h_keys[0] & 0xFFFFFFFFu);
        const sprk_pack_col& col = id_cols[c];
        std::vector<unsigned char> elem;
        const unsigned char* p = nullptr;
        size_t n = 0;
        if (col.storage == SPRK_COL_TEXT) {
            const size_t line = (size_t)col.width * (size_t)rows + row;
            const char* q = text;                                 // (error path: a walk over the block)
            for (size_t l = 0; l < line; ++l) q = (const char*)memchr(q, '\n', (size_t)(text + text_len - q)) + 1;
            p = (const unsigned char*)q;
            n = (size_t)((const char*)memchr(q, '\n', (size_t)(text + text_len - q)) - q);
        } else {
            const size_t eb = col.storage == SPRK_COL_BYTES ? (size_t)col.width : (col.storage == SPRK_COL_UCS4 ? 4 * (size_t)col.width : (size_t)kPkElemBytes[col.storage]);
            if (col.on_device) {
                elem.resize(eb);
                HIP_TRY(hipMemcpy(elem.data(), (const unsigned char*)col.data + (int64_t)row * col.stride, eb, hipMemcpyDeviceToHost));
                p = elem.data();
            } else {
                p = (const unsigned char*)col.data + (int64_t)row * col.stride;
            }
        }
        std::string tmp;
        uint32_t bits = 0;
        long long iv = 0;
        bool bad = false;
        (void)pk_host_elem(col, p, n, tmp, &bits, &iv, &bad);
        return pk_range(col, iv);
    }
    return SPRK_OK;
}

int sprk_pack_last_route(void) { return g_pack_route; }

}  // extern "C"
