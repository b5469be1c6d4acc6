// Host-side runtime pieces of the C ABI (no device code).
//
// dw_host_shuffle: CPython 3.10's random.shuffle over range(n), bit for bit, in native code.
// The reference shuffles its start-node list with the global `random` once in the
// RandomWalkDataset constructor and again at every epoch end (datasets.py:45,86-88); in Python
// that loop costs ~0.5 s per epoch for 1M nodes. The Mersenne Twister below is CPython's
// _randommodule.c genrand_uint32 (MT19937, N = 624, M = 397), `getrandbits(k) = genrand >> (32 -
// k)` for k <= 32, and Lib/random.py `_randbelow_with_getrandbits` / `shuffle`:
//     for i in reversed(range(1, n)): j = randbelow(i + 1); x[i], x[j] = x[j], x[i]
//     randbelow(m): k = m.bit_length(); r = getrandbits(k); while r >= m: r = getrandbits(k)
// The caller passes the generator state as random.getstate()[1] (624 words + index) and writes
// the advanced state back with random.setstate, so the global stream continues exactly where
// Python's own shuffle would have left it.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "dw_common.h"
#include "dw_embread.h"
#include "dw_f32text.h"
#include "dw_strtod.h"

namespace {

constexpr int MT_N = 624, MT_M = 397;
constexpr uint32_t MATRIX_A = 0x9908b0dfu, UPPER = 0x80000000u, LOWER = 0x7fffffffu;

struct MT {
    uint32_t *mt;   // 624 words
    uint32_t idx;

    uint32_t next() {
        if (idx >= MT_N) {
            int kk = 0;
            uint32_t y;
            for (; kk < MT_N - MT_M; ++kk) {
                y = (mt[kk] & UPPER) | (mt[kk + 1] & LOWER);
                mt[kk] = mt[kk + MT_M] ^ (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u);
            }
            for (; kk < MT_N - 1; ++kk) {
                y = (mt[kk] & UPPER) | (mt[kk + 1] & LOWER);
                mt[kk] = mt[kk + (MT_M - MT_N)] ^ (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u);
            }
            y = (mt[MT_N - 1] & UPPER) | (mt[0] & LOWER);
            mt[MT_N - 1] = mt[MT_M - 1] ^ (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u);
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= (y >> 11);
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= (y >> 18);
        return y;
    }
};

inline int bit_length(uint64_t m) {
    int k = 0;
    while (m) {
        ++k;
        m >>= 1;
    }
    return k;
}

// ---- 128-bit powers of five for the weighted edge-list parser (dw_strtod.h) -------------------
// Computed once with exact integer arithmetic (5^342 has 795 bits): for q >= 0 the top 128 bits
// of 5^q, truncated; for q < 0, floor(2^(b + 127) / 5^-q) + 1 with b the bit length of 5^-q
// (halved if it reaches 2^128). Both have bit 127 set.
struct Big {
    static constexpr int LIMBS = 16;   // 1024 bits, least significant first
    uint64_t v[LIMBS];

    int bits() const {
        for (int i = LIMBS - 1; i >= 0; --i)
            if (v[i]) return 64 * i + bit_length(v[i]);
        return 0;
    }
    bool bit(int k) const { return k >= 0 && ((v[k >> 6] >> (k & 63)) & 1u) != 0; }
    void times5() {
        uint64_t carry = 0;
        for (int i = 0; i < LIMBS; ++i) {
            const unsigned __int128 t = static_cast<unsigned __int128>(v[i]) * 5u + carry;
            v[i] = static_cast<uint64_t>(t);
            carry = static_cast<uint64_t>(t >> 64);
        }
    }
    void twice() {
        for (int i = LIMBS - 1; i > 0; --i) v[i] = (v[i] << 1) | (v[i - 1] >> 63);
        v[0] <<= 1;
    }
    bool at_least(const Big &o) const {
        for (int i = LIMBS - 1; i >= 0; --i)
            if (v[i] != o.v[i]) return v[i] > o.v[i];
        return true;
    }
    void minus(const Big &o) {
        uint64_t borrow = 0;
        for (int i = 0; i < LIMBS; ++i) {
            const uint64_t a = v[i], b = o.v[i];
            v[i] = a - b - borrow;
            borrow = (a < b || (a == b && borrow)) ? 1u : 0u;
        }
    }
};

struct Pow5Table {
    uint64_t w[2 * dw::strtod::TABLE_ENTRIES];

    Pow5Table() {
        Big p = {};
        p.v[0] = 1;
        for (int k = 0; k <= dw::strtod::Q_MAX || k <= -dw::strtod::Q_MIN; ++k) {
            const int b = p.bits();
            if (k <= dw::strtod::Q_MAX) {   // bits [b - 128, b) of 5^k (zeros below bit 0)
                uint64_t hi = 0, lo = 0;
                for (int j = 0; j < 64; ++j) {
                    hi = (hi << 1) | (p.bit(b - 1 - j) ? 1u : 0u);
                    lo = (lo << 1) | (p.bit(b - 65 - j) ? 1u : 0u);
                }
                set(k, hi, lo);
            }
            if (k >= 1 && k <= -dw::strtod::Q_MIN) {   // long division of 2^(b + 127) by 5^k
                Big r = {};
                r.v[(b - 1) >> 6] = 1ull << ((b - 1) & 63);   // 2^(b - 1) < 5^k: no quotient bit yet
                uint64_t hi = 0, lo = 0;
                for (int j = 0; j < 128; ++j) {
                    r.twice();
                    const bool one = r.at_least(p);
                    if (one) r.minus(p);
                    hi = (hi << 1) | (lo >> 63);
                    lo = (lo << 1) | (one ? 1u : 0u);
                }
                if (++lo == 0 && ++hi == 0) {   // reached 2^128: halve
                    hi = 1ull << 63;
                    lo = 0;
                }
                set(-k, hi, lo);
            }
            p.times5();
        }
    }
    void set(int q, uint64_t hi, uint64_t lo) {
        w[2 * (q - dw::strtod::Q_MIN)] = hi;
        w[2 * (q - dw::strtod::Q_MIN) + 1] = lo;
    }
};

const Pow5Table &pow5_table() {
    static const Pow5Table t;
    return t;
}

struct Bytes {
    const uint8_t *p;
    uint8_t operator[](int64_t i) const { return p[i]; }
};

}  // namespace

extern "C" {

int dw_pow5_table(uint64_t *out) {
    DW_REQUIRE(out, "dw_pow5_table: null pointer");
    const Pow5Table &t = pow5_table();
    for (int i = 0; i < 2 * dw::strtod::TABLE_ENTRIES; ++i) out[i] = t.w[i];
    return DW_OK;
}

int dw_weight_token_host(const uint8_t *token, int64_t n_bytes, int32_t *kind, uint64_t *bits) {
    DW_REQUIRE(kind && bits && n_bytes >= 0 && (token || n_bytes == 0),
               "dw_weight_token_host: bad arguments");
    *kind = DW_TOKEN_BAD;
    *bits = 0;
    dw::strtod::Scan s;
    int64_t p = 0;
    if (n_bytes > dw::strtod::MAX_TOKEN || !dw::strtod::scan_token(Bytes{token}, n_bytes, p, &s) ||
        p != n_bytes)
        return DW_OK;
    *kind = dw::strtod::scan_bits(s, pow5_table().w, bits) ? DW_TOKEN_DECIDED : DW_TOKEN_UNDECIDED;
    return DW_OK;
}

int dw_host_shuffle(uint32_t *mt_state, int64_t *perm, int64_t n) {
    DW_REQUIRE(mt_state && (perm || n == 0), "dw_host_shuffle: null pointer");
    DW_REQUIRE(n >= 0 && n <= (int64_t(1) << 32), "dw_host_shuffle: n must be in [0, 2^32]");
    DW_REQUIRE(mt_state[MT_N] <= static_cast<uint32_t>(MT_N), "dw_host_shuffle: bad MT index");
    MT g{mt_state, mt_state[MT_N]};
    for (int64_t i = 0; i < n; ++i) perm[i] = i;
    for (int64_t i = n - 1; i >= 1; --i) {
        const uint64_t m = static_cast<uint64_t>(i) + 1;   // randbelow(i + 1), i + 1 <= 2^32
        const int k = bit_length(m);
        uint64_t r;
        do {
            if (k <= 32) {
                r = g.next() >> (32 - k);
            } else {   // k = 33 (m = 2^32): getrandbits fills 32-bit words, least significant first
                const uint64_t lo = g.next();
                r = lo | (static_cast<uint64_t>(g.next() >> 31) << 32);
            }
        } while (r >= m);
        const int64_t j = static_cast<int64_t>(r);
        const int64_t t = perm[i];
        perm[i] = perm[j];
        perm[j] = t;
    }
    mt_state[MT_N] = g.idx;
    return DW_OK;
}

// Vose alias table over the whole vocabulary for dw_sgns_noise_alias (float64, serial, one-time):
// k_alias_build's stack discipline (dw_graph.hip) on one row of V entries — the small list grows
// from the front of `stack`, the large list from its back, both pop from the top — with the
// entry packed as {alias id << 32 | prob_thr}. An id of weight 0 has scaled weight 0, so
// prob_thr = 0 (never kept) when it meets a large id; one that rounding leaves on the small
// stack after the large stack ran out gets prob_thr = 0 and the heaviest id (the first of them)
// as its alias instead of "always". Restated in tests/noise_ref.py (Python floats: the same
// IEEE operations in the same order).
int dw_noise_alias_build(const double *weights, int64_t V, uint64_t *table) {
#pragma clang fp contract(off)
    DW_REQUIRE(V >= 1 && V < (int64_t(1) << 31),
               "dw_noise_alias_build: vocab_size must be in [1, 2^31)");
    DW_REQUIRE(weights && table, "dw_noise_alias_build: null pointer");
    double sum = 0.0;
    int64_t heaviest = 0;
    for (int64_t i = 0; i < V; ++i) {
        const double w = weights[i];
        DW_REQUIRE(w >= 0.0 && w <= 1.7976931348623157e308,
                   "dw_noise_alias_build: weight %lld is negative or not finite", (long long)i);
        sum += w;
        if (w > weights[heaviest]) heaviest = i;
    }
    DW_REQUIRE(sum > 0.0 && sum <= 1.7976931348623157e308,
               "dw_noise_alias_build: the weights must have a positive, finite sum");
    double *scaled = static_cast<double *>(malloc(sizeof(double) * static_cast<size_t>(V)));
    int32_t *stack = static_cast<int32_t *>(malloc(sizeof(int32_t) * static_cast<size_t>(V)));
    if (!scaled || !stack) {
        free(scaled);
        free(stack);
        dw::set_error("dw_noise_alias_build: out of host memory for %lld entries", (long long)V);
        return DW_E_UNSUPPORTED;
    }
    const auto entry = [](uint32_t thr, int64_t alias) {
        return (static_cast<uint64_t>(alias) << 32) | thr;
    };
    int64_t ns = 0, nl = 0;
    for (int64_t i = 0; i < V; ++i) {
        const double s = weights[i] * static_cast<double>(V) / sum;
        scaled[i] = s;
        if (s < 1.0)
            stack[ns++] = static_cast<int32_t>(i);
        else
            stack[V - 1 - nl++] = static_cast<int32_t>(i);
    }
    while (ns > 0 && nl > 0) {
        const int32_t l = stack[--ns];
        const int32_t g = stack[V - 1 - --nl];
        const double pl = scaled[l];
        table[l] = entry(static_cast<uint32_t>(fmin(floor(pl * 4294967296.0), 4294967295.0)), g);
        const double pg = (scaled[g] + pl) - 1.0;
        scaled[g] = pg;
        if (pg < 1.0)
            stack[ns++] = g;
        else
            stack[V - 1 - nl++] = g;
    }
    while (nl > 0) {
        const int32_t g = stack[V - 1 - --nl];
        table[g] = entry(0xFFFFFFFFu, g);
    }
    while (ns > 0) {
        const int32_t l = stack[--ns];
        table[l] = weights[l] == 0.0 ? entry(0u, heaviest) : entry(0xFFFFFFFFu, l);
    }
    free(scaled);
    free(stack);
    return DW_OK;
}


// The table dw_f32text.h reads, with exact integers: 5^47 < 2^110 fits an unsigned __int128, and
// the inverses come from a bit-by-bit long division whose remainder stays below 5^30 < 2^70.
int dw_f32text_table(uint64_t *out) {
    namespace ft = dw::f32text;
    DW_REQUIRE(out, "dw_f32text_table: null pointer");
    unsigned __int128 p = 1;
    for (int i = 0; i < ft::POW_ENTRIES; ++i, p *= 5) {
        const int b = static_cast<int>(ft::pow5bits(static_cast<uint32_t>(i)));
        if (i < ft::INV_ENTRIES) {   // floor(2^(b - 1 + 59) / 5^i) + 1
            unsigned __int128 r = 1;
            uint64_t q = 0;
            for (int j = 0; j < b - 1 + ft::INV_BITS; ++j) {
                r <<= 1;
                const bool one = r >= p;
                if (one) r -= p;
                q = (q << 1) | (one ? 1u : 0u);
            }
            out[i] = q + 1;
        }
        out[ft::INV_ENTRIES + i] = static_cast<uint64_t>(
            b >= ft::POW_BITS ? p >> (b - ft::POW_BITS) : p << (ft::POW_BITS - b));
    }
    return DW_OK;
}

// The host mirror of dw_embtext_sizes (out == NULL) and dw_embtext_write (out != NULL): the same
// per-value code (dw_f32text.h), one row after the other.
int dw_embtext_host(const float *table, int64_t vocab_size, int32_t dim, const int64_t *rows,
                    int64_t n_rows, const int64_t *keys_i64, const uint8_t *key_bytes,
                    const int64_t *key_off, int64_t *line_off, int64_t r0, int64_t r1,
                    uint8_t *out, int64_t capacity, int32_t *status) {
    namespace ft = dw::f32text;
    DW_REQUIRE(table && line_off && status, "dw_embtext_host: null pointer");
    DW_REQUIRE(vocab_size >= 1 && n_rows >= 0, "dw_embtext_host: bad sizes");
    DW_REQUIRE(dim >= 1, "dw_embtext_host: dim must be >= 1");
    DW_REQUIRE((keys_i64 != nullptr) != (key_bytes != nullptr && key_off != nullptr),
               "dw_embtext_host: give keys_i64 or (key_bytes, key_off), not both");
    static uint64_t tab[ft::TABLE_WORDS];
    static const int tab_ok = dw_f32text_table(tab);
    (void)tab_ok;
    if (out) {
        DW_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= n_rows, "dw_embtext_host: bad row range");
        DW_REQUIRE(capacity >= 0 && line_off[r1] - line_off[r0] <= capacity,
                   "dw_embtext_host: rows [%lld, %lld) need %lld bytes, the buffer holds %lld",
                   (long long)r0, (long long)r1, (long long)(line_off[r1] - line_off[r0]),
                   (long long)capacity);
    } else {
        r0 = 0;
        r1 = n_rows;
        line_off[0] = 0;
    }
    int32_t st = 0;
    for (int64_t r = r0; r < r1; ++r) {
        int64_t src = rows ? rows[r] : r;
        const bool bad_row = src < 0 || src >= vocab_size;
        if (bad_row) st |= DW_S_BAD_INDEX;
        int64_t key = 0, klen;
        if (keys_i64) {
            key = keys_i64[r];
            if (key < 0) {
                st |= DW_S_BAD_INDEX;
                key = 0;
            }
            klen = ft::key_digits(key);
        } else {
            klen = key_off[r + 1] - key_off[r];
            if (klen < 0) {
                st |= DW_S_BAD_INDEX;
                klen = 0;
            }
        }
        uint8_t *w = out ? out + (line_off[r] - line_off[r0]) : nullptr;
        if (w) {
            if (keys_i64) {
                uint64_t v = static_cast<uint64_t>(key);
                for (int64_t j = klen - 1; j >= 0; --j, v /= 10u)
                    w[j] = static_cast<uint8_t>('0' + v % 10u);
            } else {
                for (int64_t j = 0; j < klen; ++j) w[j] = key_bytes[key_off[r] + j];
            }
            w += klen;
        }
        int64_t len = klen + 1;
        for (int32_t c = 0; c < dim; ++c) {
            uint32_t bits = 0;
            if (!bad_row) memcpy(&bits, table + src * dim + c, 4);
            const ft::Dec d = ft::shortest(bits, tab);
            if (d.kind != ft::FINITE) st |= DW_S_NONFINITE;
            len += 1 + ft::token_len(d);
            if (w) {
                *w++ = ' ';
                ft::token_emit(d, [&w](uint8_t b) { *w++ = b; });
            }
        }
        if (w)
            *w++ = '\n';
        else
            line_off[r + 1] = line_off[r] + len;
    }
    *status |= st;
    return DW_OK;
}

int dw_f32_token_host(const uint8_t *token, int64_t n_bytes, int32_t *kind, uint32_t *bits32) {
    namespace er = dw::embread;
    DW_REQUIRE(kind && bits32 && n_bytes >= 0 && (token || n_bytes == 0),
               "dw_f32_token_host: bad arguments");
    *kind = DW_TOKEN_BAD;
    *bits32 = 0;
    if (n_bytes == 0 || er::token_end(Bytes{token}, 0, n_bytes) != n_bytes) return DW_OK;
    int64_t end = 0;
    *kind = er::value_token(Bytes{token}, 0, n_bytes, pow5_table().w, &end, bits32);
    return DW_OK;
}

// The host mirror of dw_embread_lines + dw_embread_parse: the same token code (dw_embread.h),
// one line after the other.
int dw_embread_host(const uint8_t *text, int64_t n_bytes, int32_t dim, float *table,
                    int64_t n_rows, int64_t row0, int64_t *key_off, int64_t *key_len,
                    int64_t *key_i64, int64_t *undecided, int64_t undecided_capacity,
                    int64_t *counts, int64_t *err_line, int32_t *status) {
    namespace er = dw::embread;
    DW_REQUIRE(dim >= 1, "dw_embread_host: dim must be >= 1");
    if (dim > er::MAX_DIM) {
        dw::set_error("dw_embread_host: dim %d > %d is not supported", dim, er::MAX_DIM);
        return DW_E_UNSUPPORTED;
    }
    DW_REQUIRE(n_bytes >= 0 && undecided_capacity >= 0 && row0 >= 0 && row0 <= n_rows,
               "dw_embread_host: bad sizes");
    DW_REQUIRE(counts && err_line && status && (n_bytes == 0 || text) &&
                   (row0 == n_rows || (table && key_off && key_len && key_i64)) &&
                   (undecided_capacity == 0 || undecided),
               "dw_embread_host: null pointer");
    const Bytes t{text};
    const uint64_t *pow5 = pow5_table().w;
    int64_t line = 0, n_undecided = 0, bad = -1;
    int32_t st = 0;
    for (int64_t ls = 0; ls < n_bytes; ++line) {
        int64_t le = ls;
        while (le < n_bytes && text[le] != '\n') ++le;
        const int64_t next = le < n_bytes ? le + 1 : le;
        if (row0 + line < n_rows) {
            int64_t tokens = 0;
            for (int64_t p = ls; p < le;) {   // the count first: a bad line stores nothing
                if (er::is_blank(text[p])) {
                    ++p;
                } else {
                    ++tokens;
                    p = er::token_end(t, p, le);
                }
            }
            if (tokens != dim + 1) {
                st |= DW_S_BAD_TEXT;
                if (bad < 0) bad = line;
            } else {
                const int64_t row = row0 + line;
                int64_t j = 0;
                for (int64_t p = ls; p < le;) {
                    if (er::is_blank(text[p])) {
                        ++p;
                        continue;
                    }
                    int64_t e = p;
                    if (j == 0) {
                        key_i64[row] = er::key_token(t, p, le, &e);
                        key_off[row] = p;
                        key_len[row] = e - p;
                        if (key_i64[row] < 0) st |= DW_S_TEXT_KEY;
                    } else {
                        uint32_t bits = 0;
                        const int kind = er::value_token(t, p, le, pow5, &e, &bits);
                        memcpy(table + row * dim + (j - 1), &bits, 4);
                        if (kind == er::TOKEN_UNDECIDED) {
                            if (n_undecided < undecided_capacity) {
                                int64_t *u = undecided + er::UNDECIDED_WORDS * n_undecided;
                                u[0] = row;
                                u[1] = j - 1;
                                u[2] = p;
                                u[3] = e - p;
                            }
                            ++n_undecided;
                        }
                    }
                    ++j;
                    p = e;
                }
            }
        }
        ls = next;
    }
    counts[0] = line;
    counts[1] = n_undecided;
    *err_line = bad;
    *status |= st;
    return DW_OK;
}

}  // extern "C"
