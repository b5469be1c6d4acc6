// The token grammar of the word2vec-text reader, shared by its kernels (dw_embread.hip) and by
// dw_embread_host / dw_f32_token_host (dw_host.cpp: the same code on the host). Not part of the
// ABI. Restated in tests/embread_ref.py.
//
// A line's tokens are its maximal runs of non-blank bytes; blank is what bytes.split() splits
// on, so a '\r' in front of the line end is a trailing blank. Token 0 is the key, the others are
// values: numpy.float32(float(token)), by dw_strtod.h's exact double and its integer rounding to
// float32.
#pragma once

#include "dw_strtod.h"

namespace dw {
namespace embread {

constexpr int MAX_DIM = 512;
constexpr int UNDECIDED_WORDS = 4;   // (row, column, byte offset, byte length)

enum { TOKEN_BAD = 0, TOKEN_DECIDED = 1, TOKEN_UNDECIDED = 2 };   // DW_TOKEN_* of dw_hip.h

__host__ __device__ __forceinline__ bool is_blank(uint8_t c) {
    return c == ' ' || (c >= 9 && c <= 13);   // space, \t, \n, \v, \f, \r
}

// Where the token that starts at p ends: the first blank at or behind p, or lim.
template <class T>
__host__ __device__ __forceinline__ int64_t token_end(const T &text, int64_t p, int64_t lim) {
    while (p < lim && !is_blank(text[p])) ++p;
    return p;
}

// text[p, e) against a lower-case word, in any letter case.
template <class T>
__host__ __device__ __forceinline__ bool is_word(const T &text, int64_t p, int64_t e,
                                                 const char *word, int len) {
    if (e - p != len) return false;
    for (int i = 0; i < len; ++i)
        if ((text[p + i] | 0x20) != static_cast<uint8_t>(word[i])) return false;
    return true;
}

// A number the grammar of dw_strtod.h has scanned from text[p, q): its float32, or undecided.
__host__ __device__ __forceinline__ int number_token(const strtod::Scan &s, int64_t p, int64_t q,
                                                     const uint64_t *__restrict__ pow5,
                                                     int64_t *end, uint32_t *bits) {
    *end = q;
    uint64_t b = 0;
    if (q - p > strtod::MAX_TOKEN || !strtod::scan_bits(s, pow5, &b)) return TOKEN_UNDECIDED;
    *bits = strtod::f32_from_f64_bits(b);
    return TOKEN_DECIDED;
}

// The value token at text[p, ..), in a line that ends at lim: *end = where it ends. DECIDED:
// *bits = the float32 of float(token). UNDECIDED (the host's float() decides, 0.0 meanwhile):
// what the conversion cannot fix, more than strtod::MAX_TOKEN bytes, and everything outside the
// grammar of dw_strtod.h that is no nan / inf / infinity.
template <class T>
__host__ __device__ __forceinline__ int value_token(const T &text, int64_t p, int64_t lim,
                                                    const uint64_t *__restrict__ pow5,
                                                    int64_t *end, uint32_t *bits) {
    *bits = 0;
    int64_t q = p;
    strtod::Scan s;
    if (strtod::scan_token(text, lim, q, &s) && (q == lim || is_blank(text[q])))
        return number_token(s, p, q, pow5, end, bits);
    const int64_t e = token_end(text, p, lim);
    *end = e;
    int64_t w = p;
    uint32_t sign = 0;
    if (w < e && (text[w] == '+' || text[w] == '-')) {
        sign = text[w] == '-' ? 0x80000000u : 0u;
        ++w;
    }
    if (is_word(text, w, e, "nan", 3)) {
        *bits = sign | 0x7FC00000u;
        return TOKEN_DECIDED;
    }
    if (is_word(text, w, e, "inf", 3) || is_word(text, w, e, "infinity", 8)) {
        *bits = sign | 0x7F800000u;
        return TOKEN_DECIDED;
    }
    return TOKEN_UNDECIDED;
}

// value_token for a caller that holds text[.., near_lim) in a faster form (`near`, near_lim <=
// lim): a number that ends in front of near_lim, the usual token, is read from there alone;
// whatever reaches near_lim or is no number goes the general way. The result is the same.
template <class N, class T>
__host__ __device__ __forceinline__ int value_token(const N &near, int64_t near_lim, const T &text,
                                                    int64_t p, int64_t lim,
                                                    const uint64_t *__restrict__ pow5,
                                                    int64_t *end, uint32_t *bits) {
    *bits = 0;
    int64_t q = p;
    strtod::Scan s;
    if (strtod::scan_token(near, near_lim, q, &s) &&
        (q < near_lim ? is_blank(near[q]) : q == lim))
        return number_token(s, p, q, pow5, end, bits);
    return value_token(text, p, lim, pow5, end, bits);
}

// The key token at text[p, ..): *end = where it ends; its value where it is 1 to 18 decimal
// digits without a leading zero ("0" itself is one), so that str(value) gives the bytes back;
// else -1.
template <class T>
__host__ __device__ __forceinline__ int64_t key_token(const T &text, int64_t p, int64_t lim,
                                                      int64_t *end) {
    int64_t q = p, v = 0;
    bool plain = true;
    for (; q < lim; ++q) {
        const uint8_t c = text[q];
        if (is_blank(c)) break;
        if (plain && strtod::digit_at(c) && q - p < 18)
            v = v * 10 + (c - '0');
        else
            plain = false;
    }
    *end = q;
    if (q - p > 1 && text[p] == '0') plain = false;
    return plain && q > p ? v : -1;
}

}  // namespace embread
}  // namespace dw
