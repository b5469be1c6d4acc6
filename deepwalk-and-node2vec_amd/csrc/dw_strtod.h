// Exact decimal-to-double conversion in integer arithmetic, shared by the weighted edge-list
// parser (dw_edgelist.hip: the kernel) and dw_weight_token_host (dw_host.cpp: the same code on
// the host, for CPU tests), and by the embedding text reader (dw_embread.h), which rounds the
// double on to float32 (f32_from_f64_bits). Not part of the ABI. Restated in tests/strtod_ref.py.
//
// The method is Eisel-Lemire (Lemire, "Number parsing at a gigabyte per second", 2021): a decimal
// significand w < 2^64 and a power of ten q give the double nearest w * 10^q from one or two
// 64x64->128 products of the normalised w with a 128-bit approximation of 5^q. Where the product's
// low bits cannot fix the rounding, and for subnormal, underflowing and overflowing results, the
// conversion reports "undecided" and its caller hands the token to the host's strtod.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace dw {
namespace strtod {

constexpr int Q_MIN = -342, Q_MAX = 308;          // the table's powers of ten
constexpr int TABLE_ENTRIES = Q_MAX - Q_MIN + 1;  // 651, each (high, low) 64-bit words
constexpr int MAX_TOKEN = 64;                     // bytes of a weight token
constexpr int MAX_EXP_DIGITS = 4;
constexpr int MAX_DIGITS = 19;                    // significant digits kept in w (10^19 < 2^64)

__host__ __device__ __forceinline__ uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

// Bits of the double nearest w * 10^q (ties to even), sign excluded. false: undecided — the
// low-bits test failed, or the result is subnormal, zero by underflow, or overflows.
__host__ __device__ __forceinline__ bool convert(uint64_t w, int32_t q,
                                                 const uint64_t *__restrict__ pow5,
                                                 uint64_t *bits) {
    if (w == 0) {
        *bits = 0;
        return true;
    }
    if (q < Q_MIN || q > Q_MAX) return false;
    int lz = __builtin_clzll(w);
    w <<= lz;
    const uint64_t hi5 = pow5[2 * (q - Q_MIN)];
    uint64_t upper = mulhi64(w, hi5), lower = w * hi5;
    if ((upper & 0x1FFu) == 0x1FFu) {   // the 55 bits in use may change with the low word's product
        const uint64_t second_hi = mulhi64(w, pow5[2 * (q - Q_MIN) + 1]);
        lower += second_hi;
        if (lower < second_hi) ++upper;
        if (lower == ~0ull && (q < -27 || q > 55)) return false;
    }
    const int upperbit = static_cast<int>(upper >> 63);
    const int shift = upperbit + 9;
    uint64_t mantissa = upper >> shift;
    int32_t power2 = ((217706 * q) >> 16) + 1086 + upperbit - lz;
    if (power2 <= 0) return false;
    if (lower <= 1 && q >= -4 && q <= 23 && (mantissa & 3u) == 1u && (mantissa << shift) == upper)
        mantissa &= ~1ull;   // exactly halfway: round to even
    mantissa += mantissa & 1u;
    mantissa >>= 1;
    if (mantissa >= (2ull << 52)) {
        mantissa = 1ull << 52;
        ++power2;
    }
    mantissa &= ~(1ull << 52);
    if (power2 >= 0x7FF) return false;
    *bits = (static_cast<uint64_t>(power2) << 52) | mantissa;
    return true;
}

struct Scan {
    uint64_t w;       // the first MAX_DIGITS significant digits
    int32_t q;        // the value is w * 10^q, plus the dropped digits
    bool neg;
    bool truncated;   // a dropped digit was not zero
};

__host__ __device__ __forceinline__ bool digit_at(uint8_t c) { return c >= '0' && c <= '9'; }

// The longest prefix of text[p, n) that matches the weight grammar — [+-] (digits [. digits*] |
// . digits+) [(e|E) [+-] digits{1,4}] — scanned into s; p moves behind it. false: no such prefix
// (no digit, an exponent without digits or with a fifth one). The caller checks what follows and
// the token's length. T: anything indexed by byte position (the kernel's staged text, a pointer).
template <class T>
__host__ __device__ __forceinline__ bool scan_token(const T &text, int64_t n, int64_t &p,
                                                    Scan *s) {
    int64_t i = p;
    bool neg = false;
    if (i < n && (text[i] == '+' || text[i] == '-')) {
        neg = text[i] == '-';
        ++i;
    }
    uint64_t w = 0;
    int32_t q = 0;
    int nd = 0;
    bool seen = false, truncated = false;
    for (; i < n; ++i) {   // integer part
        const uint8_t c = text[i];
        if (!digit_at(c)) break;
        seen = true;
        if (nd < MAX_DIGITS) {
            if (nd != 0 || c != '0') {
                w = w * 10 + (c - '0');
                ++nd;
            }
        } else {
            truncated = truncated || c != '0';
            ++q;
        }
    }
    if (i < n && text[i] == '.') {
        for (++i; i < n; ++i) {   // fraction
            const uint8_t c = text[i];
            if (!digit_at(c)) break;
            seen = true;
            if (nd < MAX_DIGITS) {
                if (nd != 0 || c != '0') {
                    w = w * 10 + (c - '0');
                    ++nd;
                }
                --q;
            } else {
                truncated = truncated || c != '0';
            }
        }
    }
    if (!seen) return false;
    if (i < n && (text[i] == 'e' || text[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < n && (text[i] == '+' || text[i] == '-')) {
            eneg = text[i] == '-';
            ++i;
        }
        int32_t e = 0;
        int ne = 0;
        for (; i < n; ++i) {
            const uint8_t c = text[i];
            if (!digit_at(c)) break;
            if (++ne > MAX_EXP_DIGITS) return false;
            e = e * 10 + (c - '0');
        }
        if (ne == 0) return false;
        q += eneg ? -e : e;
    }
    p = i;
    *s = Scan{w, q, neg, truncated};
    return true;
}

// The scanned token's double. With dropped digits the value lies in (w, w + 1) * 10^q: decided
// only where both ends give the same double.
__host__ __device__ __forceinline__ bool scan_bits(const Scan &s,
                                                   const uint64_t *__restrict__ pow5,
                                                   uint64_t *bits) {
    uint64_t b = 0;
    if (!convert(s.w, s.q, pow5, &b)) return false;
    if (s.truncated) {
        uint64_t b1 = 0;
        if (!convert(s.w + 1, s.q, pow5, &b1) || b1 != b) return false;
    }
    *bits = b | (s.neg ? 1ull << 63 : 0ull);
    return true;
}

// numpy.float32(x) of the double with these bits, in integer arithmetic: the 53-bit significand
// is cut to 24 bits — fewer below 2^-126, where the result is a subnormal counted in units of
// 2^-149 — and rounded to nearest, ties to even. A carry out of the significand moves into the
// exponent field by itself, so the round-up into FLT_MIN and into a power of two need no case of
// their own; from 2^128 - 2^103 on the result is inf. No hardware f64 -> f32 convert: its
// subnormal results depend on the kernel's denormal mode.
__host__ __device__ __forceinline__ uint32_t f32_from_f64_bits(uint64_t b) {
    const uint32_t sign = static_cast<uint32_t>(b >> 63) << 31;
    const int32_t e = static_cast<int32_t>((b >> 52) & 0x7FFu);
    const uint64_t m = b & ((1ull << 52) - 1);
    if (e == 0x7FF) return sign | (m ? 0x7FC00000u : 0x7F800000u);
    if (e == 0) return sign;                       // zero, or below 2^-1022
    const uint64_t sig = m | (1ull << 52);         // the value is sig * 2^(e - 1075)
    int32_t shift = 29, field = e - 1023 + 127;    // float32's exponent field, if normal
    if (field <= 0) {                              // subnormal: units of 2^-149, field 0
        shift += 1 - field;
        field = 0;
        if (shift > 54) return sign;               // below 2^-150: under half a unit
    } else {
        --field;                                   // (the significand's top bit adds it back)
    }
    const uint64_t keep = sig >> shift, rem = sig & ((1ull << shift) - 1);
    const uint64_t half = 1ull << (shift - 1);
    const uint64_t up = (rem > half || (rem == half && (keep & 1u))) ? 1u : 0u;
    const uint64_t r = (static_cast<uint64_t>(field) << 23) + keep + up;
    return sign | (r >= 0x7F800000u ? 0x7F800000u : static_cast<uint32_t>(r));
}

}  // namespace strtod
}  // namespace dw
