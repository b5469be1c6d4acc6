// Exact float32-to-shortest-decimal conversion in integer arithmetic, shared by the embedding
// text writer (dw_embtext.hip: the kernels) and dw_embtext_host (dw_host.cpp: the same code on
// the host, the CPU path and the CPU tests). Not part of the ABI. The token rule is restated with
// numpy and CPython alone in tests/embtext_ref.py.
//
// The method is Ryu for binary32 (Adams, "Ryu: fast float-to-string conversion", PLDI 2018): the
// value's rounding interval (vm, vp) and the value vr are scaled by a power of ten through one
// 32x64-bit product with a 59- or 61-bit approximation of 5^-q or 5^i, and digits are dropped
// while the interval still holds a shorter decimal; the last digit kept is rounded to the closest
// decimal, ties to the even digit, and the interval's ends count when the mantissa is even. That
// is the string numpy's Dragon4 prints in unique mode. No floating-point operation takes part.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace dw {
namespace f32text {

constexpr int INV_ENTRIES = 31;   // floor(2^(bits(5^q) - 1 + 59) / 5^q) + 1, q = 0 .. 30
constexpr int POW_ENTRIES = 48;   // the top 61 bits of 5^i, i = 0 .. 47
constexpr int TABLE_WORDS = INV_ENTRIES + POW_ENTRIES;   // 79 words: the inverses first
constexpr int INV_BITS = 59, POW_BITS = 61;
constexpr int MAX_TOKEN = 19;     // "-9999999000000000.0"

enum Kind : uint32_t { FINITE = 0, INF = 1, NAN_ = 2 };

// The decimal of one float32: the value is 0.d1 d2 .. dnd * 10^decpt, digit dj in nibble nd - j
// of bcd. Zero is the digit 0 with decpt 1.
struct Dec {
    uint64_t bcd;
    int32_t nd, decpt;
    uint32_t neg, kind;
};

__host__ __device__ __forceinline__ uint32_t pow5bits(uint32_t e) {   // bit length of 5^e
    return ((e * 1217359u) >> 19) + 1u;
}
__host__ __device__ __forceinline__ uint32_t log10_pow2(uint32_t e) { return (e * 78913u) >> 18; }
__host__ __device__ __forceinline__ uint32_t log10_pow5(uint32_t e) { return (e * 732923u) >> 20; }

// (m * factor) >> shift for shift >= 32, m < 2^32: exact, in 64-bit words.
__host__ __device__ __forceinline__ uint32_t mul_shift(uint32_t m, uint64_t factor, int32_t shift) {
    const uint64_t lo = static_cast<uint64_t>(m) * static_cast<uint32_t>(factor);
    const uint64_t hi = static_cast<uint64_t>(m) * static_cast<uint32_t>(factor >> 32);
    return static_cast<uint32_t>(((lo >> 32) + hi) >> (shift - 32));
}

__host__ __device__ __forceinline__ bool multiple_of_pow5(uint32_t v, uint32_t p) {
    uint32_t n = 0;
    for (;;) {
        const uint32_t q = v / 5u;
        if (v - 5u * q != 0u) break;
        v = q;
        ++n;
    }
    return n >= p;
}

// The shortest decimal that rounds to the float32 with these bits. tab: TABLE_WORDS words.
__host__ __device__ __forceinline__ Dec shortest(uint32_t bits, const uint64_t *tab) {
    Dec d;
    d.neg = bits >> 31;
    const uint32_t mant = bits & 0x7FFFFFu, expo = (bits >> 23) & 0xFFu;
    if (expo == 0xFFu) {
        d.kind = mant ? NAN_ : INF;
        d.bcd = 0;
        d.nd = 0;
        d.decpt = 0;
        return d;
    }
    d.kind = FINITE;
    if (expo == 0u && mant == 0u) {
        d.bcd = 0;
        d.nd = 1;
        d.decpt = 1;
        return d;
    }
    int32_t e2;
    uint32_t m2;
    if (expo == 0u) {
        e2 = 1 - 127 - 23 - 2;
        m2 = mant;
    } else {
        e2 = static_cast<int32_t>(expo) - 127 - 23 - 2;
        m2 = (1u << 23) | mant;
    }
    const bool accept = (m2 & 1u) == 0u;
    const uint32_t mv = 4u * m2, mp = 4u * m2 + 2u;
    const uint32_t mm_shift = (mant != 0u || expo <= 1u) ? 1u : 0u;
    const uint32_t mm = 4u * m2 - 1u - mm_shift;

    uint32_t vr, vp, vm, last = 0;
    int32_t e10;
    bool vm_tz = false, vr_tz = false;
    if (e2 >= 0) {
        const uint32_t q = log10_pow2(static_cast<uint32_t>(e2));
        e10 = static_cast<int32_t>(q);
        const int32_t k = INV_BITS + static_cast<int32_t>(pow5bits(q)) - 1;
        const int32_t i = -e2 + static_cast<int32_t>(q) + k;
        const uint64_t f = tab[q];
        vr = mul_shift(mv, f, i);
        vp = mul_shift(mp, f, i);
        vm = mul_shift(mm, f, i);
        if (q != 0u && (vp - 1u) / 10u <= vm / 10u) {
            const int32_t l = INV_BITS + static_cast<int32_t>(pow5bits(q - 1u)) - 1;
            last = mul_shift(mv, tab[q - 1u], -e2 + static_cast<int32_t>(q) - 1 + l) % 10u;
        }
        if (q <= 9u) {
            if (mv % 5u == 0u)
                vr_tz = multiple_of_pow5(mv, q);
            else if (accept)
                vm_tz = multiple_of_pow5(mm, q);
            else
                vp -= multiple_of_pow5(mp, q) ? 1u : 0u;
        }
    } else {
        const uint32_t q = log10_pow5(static_cast<uint32_t>(-e2));
        e10 = static_cast<int32_t>(q) + e2;
        const int32_t i = -e2 - static_cast<int32_t>(q);
        const int32_t k = static_cast<int32_t>(pow5bits(static_cast<uint32_t>(i))) - POW_BITS;
        int32_t j = static_cast<int32_t>(q) - k;
        const uint64_t f = tab[INV_ENTRIES + i];
        vr = mul_shift(mv, f, j);
        vp = mul_shift(mp, f, j);
        vm = mul_shift(mm, f, j);
        if (q != 0u && (vp - 1u) / 10u <= vm / 10u) {
            j = static_cast<int32_t>(q) - 1 -
                (static_cast<int32_t>(pow5bits(static_cast<uint32_t>(i + 1))) - POW_BITS);
            last = mul_shift(mv, tab[INV_ENTRIES + i + 1], j) % 10u;
        }
        if (q <= 1u) {
            vr_tz = true;
            if (accept)
                vm_tz = mm_shift == 1u;
            else
                --vp;
        } else if (q < 31u) {
            vr_tz = (mv & ((1u << (q - 1u)) - 1u)) == 0u;
        }
    }

    int32_t removed = 0;
    uint32_t out;
    if (vm_tz || vr_tz) {   // rare: an interval end or the value is itself a short decimal
        while (vp / 10u > vm / 10u) {
            vm_tz = vm_tz && vm % 10u == 0u;
            vr_tz = vr_tz && last == 0u;
            last = vr % 10u;
            vr /= 10u;
            vp /= 10u;
            vm /= 10u;
            ++removed;
        }
        if (vm_tz) {
            while (vm % 10u == 0u) {
                vr_tz = vr_tz && last == 0u;
                last = vr % 10u;
                vr /= 10u;
                vp /= 10u;
                vm /= 10u;
                ++removed;
            }
        }
        if (vr_tz && last == 5u && vr % 2u == 0u) last = 4u;   // exactly halfway: the even digit
        out = vr + (((vr == vm && (!accept || !vm_tz)) || last >= 5u) ? 1u : 0u);
    } else {
        while (vp / 10u > vm / 10u) {
            last = vr % 10u;
            vr /= 10u;
            vp /= 10u;
            vm /= 10u;
            ++removed;
        }
        out = vr + ((vr == vm || last >= 5u) ? 1u : 0u);
    }
    int32_t e = e10 + removed;
    while (out % 10u == 0u) {   // a round-up into a power of ten leaves zeros behind
        out /= 10u;
        ++e;
    }
    uint64_t bcd = 0;
    int32_t nd = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const uint32_t q = out / 10u;
        bcd |= static_cast<uint64_t>(out - 10u * q) << (4 * t);
        nd = (out != 0u) ? t + 1 : nd;
        out = q;
    }
    d.bcd = bcd;
    d.nd = nd;
    d.decpt = nd + e;
    return d;
}

// CPython's repr(float) layout of the digits: positional while -4 < decpt <= 16.
__host__ __device__ __forceinline__ bool positional(const Dec &d) {
    return d.decpt > -4 && d.decpt <= 16;
}

__host__ __device__ __forceinline__ int32_t token_len(const Dec &d) {
    if (d.kind == NAN_) return 3;
    if (d.kind == INF) return 3 + static_cast<int32_t>(d.neg);
    const int32_t s = static_cast<int32_t>(d.neg);
    if (positional(d)) {
        if (d.decpt <= 0) return s + 2 - d.decpt + d.nd;
        return s + (d.decpt < d.nd ? d.nd + 1 : d.decpt + 2);
    }
    return s + (d.nd == 1 ? 1 : d.nd + 1) + 4;
}

// The token's bytes, in order, through put(byte): token_len(d) of them.
template <class Put>
__host__ __device__ __forceinline__ void token_emit(const Dec &d, Put &&put) {
    if (d.kind == NAN_) {
        put('n'), put('a'), put('n');
        return;
    }
    if (d.neg) put('-');
    if (d.kind == INF) {
        put('i'), put('n'), put('f');
        return;
    }
    const uint64_t bcd = d.bcd;
    const int32_t nd = d.nd;
    auto digit = [bcd, nd](int32_t j) -> uint8_t {   // the j-th digit from the left
        return static_cast<uint8_t>('0' + ((bcd >> (4 * (nd - 1 - j))) & 15u));
    };
    if (positional(d)) {
        if (d.decpt <= 0) {
            put('0'), put('.');
            for (int32_t z = d.decpt; z < 0; ++z) put('0');
            for (int32_t j = 0; j < nd; ++j) put(digit(j));
        } else if (d.decpt < nd) {
            for (int32_t j = 0; j < nd; ++j) {
                if (j == d.decpt) put('.');
                put(digit(j));
            }
        } else {
            for (int32_t j = 0; j < nd; ++j) put(digit(j));
            for (int32_t z = nd; z < d.decpt; ++z) put('0');
            put('.'), put('0');
        }
        return;
    }
    put(digit(0));
    if (nd > 1) {
        put('.');
        for (int32_t j = 1; j < nd; ++j) put(digit(j));
    }
    int32_t x = d.decpt - 1;
    put('e');
    put(x < 0 ? '-' : '+');
    x = x < 0 ? -x : x;
    put(static_cast<uint8_t>('0' + x / 10));
    put(static_cast<uint8_t>('0' + x % 10));
}

// Decimal digits of a key >= 0 (1 .. 19).
__host__ __device__ __forceinline__ int32_t key_digits(int64_t k) {
    int32_t n = 1;
    for (uint64_t v = static_cast<uint64_t>(k); v >= 10u; v /= 10u) ++n;
    return n;
}

}  // namespace f32text
}  // namespace dw
