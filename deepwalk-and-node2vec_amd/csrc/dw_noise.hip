// Unigram^power negatives: the device sampler over a whole-vocabulary alias table.
//
// The reference draws its negatives uniformly over [0, V) (utils/sampling.py:7-21), and so do
// noise='torch' and noise='device'. word2vec.c, gensim and the node2vec reference code draw them
// from the unigram law raised to 0.75; this is that law, a documented departure from the
// reference's. The table is built once on the host (dw_noise_alias_build, dw_host.cpp); the
// kernel below draws from it with the Philox stream of the fused kernels' device negatives
// (dw_sgns.hip noise_pair / k_noise_fill: same counter, same words), so with equal weights it
// writes what dw_sgns_noise writes.
#include "dw_common.h"

namespace {

constexpr uint32_t TAG_SGNS = 0x53470000u;  // 'SG' (dw_sgns.hip)

// One draw from 64 random bits: with T = hi*V + ((lo*V) >> 32) — the quantity inside
// dw::bounded64, below 2^64 for V < 2^32 — the slot is T >> 32 (== bounded64(lo, hi, V), bias
// <= V / 2^64) and T's low word is the fractional part of r64 * V / 2^64, uniform and
// independent of the slot: it is tested against the slot's threshold. One dependent 8-B load.
__device__ __forceinline__ int64_t alias_draw(uint32_t lo, uint32_t hi, uint64_t V,
                                              const uint64_t *__restrict__ table) {
    const uint64_t T = static_cast<uint64_t>(hi) * V + ((static_cast<uint64_t>(lo) * V) >> 32);
    const uint32_t i = static_cast<uint32_t>(T >> 32);
    const uint32_t f = static_cast<uint32_t>(T);
    const uint64_t e = table[i];
    const uint32_t thr = static_cast<uint32_t>(e);
    return (thr == 0xFFFFFFFFu || f < thr) ? static_cast<int64_t>(i)
                                           : static_cast<int64_t>(e >> 32);
}

// A lane takes one Philox call: centre b's slots n = 2m (words x, y) and n = 2m + 1 (z, w),
// n = j*K + k, written to out[b*C*K + n]. PAIRED (C*K even and out 16-B aligned): the two ids
// leave as one 16-B store; otherwise two 8-B stores, the second only where the slot exists (an
// odd C*K ends every centre on a lone slot).
template <bool PAIRED>
__global__ void __launch_bounds__(256)
    k_noise_alias(int64_t batch, int32_t CK, int64_t V, const uint64_t *__restrict__ table,
                  uint32_t k0, uint32_t k1, uint64_t noise_offset, const dw_step_scalars *dyn,
                  int64_t *__restrict__ out) {
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    const int32_t calls = (CK + 1) >> 1;   // Philox calls per centre
    const int64_t n = batch * calls;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t off = dyn ? dyn->noise_offset : noise_offset;
    const uint64_t Vu = static_cast<uint64_t>(V);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t b = i / calls;
        const int32_t m = static_cast<int32_t>(i - b * calls);
        const uint64_t g = off + static_cast<uint64_t>(b);
        const dw::U4 r = dw::philox<10>(
            dw::U4{static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32),
                   static_cast<uint32_t>(m), TAG_SGNS},
            k0, k1);
        const int64_t a = alias_draw(r.x, r.y, Vu, table);
        int64_t *dst = out + b * CK + 2 * m;
        if (PAIRED) {
            const int64_t c = alias_draw(r.z, r.w, Vu, table);
            *reinterpret_cast<ll2 *>(dst) = ll2{a, c};
        } else {
            dst[0] = a;
            if (2 * m + 1 < CK) dst[1] = alias_draw(r.z, r.w, Vu, table);
        }
    }
}

}  // namespace

extern "C" {

int dw_sgns_noise_alias(int64_t batch, int32_t n_ctx, int32_t neg_samples, int64_t vocab_size,
                        const uint64_t *table, uint64_t seed, uint64_t noise_offset,
                        int64_t *noise, void *stream) {
    DW_REQUIRE(batch >= 0 && n_ctx >= 0 && neg_samples >= 0 && vocab_size >= 1 &&
                   vocab_size < (int64_t(1) << 31),
               "dw_sgns_noise_alias: bad sizes (vocab_size in [1, 2^31))");
    const int64_t ck = static_cast<int64_t>(n_ctx) * neg_samples;
    DW_REQUIRE(ck <= 0x7FFFFFFE, "dw_sgns_noise_alias: n_ctx * neg_samples must be below 2^31 - 1");
    DW_REQUIRE(ck == 0 || batch <= INT64_MAX / ck, "dw_sgns_noise_alias: batch too large");
    if (batch * ck == 0) return DW_OK;
    DW_REQUIRE(table && noise, "dw_sgns_noise_alias: null pointer");
    const int32_t CK = static_cast<int32_t>(ck);
    const int64_t n = batch * ((CK + 1) >> 1);
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;   // 256 CUs x 8 blocks; the loop strides over the rest
    const bool paired = CK % 2 == 0 && reinterpret_cast<uintptr_t>(noise) % 16 == 0;
    const auto kernel = paired ? k_noise_alias<true> : k_noise_alias<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, dw::as_stream(stream), batch,
                       CK, vocab_size, table, static_cast<uint32_t>(seed),
                       static_cast<uint32_t>(seed >> 32), noise_offset, dw::bound_step_scalars(),
                       noise);
    DW_LAUNCH_CHECK("dw_sgns_noise_alias");
    return DW_OK;
}

}  // extern "C"
