// SGD over the embedding tables: the dense step and the touched-rows step.
//
// Reference: the trainer takes any torch.optim.Optimizer from the config (`train.optimizer.
// _target_`, config_parser/core.py:43-53; word2vec/trainer.py:25-40, 163-165). The single-tensor
// update (torch/optim/sgd.py:_single_tensor_sgd, maximize=False) is restated per element with
// the scalars prepared on the host in float64 and cast to float32 (nlr = -lr, wd, mu,
// omd = 1 - dampening):
//   g1  = wd != 0 ? fma(wd, p, g) : g
//   buf = first ? g1 : fma(omd, g1, RN(mu * buf))          (mu != 0 only)
//   g2  = mu == 0 ? g1 : nesterov ? fma(mu, buf, g1) : buf
//   p   = fma(nlr, g2, p)
// Every fma is explicit and the file is compiled with -ffp-contract=off (csrc/build.py), so the
// chain rounds exactly as written: it equals torch.optim.SGD on CPU fp32 tensors bit for bit
// (tests/test_sgd.py) and both kernels below run it, which pins them to tests/sgd_ref.py.
//
// Without momentum and weight decay a row whose gradient is zero does not move, so stepping the
// rows a batch touched is the whole update: dw_sgd_rows needs no step history and no replay.
#include "dw_common.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

struct SgdScalars {
    float nlr, wd, mu, omd;
    int32_t nesterov, first;
};

template <bool MOM>
__device__ __forceinline__ void sgd_elem(float &p, float g, float &buf, const SgdScalars &s) {
    const float g1 = s.wd != 0.f ? __fmaf_rn(s.wd, p, g) : g;
    float g2 = g1;
    if (MOM) {
        buf = s.first ? g1 : __fmaf_rn(s.omd, g1, s.mu * buf);
        g2 = s.nesterov ? __fmaf_rn(s.mu, buf, g1) : buf;
    }
    p = __fmaf_rn(s.nlr, g2, p);
}

__device__ __forceinline__ bool any_bits(f4v g) {
    return (__float_as_uint(g.x) | __float_as_uint(g.y) | __float_as_uint(g.z) |
            __float_as_uint(g.w)) != 0u;
}

// ---- dw_sgd_dense ----------------------------------------------------------------------------
// One streaming pass, as k_adam (dw_adam.hip): every byte is touched once, so the 16-B loads
// and stores are non-temporal and each lane keeps U = 2 groups of every tensor in flight; g is
// re-zeroed only where its bits are not all +0. n4 = 0 (unaligned buffers): all scalar.
template <bool MOM, bool ZERO>
__global__ void __launch_bounds__(256)
    k_sgd_dense(float *__restrict__ p, float *__restrict__ g, float *__restrict__ buf, int64_t n,
                int64_t n4, SgdScalars s) {
    constexpr int U = 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    f4v *p4 = reinterpret_cast<f4v *>(p);
    f4v *g4 = reinterpret_cast<f4v *>(g);
    f4v *b4 = reinterpret_cast<f4v *>(buf);
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < n4;
         i0 += stride * U) {
        f4v pp[U], gg[U], bb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n4) {
                pp[u] = __builtin_nontemporal_load(p4 + i);
                gg[u] = __builtin_nontemporal_load(g4 + i);
                // (the first step writes the buffer without reading it)
                bb[u] = (MOM && !s.first) ? __builtin_nontemporal_load(b4 + i) : f4v(0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n4) {
                const bool dirty = any_bits(gg[u]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float pe = pp[u][k], be = bb[u][k];
                    sgd_elem<MOM>(pe, gg[u][k], be, s);
                    pp[u][k] = pe;
                    bb[u][k] = be;
                }
                __builtin_nontemporal_store(pp[u], p4 + i);
                if (MOM) __builtin_nontemporal_store(bb[u], b4 + i);
                if (ZERO && dirty) __builtin_nontemporal_store(f4v(0.f), g4 + i);
            }
        }
    }
    for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        float pe = p[i], be = (MOM && !s.first) ? buf[i] : 0.f;
        sgd_elem<MOM>(pe, g[i], be, s);
        p[i] = pe;
        if (MOM) buf[i] = be;
        if (ZERO) g[i] = 0.f;
    }
}

// ---- dw_sgd_rows -----------------------------------------------------------------------------
// A wave takes 64 ids at a time (one coalesced load). Each lane claims its id's row with one
// atomic OR on the row's bit of the claim bitmap (V / 8 bytes: 131 KB at V = 2^20, it stays in
// L2): of all the lanes, waves and blocks that list a row, exactly one sees the bit clear. The
// wave then walks the ballot of its winners, U rows per trip: all 64 lanes step one row together
// (VEC floats per lane and access), and the U rows' loads are issued before the first is used.
// Row r is read and written by its one winner only, so there is nothing to order between
// waves. The bits stay set until the launch ends (a bit cleared by its winner would let a later
// duplicate claim the row again); k_clear_words clears the bitmap behind it on the stream.
//
// p[r] = fma(nlr, g[r], p[r]); g[r] = 0. Where a chunk's gradient bits are all +0 nothing is
// stored: with nlr <= 0 (the entry point refuses another) the product is -0 and p + (-0) is p
// bit for bit, so a listed row no pair touched costs its claim and one read.
template <int VEC>
struct RowVec;
template <>
struct RowVec<4> {
    typedef f4v type;
};
template <>
struct RowVec<2> {
    typedef f2v type;
};
template <>
struct RowVec<1> {
    typedef float type;
};

template <int VEC, typename ID>
__global__ void __launch_bounds__(256)
    k_sgd_rows(float *__restrict__ p, float *__restrict__ g, int64_t V, int32_t d,
               const ID *__restrict__ ids, int64_t n_ids, uint32_t *__restrict__ claim, float nlr,
               int32_t *status) {
    typedef typename RowVec<VEC>::type vec_t;
    constexpr int U = 4;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t base = wave * 64; base < n_ids; base += n_waves * 64) {
        const int64_t i = base + lane;
        int64_t r = -1;
        bool won = false;
        if (i < n_ids) {
            r = static_cast<int64_t>(ids[i]);
            if (r < 0 || r >= V) {
                dw::status_or(status, DW_S_BAD_INDEX);
            } else {   // (the claim word is inside the bitmap: r < V)
                const uint32_t bit = 1u << (r & 31);
                won = (atomicOr(claim + (r >> 5), bit) & bit) == 0u;
            }
        }
        uint64_t todo = __ballot(won);
        const int32_t r32 = static_cast<int32_t>(r);   // V < 2^31
        while (todo) {
            int64_t row[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                row[u] = -1;
                if (todo) {
                    const int src = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    row[u] = __builtin_amdgcn_readlane(r32, src);
                }
            }
            for (int e = lane * VEC; e < d; e += 64 * VEC) {   // (one trip for d <= 64 VEC)
                vec_t pp[U], gg[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (row[u] >= 0) {
                        pp[u] = *reinterpret_cast<const vec_t *>(p + row[u] * d + e);
                        gg[u] = *reinterpret_cast<const vec_t *>(g + row[u] * d + e);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (row[u] >= 0) {
                        uint32_t bits = 0u;
                        vec_t q = pp[u];
                        if constexpr (VEC == 1) {
                            bits = __float_as_uint(gg[u]);
                            q = __fmaf_rn(nlr, gg[u], pp[u]);
                        } else {
#pragma unroll
                            for (int k = 0; k < VEC; ++k) {
                                bits |= __float_as_uint(gg[u][k]);
                                q[k] = __fmaf_rn(nlr, gg[u][k], pp[u][k]);
                            }
                        }
                        if (bits != 0u) {
                            *reinterpret_cast<vec_t *>(p + row[u] * d + e) = q;
                            *reinterpret_cast<vec_t *>(g + row[u] * d + e) = vec_t(0.f);
                        }
                    }
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_clear_words(uint32_t *__restrict__ w, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) w[i] = 0u;
}

template <int VEC, typename ID>
void rows_launch(int64_t blocks, hipStream_t s, float *p, float *g, int64_t V, int32_t d,
                 const void *ids, int64_t n_ids, uint32_t *claim, float nlr, int32_t *status) {
    hipLaunchKernelGGL((k_sgd_rows<VEC, ID>), dim3((unsigned)blocks), dim3(256), 0, s, p, g, V, d,
                       static_cast<const ID *>(ids), n_ids, claim, nlr, status);
}

}  // namespace

extern "C" {

int dw_sgd_dense(float *param, float *grad, float *momentum_buf, int64_t n_elem, float neg_lr,
                 float weight_decay, float momentum, float one_minus_dampening, int32_t nesterov,
                 int32_t first_step, int32_t zero_grad, void *stream) {
    DW_REQUIRE(n_elem >= 0, "dw_sgd_dense: negative size");
    if (n_elem == 0) return DW_OK;   // (an empty tensor's pointer may be NULL)
    DW_REQUIRE(param && grad, "dw_sgd_dense: null pointer");
    DW_REQUIRE(momentum == 0.f || momentum_buf,
               "dw_sgd_dense: momentum != 0 needs a momentum buffer");
    const bool mom = momentum != 0.f;
    const bool aligned = ((uintptr_t)param | (uintptr_t)grad |
                          (mom ? (uintptr_t)momentum_buf : (uintptr_t)0)) % 16 == 0;
    const int64_t n4 = aligned ? n_elem >> 2 : 0;
    const SgdScalars s{neg_lr, weight_decay, momentum, one_minus_dampening, nesterov != 0,
                       first_step != 0};
    int64_t blocks = ((n4 > 0 ? n4 : n_elem) + 255) / 256;
    if (blocks > 8192) blocks = 8192;   // 256 CUs x 8 resident blocks, grid-stride beyond
    hipStream_t st = dw::as_stream(stream);
#define DW_SGD_DENSE(MOM_, ZERO_)                                                              \
    hipLaunchKernelGGL((k_sgd_dense<MOM_, ZERO_>), dim3((unsigned)blocks), dim3(256), 0, st,   \
                       param, grad, momentum_buf, n_elem, n4, s)
    if (mom && zero_grad) DW_SGD_DENSE(true, true);
    else if (mom) DW_SGD_DENSE(true, false);
    else if (zero_grad) DW_SGD_DENSE(false, true);
    else DW_SGD_DENSE(false, false);
#undef DW_SGD_DENSE
    DW_LAUNCH_CHECK("dw_sgd_dense");
    return DW_OK;
}

int dw_sgd_rows(float *param, float *grad, int64_t n_table_rows, int32_t dim, const void *ids,
                int32_t id_bytes, int64_t n_ids, uint32_t *claim, float neg_lr, int32_t *status,
                void *stream) {
    DW_REQUIRE(n_table_rows >= 1 && n_table_rows < (int64_t(1) << 31),
               "dw_sgd_rows: n_table_rows must be in [1, 2^31)");
    DW_REQUIRE(dim >= 1, "dw_sgd_rows: dim must be >= 1 (got %d)", dim);
    DW_REQUIRE(id_bytes == 4 || id_bytes == 8,
               "dw_sgd_rows: id_bytes must be 4 (int32) or 8 (int64) (got %d)", id_bytes);
    DW_REQUIRE(n_ids >= 0, "dw_sgd_rows: negative id count");
    DW_REQUIRE(!(neg_lr > 0.f), "dw_sgd_rows: neg_lr must be <= 0 (it is -lr)");
    DW_REQUIRE(param && grad && claim, "dw_sgd_rows: null pointer");
    if (n_ids == 0) return DW_OK;
    DW_REQUIRE(ids, "dw_sgd_rows: null pointer");
    // the widest access that keeps every row aligned: rows start at multiples of dim floats
    const uintptr_t both = (uintptr_t)param | (uintptr_t)grad;
    const int vec = (dim % 4 == 0 && both % 16 == 0) ? 4 : (dim % 2 == 0 && both % 8 == 0) ? 2 : 1;
    int64_t blocks = (n_ids + 255) / 256;   // 4 waves of 64 ids
    if (blocks > 4096) blocks = 4096;       // 256 CUs x 16 blocks; the waves stride over the rest
    hipStream_t st = dw::as_stream(stream);
#define DW_SGD_ROWS(VEC_)                                                                      \
    do {                                                                                       \
        if (id_bytes == 4)                                                                     \
            rows_launch<VEC_, int32_t>(blocks, st, param, grad, n_table_rows, dim, ids, n_ids, \
                                       claim, neg_lr, status);                                 \
        else                                                                                   \
            rows_launch<VEC_, int64_t>(blocks, st, param, grad, n_table_rows, dim, ids, n_ids, \
                                       claim, neg_lr, status);                                 \
    } while (0)
    if (vec == 4) DW_SGD_ROWS(4);
    else if (vec == 2) DW_SGD_ROWS(2);
    else DW_SGD_ROWS(1);
#undef DW_SGD_ROWS
    DW_LAUNCH_CHECK("dw_sgd_rows");
    const int64_t words = (n_table_rows + 31) / 32;
    int64_t cblocks = (words + 255) / 256;
    if (cblocks > 1024) cblocks = 1024;
    hipLaunchKernelGGL(k_clear_words, dim3((unsigned)cblocks), dim3(256), 0, st, claim, words);
    DW_LAUNCH_CHECK("dw_sgd_rows (clear)");
    return DW_OK;
}

}  // extern "C"
