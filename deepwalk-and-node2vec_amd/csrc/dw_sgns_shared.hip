// Shared-negatives SGNS on gfx950: one walk per block, three small f32-MFMA products.
//
// A documented DEPARTURE from the reference: every centre of a walk sees
// the same S negatives (PyTorch-BigGraph / GraphVite / pWord2Vec style) instead of its own
// 2R x K. For walk w with centres i in [R, L-R):
//   A = w_in[walk[i]]                          (L-2R) x d   centre rows
//   B = [w_out[walk[0..L)]; w_out[ids[0..S)]]  (L+S) x d    the walk's own nodes, then the shared ids
//   X = A B^T                                  logits of every (centre, out row) pair
//   C = coefficient of X (dw::row_coef):       walk column j is a positive of centre i iff
//                                              0 < |j - i| <= R (else 0); every shared column is
//                                              a negative weighted lambda = 2R K / S
//   g_in[walk[i]] += C B,   g_out[B's ids] += C^T A
// so a walk reads (L-2R) + (L+S) rows and leaves as many float-atomic rows: no per-pair gathers,
// no records, no sort, no second pass, no workspace.
//
// Tiling (256 threads = 4 waves per block, blocks grid-strided over the walks):
//   1. X in 32x32 tiles on v_mfma_f32_32x32x2_f32, the tiles dealt round-robin to the waves and
//      kept in accumulator registers (at most 4 x 8 tiles: L-2R <= 128 padded, L+S <= 256);
//      A and B staged through LDS in 64-wide chunks of d (row stride 65: the operand reads walk
//      down the rows, lane l: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]).
//   2. Each lane turns its 16 logits per tile (C/D map: col = l & 31, row = (r & 3) + 8 (r >> 2)
//      + 4 (l >> 5)) into coefficients and writes them to the LDS tile C[i][j ^ (i & 31)] (the
//      staging buffer's space; the XOR keeps both the row-wise and the column-wise operand reads
//      of the two products below on 32 distinct banks).
//   3. C B (tiles of 32 centres x 32 elements) and C^T A (32 out rows x 32 elements), one
//      accumulator tile per job, jobs round-robin over the waves. C is the A operand from LDS;
//      the B operand (a table row's 32 consecutive elements per half-wave: 128-B pieces) comes
//      straight from global memory, where step 1 just left the rows in L2.
//   4. Each lane adds its 16 results to the gradient tables with float atomics: per table row
//      and element one atomic per occurrence of the row in the walk.
// Rows whose id is outside [0, V) set DW_S_BAD_INDEX and take no part (dw_sgns_walks's rule: a
// bad centre drops its terms, a bad out row drops its column); padded rows and columns are zero.
#include "dw_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr int NW = BLOCK / WAVE;
constexpr int KC = 64;               // elements of d staged per chunk
constexpr int RS = KC + 1;           // staged row stride (odd: conflict-free down the rows)
constexpr int KU = 8;                // gradient products: operand pairs loaded per batch
constexpr int MAXT_ALL = 8;          // logit tiles per wave at most: (128 / 32) * (256 / 32) / NW
constexpr int MAX_L = 128, MAX_S = 128;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct SharedArgs {
    const int32_t *walks;
    const int64_t *ids;
    int64_t n_walks;
    int32_t L, R, S, d;
    int32_t nc, ncp, nbp;    // centres per walk; centres and out rows padded to the 32-tile
    int64_t V;
    const float *w_in, *w_out;
    float *g_in, *g_out;
    float scale_pos, scale_neg;   // grad_scale, lambda * grad_scale
    double lambda;
    double *loss_acc;
    int32_t *status;
};

// row of accumulator register r of a 32x32 tile in lane l (the column is l & 31)
__device__ __forceinline__ int tile_row(int r, int lane) {
    return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

// MAXT: logit tiles per wave the instance holds in registers (16 accumulators each) — the
// launcher takes the smallest of 2, 4, 8 that covers the walk's tiles; up to 4 leave room for
// two blocks per CU.
template <int MAXT>
__global__ void __launch_bounds__(BLOCK, MAXT <= 4 ? 2 : 1) k_sgns_shared(SharedArgs a) {
    extern __shared__ float smem[];
    int32_t *cen_id = reinterpret_cast<int32_t *>(smem);   // [ncp]: table row or -1
    int32_t *out_id = cen_id + a.ncp;                      // [nbp]
    float *buf = smem + a.ncp + a.nbp;
    float *As = buf, *Bs = buf + a.ncp * RS;               // step 1: staged chunks
    float *coef = buf;                                     // steps 2-3: [ncp][nbp], swizzled

    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);   // the tile / job loops are scalar
    const int l31 = lane & 31, lh = lane >> 5;
    const int nct = a.ncp / 32, nbt = a.nbp / 32, ntiles = nct * nbt;
    const int nb = a.L + a.S;
    float acc_pos = 0.f, acc_neg = 0.f, acc_rec = 0.f, acc_prec = 0.f;

    for (int64_t w = blockIdx.x; w < a.n_walks; w += gridDim.x) {
        __syncthreads();   // the previous walk's ids and coefficients are no longer read
        const int32_t *walk = a.walks + w * a.L;
        const int64_t *sid = a.ids + w * a.S;
        for (int r = tid; r < a.ncp; r += BLOCK) {
            int32_t id = -1;
            if (r < a.nc) {
                const int32_t v = walk[a.R + r];
                if (v >= 0 && v < a.V) id = v;
            }
            cen_id[r] = id;
        }
        for (int r = tid; r < a.nbp; r += BLOCK) {
            int32_t id = -1;
            if (r < nb) {
                const int64_t v = r < a.L ? static_cast<int64_t>(walk[r]) : sid[r - a.L];
                if (v >= 0 && v < a.V)
                    id = static_cast<int32_t>(v);
                else
                    dw::status_or(a.status, DW_S_BAD_INDEX);
            }
            out_id[r] = id;
        }

        // ---- 1. X = A B^T, chunk by chunk of d ------------------------------------------------
        f32x16 x[MAXT];
#pragma unroll
        for (int t = 0; t < MAXT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) x[t][r] = 0.f;
        for (int c0 = 0; c0 < a.d; c0 += KC) {
            __syncthreads();   // ids written / the previous chunk's operand reads done
            for (int q = tid; q < (a.ncp + a.nbp) * (KC / 4); q += BLOCK) {
                const int r = q / (KC / 4), f = q - r * (KC / 4);
                const bool is_a = r < a.ncp;
                const int rr = is_a ? r : r - a.ncp;
                const int32_t id = is_a ? cen_id[rr] : out_id[rr];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (id >= 0)
                    v = *reinterpret_cast<const float4 *>((is_a ? a.w_in : a.w_out) +
                                                          static_cast<int64_t>(id) * a.d + c0 + 4 * f);
                float *dst = (is_a ? As : Bs) + rr * RS + 4 * f;
                dst[0] = v.x;
                dst[1] = v.y;
                dst[2] = v.z;
                dst[3] = v.w;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < MAXT; ++t) {
                const int T = wv + NW * t;
                if (T < ntiles) {   // wave-uniform: the MFMAs run with every lane
                    const int ti = T / nbt, tj = T - ti * nbt;
                    const float *ap = As + (ti * 32 + l31) * RS + lh;
                    const float *bp = Bs + (tj * 32 + l31) * RS + lh;
#pragma unroll 8
                    for (int k = 0; k < KC; k += 2)
                        x[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k], bp[k], x[t], 0, 0, 0);
                }
            }
        }
        __syncthreads();   // the staged rows are dead: their space becomes the coefficient tile

        // ---- 2. logits -> coefficients, loss sums ---------------------------------------------
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const int T = wv + NW * t;
            if (T < ntiles) {
                const int ti = T / nbt, tj = T - ti * nbt;
                const int col = tj * 32 + l31;
                const bool col_ok = col < nb && out_id[col] >= 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = ti * 32 + tile_row(r, lane);
                    float c = 0.f;
                    if (col_ok && row < a.nc && cen_id[row] >= 0) {
                        if (col >= a.L) {
                            c = dw::row_coef(x[t][r], false, a.scale_neg, acc_pos, acc_neg,
                                             acc_rec, acc_prec);
                        } else {
                            const int dl = col - (row + a.R);   // context offset of walk column
                            if (dl != 0 && dl >= -a.R && dl <= a.R)
                                c = dw::row_coef(x[t][r], true, a.scale_pos, acc_pos, acc_neg,
                                                 acc_rec, acc_prec);
                        }
                    }
                    coef[row * a.nbp + (col ^ (row & 31))] = c;
                }
            }
        }
        __syncthreads();

        // ---- 3./4. g_in += C B, g_out += C^T A ------------------------------------------------
        const int net = a.d / 32;
        const int n_ja = nct * net, n_jobs = n_ja + nbt * net;
        for (int job = wv; job < n_jobs; job += NW) {   // wave-uniform
            f32x16 g;
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = 0.f;
            const bool is_a = job < n_ja;
            const int jb = is_a ? job : job - n_ja;
            const int tr = jb / net, e = (jb - tr * net) * 32 + l31;
            // C B: 32 centres x 32 elements, summed over the out rows (C row-wise);
            // C^T A: 32 out rows x 32 elements, summed over the centres (C column-wise)
            const int32_t *row_ids = is_a ? cen_id : out_id, *k_ids = is_a ? out_id : cen_id;
            const float *tab = is_a ? a.w_out : a.w_in;
            float *gdst = is_a ? a.g_in : a.g_out;
            const int kn = is_a ? a.nbp : a.ncp, rc = tr * 32 + l31;
            for (int k0 = 0; k0 < kn; k0 += 2 * KU) {   // kn is a multiple of 32
                float av[KU], bv[KU];
#pragma unroll
                for (int u = 0; u < KU; ++u) {   // KU table loads in flight, then KU MFMAs
                    const int k = k0 + 2 * u + lh;
                    const int32_t id = k_ids[k];
                    bv[u] = id >= 0 ? tab[static_cast<int64_t>(id) * a.d + e] : 0.f;
                    av[u] = is_a ? coef[rc * a.nbp + (k ^ l31)] : coef[k * a.nbp + (rc ^ (k & 31))];
                }
#pragma unroll
                for (int u = 0; u < KU; ++u)
                    g = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], g, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int32_t id = row_ids[tr * 32 + tile_row(r, lane)];
                if (id >= 0 && g[r] != 0.f)
                    atomicAdd(gdst + static_cast<int64_t>(id) * a.d + e, g[r]);
            }
        }
    }

    // loss sums: one fp64 atomic per block and term (dw_sgns.hip flush_loss), the two negative
    // terms weighted lambda
    __shared__ float s_loss[NW][4];
    acc_pos = dw::wave_sum(acc_pos);
    acc_neg = dw::wave_sum(acc_neg);
    acc_rec = dw::wave_sum(acc_rec);
    acc_prec = dw::wave_sum(acc_prec);
    if (lane == 0) {
        s_loss[wv][0] = acc_pos;
        s_loss[wv][1] = acc_neg;
        s_loss[wv][2] = acc_rec;
        s_loss[wv][3] = acc_prec;
    }
    __syncthreads();
    if (a.loss_acc && tid < 4) {
        double t = 0.0;
        for (int q = 0; q < NW; ++q) t += s_loss[q][tid];
        if (tid & 1) t *= a.lambda;
        if (t != 0.0) atomicAdd(a.loss_acc + tid, t);
    }
}

constexpr int round32(int n) { return (n + 31) / 32 * 32; }

}  // namespace

extern "C" int dw_sgns_walks_shared(const int32_t *walks, int64_t n_walks, int32_t walk_length,
                                    int32_t context_radius, int32_t neg_samples, int32_t n_shared,
                                    int64_t vocab_size, int32_t dim, const float *w_in,
                                    const float *w_out, float *g_in, float *g_out,
                                    const int64_t *shared_ids, float grad_scale, double *loss_acc,
                                    int32_t *status, void *stream) {
    if (int rc = dw::require_window("dw_sgns_walks_shared", walk_length, context_radius)) return rc;
    DW_REQUIRE(walk_length <= MAX_L, "dw_sgns_walks_shared: walk_length %d > %d is not supported",
               walk_length, MAX_L);
    DW_REQUIRE(dim == 64 || dim == 128 || dim == 256,
               "dw_sgns_walks_shared: dim must be 64, 128 or 256 (got %d)", dim);
    DW_REQUIRE(n_shared >= 32 && n_shared <= MAX_S && n_shared % 32 == 0,
               "dw_sgns_walks_shared: n_shared must be a multiple of 32 in [32, %d] (got %d)",
               MAX_S, n_shared);
    DW_REQUIRE(vocab_size >= 1 && vocab_size < (1ll << 31),
               "dw_sgns_walks_shared: vocab_size must be in [1, 2^31)");
    DW_REQUIRE(neg_samples >= 0 && n_walks >= 0, "dw_sgns_walks_shared: bad sizes");
    DW_REQUIRE(walks && w_in && w_out && g_in && g_out && shared_ids && status,
               "dw_sgns_walks_shared: null pointer");
    DW_REQUIRE(((reinterpret_cast<uintptr_t>(w_in) | reinterpret_cast<uintptr_t>(w_out)) & 15) == 0,
               "dw_sgns_walks_shared: the tables must be 16-byte aligned");
    if (n_walks == 0) return DW_OK;

    SharedArgs a{};
    a.walks = walks;
    a.ids = shared_ids;
    a.n_walks = n_walks;
    a.L = walk_length;
    a.R = context_radius;
    a.S = n_shared;
    a.d = dim;
    a.nc = walk_length - 2 * context_radius;
    a.ncp = round32(a.nc);
    a.nbp = round32(walk_length + n_shared);
    a.V = vocab_size;
    a.w_in = w_in;
    a.w_out = w_out;
    a.g_in = g_in;
    a.g_out = g_out;
    a.lambda = 2.0 * context_radius * neg_samples / n_shared;
    a.scale_pos = grad_scale;
    a.scale_neg = static_cast<float>(a.lambda * grad_scale);
    a.loss_acc = loss_acc;
    a.status = status;

    const size_t stage = static_cast<size_t>(a.ncp + a.nbp) * RS;
    const size_t tile = static_cast<size_t>(a.ncp) * a.nbp;
    const size_t lds = (a.ncp + a.nbp + (stage > tile ? stage : tile)) * sizeof(float);
    const int per_wave = ((a.ncp / 32) * (a.nbp / 32) + NW - 1) / NW;
    static_assert(MAXT_ALL * NW * 32 * 32 >= round32(MAX_L) * round32(MAX_L + MAX_S), "tiles");
    void (*kernel)(SharedArgs) = per_wave <= 2   ? k_sgns_shared<2>
                                 : per_wave <= 4 ? k_sgns_shared<4>
                                                 : k_sgns_shared<MAXT_ALL>;
    if (lds > 64 * 1024) {   // at most 1.5 + 128 KiB of the CU's 160
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           static_cast<int>(lds));
        if (e != hipSuccess) {
            dw::set_error("dw_sgns_walks_shared: %zu bytes of LDS refused: %s", lds,
                          hipGetErrorString(e));
            return DW_E_HIP;
        }
    }
    int dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n_cu <= 0)
        n_cu = 256;
    int64_t blocks = n_walks;
    if (blocks > 4ll * n_cu) blocks = 4ll * n_cu;   // a couple of resident rounds (LDS-bound)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(BLOCK), lds,
                       dw::as_stream(stream), a);
    DW_LAUNCH_CHECK("dw_sgns_walks_shared");
    return DW_OK;
}
