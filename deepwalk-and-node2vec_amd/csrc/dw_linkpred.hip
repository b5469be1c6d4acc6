// Link prediction on the device: rank-sampled non-edges, edge features and a fused logistic
// regression pass over labelled node pairs (DESIGN.md "Device link prediction").
//
// The reference's link-prediction protocol (tools/graph_model_downstream_classification.py:
// 170-200, 241-299) draws a negative pair as a uniform node u and a uniform node v among the
// nodes not adjacent to u (u itself allowed), by a set difference per draw; builds
// operator(n1, n2) feature matrices (graph/edge_operators.py) and fits sklearn's logistic
// regression on them. Here the draw is one Philox call and one binary search of u's sorted row
// (the k-th non-neighbour by rank, no rejection), and the regression's loss, gradient and
// accuracy over n pairs are one gather pass that never stores a feature. For held-out link
// prediction the same pass writes each pair's score instead (dw_edge_scores),
// and dw_roc_auc turns scores and labels into the exact integer Mann-Whitney count.
//
// Compiled with -ffp-contract=off (csrc/build.py): the fp32 operator expressions round exactly
// as written, so dw_edge_features equals numpy float32 bit for bit.
#include <rocprim/device/device_radix_sort.hpp>

#include "dw_common.h"
#include "dw_ingest.h"

namespace {

constexpr uint32_t TAG_LINKPRED = 0x4C500000u;  // 'LP'

// ---- dw_negative_edges -----------------------------------------------------------------------
// Sample i, g = offset + i: words (x, y) pick u = first_node + bounded64(Nn), words (z, w) the
// rank k = bounded64(Nn - deg u) among u's non-neighbours; with c u's sorted row, the k-th
// non-neighbour is first_node + k + j for the smallest j with c[j] - first_node - j > k (the
// count of non-neighbours below c[j] exceeds k), j = deg when there is none. Distinct neighbours
// make c[j] - j non-decreasing: a binary search, log2(deg) dependent loads.
template <bool PAIRED>
__global__ void __launch_bounds__(256)
    k_negative_edges(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col_sorted,
                     int64_t n_rows, int64_t first_node, int64_t n, uint32_t k0, uint32_t k1,
                     uint64_t offset, int64_t *__restrict__ pairs, int32_t *status) {
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    const uint64_t Nn = static_cast<uint64_t>(n_rows - first_node);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t g = offset + static_cast<uint64_t>(i);
        const dw::U4 r = dw::philox<10>(
            dw::U4{static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), 0u, TAG_LINKPRED},
            k0, k1);
        const int64_t u = first_node + static_cast<int64_t>(dw::bounded64(r.x, r.y, Nn));
        const int64_t a = row_ptr[u];
        const int64_t deg = row_ptr[u + 1] - a;
        const int64_t m = static_cast<int64_t>(Nn) - deg;
        int64_t v = u;
        if (m <= 0) {   // no non-neighbour (the host refuses such a graph): never loops
            dw::status_or(status, DW_S_BAD_CSR);
        } else {
            const int64_t k =
                static_cast<int64_t>(dw::bounded64(r.z, r.w, static_cast<uint64_t>(m)));
            const int32_t *c = col_sorted + a;
            int64_t lo = 0, hi = deg;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (static_cast<int64_t>(c[mid]) - first_node - mid > k)
                    hi = mid;
                else
                    lo = mid + 1;
            }
            v = first_node + k + lo;
        }
        if (PAIRED) {
            *reinterpret_cast<ll2 *>(pairs + 2 * i) = ll2{u, v};
        } else {
            pairs[2 * i] = u;
            pairs[2 * i + 1] = v;
        }
    }
}

// ---- the edge operators (graph/edge_operators.py), fp32, in exactly this operation order -----
__device__ __forceinline__ float edge_op(int32_t op, float a, float b) {
    switch (op) {
        case 0: return (a + b) * 0.5f;   // average
        case 1: return a * b;            // hadamard
        case 2: return fabsf(a - b);     // weighted_l1
        default: {                       // weighted_l2
            const float t = a - b;
            return t * t;
        }
    }
}

template <int VEC>
struct Row;
template <>
struct Row<4> {
    typedef float type __attribute__((ext_vector_type(4)));
};
template <>
struct Row<1> {
    typedef float type;
};

__device__ __forceinline__ float elem(const float &v, int) { return v; }
__device__ __forceinline__ float elem(const Row<4>::type &v, int k) { return v[k]; }

// ---- dw_edge_features ------------------------------------------------------------------------
// One lane per VEC elements of one output row (VEC = 4: 16-B loads and stores).
template <int VEC>
__global__ void __launch_bounds__(256)
    k_edge_features(const float *__restrict__ table, int64_t V, int32_t d, int32_t op,
                    const int64_t *__restrict__ pairs, int64_t n, float *__restrict__ out,
                    int32_t *status) {
    typedef typename Row<VEC>::type vec_t;
    const int64_t chunks = d / VEC;
    const int64_t total = n * chunks;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / chunks;
        const int64_t c = i - row * chunks;
        const int64_t p0 = pairs[2 * row], p1 = pairs[2 * row + 1];
        const bool ok = p0 >= 0 && p0 < V && p1 >= 0 && p1 < V;
        float x[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) x[k] = 0.f;
        if (ok) {
            const vec_t a = *reinterpret_cast<const vec_t *>(table + p0 * d + c * VEC);
            const vec_t b = *reinterpret_cast<const vec_t *>(table + p1 * d + c * VEC);
#pragma unroll
            for (int k = 0; k < VEC; ++k) x[k] = edge_op(op, elem(a, k), elem(b, k));
        } else if (c == 0) {
            dw::status_or(status, DW_S_BAD_INDEX);
        }
        vec_t o;
        if constexpr (VEC == 4) {
            o = vec_t{x[0], x[1], x[2], x[3]};
        } else {
            o = x[0];
        }
        *reinterpret_cast<vec_t *>(out + row * d + c * VEC) = o;
    }
}

// ---- dw_edge_logreg --------------------------------------------------------------------------
// A group of G lanes owns a sample: lane gl holds the elements (c * G + gl) * VEC + k, c < C,
// k < VEC of both rows in registers (16 B per lane and load when VEC = 4). A group takes U = 4
// samples per trip, so 8 rows are in flight per group before the first is used (16 with the
// next trip's, see PIPE). Everything past
// the fp32 operator is float64: the dot product (per-lane partial, then a butterfly over the
// group), loss and residual, and the per-lane gradient sums.
// exp / log1p are evaluated once per sample, not once per lane: lane u < U of the group takes
// sample u's z and hands the residual back by a shuffle.
//
// Reproducible bit for bit: the grid is a function of (n, G), every group walks a fixed set of
// samples in a fixed order, the block adds its groups' sums in group order in LDS, writes one
// partial row to the workspace, and k_logreg_finish adds the partial rows in block order. No
// float atomics.
constexpr int LR_U = 4;
constexpr int LR_MAX_BLOCKS = 1024;   // 256 CUs x 4 blocks of 4 waves (16 waves per CU)

__host__ __device__ inline int64_t logreg_blocks(int64_t n, int groups_per_block) {
    const int64_t per = static_cast<int64_t>(groups_per_block) * LR_U;
    int64_t b = (n + per - 1) / per;
    if (b > LR_MAX_BLOCKS) b = LR_MAX_BLOCKS;
    return b < 1 ? 1 : b;
}

// SCORES (dw_edge_scores): the same gather, operator and float64 dot product, and then z itself
// goes to partial[sample] — no label, loss, gradient or sum across samples; a null coef means
// unit weights and a zero intercept.
template <int VEC, int G, int C, bool SCORES = false>
__global__ void __launch_bounds__(256)
    k_edge_logreg(const float *__restrict__ table, int64_t V, int32_t d, int32_t op,
                  const int64_t *__restrict__ pairs, const uint8_t *__restrict__ labels,
                  int64_t n, const double *__restrict__ coef, double *__restrict__ partial,
                  int32_t *status) {
    typedef typename Row<VEC>::type vec_t;
    constexpr int U = LR_U;
    static_assert(U == 4, "the joint reduction below trades halves over two lane bits");
    constexpr int GPW = 64 / G;     // groups per wave
    constexpr int GPB = 4 * GPW;    // groups per block
    constexpr int E = VEC * C;      // elements per lane
    __shared__ double s_sum[512];
    __shared__ double s_sc[4][3];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int gl = lane & (G - 1);
    const int gbase = lane & ~(G - 1);
    const int grp = wave * GPW + lane / G;

    double w[E];
    bool live[C];   // VEC = 4: d % 4 == 0, a chunk is inside the row or past it as a whole
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int e0 = (c * G + gl) * VEC;
        live[c] = e0 < d;
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            w[c * VEC + k] = live[c] ? (SCORES && !coef ? 1.0 : coef[e0 + k]) : 0.0;
    }
    const double b0 = SCORES && !coef ? 0.0 : coef[d];

    double acc[E];
#pragma unroll
    for (int j = 0; j < E; ++j) acc[j] = 0.0;
    double sum_r = 0.0, sum_loss = 0.0, sum_hit = 0.0;

    // A trip's ids, labels and flags: bit u = sample u exists, bit 8 + u = its ids are in range,
    // bit 16 + u = its label. They are loaded a trip ahead of their rows, so a trip never waits
    // for two memory latencies in a row.
    struct Ids {
        int32_t a[U], b[U];
        uint32_t flags;
    };
    auto load_ids = [&](int64_t base) {
        Ids t;
        t.flags = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t s = base + u;
            t.a[u] = t.b[u] = 0;
            if (s < n) {
                const int64_t p0 = pairs[2 * s], p1 = pairs[2 * s + 1];
                const bool ok = p0 >= 0 && p0 < V && p1 >= 0 && p1 < V;
                t.flags |= (1u << u) | (ok ? 1u << (8 + u) : 0u) |
                           (!SCORES && labels[s] != 0 ? 1u << (16 + u) : 0u);
                if (ok) {   // V < 2^31
                    t.a[u] = static_cast<int32_t>(p0);
                    t.b[u] = static_cast<int32_t>(p1);
                } else if (gl == 0) {
                    dw::status_or(status, DW_S_BAD_INDEX);
                }
            }
        }
        return t;
    };

    // The rows of a trip (zeros where the sample does not exist or an id is out of range: every
    // operator maps (0, 0) to 0).
    auto issue = [&](const Ids &t, vec_t (&a)[U][C], vec_t (&b)[U][C]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool have = ((t.flags >> u) & (t.flags >> (8 + u)) & 1u) != 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                a[u][c] = vec_t(0.f);
                b[u][c] = vec_t(0.f);
                if (have && live[c]) {
                    const int e0 = (c * G + gl) * VEC;
                    a[u][c] = *reinterpret_cast<const vec_t *>(
                        table + static_cast<int64_t>(t.a[u]) * d + e0);
                    b[u][c] = *reinterpret_cast<const vec_t *>(
                        table + static_cast<int64_t>(t.b[u]) * d + e0);
                }
            }
        }
    };

    // PIPE (rows of up to 16 B per lane): the rows of trip k + 1 are issued before trip k is
    // computed, the ids of trip k + 2 behind them — a trip costs the longer of its arithmetic
    // and one memory latency, at 16 rows in flight per group. Wider rows keep one trip in flight.
    constexpr bool PIPE = E <= 4;
    const int64_t step = (int64_t)gridDim.x * GPB * U;
    const int64_t first = ((int64_t)blockIdx.x * GPB + grp) * U;
    Ids nxt = load_ids(first);
    vec_t na[U][C], nb[U][C];
    uint32_t nflags = 0u;
    if constexpr (PIPE) {
        issue(nxt, na, nb);
        nflags = nxt.flags;
        nxt = load_ids(first + step);
    }
    for (int64_t base = first; base < n; base += step) {
        vec_t ra[U][C], rb[U][C];
        uint32_t flags;
        if constexpr (PIPE) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    ra[u][c] = na[u][c];
                    rb[u][c] = nb[u][c];
                }
            }
            flags = nflags;
            issue(nxt, na, nb);
            nflags = nxt.flags;
            nxt = load_ids(base + 2 * step);
        } else {
            issue(nxt, ra, rb);
            flags = nxt.flags;
            nxt = load_ids(base + step);
        }
        float x[U][E];
        double part[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            part[u] = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float f = edge_op(op, elem(ra[u][c], k), elem(rb[u][c], k));
                    x[u][c * VEC + k] = f;
                    part[u] = __builtin_fma(w[c * VEC + k], static_cast<double>(f), part[u]);
                }
            }
        }
        // The four dot products reduced together: lanes a bit apart trade the halves they do not
        // keep (xor 1: samples by bit 0, xor 2: by bit 1), then a butterfly over the rest of the
        // group — 3 + log2(G / 4) exchanges instead of 4 log2(G), and lane gl ends with the sum
        // of sample gl & 3 (the same bits in every such lane of the group), the one it evaluates.
        const int mine = gl & (U - 1);
        const bool b0s = (gl & 1) != 0, b1s = (gl & 2) != 0;
        const double k0 = (b0s ? part[1] : part[0]) + __shfl_xor(b0s ? part[0] : part[1], 1, 64);
        const double k1 = (b0s ? part[3] : part[2]) + __shfl_xor(b0s ? part[2] : part[3], 1, 64);
        double zs = (b1s ? k1 : k0) + __shfl_xor(b1s ? k0 : k1, 2, 64);
#pragma unroll
        for (int off = 4; off < G; off <<= 1) zs += __shfl_xor(zs, off, 64);
        zs += b0;
        const bool vs = ((flags >> mine) & 1u) != 0;
        if constexpr (SCORES) {
            if (gl < U && vs) partial[base + mine] = zs;
            continue;
        }
        const double ys = ((flags >> (16 + mine)) & 1u) ? 1.0 : 0.0;
        const double e = exp(-fabs(zs));
        const double inv = 1.0 / (1.0 + e);
        const double sig = zs >= 0.0 ? inv : e * inv;   // 1 / (1 + exp(-z)), finite for every z
        const double res = vs ? sig - ys : 0.0;
        if (gl < U && vs) {
            sum_r += res;
            sum_loss += log1p(e) + fmax(zs, 0.0) - ys * zs;
            sum_hit += ((zs > 0.0) == (ys != 0.0)) ? 1.0 : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double r = __shfl(res, gbase + u, 64);
#pragma unroll
            for (int j = 0; j < E; ++j)
                acc[j] = __builtin_fma(r, static_cast<double>(x[u][j]), acc[j]);
        }
    }

    if constexpr (SCORES) return;
    // the block's sums: groups in group order, then the waves' scalars in wave order
    for (int i = threadIdx.x; i < 512; i += 256) s_sum[i] = 0.0;
    __syncthreads();
    for (int q = 0; q < GPB; ++q) {
        if (grp == q) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const int el = (c * G + gl) * VEC + k;
                    if (el < d) s_sum[el] += acc[c * VEC + k];
                }
            }
        }
        __syncthreads();
    }
    sum_r = dw::wave_sum_d(sum_r);
    sum_loss = dw::wave_sum_d(sum_loss);
    sum_hit = dw::wave_sum_d(sum_hit);
    if (lane == 0) {
        s_sc[wave][0] = sum_r;
        s_sc[wave][1] = sum_loss;
        s_sc[wave][2] = sum_hit;
    }
    __syncthreads();
    double *dst = partial + (int64_t)blockIdx.x * (d + 3);
    for (int i = threadIdx.x; i < d; i += 256) dst[i] = s_sum[i];
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        dst[d + k] = ((s_sc[0][k] + s_sc[1][k]) + s_sc[2][k]) + s_sc[3][k];
    }
}

template <int VEC, int G, int C, bool SCORES>
void logreg_launch(int64_t blocks, hipStream_t s, const float *table, int64_t V, int32_t d,
                   int32_t op, const int64_t *pairs, const uint8_t *labels, int64_t n,
                   const double *coef, double *partial, int32_t *status) {
    hipLaunchKernelGGL((k_edge_logreg<VEC, G, C, SCORES>), dim3((unsigned)blocks), dim3(256), 0, s,
                       table, V, d, op, pairs, labels, n, coef, partial, status);
}

// The launch shape of (d, 16-B rows or not): lanes per sample G, chunks per lane C.
struct LogregShape {
    int vec, G, C;
};

LogregShape logreg_shape(int32_t d, bool vec4) {
    if (vec4) {
        const int lanes = d / 4;
        if (lanes <= 16) return {4, 16, 1};
        if (lanes <= 32) return {4, 32, 1};
        if (lanes <= 64) return {4, 64, 1};
        return {4, 64, 2};
    }
    const int c = (d + 63) / 64;
    return {1, 64, c <= 1 ? 1 : c <= 2 ? 2 : c <= 4 ? 4 : 8};
}

// One launch of the (d, alignment) shape's instantiation: the logreg pass or the scores pass.
template <bool SCORES>
void logreg_dispatch(const LogregShape &sh, int64_t blocks, hipStream_t s, const float *table,
                     int64_t V, int32_t d, int32_t op, const int64_t *pairs,
                     const uint8_t *labels, int64_t n, const double *coef, double *partial,
                     int32_t *status) {
#define DW_LR(V_, G_, C_)                                                                       \
    logreg_launch<V_, G_, C_, SCORES>(blocks, s, table, V, d, op, pairs, labels, n, coef,       \
                                      partial, status)
    if (sh.vec == 4) {
        if (sh.G == 16) DW_LR(4, 16, 1);
        else if (sh.G == 32) DW_LR(4, 32, 1);
        else if (sh.C == 1) DW_LR(4, 64, 1);
        else DW_LR(4, 64, 2);
    } else {
        if (sh.C == 1) DW_LR(1, 64, 1);
        else if (sh.C == 2) DW_LR(1, 64, 2);
        else if (sh.C == 4) DW_LR(1, 64, 4);
        else DW_LR(1, 64, 8);
    }
#undef DW_LR
}

bool sizes_ok(int64_t vocab_size, int32_t dim, int32_t op, int64_t n) {
    return vocab_size >= 1 && vocab_size < (int64_t(1) << 31) && dim >= 1 && dim <= 512 &&
           op >= 0 && op <= 3 && n >= 0;
}

// ---- dw_roc_auc ------------------------------------------------------------------------------
// The tie-aware Mann-Whitney count as an integer: U2 = sum over positives i of
// 2 #{negatives j: s_j < s_i} + #{negatives j: s_j = s_i}. A score becomes a uint64 key of the
// same order (-0.0 and +0.0 tie); the negatives' keys are sorted with every positive's slot
// holding AUC_PAD, which is above every key of a number (+inf is 0xFFF0...0), so the sorted array
// is the n_neg negatives followed by padding and the sort's length does not depend on a count
// the host would have to read first. A positive's lower bound lb and upper bound ub in it are
// the two counts: its term is lb + ub. Integer sums: one 64-bit atomic per block and counter,
// the same result in any order.
constexpr uint64_t AUC_PAD = ~uint64_t(0);
constexpr int AUC_MAX_BLOCKS = 2048;   // 256 CUs x 8 blocks; the loop strides over the rest

__device__ __forceinline__ uint64_t score_key(double s) {
    const uint64_t b = static_cast<uint64_t>(__double_as_longlong(s == 0.0 ? 0.0 : s));
    return (b >> 63) ? ~b : b | (uint64_t(1) << 63);
}

__global__ void __launch_bounds__(256)
    k_auc_keys(const double *__restrict__ scores, const uint8_t *__restrict__ labels, int64_t n,
               uint64_t *__restrict__ keys, int32_t *status) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        const double s = scores[i];
        if (s != s) dw::status_or(status, DW_S_NAN_SCORE);
        keys[i] = labels[i] != 0 ? AUC_PAD : score_key(s);
    }
}

__global__ void __launch_bounds__(256)
    k_auc_terms(const double *__restrict__ scores, const uint8_t *__restrict__ labels, int64_t n,
                const uint64_t *__restrict__ sorted, unsigned long long *out) {
    __shared__ unsigned long long s_part[4][3];
    unsigned long long u2 = 0, n_pos = 0, n_neg = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        if (labels[i] == 0) {
            ++n_neg;
            continue;
        }
        ++n_pos;
        const uint64_t k = score_key(scores[i]);
        int64_t lo = 0, hi = n;   // lb: the first index whose key is >= k
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (sorted[mid] < k)
                lo = mid + 1;
            else
                hi = mid;
        }
        const int64_t lb = lo;
        hi = n;                   // ub: the first index whose key is > k
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (sorted[mid] <= k)
                lo = mid + 1;
            else
                hi = mid;
        }
        u2 += static_cast<unsigned long long>(lb + lo);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        u2 += __shfl_xor(u2, off, 64);
        n_pos += __shfl_xor(n_pos, off, 64);
        n_neg += __shfl_xor(n_neg, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_part[wave][0] = u2;
        s_part[wave][1] = n_pos;
        s_part[wave][2] = n_neg;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        const unsigned long long t = s_part[0][k] + s_part[1][k] + s_part[2][k] + s_part[3][k];
        if (t) atomicAdd(out + k, t);
    }
}

struct AucBufs {
    uint64_t *keys0, *keys1;
    void *tmp;
    size_t tmp_bytes;
};

int plan_auc(dw::Arena &a, int64_t n, AucBufs *p) {
    const size_t m = static_cast<size_t>(n > 0 ? n : 1);
    rocprim::double_buffer<uint64_t> kb(nullptr, nullptr);
    p->tmp_bytes = 0;
    DW_HIP_OK(rocprim::radix_sort_keys(nullptr, p->tmp_bytes, kb, m, 0, 64),
              "dw_roc_auc: sort plan");
    p->keys0 = a.take<uint64_t>(m);
    p->keys1 = a.take<uint64_t>(m);
    p->tmp = a.take<char>(p->tmp_bytes);
    return DW_OK;
}

}  // namespace

extern "C" {

int dw_negative_edges(const int64_t *row_ptr, const int32_t *col_sorted, int64_t n_rows,
                      int64_t first_node, int64_t n, uint64_t seed, uint64_t offset,
                      int64_t *pairs, int32_t *status, void *stream) {
    DW_REQUIRE(n_rows >= 1 && n_rows < (int64_t(1) << 31),
               "dw_negative_edges: n_rows must be in [1, 2^31)");
    DW_REQUIRE(first_node >= 0 && first_node < n_rows,
               "dw_negative_edges: first_node must be in [0, n_rows)");
    DW_REQUIRE(n >= 0 && n <= INT64_MAX / 2, "dw_negative_edges: bad n");
    if (n == 0) return DW_OK;
    DW_REQUIRE(row_ptr && col_sorted && pairs, "dw_negative_edges: null pointer");
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;   // 256 CUs x 8 blocks; the loop strides over the rest
    const bool paired = reinterpret_cast<uintptr_t>(pairs) % 16 == 0;
    const auto kernel = paired ? k_negative_edges<true> : k_negative_edges<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, dw::as_stream(stream),
                       row_ptr, col_sorted, n_rows, first_node, n, static_cast<uint32_t>(seed),
                       static_cast<uint32_t>(seed >> 32), offset, pairs, status);
    DW_LAUNCH_CHECK("dw_negative_edges");
    return DW_OK;
}

int dw_edge_features(const float *table, int64_t vocab_size, int32_t dim, int32_t op,
                     const int64_t *pairs, int64_t n, float *out, int32_t *status,
                     void *stream) {
    DW_REQUIRE(sizes_ok(vocab_size, dim, op, n),
               "dw_edge_features: bad sizes (vocab_size in [1, 2^31), dim in [1, 512], op in "
               "[0, 3], n >= 0; got dim %d, op %d, n %lld)",
               dim, op, static_cast<long long>(n));
    DW_REQUIRE(n <= INT64_MAX / 512, "dw_edge_features: n too large");
    if (n == 0) return DW_OK;
    DW_REQUIRE(table && pairs && out, "dw_edge_features: null pointer");
    const bool vec4 = dim % 4 == 0 && reinterpret_cast<uintptr_t>(table) % 16 == 0 &&
                      reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const int64_t total = n * (vec4 ? dim / 4 : dim);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const auto kernel = vec4 ? k_edge_features<4> : k_edge_features<1>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, dw::as_stream(stream), table,
                       vocab_size, dim, op, pairs, n, out, status);
    DW_LAUNCH_CHECK("dw_edge_features");
    return DW_OK;
}

int dw_edge_logreg_workspace_bytes(int64_t n, int32_t dim, size_t *bytes) {
    DW_REQUIRE(n >= 0 && dim >= 1 && dim <= 512 && bytes,
               "dw_edge_logreg_workspace_bytes: bad sizes (n >= 0, dim in [1, 512])");
    // the scalar-row shape has the fewest groups per block, so the most blocks
    *bytes = static_cast<size_t>(logreg_blocks(n, 4)) * (dim + 3) * sizeof(double);
    return DW_OK;
}

int dw_edge_logreg(const float *table, int64_t vocab_size, int32_t dim, int32_t op,
                   const int64_t *pairs, const uint8_t *labels, int64_t n, const double *coef,
                   double *out, void *workspace, size_t workspace_bytes, int32_t *status,
                   void *stream) {
    DW_REQUIRE(sizes_ok(vocab_size, dim, op, n),
               "dw_edge_logreg: bad sizes (vocab_size in [1, 2^31), dim in [1, 512], op in "
               "[0, 3], n >= 0; got dim %d, op %d, n %lld)",
               dim, op, static_cast<long long>(n));
    DW_REQUIRE(n <= INT64_MAX / 8, "dw_edge_logreg: n too large");
    if (n == 0) return DW_OK;
    DW_REQUIRE(table && pairs && labels && coef && out && workspace,
               "dw_edge_logreg: null pointer");
    const bool vec4 = dim % 4 == 0 && reinterpret_cast<uintptr_t>(table) % 16 == 0;
    const LogregShape sh = logreg_shape(dim, vec4);
    const int64_t blocks = logreg_blocks(n, 4 * (64 / sh.G));
    const size_t need = static_cast<size_t>(blocks) * (dim + 3) * sizeof(double);
    DW_REQUIRE(workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
               "dw_edge_logreg: workspace too small or misaligned (%zu < %zu bytes)",
               workspace_bytes, need);
    double *partial = static_cast<double *>(workspace);
    hipStream_t s = dw::as_stream(stream);
    logreg_dispatch<false>(sh, blocks, s, table, vocab_size, dim, op, pairs, labels, n, coef, partial,
                           status);
    DW_LAUNCH_CHECK("dw_edge_logreg");
    const int32_t len = dim + 3;
    hipLaunchKernelGGL(dw::k_logreg_finish, dim3((unsigned)((len + 63) / 64)), dim3(64), 0, s, partial,
                       blocks, len, out);
    DW_LAUNCH_CHECK("dw_edge_logreg (finish)");
    return DW_OK;
}

int dw_edge_scores(const float *table, int64_t vocab_size, int32_t dim, int32_t op,
                   const int64_t *pairs, int64_t n, const double *coef, double *z_out,
                   int32_t *status, void *stream) {
    DW_REQUIRE(sizes_ok(vocab_size, dim, op, n),
               "dw_edge_scores: bad sizes (vocab_size in [1, 2^31), dim in [1, 512], op in "
               "[0, 3], n >= 0; got dim %d, op %d, n %lld)",
               dim, op, static_cast<long long>(n));
    DW_REQUIRE(n <= INT64_MAX / 8, "dw_edge_scores: n too large");
    if (n == 0) return DW_OK;
    DW_REQUIRE(table && pairs && z_out, "dw_edge_scores: null pointer");
    const bool vec4 = dim % 4 == 0 && reinterpret_cast<uintptr_t>(table) % 16 == 0;
    const LogregShape sh = logreg_shape(dim, vec4);
    const int64_t blocks = logreg_blocks(n, 4 * (64 / sh.G));
    logreg_dispatch<true>(sh, blocks, dw::as_stream(stream), table, vocab_size, dim, op, pairs,
                          nullptr, n, coef, z_out, status);
    DW_LAUNCH_CHECK("dw_edge_scores");
    return DW_OK;
}

int dw_roc_auc_workspace_bytes(int64_t n, size_t *bytes) {
    DW_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && bytes,
               "dw_roc_auc_workspace_bytes: n must be in [0, 2^31)");
    dw::Arena a{nullptr};
    AucBufs p;
    const int rc = plan_auc(a, n, &p);
    if (rc != DW_OK) return rc;
    *bytes = a.off;
    return DW_OK;
}

int dw_roc_auc(const double *scores, const uint8_t *labels, int64_t n, int64_t *out,
               int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    DW_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "dw_roc_auc: n must be in [0, 2^31)");
    DW_REQUIRE(out && status, "dw_roc_auc: null pointer");
    hipStream_t st = dw::as_stream(stream);
    DW_HIP_OK(hipMemsetAsync(out, 0, 3 * sizeof(int64_t), st), "dw_roc_auc: memset");
    if (n == 0) return DW_OK;
    DW_REQUIRE(scores && labels && workspace, "dw_roc_auc: null pointer");
    dw::Arena a{static_cast<char *>(workspace)};
    AucBufs p;
    const int rc = plan_auc(a, n, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off && reinterpret_cast<uintptr_t>(workspace) % 256 == 0,
               "dw_roc_auc: workspace too small or misaligned (%zu < %zu bytes)",
               workspace_bytes, a.off);
    int64_t blocks = (n + 255) / 256;
    if (blocks > AUC_MAX_BLOCKS) blocks = AUC_MAX_BLOCKS;
    hipLaunchKernelGGL(k_auc_keys, dim3((unsigned)blocks), dim3(256), 0, st, scores, labels, n,
                       p.keys0, status);
    DW_LAUNCH_CHECK("dw_roc_auc/keys");
    rocprim::double_buffer<uint64_t> kb(p.keys0, p.keys1);
    size_t tmp_bytes = p.tmp_bytes;
    DW_HIP_OK(rocprim::radix_sort_keys(p.tmp, tmp_bytes, kb, static_cast<size_t>(n), 0, 64, st),
              "dw_roc_auc: sort");
    hipLaunchKernelGGL(k_auc_terms, dim3((unsigned)blocks), dim3(256), 0, st, scores, labels, n,
                       kb.current(), reinterpret_cast<unsigned long long *>(out));
    DW_LAUNCH_CHECK("dw_roc_auc/terms");
    return DW_OK;
}

}  // extern "C"
