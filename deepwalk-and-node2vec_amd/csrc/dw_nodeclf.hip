// Node classification on the device: one pass of a multinomial logistic regression over the
// rows table[ids[i]] (DESIGN.md "Device node classification").
//
// The reference's node-classification protocol (tools/graph_model_downstream_classification.py:
// 58-86) fits sklearn's LogisticRegression on a float64 copy of the embedding table. Here the
// loss, the gradient and the predictions of one evaluation are one gather pass: the fp32 rows are
// staged once per tile in LDS, widened exactly on use, and both products — the logits
// Z = X W^T and the gradient G += R^T X — run on v_mfma_f64_16x16x4_f64.
#include "dw_common.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int NC_THREADS = 256;      // 4 waves, one per SIMD: the unified 512-register file
constexpr int NC_MAX_BLOCKS = 256;   // one block per CU (its LDS tile leaves room for one)

// The shape of an instantiation. KT: class tiles of 16 (Kp = 16 KT). CT: gradient column tiles of
// 16 per wave, so the block covers DP = 64 CT columns. A block stages TS samples per trip; its
// four waves share them.
template <int KT, int CT>
struct NcShape {
    static constexpr int TS = CT <= 4 ? 64 : 32;   // samples per trip
    static constexpr int NS = TS / 16;             // sample tiles of 16 per trip
    static constexpr int P = 4 / NS;               // waves that share a sample tile's k range
    static constexpr int DP = CT * 64;             // padded row length
    static constexpr int CH = DP / 4;              // 16-B chunks per padded row (k steps of 4)
    // fp32 words per staged row; XS % 64 == 20 keeps the logit pass's operand reads (16 rows x
    // 4 columns per wave) on distinct banks and is a multiple of 4 for the 16-B stores
    static constexpr int XS = DP + 20;
    static constexpr int KP = KT * 16;
    static constexpr int RS = KP + 2;              // doubles per logit / residual row
    static constexpr int NPF = TS * CH / NC_THREADS;   // 16-B chunks a thread stages per trip
};

__host__ __device__ inline int nc_tile_samples(int32_t dim) { return dim <= 256 ? 64 : 32; }

__host__ __device__ inline int64_t nc_blocks(int64_t n, int32_t dim) {
    const int64_t ts = nc_tile_samples(dim);
    int64_t b = (n + ts - 1) / ts;
    if (b > NC_MAX_BLOCKS) b = NC_MAX_BLOCKS;
    return b < 1 ? 1 : b;
}

// Lane maps of v_mfma_f64_16x16x4_f64, lane l: A[row l & 15][k = l >> 4],
// B[k = l >> 4][col l & 15], D[row (l >> 4) + 4 reg][col l & 15], reg < 4.
//
// A trip: (1) the TS rows (zeros where the sample does not exist, its id or label is out of range
// or the column is past dim) go from registers, where the previous trip prefetched them, to LDS;
// (2) logits: sample tile `sub`, k range `part` per wave, A = X (sample x k), B = W^T (k x class),
// partial logits to LDS; (3) softmax: 256 / TS lanes per sample share its classes, every exp
// evaluated once, residuals R (0 in the padded classes and for dropped samples) overwrite the
// logits; (4) gradient: wave w owns columns [16 CT w, 16 CT (w + 1)), A = R^T (class x sample),
// B = X (sample x column), the TS samples are TS / 4 k steps.
//
// Reproducible bit for bit: block b walks trips b, b + grid, ... in order, the accumulators are
// private to a (wave, lane, register), the scalar sums are added in a fixed lane and wave order,
// the block writes one partial row and dw::k_logreg_finish adds the rows in block order.
template <int KT, int CT>
__global__ void __launch_bounds__(NC_THREADS)
    k_node_softmax(const float *__restrict__ table, int64_t V, int32_t d,
                   const int64_t *__restrict__ ids, const int32_t *__restrict__ labels, int64_t n,
                   int32_t K, const double *__restrict__ coef, double *__restrict__ partial,
                   int32_t *__restrict__ pred, int32_t *status, int32_t vec4) {
    typedef NcShape<KT, CT> S;
    constexpr int TS = S::TS, NS = S::NS, P = S::P, CH = S::CH, XS = S::XS, RS = S::RS;
    constexpr int NPF = S::NPF;
    constexpr int L = NC_THREADS / TS;   // lanes per sample in the softmax
    __shared__ __attribute__((aligned(16))) float s_x[TS * XS];
    __shared__ double s_z[64 * RS];   // [P][TS][RS] partial logits, then [TS][RS] residuals
    __shared__ int32_t s_y[TS];       // the sample's label, -1: contributes nothing
    __shared__ double s_sc[4][2];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int64_t ld = static_cast<int64_t>(d) + 1;   // coef row length
    const int64_t n_trips = (n + TS - 1) / TS;

    d4 acc[KT][CT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[kt][c] = d4{0.0, 0.0, 0.0, 0.0};
    double sum_loss = 0.0, sum_hit = 0.0;

    // A thread's chunks of a trip: chunk e = tid + 256 j is columns 4 (e % CH) ... + 3 of
    // sample e / CH.
    // The loads are unconditional, so that a thread's ids, then its rows, are all in flight
    // together: a chunk that contributes nothing reads row 0 / column 0 / sample n - 1 instead
    // (always in range) and is zeroed afterwards. rid: the chunk's row, -1 for such a chunk.
    f4 pf[NPF];
    int32_t rid[NPF];
    auto issue_ids = [&](int64_t trip, int j0, int j1) {
#pragma unroll
        for (int j = j0; j < j1; ++j) {
            const int e = tid + NC_THREADS * j;
            const int64_t i = trip * TS + e / CH;
            const int64_t ic = i < n ? i : n - 1;
            const int64_t id = ids[ic];
            const int32_t y = labels[ic];
            const bool ok = i < n && 4 * (e % CH) < d && id >= 0 && id < V && y >= 0 && y < K;
            rid[j] = ok ? static_cast<int32_t>(id) : -1;   // V < 2^31
        }
    };
    auto issue_rows = [&](int j0, int j1) {
#pragma unroll
        for (int j = j0; j < j1; ++j) {
            const int col = 4 * ((tid + NC_THREADS * j) % CH);
            const bool ok = rid[j] >= 0;
            const float *row = table + static_cast<int64_t>(ok ? rid[j] : 0) * d;
            f4 v;
            if (vec4) {   // d % 4 == 0 and a 16-B aligned table
                v = *reinterpret_cast<const f4 *>(row + (ok ? col : 0));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool in = ok && col + k < d;
                    const float x = row[in ? col + k : 0];
                    v[k] = in ? x : 0.f;
                }
            }
            pf[j] = ok ? v : f4{0.f, 0.f, 0.f, 0.f};
        }
    };

    // Sample tid of a trip (threads below TS): its label, -1 when its id or label is out of
    // range, -2 when the trip has no such sample.
    int32_t my = -2;
    auto meta = [&](int64_t trip) {
        my = -2;
        const int64_t i = trip * TS + tid;
        if (tid < TS && i < n) {
            const int64_t id = ids[i];
            const int32_t y = labels[i];
            my = (id >= 0 && id < V && y >= 0 && y < K) ? y : -1;
        }
    };

    // The logit pass of this wave: sample tile `sub` and k steps [st_begin, st_end) of the row's
    // CH, in chunks of UN steps (what the registers beside the accumulators hold). The P waves of
    // a tile split the (d + 3) / 4 steps that hold data at a multiple of two chunks, so a chunk
    // lies inside the padded row as a whole; the steps past d multiply zeros.
    constexpr int UN = KT * CT >= 32 ? 2 : KT >= 3 ? 4 : 8;
    static_assert(CH % (2 * UN) == 0, "chunk pairs tile the padded row");
    const int sub = wave % NS, part = wave / NS;
    const int steps = (d + 3) >> 2;
    const int per = ((steps + P - 1) / P + 2 * UN - 1) / (2 * UN) * (2 * UN);
    const int st_begin = part * per, st_end = min(min(CH, steps), (part + 1) * per);
    double wa[UN][KT], wb[UN][KT];
    auto load_w = [&](int st0, double (&w)[UN][KT]) {
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int kk = 4 * (st0 + u) + l4;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const int cls = kt * 16 + l15;
                w[u][kt] = (cls < K && kk < d) ? coef[cls * ld + kk] : 0.0;
            }
        }
    };
    // this lane's share of the intercept column: class tid % L + q L, slot tid / L
    double sb[S::KP / L];
#pragma unroll
    for (int q = 0; q < S::KP / L; ++q) sb[q] = 0.0;

    // The next trip's rows are fetched behind the current trip's arithmetic, except where the
    // accumulators leave no registers to hold them (Kp = 64 with dim > 256).
    constexpr bool AHEAD = KT * CT < 32;
    if (AHEAD) {
        issue_ids(blockIdx.x, 0, NPF);
        issue_rows(0, NPF);
    }
    meta(blockIdx.x);
    for (int64_t trip = blockIdx.x; trip < n_trips; trip += gridDim.x) {
        load_w(st_begin, wa);
        __syncthreads();   // the previous trip's gradient pass has read s_x and s_z
        constexpr int GRP = AHEAD ? NPF : 4;   // chunks in registers at a time
#pragma unroll
        for (int j0 = 0; j0 < NPF; j0 += GRP) {
            if (!AHEAD) {
                issue_ids(trip, j0, j0 + GRP);
                issue_rows(j0, j0 + GRP);
            }
#pragma unroll
            for (int j = j0; j < j0 + GRP; ++j) {
                const int e = tid + NC_THREADS * j;
                *reinterpret_cast<f4 *>(&s_x[(e / CH) * XS + 4 * (e % CH)]) = pf[j];
            }
        }
        if (tid < TS) {
            if (my == -1) {
                dw::status_or(status, DW_S_BAD_INDEX);
                if (pred) pred[trip * TS + tid] = -1;
            }
            s_y[tid] = my < 0 ? -1 : my;
        }
        __syncthreads();
        if (trip + gridDim.x < n_trips) {   // in flight behind the trip
            if (AHEAD) {
                issue_ids(trip + gridDim.x, 0, NPF);
                issue_rows(0, NPF);
            }
            meta(trip + gridDim.x);
        }

        // ---- logits: this wave's sample tile and share of the k steps. The coefficient
        // fragments come from global memory (L2) UN steps at a time, a chunk ahead of the MFMAs
        // that use them; the trip's first chunk was issued before the staging above.
        {
            d4 z[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) z[kt] = d4{0.0, 0.0, 0.0, 0.0};
            const float *xrow = &s_x[(sub * 16 + l15) * XS + l4];
            auto mfmas = [&](int st0, const double (&w)[UN][KT]) {
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const double a = static_cast<double>(xrow[4 * (st0 + u)]);
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
                        z[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, w[u][kt], z[kt], 0, 0, 0);
                }
            };
            for (int st0 = st_begin; st0 < st_end; st0 += 2 * UN) {
                load_w(st0 + UN, wb);
                mfmas(st0, wa);
                if (st0 + 2 * UN < st_end) load_w(st0 + 2 * UN, wa);
                mfmas(st0 + UN, wb);
            }
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    s_z[(part * TS + sub * 16 + l4 + 4 * r) * RS + kt * 16 + l15] = z[kt][r];
        }
        __syncthreads();

        // ---- softmax: L lanes per sample, lane j takes classes j, j + L, ...; a class's slot in
        // part 0 of s_z is read and written by its lane alone
        {
            const int s = tid / L, j = tid % L;
            const int32_t y = s_y[s];
            double *zrow = &s_z[s * RS];
            double m = -INFINITY, zy = 0.0;
            int32_t arg = 0x7fffffff;
            for (int c = j; c < K; c += L) {
                double zc = zrow[c];
#pragma unroll
                for (int p = 1; p < P; ++p) zc += s_z[(p * TS + s) * RS + c];
                zc += coef[c * ld + d];
                zrow[c] = zc;
                if (zc > m) {   // ascending c: the lowest class of a tie stays
                    m = zc;
                    arg = c;
                }
                if (c == y) zy = zc;
            }
#pragma unroll
            for (int off = 1; off < L; off <<= 1) {
                const double om = __shfl_xor(m, off, 64);
                const int32_t oa = __shfl_xor(arg, off, 64);
                if (om > m || (om == m && oa < arg)) {
                    m = om;
                    arg = oa;
                }
                zy += __shfl_xor(zy, off, 64);   // one lane's is non-zero
            }
            double se = 0.0;
            for (int c = j; c < K; c += L) {
                const double e = exp(zrow[c] - m);
                zrow[c] = e;
                se += e;
            }
#pragma unroll
            for (int off = 1; off < L; off <<= 1) se += __shfl_xor(se, off, 64);
            const double inv = 1.0 / se;
#pragma unroll
            for (int q = 0; q < S::KP / L; ++q) {
                const int c = j + q * L;
                double r = 0.0;
                if (y >= 0 && c < K) r = zrow[c] * inv - (c == y ? 1.0 : 0.0);
                zrow[c] = r;
                sb[q] += r;   // the intercept column: a plain sum, in trip order
            }
            if (j == 0 && y >= 0) {
                sum_loss += m + log(se) - zy;
                sum_hit += arg == y ? 1.0 : 0.0;
                if (pred) pred[trip * TS + s] = arg;
            }
        }
        __syncthreads();

        // ---- gradient: this wave's CT column tiles, all KT class tiles
#pragma unroll 4
        for (int q = 0; q < TS / 4; ++q) {
            const int smp = 4 * q + l4;
            double a[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) a[kt] = s_z[smp * RS + kt * 16 + l15];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const int col0 = (wave * CT + c) * 16;
                if (col0 < d) {   // uniform over the wave
                    const double b = static_cast<double>(s_x[smp * XS + col0 + l15]);
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
                        acc[kt][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kt], b, acc[kt][c], 0,
                                                                          0, 0);
                }
            }
        }
    }

    // ---- the block's partial row
    const int32_t len = K * (d + 1) + 2;
    double *dst = partial + static_cast<int64_t>(blockIdx.x) * len;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = (wave * CT + c) * 16 + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cls = kt * 16 + l4 + 4 * r;
                if (cls < K && col < d) dst[cls * ld + col] = acc[kt][c][r];
            }
        }
    }
    // the intercept column: the lanes' sums laid out as a residual tile, added in slot order
    __syncthreads();
#pragma unroll
    for (int q = 0; q < S::KP / L; ++q) s_z[(tid / L) * RS + tid % L + q * L] = sb[q];
    __syncthreads();
    if (tid < K) {
        double sum_b = 0.0;
        for (int s = 0; s < TS; ++s) sum_b += s_z[s * RS + tid];
        dst[tid * ld + d] = sum_b;
    }
    sum_loss = dw::wave_sum_d(sum_loss);
    sum_hit = dw::wave_sum_d(sum_hit);
    if (lane == 0) {
        s_sc[wave][0] = sum_loss;
        s_sc[wave][1] = sum_hit;
    }
    __syncthreads();
    if (tid < 2)
        dst[len - 2 + tid] = ((s_sc[0][tid] + s_sc[1][tid]) + s_sc[2][tid]) + s_sc[3][tid];
}

template <int KT, int CT>
void nc_launch(int64_t blocks, hipStream_t s, const float *table, int64_t V, int32_t d,
               const int64_t *ids, const int32_t *labels, int64_t n, int32_t K, const double *coef,
               double *partial, int32_t *pred, int32_t *status, int32_t vec4) {
    hipLaunchKernelGGL((k_node_softmax<KT, CT>), dim3((unsigned)blocks), dim3(NC_THREADS), 0, s,
                       table, V, d, ids, labels, n, K, coef, partial, pred, status, vec4);
}

template <int CT>
void nc_launch_kt(int kt, int64_t blocks, hipStream_t s, const float *table, int64_t V, int32_t d,
                  const int64_t *ids, const int32_t *labels, int64_t n, int32_t K,
                  const double *coef, double *partial, int32_t *pred, int32_t *status,
                  int32_t vec4) {
#define DW_NC(KT_)                                                                                 \
    nc_launch<KT_, CT>(blocks, s, table, V, d, ids, labels, n, K, coef, partial, pred, status, vec4)
    if (kt == 1) DW_NC(1);
    else if (kt == 2) DW_NC(2);
    else if (kt == 3) DW_NC(3);
    else DW_NC(4);
#undef DW_NC
}

bool nc_sizes_ok(int64_t n, int32_t dim, int32_t n_classes) {
    return n >= 0 && n <= INT64_MAX / 64 && dim >= 1 && dim <= 512 && n_classes >= 2 &&
           n_classes <= 64;
}

size_t nc_row_len(int32_t dim, int32_t n_classes) {
    return static_cast<size_t>(n_classes) * (dim + 1) + 2;
}

}  // namespace

extern "C" {

int dw_node_softmax_workspace_bytes(int64_t n, int32_t dim, int32_t n_classes, size_t *bytes) {
    DW_REQUIRE(nc_sizes_ok(n, dim, n_classes) && bytes,
               "dw_node_softmax_workspace_bytes: bad sizes (n >= 0, dim in [1, 512], n_classes in "
               "[2, 64]; got dim %d, n_classes %d)",
               dim, n_classes);
    *bytes = static_cast<size_t>(nc_blocks(n, dim)) * nc_row_len(dim, n_classes) * sizeof(double);
    return DW_OK;
}

int dw_node_softmax(const float *table, int64_t vocab_size, int32_t dim, const int64_t *ids,
                    const int32_t *labels, int64_t n, int32_t n_classes, const double *coef,
                    double *out, int32_t *pred, void *workspace, size_t workspace_bytes,
                    int32_t *status, void *stream) {
    DW_REQUIRE(nc_sizes_ok(n, dim, n_classes) && vocab_size >= 1 &&
                   vocab_size < (int64_t(1) << 31),
               "dw_node_softmax: bad sizes (vocab_size in [1, 2^31), dim in [1, 512], n_classes in "
               "[2, 64], n >= 0; got dim %d, n_classes %d, n %lld)",
               dim, n_classes, static_cast<long long>(n));
    if (n == 0) return DW_OK;
    DW_REQUIRE(table && ids && labels && coef && out && workspace,
               "dw_node_softmax: null pointer");
    const int64_t blocks = nc_blocks(n, dim);
    const size_t len = nc_row_len(dim, n_classes);
    const size_t need = static_cast<size_t>(blocks) * len * sizeof(double);
    DW_REQUIRE(workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
               "dw_node_softmax: workspace too small or misaligned (%zu < %zu bytes)",
               workspace_bytes, need);
    const int32_t vec4 = dim % 4 == 0 && reinterpret_cast<uintptr_t>(table) % 16 == 0;
    const int kt = (n_classes + 15) / 16;
    double *partial = static_cast<double *>(workspace);
    hipStream_t s = dw::as_stream(stream);
#define DW_NC(CT_)                                                                              \
    nc_launch_kt<CT_>(kt, blocks, s, table, vocab_size, dim, ids, labels, n, n_classes, coef,   \
                      partial, pred, status, vec4)
    if (dim <= 128) DW_NC(2);
    else if (dim <= 256) DW_NC(4);
    else DW_NC(8);
#undef DW_NC
    DW_LAUNCH_CHECK("dw_node_softmax");
    hipLaunchKernelGGL(dw::k_logreg_finish, dim3((unsigned)((len + 63) / 64)), dim3(64), 0, s,
                       partial, blocks, static_cast<int32_t>(len), out);
    DW_LAUNCH_CHECK("dw_node_softmax (finish)");
    return DW_OK;
}

}  // extern "C"
