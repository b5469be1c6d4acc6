// Node classification on the device: one pass of a multinomial logistic regression over the
// rows table[ids[i]] (DESIGN.md "Device node classification").
//
// The reference's node-classification protocol (tools/graph_model_downstream_classification.py:
// 58-86) fits sklearn's LogisticRegression on a float64 copy of the embedding table. Here the
// loss, the gradient and the predictions of one evaluation are one gather pass: the fp32 rows are
// staged once per tile in LDS, widened exactly on use, and both products — the logits
// Z = X W^T and the gradient G += R^T X — run on v_mfma_f64_16x16x4_f64.
//
// The same pass serves the multi-label task (one-vs-rest logistic regression, a departure: the
// reference has no multi-label task): only the per-sample stage between the two products
// differs, K sigmoids, a decision rule and per-class counts instead of one softmax. That stage,
// with the label and prediction types it implies, is the kernel's policy M.
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

// ---- the per-sample stage ----------------------------------------------------------------------
// A policy M names the label a sample carries (label_t in global memory, slot_t per staged
// sample in LDS), what a dropped sample's prediction is, the scalar sums (NSC) and the length of
// the tail that follows the gradient rows, and stage(): from the partial logits in s_z
// ([P][TS][RS]) to the residuals R in part 0 (0 in the padded classes and for dropped samples),
// the lane's share sb of the intercept column, the scalar sums sc and the predictions.

struct NcSoftmax {
    typedef int32_t label_t;
    typedef int32_t pred_t;
    typedef int32_t slot_t;   // the label; -1: contributes nothing, -2: no such sample
    static constexpr bool COUNTS = false;
    static constexpr int NSC = 2;   // loss, hits
    static constexpr pred_t DROPPED = -1;
    template <int TS>
    struct Shared {
        slot_t y[TS];
    };
    __host__ __device__ static constexpr int32_t tail(int32_t) { return NSC; }
    __device__ static slot_t none() { return -2; }
    __device__ static bool valid(int64_t id, label_t y, int64_t V, int32_t K) {
        return id >= 0 && id < V && y >= 0 && y < K;
    }
    __device__ static slot_t slot(int64_t id, label_t y, int64_t V, int32_t K) {
        return valid(id, y, V, K) ? y : -1;
    }
    __device__ static bool dropped(slot_t my) { return my == -1; }
    __device__ static slot_t staged(slot_t my) { return my < 0 ? -1 : my; }

    // softmax: L lanes per sample, lane j takes classes j, j + L, ...; a class's slot in part 0
    // of s_z is read and written by its lane alone
    template <class S, int NQ>
    __device__ __forceinline__ static void stage(double *s_z, Shared<S::TS> &sh,
                                                 const double *__restrict__ coef, int64_t ld,
                                                 int32_t d, int32_t K, int tid, double (&sb)[NQ],
                                                 double (&sc)[NSC], pred_t *__restrict__ pred,
                                                 int64_t i0) {
        constexpr int TS = S::TS, P = S::P, RS = S::RS, L = NC_THREADS / TS;
        const int s = tid / L, j = tid % L;
        const int32_t y = sh.y[s];
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
        for (int q = 0; q < NQ; ++q) {
            const int c = j + q * L;
            double r = 0.0;
            if (y >= 0 && c < K) r = zrow[c] * inv - (c == y ? 1.0 : 0.0);
            zrow[c] = r;
            sb[q] += r;   // the intercept column: a plain sum, in trip order
        }
        if (j == 0 && y >= 0) {
            sc[0] += m + log(se) - zy;
            sc[1] += arg == y ? 1.0 : 0.0;
            if (pred) pred[i0 + s] = arg;
        }
    }
};

// One-vs-rest: bit c of a sample's uint64 mask says it has label c; mask 0 is a sample of no
// label. RULE 0 predicts class c when z_c > 0, RULE 1 the popcount(mask) classes of the highest
// logits (ties to the lowest class). The tail is the loss, then tp[K], predicted[K], true[K].
struct NcMask {
    uint64_t mask;
    int32_t state;   // 1: a sample, -1: contributes nothing, -2: no such sample
};

template <int RULE>
struct NcOvr {
    typedef uint64_t label_t;
    typedef uint64_t pred_t;
    typedef NcMask slot_t;
    static constexpr bool COUNTS = true;
    static constexpr int NSC = 1;   // loss
    static constexpr pred_t DROPPED = 0;
    template <int TS>
    struct Shared {
        slot_t y[TS];
        // per class over the block's samples; 16 n bytes of ids and masks keep a block's share
        // of n far below 2^32
        uint32_t cnt[3][64];
    };
    __host__ __device__ static constexpr int32_t tail(int32_t K) { return NSC + 3 * K; }
    __device__ static slot_t none() { return NcMask{0, -2}; }
    __device__ static bool valid(int64_t id, label_t y, int64_t V, int32_t K) {
        return id >= 0 && id < V && (K >= 64 || (y >> K) == 0);   // no shift by 64
    }
    __device__ static slot_t slot(int64_t id, label_t y, int64_t V, int32_t K) {
        return NcMask{y, valid(id, y, V, K) ? 1 : -1};
    }
    __device__ static bool dropped(const slot_t &my) { return my.state == -1; }
    __device__ static slot_t staged(const slot_t &my) { return my; }

    // L lanes per sample, lane j takes classes j, j + L, ... First every lane completes its
    // classes' logits in part 0 of s_z. The rank of a class reads all K of them, the other
    // lanes' too: a barrier before it, and one after it, before the residuals overwrite them.
    template <class S, int NQ>
    __device__ __forceinline__ static void stage(double *s_z, Shared<S::TS> &sh,
                                                 const double *__restrict__ coef, int64_t ld,
                                                 int32_t d, int32_t K, int tid, double (&sb)[NQ],
                                                 double (&sc)[NSC], pred_t *__restrict__ pred,
                                                 int64_t i0) {
        constexpr int TS = S::TS, P = S::P, RS = S::RS, L = NC_THREADS / TS;
        const int s = tid / L, j = tid % L, lane = tid & 63;
        const bool ok = sh.y[s].state == 1;
        const uint64_t mask = sh.y[s].mask;
        double *zrow = &s_z[s * RS];
        for (int c = j; c < K; c += L) {
            double zc = zrow[c];
#pragma unroll
            for (int p = 1; p < P; ++p) zc += s_z[(p * TS + s) * RS + c];
            zrow[c] = zc + coef[c * ld + d];
        }
        uint32_t top = 0;   // bit q: class j + q L is among the sample's top k
        if constexpr (RULE == 1) {
            __syncthreads();
            const int k = __popcll(mask);
            // own classes ranked per sweep of the row: 4, or 2 where NQ is no multiple of 4 or
            // the accumulators leave no registers (Kp = 64 with dim > 256)
            constexpr int QB = NQ % 4 == 0 && S::KP * S::DP < 64 * 512 ? 4 : 2;
#pragma unroll
            for (int q0 = 0; q0 < NQ; q0 += QB) {
                if (q0 * L >= K) break;   // uniform over the block
                double zq[QB];
                int32_t rank[QB];
#pragma unroll
                for (int u = 0; u < QB; ++u) {
                    const int c = j + (q0 + u) * L;
                    zq[u] = c < K ? zrow[c] : 0.0;
                    rank[u] = 0;
                }
                for (int o = 0; o < K; ++o) {   // the padded classes enter no rank
                    const double zo = zrow[o];
#pragma unroll
                    for (int u = 0; u < QB; ++u)
                        rank[u] += zo > zq[u] || (zo == zq[u] && o < j + (q0 + u) * L);
                }
#pragma unroll
                for (int u = 0; u < QB; ++u)
                    if (j + (q0 + u) * L < K && rank[u] < k) top |= 1u << (q0 + u);
            }
            __syncthreads();
        }
        // the wave's lanes of this lane's classes; the first of them adds their count
        const uint64_t peers = (L == 4 ? 0x1111111111111111ull : 0x0101010101010101ull) << j;
        auto tally = [&](int which, int c, bool bit) {
            const uint64_t votes = __ballot(bit) & peers;
            if (lane < L && c < K) atomicAdd(&sh.cnt[which][c], (uint32_t)__popcll(votes));
        };
        double loss = 0.0;
        uint64_t pm = 0;
        // one class at a time, so that one exp and one log1p are live beside the accumulators;
        // uniform over the wave (the votes)
#pragma unroll 1
        for (int q = 0; q * L < K; ++q) {
            const int c = j + q * L;   // < 64
            const bool on = ok && c < K;
            const double z = on ? zrow[c] : 0.0;
            const bool t = on && ((mask >> c) & 1);
            const bool p = on && (RULE == 1 ? (top >> q) & 1 : z > 0.0);
            // sigmoid(|z|) and sigmoid(-|z|) from one exp(-|z|): finite for every z
            const double e = exp(-fabs(z));
            const double hi = 1.0 / (1.0 + e), lo = e * hi;
            if (on) {
                zrow[c] = t ? -(z >= 0.0 ? lo : hi) : (z >= 0.0 ? hi : lo);   // sigmoid(z) - y
                loss += (fmax(z, 0.0) - (t ? z : 0.0)) + log1p(e);
            }
            if (p) pm |= 1ull << c;
            tally(0, c, p && t);
            tally(1, c, p);
            tally(2, c, t);
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = j + q * L;
            const double r = ok && c < K ? zrow[c] : 0.0;
            zrow[c] = r;
            sb[q] += r;   // the intercept column: a plain sum, in trip order
        }
#pragma unroll
        for (int off = 1; off < L; off <<= 1) {
            loss += __shfl_xor(loss, off, 64);
            pm |= __shfl_xor(pm, off, 64);
        }
        if (j == 0 && ok) {
            sc[0] += loss;
            if (pred) pred[i0 + s] = pm;
        }
    }
};

// Lane maps of v_mfma_f64_16x16x4_f64, lane l: A[row l & 15][k = l >> 4],
// B[k = l >> 4][col l & 15], D[row (l >> 4) + 4 reg][col l & 15], reg < 4.
//
// A trip: (1) the TS rows (zeros where the sample does not exist, its id or label is out of range
// or the column is past dim) go from registers, where the previous trip prefetched them, to LDS;
// (2) logits: sample tile `sub`, k range `part` per wave, A = X (sample x k), B = W^T (k x class),
// partial logits to LDS; (3) M::stage: 256 / TS lanes per sample share its classes, every exp
// evaluated once, residuals R (0 in the padded classes and for dropped samples) overwrite the
// logits; (4) gradient: wave w owns columns [16 CT w, 16 CT (w + 1)), A = R^T (class x sample),
// B = X (sample x column), the TS samples are TS / 4 k steps.
//
// Reproducible bit for bit: block b walks trips b, b + grid, ... in order, the accumulators are
// private to a (wave, lane, register), the scalar sums are added in a fixed lane and wave order,
// the block writes one partial row and dw::k_logreg_finish adds the rows in block order.
template <int KT, int CT, class M>
__global__ void __launch_bounds__(NC_THREADS)
    k_node_logreg(const float *__restrict__ table, int64_t V, int32_t d,
                  const int64_t *__restrict__ ids, const typename M::label_t *__restrict__ labels,
                  int64_t n, int32_t K, const double *__restrict__ coef,
                  double *__restrict__ partial, typename M::pred_t *__restrict__ pred,
                  int32_t *status, int32_t vec4) {
    typedef NcShape<KT, CT> S;
    constexpr int TS = S::TS, NS = S::NS, P = S::P, CH = S::CH, XS = S::XS, RS = S::RS;
    constexpr int NPF = S::NPF;
    constexpr int L = NC_THREADS / TS;   // lanes per sample in the stage
    __shared__ __attribute__((aligned(16))) float s_x[TS * XS];
    __shared__ double s_z[64 * RS];   // [P][TS][RS] partial logits, then [TS][RS] residuals
    __shared__ typename M::template Shared<TS> sh;   // the samples' labels (and counts)
    __shared__ double s_sc[4][M::NSC];

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
    double sc[M::NSC];   // the scalar sums
#pragma unroll
    for (int t = 0; t < M::NSC; ++t) sc[t] = 0.0;
    if constexpr (M::COUNTS)   // the first trip's barriers come before the first count
        if (tid < 3 * 64) (&sh.cnt[0][0])[tid] = 0;

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
            const bool ok = i < n && 4 * (e % CH) < d && M::valid(id, labels[ic], V, K);
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

    // Sample tid of a trip (threads below TS): its label, marked when its id or label is out of
    // range or when the trip has no such sample.
    typename M::slot_t my = M::none();
    auto meta = [&](int64_t trip) {
        my = M::none();
        const int64_t i = trip * TS + tid;
        if (tid < TS && i < n) my = M::slot(ids[i], labels[i], V, K);
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
            if (M::dropped(my)) {
                dw::status_or(status, DW_S_BAD_INDEX);
                if (pred) pred[trip * TS + tid] = M::DROPPED;
            }
            sh.y[tid] = M::staged(my);
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

        // ---- the per-sample stage: partial logits to residuals
        M::template stage<S>(s_z, sh, coef, ld, d, K, tid, sb, sc, pred, trip * TS);
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
    const int32_t len = K * (d + 1) + M::tail(K);
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
        if constexpr (M::COUNTS) {
            for (int w = 0; w < 3; ++w)
                dst[K * ld + M::NSC + w * K + tid] = static_cast<double>(sh.cnt[w][tid]);
        }
    }
#pragma unroll
    for (int t = 0; t < M::NSC; ++t) {
        sc[t] = dw::wave_sum_d(sc[t]);
        if (lane == 0) s_sc[wave][t] = sc[t];
    }
    __syncthreads();
    if (tid < M::NSC)
        dst[K * ld + tid] = ((s_sc[0][tid] + s_sc[1][tid]) + s_sc[2][tid]) + s_sc[3][tid];
}

template <class M, int CT>
void nc_launch(int kt, int64_t blocks, hipStream_t s, const float *table, int64_t V, int32_t d,
               const int64_t *ids, const typename M::label_t *labels, int64_t n, int32_t K,
               const double *coef, double *partial, typename M::pred_t *pred, int32_t *status,
               int32_t vec4) {
#define DW_NC(KT_)                                                                              \
    hipLaunchKernelGGL((k_node_logreg<KT_, CT, M>), dim3((unsigned)blocks), dim3(NC_THREADS), 0, \
                       s, table, V, d, ids, labels, n, K, coef, partial, pred, status, vec4)
    if (kt == 1) DW_NC(1);
    else if (kt == 2) DW_NC(2);
    else if (kt == 3) DW_NC(3);
    else DW_NC(4);
#undef DW_NC
}

bool nc_sizes_ok(int64_t n, int32_t dim, int32_t n_classes, int32_t min_classes) {
    return n >= 0 && n <= INT64_MAX / 64 && dim >= 1 && dim <= 512 && n_classes >= min_classes &&
           n_classes <= 64;
}

int nc_workspace_bytes(const char *what, int32_t min_classes, int32_t tail, int64_t n,
                       int32_t dim, int32_t n_classes, size_t *bytes) {
    DW_REQUIRE(nc_sizes_ok(n, dim, n_classes, min_classes) && bytes,
               "%s_workspace_bytes: bad sizes (n >= 0, dim in [1, 512], n_classes in [%d, 64]; "
               "got dim %d, n_classes %d)",
               what, min_classes, dim, n_classes);
    const size_t len = static_cast<size_t>(n_classes) * (dim + 1) + tail;
    *bytes = static_cast<size_t>(nc_blocks(n, dim)) * len * sizeof(double);
    return DW_OK;
}

// One pass under the stage M: the size checks come before the pointers, then the pass and the
// kernel that adds the blocks' partial rows in block order.
template <class M>
int nc_pass(const char *what, int32_t min_classes, const float *table, int64_t vocab_size,
            int32_t dim, const int64_t *ids, const typename M::label_t *labels, int64_t n,
            int32_t n_classes, const double *coef, double *out, typename M::pred_t *pred,
            void *workspace, size_t workspace_bytes, int32_t *status, void *stream) {
    DW_REQUIRE(nc_sizes_ok(n, dim, n_classes, min_classes) && vocab_size >= 1 &&
                   vocab_size < (int64_t(1) << 31),
               "%s: bad sizes (vocab_size in [1, 2^31), dim in [1, 512], n_classes in [%d, 64], "
               "n >= 0; got dim %d, n_classes %d, n %lld)",
               what, min_classes, dim, n_classes, static_cast<long long>(n));
    if (n == 0) return DW_OK;
    DW_REQUIRE(table && ids && labels && coef && out && workspace, "%s: null pointer", what);
    const int64_t blocks = nc_blocks(n, dim);
    const size_t len = static_cast<size_t>(n_classes) * (dim + 1) + M::tail(n_classes);
    const size_t need = static_cast<size_t>(blocks) * len * sizeof(double);
    DW_REQUIRE(workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
               "%s: workspace too small or misaligned (%zu < %zu bytes)", what, workspace_bytes,
               need);
    const int32_t vec4 = dim % 4 == 0 && reinterpret_cast<uintptr_t>(table) % 16 == 0;
    const int kt = (n_classes + 15) / 16;
    double *partial = static_cast<double *>(workspace);
    hipStream_t s = dw::as_stream(stream);
#define DW_NC(CT_)                                                                            \
    nc_launch<M, CT_>(kt, blocks, s, table, vocab_size, dim, ids, labels, n, n_classes, coef, \
                      partial, pred, status, vec4)
    if (dim <= 128) DW_NC(2);
    else if (dim <= 256) DW_NC(4);
    else DW_NC(8);
#undef DW_NC
    DW_LAUNCH_CHECK(what);
    hipLaunchKernelGGL(dw::k_logreg_finish, dim3((unsigned)((len + 63) / 64)), dim3(64), 0, s,
                       partial, blocks, static_cast<int32_t>(len), out);
    DW_LAUNCH_CHECK(what);
    return DW_OK;
}

}  // namespace

extern "C" {

int dw_node_softmax_workspace_bytes(int64_t n, int32_t dim, int32_t n_classes, size_t *bytes) {
    return nc_workspace_bytes("dw_node_softmax", 2, NcSoftmax::tail(n_classes), n, dim, n_classes,
                              bytes);
}

int dw_node_softmax(const float *table, int64_t vocab_size, int32_t dim, const int64_t *ids,
                    const int32_t *labels, int64_t n, int32_t n_classes, const double *coef,
                    double *out, int32_t *pred, void *workspace, size_t workspace_bytes,
                    int32_t *status, void *stream) {
    return nc_pass<NcSoftmax>("dw_node_softmax", 2, table, vocab_size, dim, ids, labels, n,
                              n_classes, coef, out, pred, workspace, workspace_bytes, status,
                              stream);
}

int dw_node_ovr_workspace_bytes(int64_t n, int32_t dim, int32_t n_classes, size_t *bytes) {
    return nc_workspace_bytes("dw_node_ovr", 1, NcOvr<0>::tail(n_classes), n, dim, n_classes,
                              bytes);
}

int dw_node_ovr(const float *table, int64_t vocab_size, int32_t dim, const int64_t *ids,
                const uint64_t *masks, int64_t n, int32_t n_classes, const double *coef,
                int32_t rule, double *out, uint64_t *pred, void *workspace,
                size_t workspace_bytes, int32_t *status, void *stream) {
    DW_REQUIRE(rule == DW_OVR_THRESHOLD || rule == DW_OVR_TOP_K,
               "dw_node_ovr: bad rule %d (0: threshold, 1: top-k)", rule);
    if (rule == DW_OVR_THRESHOLD)
        return nc_pass<NcOvr<0>>("dw_node_ovr", 1, table, vocab_size, dim, ids, masks, n,
                                 n_classes, coef, out, pred, workspace, workspace_bytes, status,
                                 stream);
    return nc_pass<NcOvr<1>>("dw_node_ovr", 1, table, vocab_size, dim, ids, masks, n, n_classes,
                             coef, out, pred, workspace, workspace_bytes, status, stream);
}

}  // extern "C"
