// Community detection on the device: one Lloyd pass of k-means over the rows table[ids[i]],
// k-means++ seeding, and the integer tables behind NMI / ARI and modularity (DESIGN.md "Device
// community detection").
//
// node2vec section 4.1 clusters the embeddings with k-means; the reference has no clustering
// task (a departure). As in dw_nodeclf.hip the fp32 rows are staged once per tile in LDS and
// widened exactly on use, and both products run on v_mfma_f64_16x16x4_f64: the scores
// S = X C^T (streamed over centroid tiles of 16 with a running (min, argmin)) and the per-cluster
// sums (one-hot)^T X. Every float sum is added in an order that depends on the shape only.
#include "dw_common.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int KM_THREADS = 256;        // 4 waves
constexpr int KM_GROUP = 64;           // clusters whose sums one block keeps in registers
constexpr int KM_MAX_K = 1024;
constexpr uint32_t TAG_KMEANS = 0x4B4D0000u;   // 'KM'

// The staging shape of dw_nodeclf.hip: CT column tiles of 16 per wave, DP = 64 CT padded columns.
template <int CT>
struct KmShape {
    static constexpr int TS = CT <= 4 ? 64 : 32;   // samples per trip
    static constexpr int NS = TS / 16;             // sample tiles of 16 per trip
    static constexpr int DP = CT * 64;
    static constexpr int CH = DP / 4;              // 16-B chunks per padded row
    static constexpr int XS = DP + 20;             // XS % 64 == 20: operand reads on distinct banks
    static constexpr int NPF = TS * CH / KM_THREADS;
};

__host__ __device__ inline int km_tile_samples(int32_t dim) { return dim <= 256 ? 64 : 32; }

inline int64_t km_trips(int64_t n, int32_t dim) {
    const int64_t ts = km_tile_samples(dim);
    return (n + ts - 1) / ts;
}

// Grids, functions of the shape only. The assign pass keeps a tile in LDS and four running
// minima per lane: several blocks per CU. The sums pass keeps a group's accumulators in
// registers and one partial row per block: groups x blocks is held near 512.
inline int64_t km_assign_blocks(int64_t n, int32_t dim) {
    const int64_t cap = dim <= 128 ? 1024 : 512;
    const int64_t t = km_trips(n, dim);
    return t < 1 ? 1 : (t < cap ? t : cap);
}
inline int32_t km_groups(int32_t K) { return (K + KM_GROUP - 1) / KM_GROUP; }
inline int64_t km_sums_blocks(int64_t n, int32_t dim, int32_t K) {
    const int64_t cap = 512 / km_groups(K);   // >= 32
    const int64_t t = km_trips(n, dim);
    return t < 1 ? 1 : (t < cap ? t : cap);
}

// Stages the TS rows of a trip as fp32 in s_x: zeros where keep(i, id) is false, where the
// sample does not exist or the column is past dim. The loads are unconditional (a chunk that
// contributes nothing reads row 0 / column 0 / sample n - 1, always in range) so that a thread's
// ids, then its rows, are in flight together.
template <class S, class Keep>
__device__ __forceinline__ void km_stage(float *s_x, const float *__restrict__ table, int32_t d,
                                         const int64_t *__restrict__ ids, int64_t n, int64_t trip,
                                         int32_t vec4, int tid, Keep keep) {
    constexpr int TS = S::TS, CH = S::CH, XS = S::XS, NPF = S::NPF;
    constexpr int GRP = NPF < 8 ? NPF : 8;
#pragma unroll
    for (int j0 = 0; j0 < NPF; j0 += GRP) {
        int32_t rid[GRP];
        f4 pf[GRP];
#pragma unroll
        for (int j = 0; j < GRP; ++j) {
            const int e = tid + KM_THREADS * (j0 + j);
            const int64_t i = trip * TS + e / CH;
            const int64_t ic = i < n ? i : n - 1;
            const int64_t id = ids[ic];
            const bool ok = i < n && 4 * (e % CH) < d && keep(ic, id);
            rid[j] = ok ? static_cast<int32_t>(id) : -1;   // V < 2^31
        }
#pragma unroll
        for (int j = 0; j < GRP; ++j) {
            const int col = 4 * ((tid + KM_THREADS * (j0 + j)) % CH);
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
#pragma unroll
        for (int j = 0; j < GRP; ++j) {
            const int e = tid + KM_THREADS * (j0 + j);
            *reinterpret_cast<f4 *>(&s_x[(e / CH) * XS + 4 * (e % CH)]) = pf[j];
        }
    }
}

// ||c_k||^2, columns added in ascending order.
__global__ void __launch_bounds__(64)
    k_km_cnorm(const double *__restrict__ cent, int32_t K, int32_t d, double *__restrict__ cnorm) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    const double *c = cent + static_cast<int64_t>(k) * d;
    double s = 0.0;
    for (int j = 0; j < d; ++j) s = fma(c[j], c[j], s);
    cnorm[k] = s;
}

// Lane maps of v_mfma_f64_16x16x4_f64, lane l: A[row l & 15][k = l >> 4],
// B[k = l >> 4][col l & 15], D[row (l >> 4) + 4 reg][col l & 15], reg < 4.
//
// The scores of NSW sample tiles (from tile0) against the centroid tiles kt0, kt0 + kstep, ...:
// A = X (sample x k) from LDS, B = C^T (k x centroid) from global memory (L2). Per (lane, reg)
// a running (min, argmin) over the tiles in ascending order, then over the 16 lanes that hold a
// sample's 16 centroids; equal scores keep the lowest centroid. A padded centroid column scores
// +inf and is never taken.
template <class S, int NSW>
__device__ __forceinline__ void km_scores(const float *s_x, const double *__restrict__ cent,
                                          const double *__restrict__ cnorm, int32_t d, int32_t K,
                                          int tile0, int kt0, int kstep, int lane,
                                          double *s_best, int32_t *s_arg) {
    constexpr int XS = S::XS;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int KT = (K + 15) >> 4, steps = (d + 3) >> 2;
    double best[NSW][4];
    int32_t arg[NSW][4];
#pragma unroll
    for (int t = 0; t < NSW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            best[t][r] = INFINITY;
            arg[t][r] = 0x7fffffff;
        }
    for (int kt = kt0; kt < KT; kt += kstep) {
        const int cls = kt * 16 + l15;
        const bool cv = cls < K;
        const double *crow = cent + static_cast<int64_t>(cv ? cls : 0) * d;
        d4 acc[NSW];
#pragma unroll
        for (int t = 0; t < NSW; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int st = 0; st < steps; ++st) {
            const int kk = 4 * st + l4;
            const bool in = cv && kk < d;
            const double c = crow[in ? kk : 0];
            const double b = in ? c : 0.0;
#pragma unroll
            for (int t = 0; t < NSW; ++t) {
                const double a = static_cast<double>(s_x[((tile0 + t) * 16 + l15) * XS + kk]);
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
            }
        }
        const double cn = cv ? cnorm[cls] : INFINITY;
#pragma unroll
        for (int t = 0; t < NSW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double s = cn - 2.0 * acc[t][r];   // 2 acc is exact: one rounding
                if (s < best[t][r]) {
                    best[t][r] = s;
                    arg[t][r] = cls;
                }
            }
    }
#pragma unroll
    for (int t = 0; t < NSW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double m = best[t][r];
            int32_t a = arg[t][r];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const double om = __shfl_xor(m, off, 64);
                const int32_t oa = __shfl_xor(a, off, 64);
                if (om < m || (om == m && oa < a)) {
                    m = om;
                    a = oa;
                }
            }
            if (l15 == 0) {
                const int s = (tile0 + t) * 16 + l4 + 4 * r;
                s_best[s] = m;
                s_arg[s] = a;
            }
        }
}

// The assign pass. A trip: (1) the TS rows to LDS; (2) ||x||^2 per sample, 256 / TS lanes per
// sample over strided columns, added in a fixed lane order; (3) the scores: with two or more
// centroid tiles wave w takes the tiles w, w + 4, ... against every sample tile (a centroid
// fragment from L2 serves NS MFMAs; with three tiles one wave idles, which still beats one MFMA
// per fragment), with one tile the waves split the sample tiles; (4) per sample the minimum over
// the waves' candidates, the label, the inertia term and the changed count.
// Block b walks trips b, b + grid, ... in order; thread s keeps sample slot s's running sums,
// which thread 0 adds in slot order into the block's partial pair.
template <int CT>
__global__ void __launch_bounds__(KM_THREADS)
    k_km_assign(const float *__restrict__ table, int64_t V, int32_t d,
                const int64_t *__restrict__ ids, int64_t n, const double *__restrict__ cent,
                const double *__restrict__ cnorm, int32_t K, const int32_t *__restrict__ prev,
                int32_t *__restrict__ labels, double *__restrict__ partial, int32_t *status,
                int32_t vec4) {
    typedef KmShape<CT> S;
    constexpr int TS = S::TS, NS = S::NS, XS = S::XS;
    constexpr int L = KM_THREADS / TS;   // lanes per sample for ||x||^2
    __shared__ __attribute__((aligned(16))) float s_x[TS * XS];
    __shared__ double s_best[4][TS];
    __shared__ int32_t s_arg[4][TS];
    __shared__ double s_xn[TS];
    __shared__ double s_fin[TS];
    __shared__ long long s_chg[TS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n_trips = (n + TS - 1) / TS;
    const int KT = (K + 15) >> 4;
    double inertia = 0.0;
    long long changed = 0;

    for (int64_t trip = blockIdx.x; trip < n_trips; trip += gridDim.x) {
        __syncthreads();   // the previous trip has read s_x, s_best and s_xn
        km_stage<S>(s_x, table, d, ids, n, trip, vec4, tid,
                    [&](int64_t, int64_t id) { return id >= 0 && id < V; });
        for (int e = tid; e < 4 * TS; e += KM_THREADS) {
            (&s_best[0][0])[e] = INFINITY;
            (&s_arg[0][0])[e] = 0x7fffffff;
        }
        __syncthreads();
        {
            const int s = tid / L, j = tid % L;
            double q = 0.0;
            for (int c = j; c < d; c += L) {
                const double x = static_cast<double>(s_x[s * XS + c]);
                q = fma(x, x, q);
            }
#pragma unroll
            for (int off = 1; off < L; off <<= 1) q += __shfl_xor(q, off, 64);
            if (j == 0) s_xn[s] = q;
        }
        if (KT >= 2) {
            km_scores<S, NS>(s_x, cent, cnorm, d, K, 0, wave, 4, lane, s_best[wave],
                             s_arg[wave]);
        } else {
            constexpr int P = 4 / NS;   // waves that share a sample tile
            km_scores<S, 1>(s_x, cent, cnorm, d, K, wave % NS, wave / NS, P, lane, s_best[wave],
                            s_arg[wave]);
        }
        __syncthreads();
        const int64_t i = trip * TS + tid;
        if (tid < TS && i < n) {
            double m = s_best[0][tid];
            int32_t a = s_arg[0][tid];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const double om = s_best[w][tid];
                const int32_t oa = s_arg[w][tid];
                if (om < m || (om == m && oa < a)) {
                    m = om;
                    a = oa;
                }
            }
            const int64_t id = ids[i];
            const bool ok = id >= 0 && id < V;
            if (!ok) dw::status_or(status, DW_S_BAD_INDEX);
            // (a row of NaNs compares below nothing: cluster 0)
            const int32_t lab = ok ? (a < K ? a : 0) : -1;
            labels[i] = lab;
            if (ok) inertia += s_xn[tid] + m;
            changed += prev ? (prev[i] != lab) : 1;
        }
    }
    __syncthreads();
    if (tid < TS) {
        s_fin[tid] = inertia;
        s_chg[tid] = changed;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        long long c = 0;
        for (int s = 0; s < TS; ++s) {
            a += s_fin[s];
            c += s_chg[s];
        }
        partial[2 * blockIdx.x] = a;
        partial[2 * blockIdx.x + 1] = static_cast<double>(c);
    }
}

// The sums pass of cluster group g = blockIdx.y (clusters [64 g, 64 g + 64)): the rows of the
// samples whose label lies in the group are staged (zeros otherwise), and
// acc[class tile][column tile] += (one-hot)^T X with A = the one-hot labels (class x sample,
// built from the trip's labels), B = X (sample x column); wave w owns columns
// [16 CT w, 16 CT (w + 1)). Member counts are integers kept by thread c for cluster c. The block
// writes one partial row [64][dim + 1]; k_km_finish adds the rows in block order.
template <int KT, int CT>
__global__ void __launch_bounds__(KM_THREADS)
    k_km_sums(const float *__restrict__ table, int64_t V, int32_t d,
              const int64_t *__restrict__ ids, int64_t n, const int32_t *__restrict__ labels,
              int32_t K, double *__restrict__ partial, int32_t vec4) {
    typedef KmShape<CT> S;
    constexpr int TS = S::TS, XS = S::XS;
    __shared__ __attribute__((aligned(16))) float s_x[TS * XS];
    __shared__ int32_t s_lab[TS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int32_t c0 = blockIdx.y * KM_GROUP;
    const int32_t kg = min(KM_GROUP, K - c0);
    const int64_t n_trips = (n + TS - 1) / TS;
    const int64_t ld = static_cast<int64_t>(d) + 1;

    d4 acc[KT][CT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[kt][c] = d4{0.0, 0.0, 0.0, 0.0};
    long long count = 0;

    auto member = [&](int64_t i, int64_t id) {
        const int32_t lab = labels[i];
        return id >= 0 && id < V && lab >= c0 && lab < c0 + kg;
    };
    for (int64_t trip = blockIdx.x; trip < n_trips; trip += gridDim.x) {
        __syncthreads();   // the previous trip has read s_x and s_lab
        km_stage<S>(s_x, table, d, ids, n, trip, vec4, tid, member);
        if (tid < TS) {
            const int64_t i = trip * TS + tid;
            s_lab[tid] = (i < n && member(i, ids[i])) ? labels[i] - c0 : -1;
        }
        __syncthreads();
        if (tid < kg) {
            for (int s = 0; s < TS; ++s) count += s_lab[s] == tid;
        }
#pragma unroll 4
        for (int q = 0; q < TS / 4; ++q) {
            const int smp = 4 * q + l4;
            const int32_t lab = s_lab[smp];
            double a[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) a[kt] = lab == kt * 16 + l15 ? 1.0 : 0.0;
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
    double *dst = partial +
                  (static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x) * KM_GROUP * ld;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = (wave * CT + c) * 16 + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cls = kt * 16 + l4 + 4 * r;
                if (cls < kg && col < d) dst[cls * ld + col] = acc[kt][c][r];
            }
        }
    if (tid < kg) dst[tid * ld + d] = static_cast<double>(count);
}

// Entry t of out: the partial rows of t's cluster group added in block order, then the assign
// pass's pairs (inertia, changed) likewise.
__global__ void __launch_bounds__(64)
    k_km_finish(const double *__restrict__ part_sums, int64_t sums_blocks,
                const double *__restrict__ part_assign, int64_t assign_blocks, int32_t K,
                int32_t d, double *__restrict__ out) {
    const int64_t ld = static_cast<int64_t>(d) + 1;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
    if (t >= K * ld + 2) return;
    const double *p;
    int64_t stride, nb;
    if (t < K * ld) {
        const int64_t cls = t / ld, j = t % ld;
        p = part_sums + (cls / KM_GROUP) * sums_blocks * KM_GROUP * ld + (cls % KM_GROUP) * ld + j;
        stride = KM_GROUP * ld;
        nb = sums_blocks;
    } else {
        p = part_assign + (t - K * ld);
        stride = 2;
        nb = assign_blocks;
    }
    double s = 0.0;
    int64_t b = 0;
    for (; b + 16 <= nb; b += 16) {   // 16 loads in flight, added in block order
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = p[(b + k) * stride];
#pragma unroll
        for (int k = 0; k < 16; ++k) s += v[k];
    }
    for (; b < nb; ++b) s += p[b * stride];
    out[t] = s;
}

struct KmPlan {
    double *cnorm, *part_assign, *part_sums;
    int64_t assign_blocks, sums_blocks;
};

KmPlan km_plan(dw::Arena &a, int64_t n, int32_t dim, int32_t K) {
    KmPlan p;
    p.assign_blocks = km_assign_blocks(n, dim);
    p.sums_blocks = km_sums_blocks(n, dim, K);
    p.cnorm = a.take<double>(static_cast<size_t>(K));
    p.part_assign = a.take<double>(static_cast<size_t>(2 * p.assign_blocks));
    p.part_sums = a.take<double>(static_cast<size_t>(km_groups(K)) * p.sums_blocks * KM_GROUP *
                                 (static_cast<size_t>(dim) + 1));
    return p;
}

bool km_sizes_ok(int64_t n, int32_t dim, int32_t K) {
    return n >= 0 && n <= INT64_MAX / 64 && dim >= 1 && dim <= 512 && K >= 1 && K <= KM_MAX_K;
}

template <int CT>
void km_launch_sums(int kt, dim3 grid, hipStream_t s, const float *table, int64_t V, int32_t d,
                    const int64_t *ids, int64_t n, const int32_t *labels, int32_t K,
                    double *partial, int32_t vec4) {
#define DW_KM(KT_)                                                                              \
    hipLaunchKernelGGL((k_km_sums<KT_, CT>), grid, dim3(KM_THREADS), 0, s, table, V, d, ids, n, \
                       labels, K, partial, vec4)
    if (kt == 1) DW_KM(1);
    else if (kt == 2) DW_KM(2);
    else if (kt == 3) DW_KM(3);
    else DW_KM(4);
#undef DW_KM
}

// ---- k-means++ seeding -------------------------------------------------------------------------
constexpr int SEED_BLOCK = 256;

// U in [0, 1) keyed by (seed, j): Philox counter (j, 0, 0, 'KM'), the words split as
// genrand_res53 splits them (oracle/philox.py uniform53).
__device__ __forceinline__ double seed_uniform(uint64_t seed, uint32_t j) {
    const dw::U4 r = dw::philox(dw::U4{j, 0u, 0u, TAG_KMEANS}, static_cast<uint32_t>(seed),
                                static_cast<uint32_t>(seed >> 32));
    const uint64_t bits = (static_cast<uint64_t>(r.x >> 5) << 26) | (r.y >> 6);
    return static_cast<double>(bits) * 0x1p-53;
}

// Centre j's row, widened, into centroids[j]; a chosen sample whose id is out of range gives a
// row of zeros (and has set the status).
__device__ __forceinline__ void seed_copy_row(const float *__restrict__ table, int64_t V,
                                              int32_t d, const int64_t *__restrict__ ids,
                                              int64_t pick, double *__restrict__ crow, int tid) {
    const int64_t id = ids[pick];
    const bool ok = id >= 0 && id < V;
    for (int c = tid; c < d; c += SEED_BLOCK)
        crow[c] = ok ? static_cast<double>(table[id * d + c]) : 0.0;
}

__global__ void __launch_bounds__(SEED_BLOCK)
    k_seed_first(const float *__restrict__ table, int64_t V, int32_t d,
                 const int64_t *__restrict__ ids, int64_t n, uint64_t seed,
                 int64_t *__restrict__ chosen, double *__restrict__ cent) {
    int64_t pick = static_cast<int64_t>(seed_uniform(seed, 0) * static_cast<double>(n));
    if (pick > n - 1) pick = n - 1;
    if (threadIdx.x == 0) chosen[0] = pick;
    seed_copy_row(table, V, d, ids, pick, cent, threadIdx.x);
}

// One pass per centre: D2[i] = min(D2[i], ||x_i - c_j||^2) (columns added in ascending order;
// the first pass stores the distance itself), 0 for an id out of range, and the block's sum of
// D2 in index order.
__global__ void __launch_bounds__(SEED_BLOCK)
    k_seed_update(const float *__restrict__ table, int64_t V, int32_t d,
                  const int64_t *__restrict__ ids, int64_t n, const double *__restrict__ crow,
                  int32_t first, double *__restrict__ d2, double *__restrict__ bsum,
                  int32_t *status) {
    __shared__ double s_v[SEED_BLOCK];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * SEED_BLOCK + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        const int64_t id = ids[i];
        if (id >= 0 && id < V) {
            const float *row = table + id * d;
            double s = 0.0;
            for (int c = 0; c < d; ++c) {
                const double t = static_cast<double>(row[c]) - crow[c];
                s = fma(t, t, s);
            }
            v = first ? s : fmin(d2[i], s);
        } else if (first) {
            dw::status_or(status, DW_S_BAD_INDEX);
        }
        d2[i] = v;
    }
    s_v[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int t = 0; t < SEED_BLOCK; ++t) s += s_v[t];
        bsum[blockIdx.x] = s;
    }
}

// The first index of v[0, len) with v > 0 whose running sum (from `run`) exceeds r, else the last
// index with v > 0 (rounding left r at or above the sums; the caller's total over v is > 0).
// `run` leaves as the sum before the returned index.
__device__ inline int64_t seed_search(const double *v, int64_t len, double r, double &run) {
    int64_t last = 0;
    double run_last = run;
    for (int64_t i = 0; i < len; ++i) {
        const double x = v[i];
        if (x > 0.0) {
            if (run + x > r) return i;
            last = i;
            run_last = run;
        }
        run += x;
    }
    run = run_last;
    return last;
}

// The draw of centre j (one block). The sums are hierarchical: D2 in index order inside a block
// of 256 samples (k_seed_update), blocks in order inside 256 chunks, T = the chunks in order.
// r = U T; seed_search descends chunk, block, sample. No sample with D2 = 0 is drawn. T = 0
// (every row equals a chosen centre): the lowest index not chosen yet, which is at most j.
__global__ void __launch_bounds__(SEED_BLOCK)
    k_seed_pick(const float *__restrict__ table, int64_t V, int32_t d,
                const int64_t *__restrict__ ids, int64_t n, uint64_t seed, int32_t j,
                const double *__restrict__ d2, const double *__restrict__ bsum, int64_t n_blocks,
                int64_t *__restrict__ chosen, double *__restrict__ cent) {
    __shared__ int64_t s_pick;
    __shared__ int s_free[SEED_BLOCK];
    __shared__ double s_v[SEED_BLOCK];
    __shared__ double s_run, s_r;
    const int tid = threadIdx.x;
    // chunk t: the blocks [t per, (t + 1) per), their sums added in block order
    const int64_t per = (n_blocks + SEED_BLOCK - 1) / SEED_BLOCK;
    {
        const int64_t lo = tid * per, hi = min(n_blocks, lo + per);
        double c = 0.0;
        for (int64_t b = lo; b < hi; ++b) c += bsum[b];
        s_v[tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double T = 0.0;
        for (int t = 0; t < SEED_BLOCK; ++t) T += s_v[t];
        int64_t blk = -1;
        if (T > 0.0) {
            const double r = seed_uniform(seed, static_cast<uint32_t>(j)) * T;
            double run = 0.0;
            const int64_t lo = seed_search(s_v, SEED_BLOCK, r, run) * per;
            blk = lo + seed_search(bsum + lo, min(n_blocks, lo + per) - lo, r, run);
            s_run = run;
            s_r = r;
        }
        s_pick = blk;
    }
    __syncthreads();
    if (s_pick >= 0) {   // uniform over the block: the chosen block's D2, then the draw inside it
        const int64_t lo = s_pick * SEED_BLOCK;
        __syncthreads();
        s_v[tid] = lo + tid < n ? d2[lo + tid] : 0.0;
        __syncthreads();
        if (tid == 0) {
            double run = s_run;
            s_pick = lo + seed_search(s_v, SEED_BLOCK, s_r, run);
        }
    }
    __syncthreads();
    if (s_pick < 0) {   // uniform over the block
        // candidates 0 .. j (j chosen indices leave one of them free), thread t takes t, t + 256..
        int mine = 0x7fffffff;
        for (int c = tid; c <= j && c < n; c += SEED_BLOCK) {
            bool taken = false;
            for (int q = 0; q < j; ++q) taken = taken || chosen[q] == c;
            if (!taken) {
                mine = c;
                break;
            }
        }
        s_free[tid] = mine;
        __syncthreads();
        if (tid == 0) {
            int m = 0x7fffffff;
            for (int t = 0; t < SEED_BLOCK; ++t) m = min(m, s_free[t]);
            s_pick = m;   // n >= n_clusters: a free index exists
        }
        __syncthreads();
    }
    const int64_t pick = s_pick;
    if (tid == 0) chosen[j] = pick;
    seed_copy_row(table, V, d, ids, pick, cent + static_cast<int64_t>(j) * d, tid);
}

struct SeedPlan {
    double *d2, *bsum;
    int64_t n_blocks;
};

SeedPlan seed_plan(dw::Arena &a, int64_t n) {
    SeedPlan p;
    p.n_blocks = (n + SEED_BLOCK - 1) / SEED_BLOCK;
    p.d2 = a.take<double>(static_cast<size_t>(n));
    p.bsum = a.take<double>(static_cast<size_t>(p.n_blocks));
    return p;
}

// ---- partition tables --------------------------------------------------------------------------
__device__ __forceinline__ void add_i64(int64_t *dst, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(dst), static_cast<unsigned long long>(v));
}

__global__ void __launch_bounds__(256)
    k_partition_counts(const int32_t *__restrict__ a, int32_t Ka, const int32_t *__restrict__ b,
                       int32_t Kb, int64_t n, int64_t *__restrict__ table, int32_t *status) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    bool bad = false;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) {
        const int32_t x = a[i], y = b[i];
        if (x < -1 || x >= Ka || y < -1 || y >= Kb) {
            bad = true;
            continue;
        }
        if (x < 0 || y < 0) continue;
        add_i64(&table[static_cast<int64_t>(x) * Kb + y], 1);
    }
    if (bad) dw::status_or(status, DW_S_BAD_INDEX);
}

// One wave per CSR row u: over its entries v, the entries with label[v] == label[u] and the
// row's degree (a self-loop entry counts twice in both), one integer atomic each per row.
__global__ void __launch_bounds__(256)
    k_modularity_counts(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                        int64_t n_rows, int64_t nnz, const int32_t *__restrict__ labels,
                        int32_t K, int64_t *__restrict__ out, int32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t u = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (u >= n_rows) return;
    const int32_t lu = labels[u];
    const int64_t a = row_ptr[u], b = row_ptr[u + 1];
    bool bad = lu < -1 || lu >= K || a < 0 || b < a || b > nnz;
    long long in = 0, deg = 0;
    if (!bad && lu >= 0) {
        for (int64_t e = a + lane; e < b; e += 64) {
            const int32_t v = col[e];
            if (v < 0 || v >= n_rows) {
                bad = true;
                continue;
            }
            const int w = v == u ? 2 : 1;
            deg += w;
            if (labels[v] == lu) in += w;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        in += __shfl_xor(in, off, 64);
        deg += __shfl_xor(deg, off, 64);
    }
    if (__any(bad)) {
        if (lane == 0) dw::status_or(status, DW_S_BAD_INDEX);
        return;
    }
    if (lane == 0 && lu >= 0) {
        if (in) add_i64(&out[2 * lu], in);
        if (deg) add_i64(&out[2 * lu + 1], deg);
    }
}

}  // namespace

extern "C" {

int dw_kmeans_step_workspace_bytes(int64_t n, int32_t dim, int32_t n_clusters, size_t *bytes) {
    DW_REQUIRE(km_sizes_ok(n, dim, n_clusters) && bytes,
               "dw_kmeans_step_workspace_bytes: bad sizes (n >= 0, dim in [1, 512], n_clusters in "
               "[1, 1024]; got dim %d, n_clusters %d)", dim, n_clusters);
    dw::Arena a{nullptr};
    km_plan(a, n, dim, n_clusters);
    *bytes = a.off;
    return DW_OK;
}

int dw_kmeans_step(const float *table, int64_t vocab_size, int32_t dim, const int64_t *ids,
                   int64_t n, const double *centroids, int32_t n_clusters,
                   const int32_t *prev_labels, int32_t *labels_out, double *out, void *workspace,
                   size_t workspace_bytes, int32_t *status, void *stream) {
    DW_REQUIRE(km_sizes_ok(n, dim, n_clusters) && vocab_size >= 1 &&
                   vocab_size < (int64_t(1) << 31),
               "dw_kmeans_step: bad sizes (vocab_size in [1, 2^31), dim in [1, 512], n_clusters "
               "in [1, 1024], n >= 0; got dim %d, n_clusters %d, n %lld)",
               dim, n_clusters, static_cast<long long>(n));
    if (n == 0) return DW_OK;
    DW_REQUIRE(table && ids && centroids && labels_out && out && workspace,
               "dw_kmeans_step: null pointer");
    DW_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 256 == 0,
               "dw_kmeans_step: workspace must be 256-byte aligned");
    dw::Arena a{static_cast<char *>(workspace)};
    const KmPlan p = km_plan(a, n, dim, n_clusters);
    DW_REQUIRE(workspace_bytes >= a.off, "dw_kmeans_step: workspace too small (%zu < %zu bytes)",
               workspace_bytes, a.off);
    const int32_t vec4 = dim % 4 == 0 && reinterpret_cast<uintptr_t>(table) % 16 == 0;
    const int32_t K = n_clusters;
    hipStream_t s = dw::as_stream(stream);
    hipLaunchKernelGGL(k_km_cnorm, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, s, centroids, K,
                       dim, p.cnorm);
    DW_LAUNCH_CHECK("dw_kmeans_step");
#define DW_KM(CT_)                                                                             \
    hipLaunchKernelGGL((k_km_assign<CT_>), dim3((unsigned)p.assign_blocks), dim3(KM_THREADS), 0, \
                       s, table, vocab_size, dim, ids, n, centroids, p.cnorm, K, prev_labels,  \
                       labels_out, p.part_assign, status, vec4)
    if (dim <= 128) DW_KM(2);
    else if (dim <= 256) DW_KM(4);
    else DW_KM(8);
#undef DW_KM
    DW_LAUNCH_CHECK("dw_kmeans_step");
    const dim3 grid((unsigned)p.sums_blocks, (unsigned)km_groups(K));
    const int kt = K >= KM_GROUP ? 4 : (K + 15) / 16;
    if (dim <= 128)
        km_launch_sums<2>(kt, grid, s, table, vocab_size, dim, ids, n, labels_out, K, p.part_sums,
                          vec4);
    else if (dim <= 256)
        km_launch_sums<4>(kt, grid, s, table, vocab_size, dim, ids, n, labels_out, K, p.part_sums,
                          vec4);
    else
        km_launch_sums<8>(kt, grid, s, table, vocab_size, dim, ids, n, labels_out, K, p.part_sums,
                          vec4);
    DW_LAUNCH_CHECK("dw_kmeans_step");
    const int64_t len = static_cast<int64_t>(K) * (dim + 1) + 2;
    hipLaunchKernelGGL(k_km_finish, dim3((unsigned)((len + 63) / 64)), dim3(64), 0, s,
                       p.part_sums, p.sums_blocks, p.part_assign, p.assign_blocks, K, dim, out);
    DW_LAUNCH_CHECK("dw_kmeans_step");
    return DW_OK;
}

int dw_kmeans_seed_workspace_bytes(int64_t n, size_t *bytes) {
    DW_REQUIRE(n >= 0 && n <= INT64_MAX / 64 && bytes, "dw_kmeans_seed_workspace_bytes: bad n");
    dw::Arena a{nullptr};
    seed_plan(a, n);
    *bytes = a.off;
    return DW_OK;
}

int dw_kmeans_seed(const float *table, int64_t vocab_size, int32_t dim, const int64_t *ids,
                   int64_t n, int32_t n_clusters, uint64_t seed, int64_t *chosen_out,
                   double *centroids_out, void *workspace, size_t workspace_bytes,
                   int32_t *status, void *stream) {
    DW_REQUIRE(km_sizes_ok(n, dim, n_clusters) && vocab_size >= 1 &&
                   vocab_size < (int64_t(1) << 31) && n < (int64_t(1) << 53),
               "dw_kmeans_seed: bad sizes (vocab_size in [1, 2^31), dim in [1, 512], n_clusters "
               "in [1, 1024]; got dim %d, n_clusters %d, n %lld)",
               dim, n_clusters, static_cast<long long>(n));
    if (n == 0) return DW_OK;
    DW_REQUIRE(n >= n_clusters, "dw_kmeans_seed: %d centres from %lld samples", n_clusters,
               static_cast<long long>(n));
    DW_REQUIRE(table && ids && chosen_out && centroids_out && workspace,
               "dw_kmeans_seed: null pointer");
    DW_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 256 == 0,
               "dw_kmeans_seed: workspace must be 256-byte aligned");
    dw::Arena a{static_cast<char *>(workspace)};
    const SeedPlan p = seed_plan(a, n);
    DW_REQUIRE(workspace_bytes >= a.off, "dw_kmeans_seed: workspace too small (%zu < %zu bytes)",
               workspace_bytes, a.off);
    hipStream_t s = dw::as_stream(stream);
    hipLaunchKernelGGL(k_seed_first, dim3(1), dim3(SEED_BLOCK), 0, s, table, vocab_size, dim, ids,
                       n, seed, chosen_out, centroids_out);
    DW_LAUNCH_CHECK("dw_kmeans_seed");
    for (int32_t j = 1; j < n_clusters; ++j) {
        hipLaunchKernelGGL(k_seed_update, dim3((unsigned)p.n_blocks), dim3(SEED_BLOCK), 0, s,
                           table, vocab_size, dim, ids, n,
                           centroids_out + static_cast<int64_t>(j - 1) * dim, j == 1 ? 1 : 0, p.d2,
                           p.bsum, status);
        hipLaunchKernelGGL(k_seed_pick, dim3(1), dim3(SEED_BLOCK), 0, s, table, vocab_size, dim,
                           ids, n, seed, j, p.d2, p.bsum, p.n_blocks, chosen_out, centroids_out);
        DW_LAUNCH_CHECK("dw_kmeans_seed");
    }
    return DW_OK;
}

int dw_partition_counts(const int32_t *labels_a, int32_t n_a_classes, const int32_t *labels_b,
                        int32_t n_b_classes, int64_t n, int64_t *table_out, int32_t *status,
                        void *stream) {
    DW_REQUIRE(n >= 0 && n_a_classes >= 1 && n_b_classes >= 1 &&
                   static_cast<int64_t>(n_a_classes) * n_b_classes <= (int64_t(1) << 24),
               "dw_partition_counts: bad sizes (n >= 0, classes >= 1, Ka Kb <= 2^24; got %d x %d)",
               n_a_classes, n_b_classes);
    if (n == 0) return DW_OK;
    DW_REQUIRE(labels_a && labels_b && table_out, "dw_partition_counts: null pointer");
    hipStream_t s = dw::as_stream(stream);
    const size_t cells = static_cast<size_t>(n_a_classes) * n_b_classes;
    if (hipMemsetAsync(table_out, 0, cells * sizeof(int64_t), s) != hipSuccess) {
        dw::set_error("dw_partition_counts: hipMemsetAsync failed");
        return DW_E_HIP;
    }
    int64_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_partition_counts, dim3((unsigned)blocks), dim3(256), 0, s, labels_a,
                       n_a_classes, labels_b, n_b_classes, n, table_out, status);
    DW_LAUNCH_CHECK("dw_partition_counts");
    return DW_OK;
}

int dw_modularity_counts(const int64_t *row_ptr, const int32_t *col, int64_t n_rows, int64_t nnz,
                         const int32_t *labels, int32_t n_clusters, int64_t *out, int32_t *status,
                         void *stream) {
    DW_REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 31) && nnz >= 0 && n_clusters >= 1 &&
                   n_clusters <= (1 << 24),
               "dw_modularity_counts: bad sizes (n_rows in [0, 2^31), nnz >= 0, n_clusters in "
               "[1, 2^24]; got n_clusters %d)", n_clusters);
    if (n_rows == 0) return DW_OK;
    DW_REQUIRE(row_ptr && labels && out && (col || nnz == 0),
               "dw_modularity_counts: null pointer");
    hipStream_t s = dw::as_stream(stream);
    if (hipMemsetAsync(out, 0, 2 * static_cast<size_t>(n_clusters) * sizeof(int64_t), s) !=
        hipSuccess) {
        dw::set_error("dw_modularity_counts: hipMemsetAsync failed");
        return DW_E_HIP;
    }
    hipLaunchKernelGGL(k_modularity_counts, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s,
                       row_ptr, col, n_rows, nnz, labels, n_clusters, out, status);
    DW_LAUNCH_CHECK("dw_modularity_counts");
    return DW_OK;
}

}  // extern "C"
