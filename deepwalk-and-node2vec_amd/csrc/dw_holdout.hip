// Held-out edge split on gfx950 (DESIGN.md §4.4 "Held-out link prediction";
// shallow_encoders/graph/holdout.py): a simple undirected CSR, a 64-bit seed and a count of edges
// to hide -> the train CSR and the list of hidden edges, every node keeping an edge.
//
//   prio{u, v} = mix64(((u << 32) | v) ^ mix64(seed)), u < v   (splitmix64's finaliser: a
//                bijection, so no two edges tie under one seed)
//   protected  = the non-loop edge of smallest priority at either endpoint
//   held       = the n_hold unprotected non-loop edges of smallest priority (prio <= T)
//
//   dw_edge_holdout_count   per-node minimum priority; the unprotected priorities, compacted;
//                           E_nl and n_candidates for the host, which fixes n_hold
//   dw_edge_holdout         sort the candidates (T = the n_hold-th), flag every entry, scan, write
//   dw_edge_forest          the minimum spanning forest of the non-loop edges under prio (Boruvka,
//                           below) and every row's connected component
//   dw_edge_holdout_count_protected / dw_edge_holdout_protected
//                           the same split with the protected entries given as flags (the forest:
//                           the residual graph keeps the full graph's components)
//
// Every kernel is entry-parallel: thread e owns directed entry e and finds its row by a binary
// search of row_ptr once (k_min_prio keeps it in `rows`), so a 44,848-neighbour hub and a
// degree-1 leaf cost the same per entry. The per-node minimum is a 64-bit integer atomicMin per
// run of a row's entries inside a wave: exact and order-independent. Each entry decides from
// minp[x], minp[y], its own priority and T alone; the mate entry computes the same priority and
// reaches the same verdict, so no search for it is needed. Integer atomics, a radix sort of
// distinct keys and a scan: reruns are bit-identical.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "dw_common.h"
#include "dw_ingest.h"

namespace {

using dw::Arena;
using dw::ingest::grid_of;

constexpr uint64_t NO_PRIO = ~uint64_t(0);
constexpr int64_t LIMIT_31 = int64_t(1) << 31;

__host__ __device__ inline uint64_t mix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t edge_prio(int64_t x, int64_t y, uint64_t mseed) {
    const uint64_t u = static_cast<uint64_t>(x < y ? x : y), v = static_cast<uint64_t>(x < y ? y : x);
    return mix64(((u << 32) | v) ^ mseed);
}

// An entry x -> y the rule applies to: both ends are nodes (rows 1 .. n_rows - 1). Anything else
// is a malformed CSR: flagged, kept as it is, and never used as an index.
__device__ __forceinline__ bool entry_ok(int64_t x, int64_t y, int64_t n_rows) {
    return x >= 1 && y >= 1 && y < n_rows;
}

struct Bufs {
    uint64_t *minp, *cand0, *cand1, *flags, *scan;
    int32_t *rows;
    void *tmp;
    size_t tmp_bytes;
};

int plan(Arena &a, int64_t n_rows, int64_t nnz, Bufs *p) {
    const size_t n = static_cast<size_t>(nnz > 0 ? nnz : 1);
    size_t s1 = 0, s2 = 0;
    rocprim::double_buffer<uint64_t> kb(nullptr, nullptr);
    DW_HIP_OK(rocprim::radix_sort_keys(nullptr, s1, kb, n, 0, 64), "dw_edge_holdout: sort plan");
    DW_HIP_OK(rocprim::exclusive_scan(nullptr, s2, static_cast<const uint64_t *>(nullptr),
                                      static_cast<uint64_t *>(nullptr), uint64_t(0), n + 1,
                                      rocprim::plus<uint64_t>()),
              "dw_edge_holdout: scan plan");
    p->minp = a.take<uint64_t>(static_cast<size_t>(n_rows));
    p->cand0 = a.take<uint64_t>(n);
    p->cand1 = a.take<uint64_t>(n);
    p->flags = a.take<uint64_t>(n + 1);
    p->scan = a.take<uint64_t>(n + 1);
    p->rows = a.take<int32_t>(n);
    p->tmp_bytes = s1 > s2 ? s1 : s2;
    p->tmp = a.take<char>(p->tmp_bytes);
    return DW_OK;
}

// The row of entry e: the r in [0, n_rows - 1] with row_ptr[r] <= e < row_ptr[r + 1].
__device__ __forceinline__ int32_t row_of(const int64_t *__restrict__ row_ptr, int64_t n_rows,
                                          int64_t e) {
    int64_t lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row_ptr[mid + 1] > e)
            hi = mid;
        else
            lo = mid + 1;
    }
    return static_cast<int32_t>(lo);
}

// Which non-loop entries the split never hides: entry e = x -> y of priority p. Both directed
// entries of an edge get the same answer under either rule.
struct ByMinimum {   // the edge of smallest priority at either endpoint
    const uint64_t *__restrict__ minp;
    __device__ __forceinline__ bool operator()(int64_t, int64_t x, int64_t y, uint64_t p) const {
        return p == minp[x] || p == minp[y];
    }
};
struct ByFlag {      // the caller's flags (dw_edge_forest's)
    const uint8_t *__restrict__ flag;
    __device__ __forceinline__ bool operator()(int64_t e, int64_t, int64_t, uint64_t) const {
        return flag[e] != 0;
    }
};

__global__ void __launch_bounds__(256) k_fill(uint64_t *__restrict__ dst, int64_t n, uint64_t v) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i < n) dst[i] = v;
}

// rows[e] = the row of entry e (the r with row_ptr[r] <= e < row_ptr[r + 1]); minp[x] = the
// smallest priority among x's non-loop entries.
__global__ void __launch_bounds__(256)
    k_min_prio(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
               int64_t n_rows, int64_t nnz, uint64_t mseed, int32_t *__restrict__ rows,
               uint64_t *__restrict__ minp, int32_t *status) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t row = INT32_MAX;   // past the end: above every row, so a wave's rows stay sorted
    uint64_t p = NO_PRIO;
    if (e < nnz) {
        row = row_of(row_ptr, n_rows, e);
        rows[e] = row;
        const int64_t x = row, y = col[e];
        if (!entry_ok(x, y, n_rows))
            dw::status_or(status, DW_S_BAD_CSR);
        else if (x != y)
            p = edge_prio(x, y, mseed);
    }
    // A wave's 64 entries are consecutive, so equal rows are runs of lanes: a segmented minimum
    // over the runs (after the step at `off`, a lane holds the minimum of its row's lanes among
    // the next 2 off), then one atomic per run instead of one per entry — a hub row's 44,848
    // entries reach its word about 700 times, a row inside one wave once.
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t other = __shfl_down(static_cast<unsigned long long>(p), off, 64);
        const int32_t other_row = __shfl_down(row, off, 64);
        if (lane + off < 64 && other_row == row && other < p) p = other;
    }
    const int32_t before = __shfl_up(row, 1, 64);
    if ((lane == 0 || before != row) && p != NO_PRIO)
        atomicMin(reinterpret_cast<unsigned long long *>(minp + row),
                  static_cast<unsigned long long>(p));
}

// counts[0] += the non-loop edges (entries with col > row), counts[1] += the unprotected ones,
// whose priorities are appended to cand in any order (they are sorted next). A block owns
// CAND_TILE consecutive entries, counts both in LDS and takes its range of cand with one atomic:
// one atomic per entry on the two counters ran at the rate of a single L2 word (7.4 ms of the
// first version's 13.5 at R-MAT 20).
constexpr int CAND_PER = 8;
constexpr int CAND_TILE = 256 * CAND_PER;

template <class Protect>
__global__ void __launch_bounds__(256)
    k_candidates(const int32_t *__restrict__ col, const int32_t *__restrict__ rows,
                 int64_t n_rows, int64_t nnz, uint64_t mseed, const Protect is_protected,
                 uint64_t *__restrict__ cand, unsigned long long *counts) {
    __shared__ uint32_t s_cand[4], s_edges[4];
    __shared__ unsigned long long s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = blockIdx.x * static_cast<int64_t>(CAND_TILE);
    uint64_t p[CAND_PER];
    uint32_t mask = 0, n_edges = 0;
#pragma unroll
    for (int k = 0; k < CAND_PER; ++k) {
        const int64_t e = tile + k * 256 + threadIdx.x;
        p[k] = NO_PRIO;
        if (e < nnz) {
            const int64_t x = rows[e], y = col[e];
            if (entry_ok(x, y, n_rows) && y > x) {
                ++n_edges;
                p[k] = edge_prio(x, y, mseed);
                if (!is_protected(e, x, y, p[k])) mask |= 1u << k;
            }
        }
    }
    const uint32_t mine = __popc(mask);
    uint32_t incl = mine;   // candidates of the wave's lanes up to this one
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n_edges += __shfl_xor(n_edges, off, 64);
    if (lane == 63) s_cand[wave] = incl;
    if (lane == 0) s_edges[wave] = n_edges;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t c = s_cand[0] + s_cand[1] + s_cand[2] + s_cand[3];
        const uint32_t m = s_edges[0] + s_edges[1] + s_edges[2] + s_edges[3];
        if (m) atomicAdd(counts, static_cast<unsigned long long>(m));
        s_base = c ? atomicAdd(counts + 1, static_cast<unsigned long long>(c)) : 0ull;
    }
    __syncthreads();
    unsigned long long at = s_base + (incl - mine);
    for (int w = 0; w < wave; ++w) at += s_cand[w];
#pragma unroll
    for (int k = 0; k < CAND_PER; ++k) {
        if (mask & (1u << k)) {
            if (at < static_cast<unsigned long long>(nnz)) cand[at] = p[k];
            ++at;
        }
    }
}

// flags[e]: bit 0 = the entry stays in the train CSR, bit 32 = it is the col > row entry of a
// held edge (one sum scans both counts: each stays below 2^31). flags[nnz] = 0 closes the scan.
template <class Protect>
__global__ void __launch_bounds__(256)
    k_flags(const int32_t *__restrict__ col, const int32_t *__restrict__ rows, int64_t n_rows,
            int64_t nnz, uint64_t mseed, const Protect is_protected,
            const uint64_t *__restrict__ threshold, uint64_t *__restrict__ flags) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (e > nnz) return;
    uint64_t f = 0;
    if (e < nnz) {
        f = 1;
        const int64_t x = rows[e], y = col[e];
        if (threshold && entry_ok(x, y, n_rows) && x != y) {
            const uint64_t p = edge_prio(x, y, mseed);
            if (!is_protected(e, x, y, p) && p <= *threshold)
                f = y > x ? uint64_t(1) << 32 : 0;
        }
    }
    flags[e] = f;
}

__global__ void __launch_bounds__(256)
    k_write(const int32_t *__restrict__ col, const double *__restrict__ weights,
            const int32_t *__restrict__ rows, int64_t nnz, const uint64_t *__restrict__ flags,
            const uint64_t *__restrict__ scan, int64_t nnz_out, int64_t n_hold,
            int32_t *__restrict__ col_out, double *__restrict__ weights_out,
            int64_t *__restrict__ held, int32_t *status) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (e >= nnz) return;
    const uint64_t f = flags[e], s = scan[e];
    if (f & 1u) {
        const int64_t at = static_cast<int64_t>(s & 0xFFFFFFFFull);
        if (at >= nnz_out) {   // more entries stay than the host counted: not a simple graph
            dw::status_or(status, DW_S_DUP_NEIGHBOR);
            return;
        }
        col_out[at] = col[e];
        if (weights) weights_out[at] = weights[e];
    } else if (f >> 32) {
        const int64_t at = static_cast<int64_t>(s >> 32);
        if (at >= n_hold) {
            dw::status_or(status, DW_S_DUP_NEIGHBOR);
            return;
        }
        held[2 * at] = rows[e];
        held[2 * at + 1] = col[e];
    }
}

// row_ptr_out[r] = the entries that stay before row r; the totals are checked against the host's.
__global__ void __launch_bounds__(256)
    k_row_ptr(const int64_t *__restrict__ row_ptr, int64_t n_rows, int64_t nnz,
              const uint64_t *__restrict__ scan, int64_t nnz_out, int64_t n_hold,
              int64_t *__restrict__ row_ptr_out, int32_t *status) {
    const int64_t r = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (r > n_rows) return;
    int64_t e = row_ptr[r];
    e = e < 0 ? 0 : e > nnz ? nnz : e;
    row_ptr_out[r] = static_cast<int64_t>(scan[e] & 0xFFFFFFFFull);
    if (r == n_rows && (static_cast<int64_t>(scan[nnz] & 0xFFFFFFFFull) != nnz_out ||
                        static_cast<int64_t>(scan[nnz] >> 32) != n_hold))
        dw::status_or(status, DW_S_DUP_NEIGHBOR);
}

int check_sizes(const char *who, int64_t n_rows, int64_t nnz) {
    DW_REQUIRE(n_rows >= 1 && n_rows < LIMIT_31 && nnz >= 0 && nnz < LIMIT_31,
               "%s: n_rows must be in [1, 2^31) and nnz in [0, 2^31)", who);
    return DW_OK;
}

// ---- minimum spanning forest and connected components (Boruvka on the CSR) -----------------------
// Every vertex carries the label comp[v] of its tree's root; parent[c] == c marks a root. A round:
//
//   k_comp_min   best[c] = the smallest priority among the entries that leave component c
//   k_hook       the entry that holds best[c] is a forest edge and hangs c under the other side's
//                root; two components that pick the same edge keep the smaller label as the root.
//                Distinct priorities allow no other cycle: along a chain of hooks best[] falls
//                strictly (the far side sees the mate entry, so its best is <= this one's), and a
//                far side whose best is larger (a CSR that lacks the mate entry) is refused
//   k_compress   comp[v] = the root above comp[v]; best[] is cleared for the next round
//
// Components that still have a leaving edge at least halve per round, so ceil(log2 n_rows) rounds
// always suffice and that many are launched, with no host read in between: ctrl[r + 1] says
// whether round r hooked anything (ctrl[0] = 1), and a round's kernels return at once when the
// round before hooked nothing. Integer atomics and same-value stores only: reruns are identical.
struct ForestBufs {
    int32_t *rows, *comp, *parent, *minid, *ctrl;
    uint64_t *best;
};

int forest_rounds(int64_t n_rows) {   // ceil(log2(n_rows)), at least 1
    int r = 0;
    while ((int64_t(1) << r) < n_rows) ++r;
    return r > 0 ? r : 1;
}

void forest_plan(Arena &a, int64_t n_rows, int64_t nnz, ForestBufs *p) {
    const size_t n = static_cast<size_t>(nnz > 0 ? nnz : 1), v = static_cast<size_t>(n_rows);
    p->rows = a.take<int32_t>(n);
    p->comp = a.take<int32_t>(v);
    p->parent = a.take<int32_t>(v);
    p->minid = a.take<int32_t>(v);
    p->ctrl = a.take<int32_t>(static_cast<size_t>(forest_rounds(n_rows)) + 1);
    p->best = a.take<uint64_t>(v);
}

__global__ void __launch_bounds__(256)
    k_forest_init(int64_t n_rows, int n_ctrl, int32_t *__restrict__ comp,
                  int32_t *__restrict__ parent, int32_t *__restrict__ minid,
                  uint64_t *__restrict__ best, int32_t *__restrict__ ctrl) {
    const int64_t v = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (v < n_ctrl) ctrl[v] = v == 0;
    if (v >= n_rows) return;
    comp[v] = parent[v] = static_cast<int32_t>(v);
    minid[v] = INT32_MAX;
    best[v] = NO_PRIO;
}

__global__ void __launch_bounds__(256)
    k_forest_rows(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                  int64_t n_rows, int64_t nnz, int32_t *__restrict__ rows, int32_t *status) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (e >= nnz) return;
    const int32_t row = row_of(row_ptr, n_rows, e);
    rows[e] = row;
    if (!entry_ok(row, col[e], n_rows)) dw::status_or(status, DW_S_BAD_CSR);
}

// A value that only falls, so a stale read is safe: it can only let through an atomic that
// changes nothing. Without the read, the late rounds send every boundary entry of the giant
// component to one L2 word (k_candidates' note has what that costs).
__device__ __forceinline__ void min_if_lower(uint64_t *word, uint64_t p) {
    if (p < __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(reinterpret_cast<unsigned long long *>(word), static_cast<unsigned long long>(p));
}

__global__ void __launch_bounds__(256)
    k_comp_min(const int32_t *__restrict__ col, const int32_t *__restrict__ rows, int64_t n_rows,
               int64_t nnz, uint64_t mseed, const int32_t *__restrict__ comp,
               const int32_t *__restrict__ gate, uint64_t *best) {
    if (*gate == 0) return;
    const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t row = INT32_MAX;
    uint64_t p = NO_PRIO;
    if (e < nnz) {
        row = rows[e];
        const int64_t x = row, y = col[e];
        if (entry_ok(x, y, n_rows) && x != y && comp[x] != comp[y]) p = edge_prio(x, y, mseed);
    }
    // k_min_prio's segmented minimum: a row's entries share comp[row]
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t other = __shfl_down(static_cast<unsigned long long>(p), off, 64);
        const int32_t other_row = __shfl_down(row, off, 64);
        if (lane + off < 64 && other_row == row && other < p) p = other;
    }
    const int32_t before = __shfl_up(row, 1, 64);
    if ((lane == 0 || before != row) && p != NO_PRIO) min_if_lower(best + comp[row], p);
}

__global__ void __launch_bounds__(256)
    k_hook(const int32_t *__restrict__ col, const int32_t *__restrict__ rows, int64_t n_rows,
           int64_t nnz, uint64_t mseed, const int32_t *__restrict__ comp,
           const uint64_t *__restrict__ best, const int32_t *__restrict__ gate,
           int32_t *__restrict__ parent, uint8_t *__restrict__ forest, int32_t *__restrict__ hooked,
           int32_t *status) {
    if (*gate == 0) return;
    const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (e >= nnz) return;
    const int64_t x = rows[e], y = col[e];
    if (!entry_ok(x, y, n_rows) || x == y) return;
    const int32_t cx = comp[x], cy = comp[y];
    if (cx == cy) return;
    const uint64_t p = edge_prio(x, y, mseed), bx = best[cx], by = best[cy];
    if (p == bx || p == by) forest[e] = 1;
    if (p != bx) return;
    if (by > p) {   // y's side never saw this edge: the CSR lacks the entry y -> x
        dw::status_or(status, DW_S_BAD_CSR);
        return;
    }
    if (by == p && cx < cy) return;   // a mutual pick: the smaller label stays the root
    parent[cx] = cy;
    *hooked = 1;
}

__global__ void __launch_bounds__(256)
    k_compress(int64_t n_rows, const int32_t *__restrict__ parent,
               const int32_t *__restrict__ gate, int32_t *__restrict__ comp,
               uint64_t *__restrict__ best) {
    if (*gate == 0) return;
    const int64_t v = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (v >= n_rows) return;
    int32_t c = comp[v], q;
    while ((q = parent[c]) != c) c = q;   // parent is not written here and holds no cycle
    comp[v] = c;
    best[v] = NO_PRIO;
}

// minid[c] = the smallest row of the tree rooted at c. Lanes hold ascending rows, so the first
// lane of a run of equal roots has the run's smallest; it reads before it asks, as above.
__global__ void __launch_bounds__(256)
    k_comp_minid(int64_t n_rows, const int32_t *__restrict__ comp, int32_t *minid) {
    const int64_t v = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t c = v < n_rows ? comp[v] : -1;
    const int32_t before = __shfl_up(c, 1, 64);
    if (c >= 0 && (lane == 0 || before != c) &&
        static_cast<int32_t>(v) < __hip_atomic_load(minid + c, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(minid + c, static_cast<int32_t>(v));
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *s_part) {   // 256 threads
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// component[v] = its tree's smallest row; counts[2] += the components that hold a non-loop edge
// (their smallest row has one); counts[3] = the rounds that hooked; the last allowed round must
// not have.
__global__ void __launch_bounds__(256)
    k_forest_labels(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                    int64_t n_rows, int64_t nnz, const int32_t *__restrict__ comp,
                    const int32_t *__restrict__ minid, const int32_t *__restrict__ ctrl,
                    int max_rounds, int32_t *__restrict__ component, unsigned long long *counts,
                    int32_t *status) {
    __shared__ uint32_t s_part[4];
    const int64_t v = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    uint32_t heads = 0;
    if (v < n_rows) {
        const int32_t label = minid[comp[v]];
        component[v] = label;
        if (label == v && v >= 1) {
            int64_t e = row_ptr[v], end = row_ptr[v + 1];
            e = e < 0 ? 0 : e;
            end = end > nnz ? nnz : end;
            for (; e < end && !heads; ++e) heads = col[e] != v;
        }
    }
    const uint32_t total = block_sum(heads, s_part);
    if (threadIdx.x == 0 && total) atomicAdd(counts + 2, static_cast<unsigned long long>(total));
    if (v == 0) {
        int used = 0;
        for (int r = 1; r <= max_rounds; ++r) used += ctrl[r] != 0;
        counts[3] = static_cast<unsigned long long>(used);
        if (ctrl[max_rounds] != 0) dw::status_or(status, DW_S_FOREST_ROUNDS);
    }
}

// counts[0] += the non-loop edges (entries with col > row), counts[1] += those in the forest. A
// block owns CAND_TILE entries, as in k_candidates: with 256 per block the two atomics of
// 78,000 blocks on neighbouring words took 1.86 ms of the call's 5.0 at R-MAT 20.
__global__ void __launch_bounds__(256)
    k_forest_count(const int32_t *__restrict__ col, const int32_t *__restrict__ rows,
                   int64_t n_rows, int64_t nnz, const uint8_t *__restrict__ forest,
                   unsigned long long *counts) {
    __shared__ uint32_t s_edges[4], s_forest[4];
    const int64_t tile = blockIdx.x * static_cast<int64_t>(CAND_TILE);
    uint32_t edge = 0, in_forest = 0;
#pragma unroll
    for (int k = 0; k < CAND_PER; ++k) {
        const int64_t e = tile + k * 256 + threadIdx.x;
        if (e < nnz) {
            const int64_t x = rows[e], y = col[e];
            const bool upper = entry_ok(x, y, n_rows) && y > x;
            edge += upper;
            in_forest += upper && forest[e];
        }
    }
    const uint32_t n_edges = block_sum(edge, s_edges), n_forest = block_sum(in_forest, s_forest);
    if (threadIdx.x == 0) {
        if (n_edges) atomicAdd(counts, static_cast<unsigned long long>(n_edges));
        if (n_forest) atomicAdd(counts + 1, static_cast<unsigned long long>(n_forest));
    }
}

// The two calls of the split behind both pairs of entry points: `protect` NULL = the per-node
// minimum rule, else the caller's flags.
int count_impl(const char *who, const int64_t *row_ptr, const int32_t *col, int64_t n_rows,
               int64_t nnz, uint64_t seed, const uint8_t *protect, int64_t *counts,
               int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    int rc = check_sizes(who, n_rows, nnz);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(row_ptr && (col || nnz == 0) && counts && status && workspace,
               "%s: null pointer", who);
    Arena a{static_cast<char *>(workspace)};
    Bufs p;
    rc = plan(a, n_rows, nnz, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off && reinterpret_cast<uintptr_t>(workspace) % 256 == 0,
               "%s: workspace too small or misaligned (%zu < %zu)", who, workspace_bytes, a.off);
    hipStream_t st = dw::as_stream(stream);
    const uint64_t mseed = mix64(seed);
    DW_HIP_OK(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st), who);
    hipLaunchKernelGGL(k_fill, dim3(grid_of(n_rows)), dim3(256), 0, st, p.minp, n_rows, NO_PRIO);
    DW_LAUNCH_CHECK(who);
    if (nnz == 0) return DW_OK;
    hipLaunchKernelGGL(k_min_prio, dim3(grid_of(nnz)), dim3(256), 0, st, row_ptr, col, n_rows, nnz,
                       mseed, p.rows, p.minp, status);
    DW_LAUNCH_CHECK(who);
    const dim3 tiles(static_cast<unsigned>((nnz + CAND_TILE - 1) / CAND_TILE));
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counts);
    if (protect)
        hipLaunchKernelGGL(k_candidates<ByFlag>, tiles, dim3(256), 0, st, col, p.rows, n_rows, nnz,
                           mseed, ByFlag{protect}, p.cand0, cnt);
    else
        hipLaunchKernelGGL(k_candidates<ByMinimum>, tiles, dim3(256), 0, st, col, p.rows, n_rows,
                           nnz, mseed, ByMinimum{p.minp}, p.cand0, cnt);
    DW_LAUNCH_CHECK(who);
    return DW_OK;
}

int split_impl(const char *who, const int64_t *row_ptr, const int32_t *col, const double *weights,
               int64_t n_rows, int64_t nnz, uint64_t seed, const uint8_t *protect,
               int64_t n_candidates, int64_t n_hold, int64_t *row_ptr_out, int32_t *col_out,
               double *weights_out, int64_t *held, int32_t *status, void *workspace,
               size_t workspace_bytes, void *stream) {
    int rc = check_sizes(who, n_rows, nnz);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(n_candidates >= 0 && 2 * n_candidates <= nnz && n_hold >= 0 &&
                   n_hold <= n_candidates,
               "%s: need 0 <= n_hold <= n_candidates <= nnz / 2 (got %lld, %lld)", who,
               static_cast<long long>(n_hold), static_cast<long long>(n_candidates));
    DW_REQUIRE(row_ptr && row_ptr_out && status && workspace &&
                   (nnz == 0 || (col && col_out)) && (!weights || weights_out) &&
                   (n_hold == 0 || held),
               "%s: null pointer", who);
    Arena a{static_cast<char *>(workspace)};
    Bufs p;
    rc = plan(a, n_rows, nnz, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off && reinterpret_cast<uintptr_t>(workspace) % 256 == 0,
               "%s: workspace too small or misaligned (%zu < %zu)", who, workspace_bytes, a.off);
    hipStream_t st = dw::as_stream(stream);
    const uint64_t mseed = mix64(seed);
    const int64_t nnz_out = nnz - 2 * n_hold;

    const uint64_t *threshold = nullptr;
    if (n_hold > 0) {   // T = the n_hold-th smallest candidate priority
        rocprim::double_buffer<uint64_t> kb(p.cand0, p.cand1);
        size_t tmp_bytes = 0;   // (the plan sized the storage for nnz keys: check this count's)
        DW_HIP_OK(rocprim::radix_sort_keys(nullptr, tmp_bytes, kb,
                                           static_cast<size_t>(n_candidates), 0, 64, st),
                  who);
        DW_REQUIRE(tmp_bytes <= p.tmp_bytes, "%s: sort storage %zu > planned %zu", who, tmp_bytes,
                   p.tmp_bytes);
        tmp_bytes = p.tmp_bytes;
        DW_HIP_OK(rocprim::radix_sort_keys(p.tmp, tmp_bytes, kb, static_cast<size_t>(n_candidates),
                                           0, 64, st),
                  who);
        threshold = kb.current() + (n_hold - 1);
    }
    if (protect)
        hipLaunchKernelGGL(k_flags<ByFlag>, dim3(grid_of(nnz + 1)), dim3(256), 0, st, col, p.rows,
                           n_rows, nnz, mseed, ByFlag{protect}, threshold, p.flags);
    else
        hipLaunchKernelGGL(k_flags<ByMinimum>, dim3(grid_of(nnz + 1)), dim3(256), 0, st, col,
                           p.rows, n_rows, nnz, mseed, ByMinimum{p.minp}, threshold, p.flags);
    DW_LAUNCH_CHECK(who);
    size_t tmp_bytes = p.tmp_bytes;
    DW_HIP_OK(rocprim::exclusive_scan(p.tmp, tmp_bytes, static_cast<const uint64_t *>(p.flags),
                                      p.scan, uint64_t(0), static_cast<size_t>(nnz + 1),
                                      rocprim::plus<uint64_t>(), st),
              who);
    if (nnz > 0) {
        hipLaunchKernelGGL(k_write, dim3(grid_of(nnz)), dim3(256), 0, st, col, weights, p.rows, nnz,
                           p.flags, p.scan, nnz_out, n_hold, col_out, weights_out, held, status);
        DW_LAUNCH_CHECK(who);
    }
    hipLaunchKernelGGL(k_row_ptr, dim3(grid_of(n_rows + 1)), dim3(256), 0, st, row_ptr, n_rows, nnz,
                       p.scan, nnz_out, n_hold, row_ptr_out, status);
    DW_LAUNCH_CHECK(who);
    return DW_OK;
}

}  // namespace

extern "C" {

int dw_edge_forest_workspace_bytes(int64_t n_rows, int64_t nnz, size_t *bytes) {
    int rc = check_sizes("dw_edge_forest_workspace_bytes", n_rows, nnz);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(bytes, "dw_edge_forest_workspace_bytes: null pointer");
    Arena a{nullptr};
    ForestBufs p;
    forest_plan(a, n_rows, nnz, &p);
    *bytes = a.off;
    return DW_OK;
}

int dw_edge_forest(const int64_t *row_ptr, const int32_t *col, int64_t n_rows, int64_t nnz,
                   uint64_t seed, uint8_t *forest, int32_t *component, int64_t *counts,
                   int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    int rc = check_sizes("dw_edge_forest", n_rows, nnz);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(row_ptr && (nnz == 0 || (col && forest)) && component && counts && status &&
                   workspace,
               "dw_edge_forest: null pointer");
    Arena a{static_cast<char *>(workspace)};
    ForestBufs p;
    forest_plan(a, n_rows, nnz, &p);
    DW_REQUIRE(workspace_bytes >= a.off && reinterpret_cast<uintptr_t>(workspace) % 256 == 0,
               "dw_edge_forest: workspace too small or misaligned (%zu < %zu)", workspace_bytes,
               a.off);
    hipStream_t st = dw::as_stream(stream);
    const uint64_t mseed = mix64(seed);
    const int max_rounds = forest_rounds(n_rows);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counts);
    DW_HIP_OK(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st), "dw_edge_forest: memset");
    const int64_t n_init = n_rows > max_rounds + 1 ? n_rows : max_rounds + 1;
    hipLaunchKernelGGL(k_forest_init, dim3(grid_of(n_init)), dim3(256), 0, st, n_rows,
                       max_rounds + 1, p.comp, p.parent, p.minid, p.best, p.ctrl);
    DW_LAUNCH_CHECK("dw_edge_forest/init");
    if (nnz > 0) {
        DW_HIP_OK(hipMemsetAsync(forest, 0, static_cast<size_t>(nnz), st),
                  "dw_edge_forest: memset");
        const dim3 per_entry(grid_of(nnz)), per_row(grid_of(n_rows));
        hipLaunchKernelGGL(k_forest_rows, per_entry, dim3(256), 0, st, row_ptr, col, n_rows, nnz,
                           p.rows, status);
        DW_LAUNCH_CHECK("dw_edge_forest/rows");
        for (int r = 0; r < max_rounds; ++r) {
            hipLaunchKernelGGL(k_comp_min, per_entry, dim3(256), 0, st, col, p.rows, n_rows, nnz,
                               mseed, p.comp, p.ctrl + r, p.best);
            hipLaunchKernelGGL(k_hook, per_entry, dim3(256), 0, st, col, p.rows, n_rows, nnz,
                               mseed, p.comp, p.best, p.ctrl + r, p.parent, forest,
                               p.ctrl + r + 1, status);
            hipLaunchKernelGGL(k_compress, per_row, dim3(256), 0, st, n_rows, p.parent,
                               p.ctrl + r + 1, p.comp, p.best);
            DW_LAUNCH_CHECK("dw_edge_forest/round");
        }
        hipLaunchKernelGGL(k_forest_count,
                           dim3(static_cast<unsigned>((nnz + CAND_TILE - 1) / CAND_TILE)),
                           dim3(256), 0, st, col, p.rows, n_rows, nnz, forest, cnt);
        DW_LAUNCH_CHECK("dw_edge_forest/count");
    }
    hipLaunchKernelGGL(k_comp_minid, dim3(grid_of(n_rows)), dim3(256), 0, st, n_rows, p.comp,
                       p.minid);
    hipLaunchKernelGGL(k_forest_labels, dim3(grid_of(n_rows)), dim3(256), 0, st, row_ptr, col,
                       n_rows, nnz, p.comp, p.minid, p.ctrl, max_rounds, component, cnt, status);
    DW_LAUNCH_CHECK("dw_edge_forest/labels");
    return DW_OK;
}

int dw_edge_holdout_workspace_bytes(int64_t n_rows, int64_t nnz, size_t *bytes) {
    int rc = check_sizes("dw_edge_holdout_workspace_bytes", n_rows, nnz);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(bytes, "dw_edge_holdout_workspace_bytes: null pointer");
    Arena a{nullptr};
    Bufs p;
    rc = plan(a, n_rows, nnz, &p);
    if (rc != DW_OK) return rc;
    *bytes = a.off;
    return DW_OK;
}

int dw_edge_holdout_count(const int64_t *row_ptr, const int32_t *col, int64_t n_rows, int64_t nnz,
                          uint64_t seed, int64_t *counts, int32_t *status, void *workspace,
                          size_t workspace_bytes, void *stream) {
    return count_impl("dw_edge_holdout_count", row_ptr, col, n_rows, nnz, seed, nullptr, counts,
                      status, workspace, workspace_bytes, stream);
}

int dw_edge_holdout(const int64_t *row_ptr, const int32_t *col, const double *weights,
                    int64_t n_rows, int64_t nnz, uint64_t seed, int64_t n_candidates,
                    int64_t n_hold, int64_t *row_ptr_out, int32_t *col_out, double *weights_out,
                    int64_t *held, int32_t *status, void *workspace, size_t workspace_bytes,
                    void *stream) {
    return split_impl("dw_edge_holdout", row_ptr, col, weights, n_rows, nnz, seed, nullptr,
                      n_candidates, n_hold, row_ptr_out, col_out, weights_out, held, status,
                      workspace, workspace_bytes, stream);
}

int dw_edge_holdout_count_protected(const int64_t *row_ptr, const int32_t *col, int64_t n_rows,
                                    int64_t nnz, uint64_t seed, const uint8_t *protect,
                                    int64_t *counts, int32_t *status, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    DW_REQUIRE(protect, "dw_edge_holdout_count_protected: null pointer");
    return count_impl("dw_edge_holdout_count_protected", row_ptr, col, n_rows, nnz, seed, protect,
                      counts, status, workspace, workspace_bytes, stream);
}

int dw_edge_holdout_protected(const int64_t *row_ptr, const int32_t *col, const double *weights,
                              int64_t n_rows, int64_t nnz, uint64_t seed, const uint8_t *protect,
                              int64_t n_candidates, int64_t n_hold, int64_t *row_ptr_out,
                              int32_t *col_out, double *weights_out, int64_t *held,
                              int32_t *status, void *workspace, size_t workspace_bytes,
                              void *stream) {
    DW_REQUIRE(protect, "dw_edge_holdout_protected: null pointer");
    return split_impl("dw_edge_holdout_protected", row_ptr, col, weights, n_rows, nnz, seed,
                      protect, n_candidates, n_hold, row_ptr_out, col_out, weights_out, held,
                      status, workspace, workspace_bytes, stream);
}

}  // extern "C"
