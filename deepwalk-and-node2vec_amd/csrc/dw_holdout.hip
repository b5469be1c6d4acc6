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
        int64_t lo = 0, hi = n_rows - 1;   // the answer lies in [0, n_rows - 1]
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (row_ptr[mid + 1] > e)
                hi = mid;
            else
                lo = mid + 1;
        }
        row = static_cast<int32_t>(lo);
        rows[e] = row;
        const int64_t x = lo, y = col[e];
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

__global__ void __launch_bounds__(256)
    k_candidates(const int32_t *__restrict__ col, const int32_t *__restrict__ rows,
                 int64_t n_rows, int64_t nnz, uint64_t mseed, const uint64_t *__restrict__ minp,
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
                if (p[k] != minp[x] && p[k] != minp[y]) mask |= 1u << k;
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
__global__ void __launch_bounds__(256)
    k_flags(const int32_t *__restrict__ col, const int32_t *__restrict__ rows, int64_t n_rows,
            int64_t nnz, uint64_t mseed, const uint64_t *__restrict__ minp,
            const uint64_t *__restrict__ threshold, uint64_t *__restrict__ flags) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (e > nnz) return;
    uint64_t f = 0;
    if (e < nnz) {
        f = 1;
        const int64_t x = rows[e], y = col[e];
        if (threshold && entry_ok(x, y, n_rows) && x != y) {
            const uint64_t p = edge_prio(x, y, mseed);
            if (p != minp[x] && p != minp[y] && p <= *threshold)
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

}  // namespace

extern "C" {

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
    int rc = check_sizes("dw_edge_holdout_count", n_rows, nnz);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(row_ptr && (col || nnz == 0) && counts && status && workspace,
               "dw_edge_holdout_count: null pointer");
    Arena a{static_cast<char *>(workspace)};
    Bufs p;
    rc = plan(a, n_rows, nnz, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off && reinterpret_cast<uintptr_t>(workspace) % 256 == 0,
               "dw_edge_holdout_count: workspace too small or misaligned (%zu < %zu)",
               workspace_bytes, a.off);
    hipStream_t st = dw::as_stream(stream);
    const uint64_t mseed = mix64(seed);
    DW_HIP_OK(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st), "dw_edge_holdout_count: memset");
    hipLaunchKernelGGL(k_fill, dim3(grid_of(n_rows)), dim3(256), 0, st, p.minp, n_rows, NO_PRIO);
    DW_LAUNCH_CHECK("dw_edge_holdout_count/fill");
    if (nnz == 0) return DW_OK;
    hipLaunchKernelGGL(k_min_prio, dim3(grid_of(nnz)), dim3(256), 0, st, row_ptr, col, n_rows, nnz,
                       mseed, p.rows, p.minp, status);
    DW_LAUNCH_CHECK("dw_edge_holdout_count/min");
    hipLaunchKernelGGL(k_candidates, dim3(static_cast<unsigned>((nnz + CAND_TILE - 1) / CAND_TILE)),
                       dim3(256), 0, st, col, p.rows, n_rows,
                       nnz, mseed, p.minp, p.cand0,
                       reinterpret_cast<unsigned long long *>(counts));
    DW_LAUNCH_CHECK("dw_edge_holdout_count/candidates");
    return DW_OK;
}

int dw_edge_holdout(const int64_t *row_ptr, const int32_t *col, const double *weights,
                    int64_t n_rows, int64_t nnz, uint64_t seed, int64_t n_candidates,
                    int64_t n_hold, int64_t *row_ptr_out, int32_t *col_out, double *weights_out,
                    int64_t *held, int32_t *status, void *workspace, size_t workspace_bytes,
                    void *stream) {
    int rc = check_sizes("dw_edge_holdout", n_rows, nnz);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(n_candidates >= 0 && 2 * n_candidates <= nnz && n_hold >= 0 &&
                   n_hold <= n_candidates,
               "dw_edge_holdout: need 0 <= n_hold <= n_candidates <= nnz / 2 (got %lld, %lld)",
               static_cast<long long>(n_hold), static_cast<long long>(n_candidates));
    DW_REQUIRE(row_ptr && row_ptr_out && status && workspace &&
                   (nnz == 0 || (col && col_out)) && (!weights || weights_out) &&
                   (n_hold == 0 || held),
               "dw_edge_holdout: null pointer");
    Arena a{static_cast<char *>(workspace)};
    Bufs p;
    rc = plan(a, n_rows, nnz, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off && reinterpret_cast<uintptr_t>(workspace) % 256 == 0,
               "dw_edge_holdout: workspace too small or misaligned (%zu < %zu)", workspace_bytes,
               a.off);
    hipStream_t st = dw::as_stream(stream);
    const uint64_t mseed = mix64(seed);
    const int64_t nnz_out = nnz - 2 * n_hold;

    const uint64_t *threshold = nullptr;
    if (n_hold > 0) {   // T = the n_hold-th smallest candidate priority
        rocprim::double_buffer<uint64_t> kb(p.cand0, p.cand1);
        size_t tmp_bytes = 0;   // (the plan sized the storage for nnz keys: check this count's)
        DW_HIP_OK(rocprim::radix_sort_keys(nullptr, tmp_bytes, kb,
                                           static_cast<size_t>(n_candidates), 0, 64, st),
                  "dw_edge_holdout: candidate sort plan");
        DW_REQUIRE(tmp_bytes <= p.tmp_bytes, "dw_edge_holdout: sort storage %zu > planned %zu",
                   tmp_bytes, p.tmp_bytes);
        tmp_bytes = p.tmp_bytes;
        DW_HIP_OK(rocprim::radix_sort_keys(p.tmp, tmp_bytes, kb, static_cast<size_t>(n_candidates),
                                           0, 64, st),
                  "dw_edge_holdout: candidate sort");
        threshold = kb.current() + (n_hold - 1);
    }
    hipLaunchKernelGGL(k_flags, dim3(grid_of(nnz + 1)), dim3(256), 0, st, col, p.rows, n_rows, nnz,
                       mseed, p.minp, threshold, p.flags);
    DW_LAUNCH_CHECK("dw_edge_holdout/flags");
    size_t tmp_bytes = p.tmp_bytes;
    DW_HIP_OK(rocprim::exclusive_scan(p.tmp, tmp_bytes, static_cast<const uint64_t *>(p.flags),
                                      p.scan, uint64_t(0), static_cast<size_t>(nnz + 1),
                                      rocprim::plus<uint64_t>(), st),
              "dw_edge_holdout: scan");
    if (nnz > 0) {
        hipLaunchKernelGGL(k_write, dim3(grid_of(nnz)), dim3(256), 0, st, col, weights, p.rows, nnz,
                           p.flags, p.scan, nnz_out, n_hold, col_out, weights_out, held, status);
        DW_LAUNCH_CHECK("dw_edge_holdout/write");
    }
    hipLaunchKernelGGL(k_row_ptr, dim3(grid_of(n_rows + 1)), dim3(256), 0, st, row_ptr, n_rows, nnz,
                       p.scan, nnz_out, n_hold, row_ptr_out, status);
    DW_LAUNCH_CHECK("dw_edge_holdout/row_ptr");
    return DW_OK;
}

}  // extern "C"
