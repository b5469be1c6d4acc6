// Graph ingestion on gfx950: R-MAT edge lists and CSR built in HBM.
//
// Follows the generator spec of shallow_encoders/graph/rmat.py bit for bit:
//   * the uniforms are numpy's default_rng(seed).random() stream — PCG64 (128-bit LCG,
//     XSL-RR output, double = (x >> 11) * 2^-53) — level-major: draw l * n_edges + e is the
//     level-l uniform of edge e. The host hands over the 128-bit state before each level's
//     first draw and a 2^i jump table, so every thread jumps straight to its edges;
//   * src |= (r >= a+b), dst |= (a <= r < a+b) | (r >= a+b+c) at bit (scale-1-level);
//   * self-loops dropped, undirected duplicates removed keeping the FIRST draw (stable radix
//     sort of (min, max) keys carrying the draw index, the first of every run kept, then a
//     stream compaction in draw order);
//   * isolated nodes listed in increasing order (the host draws their patch edges from the
//     same numpy stream, advanced past the edge draws);
//   * CSR rows in edge-list order — what networkx's add_edges_from gives: each edge (u, v)
//     contributes u->v then v->u, stably sorted by source; column ids are vocabulary ids
//     (node + 1), row 0 is <unk>.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "dw_common.h"
#include "dw_ingest.h"

namespace {

struct U128 {
    uint64_t lo, hi;
};

__device__ __forceinline__ U128 mul128(U128 a, U128 b) {
    return U128{a.lo * b.lo, __umul64hi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo};
}

__device__ __forceinline__ U128 add128(U128 a, U128 b) {
    const uint64_t lo = a.lo + b.lo;
    return U128{lo, a.hi + b.hi + (lo < a.lo ? 1ull : 0ull)};
}

constexpr uint64_t PCG_MULT_LO = 0x4385DF649FCCF645ull;  // 0x2360ED051FC65DA4_4385DF649FCCF645
constexpr uint64_t PCG_MULT_HI = 0x2360ED051FC65DA4ull;

// numpy PCG64: state = state * M + inc, then the XSL-RR output of the NEW state.
__device__ __forceinline__ double pcg64_next_double(U128 &s, U128 inc) {
    s = add128(mul128(s, U128{PCG_MULT_LO, PCG_MULT_HI}), inc);
    const uint64_t x = s.hi ^ s.lo;
    const unsigned r = static_cast<unsigned>(s.hi >> 58);
    const uint64_t out = (x >> r) | (x << ((64u - r) & 63u));
    return static_cast<double>(out >> 11) * 0x1.0p-53;
}

constexpr int RMAT_EDGES_PER_THREAD = 16;

// One thread = RMAT_EDGES_PER_THREAD consecutive edges, all levels; per level one jump from
// the level's base state (<= log2(n_edges) table steps) then sequential draws.
__global__ void __launch_bounds__(256)
    k_rmat_draw(int32_t scale, int64_t n, const uint64_t *__restrict__ level_state,
                const uint64_t *__restrict__ jump, U128 inc, double t1, double t2, double t3,
                uint64_t *__restrict__ edges) {
    const int64_t e0 =
        (blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) * RMAT_EDGES_PER_THREAD;
    if (e0 >= n) return;
    uint32_t src[RMAT_EDGES_PER_THREAD], dst[RMAT_EDGES_PER_THREAD];
#pragma unroll
    for (int j = 0; j < RMAT_EDGES_PER_THREAD; ++j) src[j] = dst[j] = 0u;
    for (int l = 0; l < scale; ++l) {
        U128 s{level_state[2 * l], level_state[2 * l + 1]};
        uint64_t k = static_cast<uint64_t>(e0);
        for (int i = 0; k != 0; ++i, k >>= 1)
            if (k & 1ull)
                s = add128(mul128(s, U128{jump[4 * i], jump[4 * i + 1]}),
                           U128{jump[4 * i + 2], jump[4 * i + 3]});
        const uint32_t bit = 1u << (scale - 1 - l);
#pragma unroll
        for (int j = 0; j < RMAT_EDGES_PER_THREAD; ++j) {
            if (e0 + j < n) {
                const double r = pcg64_next_double(s, inc);
                if (r >= t2) src[j] |= bit;
                if ((r >= t1 && r < t2) || r >= t3) dst[j] |= bit;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < RMAT_EDGES_PER_THREAD; ++j)
        if (e0 + j < n) edges[e0 + j] = (static_cast<uint64_t>(src[j]) << 32) | dst[j];
}

__global__ void __launch_bounds__(256)
    k_rmat_keys(const uint64_t *__restrict__ edges, int64_t n, int32_t scale,
                uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const uint64_t e = edges[i];
    const uint64_t u = e >> 32, v = e & 0xFFFFFFFFull;
    keys[i] = u == v ? (1ull << (2 * scale))  // self-loop: sorts last, never kept
                     : ((u < v ? u : v) << scale) | (u < v ? v : u);
    idx[i] = static_cast<uint32_t>(i);
}

// keep[draw] = 1 for the first draw of every distinct undirected edge (runs of equal keys are
// in draw order: the radix sort is stable).
__global__ void __launch_bounds__(256)
    k_rmat_first(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, int64_t n,
                 uint64_t invalid, uint8_t *__restrict__ keep) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    keep[idx[i]] = (k != invalid && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
    k_zero_flags(const uint32_t *__restrict__ deg, int64_t n, uint8_t *__restrict__ flag) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i < n) flag[i] = deg[i] == 0u ? 1 : 0;
}

// Directed CSR entries: edge i -> (u -> v+1) at 2i and (v -> u+1) at 2i+1.
__global__ void __launch_bounds__(256)
    k_csr_entries(const uint64_t *__restrict__ edges, int64_t m, uint32_t *__restrict__ keys,
                  uint32_t *__restrict__ vals) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= m) return;
    const uint64_t e = edges[i];
    const uint32_t u = static_cast<uint32_t>(e >> 32), v = static_cast<uint32_t>(e);
    keys[2 * i] = u;
    vals[2 * i] = v + 1u;
    keys[2 * i + 1] = v;
    vals[2 * i + 1] = u + 1u;
}

using dw::ingest::Arena;   // (shared with dw_edgelist.hip: dw_ingest.h)
using dw::ingest::bits_for;
using dw::ingest::grid_of;
using dw::ingest::k_degree;
using dw::ingest::k_row_ptr_head;

// ---- workspace plans (one size serves the three calls) ----------------------------------------
struct RmatBufs {
    uint64_t *raw, *keys0, *keys1;
    uint32_t *idx0, *idx1;
    uint8_t *keep;
    char *sort_tmp, *sel_tmp;
    size_t sort_tmp_bytes, sel_tmp_bytes;
};

int plan_rmat(Arena &a, int32_t scale, int64_t n, RmatBufs *p) {
    rocprim::double_buffer<uint64_t> kb(nullptr, nullptr);
    rocprim::double_buffer<uint32_t> vb(nullptr, nullptr);
    DW_HIP_OK(rocprim::radix_sort_pairs(nullptr, p->sort_tmp_bytes, kb, vb,
                                        static_cast<uint32_t>(n), 0,
                                        2 * scale + 1),
              "dw_rmat: sort size query");
    DW_HIP_OK(rocprim::select(nullptr, p->sel_tmp_bytes, static_cast<const uint64_t *>(nullptr),
                              static_cast<const uint8_t *>(nullptr),
                              static_cast<uint64_t *>(nullptr), static_cast<int64_t *>(nullptr),
                              static_cast<size_t>(n)),
              "dw_rmat: select size query");
    p->raw = a.take<uint64_t>(n);
    p->keys0 = a.take<uint64_t>(n);
    p->keys1 = a.take<uint64_t>(n);
    p->idx0 = a.take<uint32_t>(n);
    p->idx1 = a.take<uint32_t>(n);
    p->keep = a.take<uint8_t>(n);
    p->sort_tmp = a.take<char>(p->sort_tmp_bytes);
    p->sel_tmp = a.take<char>(p->sel_tmp_bytes);
    return DW_OK;
}

struct CsrBufs {
    uint32_t *keys0, *keys1, *vals0, *vals1, *deg;
    uint8_t *flags;
    char *sort_tmp, *scan_tmp, *sel_tmp;
    size_t sort_tmp_bytes, scan_tmp_bytes, sel_tmp_bytes;
};

int plan_csr(Arena &a, int64_t m, int64_t n_nodes, CsrBufs *p) {
    const int64_t nnz = 2 * m;
    rocprim::double_buffer<uint32_t> kb(nullptr, nullptr), vb(nullptr, nullptr);
    DW_HIP_OK(rocprim::radix_sort_pairs(nullptr, p->sort_tmp_bytes, kb, vb,
                                        static_cast<uint32_t>(nnz > 0 ? nnz : 1), 0,
                                        bits_for(n_nodes)),
              "dw_csr_from_edges: sort size query");
    DW_HIP_OK(rocprim::inclusive_scan(nullptr, p->scan_tmp_bytes,
                                      static_cast<const uint32_t *>(nullptr),
                                      static_cast<int64_t *>(nullptr),
                                      static_cast<size_t>(n_nodes), rocprim::plus<int64_t>()),
              "dw_csr_from_edges: scan size query");
    DW_HIP_OK(rocprim::select(nullptr, p->sel_tmp_bytes, rocprim::counting_iterator<int32_t>(0),
                              static_cast<const uint8_t *>(nullptr),
                              static_cast<int32_t *>(nullptr), static_cast<int64_t *>(nullptr),
                              static_cast<size_t>(n_nodes)),
              "dw_graph_isolated: select size query");
    p->keys0 = a.take<uint32_t>(nnz);
    p->keys1 = a.take<uint32_t>(nnz);
    p->vals0 = a.take<uint32_t>(nnz);
    p->vals1 = a.take<uint32_t>(nnz);
    p->deg = a.take<uint32_t>(n_nodes);
    p->flags = a.take<uint8_t>(n_nodes);
    p->sort_tmp = a.take<char>(p->sort_tmp_bytes);
    p->scan_tmp = a.take<char>(p->scan_tmp_bytes);
    p->sel_tmp = a.take<char>(p->sel_tmp_bytes);
    return DW_OK;
}

}  // namespace

extern "C" {

int dw_ingest_workspace_bytes(int32_t scale, int64_t n_edges, int64_t n_nodes, size_t *bytes) {
    DW_REQUIRE(bytes && scale >= 1 && scale <= 31 && n_edges >= 0 && n_nodes >= 1,
               "dw_ingest_workspace_bytes: bad arguments");
    DW_REQUIRE(n_edges < (int64_t(1) << 31) && n_nodes < (int64_t(1) << 31),
               "dw_ingest_workspace_bytes: sizes must fit int32");
    Arena ra{nullptr}, ca{nullptr};
    RmatBufs r;
    CsrBufs c;
    int rc = plan_rmat(ra, scale, n_edges > 0 ? n_edges : 1, &r);
    if (rc != DW_OK) return rc;
    rc = plan_csr(ca, n_edges > 0 ? n_edges : 1, n_nodes, &c);
    if (rc != DW_OK) return rc;
    *bytes = ra.off > ca.off ? ra.off : ca.off;
    return DW_OK;
}

int dw_rmat_edges(int32_t scale, int64_t n_edges, const uint64_t *level_state,
                  const uint64_t *jump, uint64_t inc_lo, uint64_t inc_hi, double t1, double t2,
                  double t3, uint64_t *edges, int64_t *n_unique, void *workspace,
                  size_t workspace_bytes, void *stream) {
    DW_REQUIRE(scale >= 1 && scale <= 31 && n_edges >= 1 && n_edges < (int64_t(1) << 31),
               "dw_rmat_edges: bad sizes");
    DW_REQUIRE(level_state && jump && edges && n_unique && workspace,
               "dw_rmat_edges: null pointer");
    Arena a{static_cast<char *>(workspace)};
    RmatBufs p;
    int rc = plan_rmat(a, scale, n_edges, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off, "dw_rmat_edges: workspace too small (%zu < %zu)",
               workspace_bytes, a.off);
    hipStream_t st = dw::as_stream(stream);
    const int64_t n_threads = (n_edges + RMAT_EDGES_PER_THREAD - 1) / RMAT_EDGES_PER_THREAD;
    hipLaunchKernelGGL(k_rmat_draw, dim3(grid_of(n_threads)), dim3(256), 0, st, scale, n_edges,
                       level_state, jump, U128{inc_lo, inc_hi}, t1, t2, t3, p.raw);
    DW_LAUNCH_CHECK("dw_rmat_edges/draw");
    hipLaunchKernelGGL(k_rmat_keys, dim3(grid_of(n_edges)), dim3(256), 0, st, p.raw, n_edges,
                       scale, p.keys0, p.idx0);
    DW_LAUNCH_CHECK("dw_rmat_edges/keys");
    rocprim::double_buffer<uint64_t> kb(p.keys0, p.keys1);
    rocprim::double_buffer<uint32_t> vb(p.idx0, p.idx1);
    DW_HIP_OK(rocprim::radix_sort_pairs(p.sort_tmp, p.sort_tmp_bytes, kb, vb,
                                        static_cast<uint32_t>(n_edges), 0, 2 * scale + 1, st),
              "dw_rmat_edges: sort");
    hipLaunchKernelGGL(k_rmat_first, dim3(grid_of(n_edges)), dim3(256), 0, st, kb.current(),
                       vb.current(), n_edges, 1ull << (2 * scale), p.keep);
    DW_LAUNCH_CHECK("dw_rmat_edges/first");
    DW_HIP_OK(rocprim::select(p.sel_tmp, p.sel_tmp_bytes, static_cast<const uint64_t *>(p.raw),
                              static_cast<const uint8_t *>(p.keep), edges, n_unique,
                              static_cast<size_t>(n_edges), st),
              "dw_rmat_edges: compaction");
    return DW_OK;
}

int dw_graph_isolated(const uint64_t *edges, int64_t n_edges, int64_t n_nodes,
                      int32_t *isolated, int64_t *n_isolated, int32_t *status, void *workspace,
                      size_t workspace_bytes, void *stream) {
    DW_REQUIRE(n_edges >= 0 && n_nodes >= 1 && n_nodes < (int64_t(1) << 31),
               "dw_graph_isolated: bad sizes");
    DW_REQUIRE(isolated && n_isolated && status && workspace && (edges || n_edges == 0),
               "dw_graph_isolated: null pointer");
    Arena a{static_cast<char *>(workspace)};
    CsrBufs p;
    int rc = plan_csr(a, n_edges > 0 ? n_edges : 1, n_nodes, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off, "dw_graph_isolated: workspace too small");
    hipStream_t st = dw::as_stream(stream);
    DW_HIP_OK(hipMemsetAsync(p.deg, 0, n_nodes * 4, st), "dw_graph_isolated: memset");
    if (n_edges > 0) {
        hipLaunchKernelGGL(k_degree<false>, dim3(grid_of(n_edges)), dim3(256), 0, st, edges,
                           n_edges, n_nodes, p.deg, status);
        DW_LAUNCH_CHECK("dw_graph_isolated/degree");
    }
    hipLaunchKernelGGL(k_zero_flags, dim3(grid_of(n_nodes)), dim3(256), 0, st, p.deg, n_nodes,
                       p.flags);
    DW_LAUNCH_CHECK("dw_graph_isolated/flags");
    DW_HIP_OK(rocprim::select(p.sel_tmp, p.sel_tmp_bytes, rocprim::counting_iterator<int32_t>(0),
                              static_cast<const uint8_t *>(p.flags), isolated, n_isolated,
                              static_cast<size_t>(n_nodes), st),
              "dw_graph_isolated: compaction");
    return DW_OK;
}

int dw_csr_from_edges(const uint64_t *edges, int64_t n_edges, int64_t n_nodes,
                      int64_t *row_ptr, int32_t *col, int32_t *status, void *workspace,
                      size_t workspace_bytes, void *stream) {
    DW_REQUIRE(n_edges >= 0 && n_nodes >= 1 && n_nodes < (int64_t(1) << 31) &&
                   2 * n_edges < (int64_t(1) << 31),
               "dw_csr_from_edges: bad sizes");
    DW_REQUIRE(row_ptr && status && workspace && (n_edges == 0 || (edges && col)),
               "dw_csr_from_edges: null pointer");
    Arena a{static_cast<char *>(workspace)};
    CsrBufs p;
    int rc = plan_csr(a, n_edges > 0 ? n_edges : 1, n_nodes, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off, "dw_csr_from_edges: workspace too small");
    hipStream_t st = dw::as_stream(stream);
    DW_HIP_OK(hipMemsetAsync(p.deg, 0, n_nodes * 4, st), "dw_csr_from_edges: memset");
    hipLaunchKernelGGL(k_row_ptr_head, dim3(1), dim3(1), 0, st, row_ptr);
    DW_LAUNCH_CHECK("dw_csr_from_edges/head");
    if (n_edges > 0) {
        hipLaunchKernelGGL(k_degree<false>, dim3(grid_of(n_edges)), dim3(256), 0, st, edges,
                           n_edges, n_nodes, p.deg, status);
        DW_LAUNCH_CHECK("dw_csr_from_edges/degree");
        const int64_t nnz = 2 * n_edges;
        hipLaunchKernelGGL(k_csr_entries, dim3(grid_of(n_edges)), dim3(256), 0, st, edges,
                           n_edges, p.keys0, p.vals0);
        DW_LAUNCH_CHECK("dw_csr_from_edges/entries");
        rocprim::double_buffer<uint32_t> kb(p.keys0, p.keys1), vb(p.vals0, p.vals1);
        DW_HIP_OK(rocprim::radix_sort_pairs(p.sort_tmp, p.sort_tmp_bytes, kb, vb,
                                            static_cast<uint32_t>(nnz), 0, bits_for(n_nodes),
                                            st),
                  "dw_csr_from_edges: sort");
        DW_HIP_OK(hipMemcpyAsync(col, vb.current(), nnz * 4, hipMemcpyDeviceToDevice, st),
                  "dw_csr_from_edges: copy");
    }
    DW_HIP_OK(rocprim::inclusive_scan(p.scan_tmp, p.scan_tmp_bytes,
                                      static_cast<const uint32_t *>(p.deg), row_ptr + 2,
                                      static_cast<size_t>(n_nodes), rocprim::plus<int64_t>(), st),
              "dw_csr_from_edges: scan");
    return DW_OK;
}

}  // extern "C"
