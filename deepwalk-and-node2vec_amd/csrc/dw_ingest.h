// Helpers shared by the graph-ingestion sources (dw_rmat.hip, dw_edgelist.hip): the HIP error
// check of their rocprim calls and the two kernels both CSR builders start with. Not part of the
// ABI.
#pragma once

#include "dw_common.h"

namespace dw {
namespace ingest {

using dw::Arena;   // the workspace arena (dw_common.h)

inline int bits_for(int64_t n) {  // bits of values < n
    int b = 1;
    while (b < 63 && (static_cast<uint64_t>(n - 1) >> b) != 0) ++b;
    return b;
}

inline unsigned grid_of(int64_t n) { return static_cast<unsigned>((n + 255) / 256); }

// row_ptr[0] = row_ptr[1] = 0: row 0 is <unk>; the degree scan fills row_ptr[2:].
static __global__ void k_row_ptr_head(int64_t *row_ptr) {
    row_ptr[0] = 0;
    row_ptr[1] = 0;
}

// Degree of every endpoint of the packed edges (u << 32 | v). LOOPS: a self-loop is one entry
// (dw_csr_from_edges_loops); without it the callers' edges hold none and both ends count.
template <bool LOOPS>
static __global__ void __launch_bounds__(256)
    k_degree(const uint64_t *__restrict__ edges, int64_t m, int64_t n_nodes,
             uint32_t *__restrict__ deg, int32_t *status) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= m) return;
    const uint64_t e = edges[i];
    const uint64_t u = e >> 32, v = e & 0xFFFFFFFFull;
    if (u >= static_cast<uint64_t>(n_nodes) || v >= static_cast<uint64_t>(n_nodes)) {
        dw::status_or(status, DW_S_BAD_CSR);
        return;
    }
    atomicAdd(deg + u, 1u);
    if (!LOOPS || u != v) atomicAdd(deg + v, 1u);
}

}  // namespace ingest
}  // namespace dw

#define DW_HIP_OK(expr, what)                                                       \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess) {                                                     \
            ::dw::set_error("%s: %s", what, hipGetErrorString(e_));                 \
            return DW_E_HIP;                                                        \
        }                                                                           \
    } while (0)
