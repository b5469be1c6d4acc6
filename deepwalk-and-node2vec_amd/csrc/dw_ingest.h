// Host-side helpers shared by the graph-ingestion sources (dw_rmat.hip, dw_edgelist.hip): the
// workspace layout arithmetic and the HIP error check of their rocprim calls. Not part of the ABI.
#pragma once

#include "dw_common.h"

namespace dw {
namespace ingest {

inline size_t a256(size_t x) { return (x + 255) & ~size_t(255); }

inline int bits_for(int64_t n) {  // bits of values < n
    int b = 1;
    while (b < 63 && (static_cast<uint64_t>(n - 1) >> b) != 0) ++b;
    return b;
}

inline unsigned grid_of(int64_t n) { return static_cast<unsigned>((n + 255) / 256); }

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
