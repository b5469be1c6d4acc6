// Edge-list ingestion on gfx950 (shallow_encoders/graph/edge_list.py): a
// user's edge list — text already in HBM, or two id arrays — to the CSR the walkers use, equal bit
// for bit to CSRGraph.from_networkx(nx.Graph().add_edges_from(...)) over zero-padded names.
//
//   dw_edgelist_parse        text -> src, dst int64 in file order
//   dw_edgelist_parse_weighted  "u v w" text -> src, dst, and float(w) bit for bit (float64)
//   dw_edges_canonical       raw ids -> sorted distinct ids, unique edges packed by rank (first
//                            occurrence kept, either orientation), their last-occurrence weights
//   dw_csr_from_edges_loops  packed edges -> CSR; a self-loop is one entry; weights by gather
//
// The two text entry points are one parser: parse_line<WEIGHTED> is the line grammar, k_parse<
// WEIGHTED, WRITE> the kernel and parse_text<WEIGHTED> the launcher; the id-only instantiations
// hold nothing of the weight token's scan and take none of its arguments.
//
// Every output is a pure function of the input: integer atomics only (degree counts, the
// smallest offending line), stable radix sorts, scans and selects — reruns are bit-identical.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include "dw_common.h"
#include "dw_ingest.h"
#include "dw_strtod.h"

namespace {

using dw::ingest::Arena;
using dw::ingest::bits_for;
using dw::ingest::grid_of;
using dw::ingest::k_degree;
using dw::ingest::k_row_ptr_head;

// ---- text ------------------------------------------------------------------------------------
// One lane owns PARSE_SEG consecutive bytes and parses every line that STARTS in them (reading
// on to the line's end, never past n_bytes). Lines are ~16 B, so a lane sees ~4 of them. A block
// first stages its 16 KiB of text (and PARSE_OVER bytes behind it, for lines that run on) in LDS
// with coalesced 16-byte loads, so the chunk is read from HBM once per pass in full lines; the
// lanes' byte reads then go to LDS, each 64-B segment padded by 4 B so that the lanes' segments
// fall on distinct banks. A line that runs past the staged bytes is read from memory directly.
// Three passes (count lines; count data lines + errors; write) with a scan between them keep
// file order without a per-byte or per-line array: the scratch is 24 B per segment.
constexpr int PARSE_SEG = 64;
constexpr int PARSE_BLOCK = 256;
constexpr int PARSE_STAGE = PARSE_BLOCK * PARSE_SEG;
constexpr int PARSE_OVER = 256;
constexpr int PARSE_LDS_BYTES = (PARSE_STAGE + PARSE_OVER) / PARSE_SEG * (PARSE_SEG + 4);

struct Text {
    const uint8_t *__restrict__ t;   // the chunk in memory, n bytes
    int64_t n;
    const uint8_t *lds;              // bytes [base, end) of it, staged (padded segments)
    int64_t base, end;
    __device__ __forceinline__ uint8_t operator[](int64_t q) const {
        if (q >= base && q < end) {
            const uint32_t o = static_cast<uint32_t>(q - base);
            return lds[o + (o >> 6) * 4u];
        }
        return t[q];
    }
};

// Stages the block's text; every thread of the block calls it (it ends in a barrier).
__device__ __forceinline__ Text stage_text(const uint8_t *__restrict__ t, int64_t n,
                                           uint32_t *stage) {
    uint8_t *lds = reinterpret_cast<uint8_t *>(stage);
    const int64_t base = blockIdx.x * static_cast<int64_t>(PARSE_STAGE);
    const int64_t end = base + PARSE_STAGE + PARSE_OVER < n ? base + PARSE_STAGE + PARSE_OVER : n;
    const uint32_t len = end > base ? static_cast<uint32_t>(end - base) : 0u;
    uint32_t done = 0;
    if ((reinterpret_cast<uintptr_t>(t) & 15u) == 0) {   // (base is a multiple of 16)
        done = len & ~15u;
        for (uint32_t o = threadIdx.x * 16u; o < done; o += PARSE_BLOCK * 16u) {
            const uint4 v = *reinterpret_cast<const uint4 *>(t + base + o);
            uint32_t *d = stage + ((o + (o >> 6) * 4u) >> 2);
            d[0] = v.x;
            d[1] = v.y;
            d[2] = v.z;
            d[3] = v.w;
        }
    }
    for (uint32_t o = done + threadIdx.x; o < len; o += PARSE_BLOCK)
        lds[o + (o >> 6) * 4u] = t[base + o];
    __syncthreads();
    return Text{t, n, lds, base, end};
}

__device__ __forceinline__ bool is_blank(uint8_t c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ bool is_sep(uint8_t c) { return c == ' ' || c == '\t' || c == ','; }
__device__ __forceinline__ bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// The line's content ends at q: the text's end, a '\n', or a '\r' that closes the line.
__device__ __forceinline__ bool at_eol(const Text &t, int64_t q) {
    if (q >= t.n) return true;
    const uint8_t c = t[q];
    return c == '\n' || (c == '\r' && (q + 1 >= t.n || t[q + 1] == '\n'));
}

// 1-18 digits at q (leading zeros allowed); false on none or a 19th.
__device__ __forceinline__ bool parse_id(const Text &t, int64_t &q, int64_t &value) {
    int nd = 0;
    int64_t v = 0;
    while (q < t.n) {
        const uint8_t c = t[q];
        if (!is_digit(c)) break;
        if (++nd > 18) return false;
        v = v * 10 + (c - '0');
        ++q;
    }
    value = v;
    return nd > 0;
}

enum { LINE_SKIP = 0, LINE_DATA = 1, LINE_BAD = 2 };

// A line's weight token (dw_strtod.h): where it starts, and its digits for the write pass to
// convert.
struct WeightToken {
    int64_t at;
    dw::strtod::Scan scan;
};

// The line grammar: blanks, a comment or the first id, separators, the second id; WEIGHTED:
// separators and a weight token of at most MAX_TOKEN bytes behind it (into w, untouched
// otherwise); then the line's end or a separator.
template <bool WEIGHTED>
__device__ __forceinline__ int parse_line(const Text &t, int64_t p, int64_t &a, int64_t &b,
                                          WeightToken &w) {
    int64_t q = p;
    while (q < t.n && is_blank(t[q])) ++q;
    if (at_eol(t, q)) return LINE_SKIP;
    const uint8_t c = t[q];
    if (c == '#' || c == '%') return LINE_SKIP;
    if (!parse_id(t, q, a)) return LINE_BAD;
    if (at_eol(t, q) || !is_sep(t[q])) return LINE_BAD;
    while (q < t.n && is_sep(t[q])) ++q;
    if (at_eol(t, q)) return LINE_BAD;
    if (!parse_id(t, q, b)) return LINE_BAD;
    if constexpr (WEIGHTED) {
        if (at_eol(t, q) || !is_sep(t[q])) return LINE_BAD;
        while (q < t.n && is_sep(t[q])) ++q;
        if (at_eol(t, q)) return LINE_BAD;   // no third field
        w.at = q;
        if (!dw::strtod::scan_token(t, t.n, q, &w.scan)) return LINE_BAD;
        if (q - w.at > dw::strtod::MAX_TOKEN) return LINE_BAD;
    }
    if (!at_eol(t, q) && !is_sep(t[q])) return LINE_BAD;
    return LINE_DATA;   // (the rest of the line is ignored)
}

__device__ __forceinline__ bool line_starts_at(const Text &t, int64_t p) {
    return p == 0 || t[p - 1] == '\n';
}

// Bit k: a line starts at lo + k. Found in one uniform loop, so that the lanes of a wave then
// parse their k-th lines together instead of each waiting for the others' line starts.
__device__ __forceinline__ uint64_t line_starts(const Text &t, int64_t lo, int64_t hi) {
    uint64_t m = 0;
    for (int k = 0; k < static_cast<int>(hi - lo); ++k)
        m |= line_starts_at(t, lo + k) ? (1ull << k) : 0ull;
    return m;
}

__global__ void __launch_bounds__(PARSE_BLOCK)
    k_count_lines(const uint8_t *__restrict__ text, int64_t n, int64_t n_seg,
                  uint32_t *__restrict__ cnt) {
    __shared__ uint32_t stage[PARSE_LDS_BYTES / 4];
    const Text t = stage_text(text, n, stage);
    const int64_t s = blockIdx.x * static_cast<int64_t>(PARSE_BLOCK) + threadIdx.x;
    if (s >= n_seg) return;
    const int64_t lo = s * PARSE_SEG;
    const int64_t hi = lo + PARSE_SEG < n ? lo + PARSE_SEG : n;
    cnt[s] = static_cast<uint32_t>(__popcll(line_starts(t, lo, hi)));
}

// Where the edges go. The weighted parser's extra arguments live in its own bundle, so the
// id-only kernels take (and keep in registers) nothing of them.
template <bool WEIGHTED>
struct ParseOut;

template <>
struct ParseOut<false> {
    int64_t *__restrict__ src, *__restrict__ dst;
    int64_t capacity;
};

template <>
struct ParseOut<true> {
    const uint64_t *__restrict__ pow5;   // dw_pow5_table, in HBM
    int64_t *__restrict__ src, *__restrict__ dst;
    double *__restrict__ weight;
    int64_t capacity;
    int64_t *__restrict__ undecided;     // (edge index, token offset) pairs
    int64_t undecided_capacity;
    unsigned long long *n_undecided;
};

// WRITE = false: data lines per segment, and the smallest bad line (WEIGHTED: the token's
// grammar is checked, nothing converted). WRITE = true: the edges; WEIGHTED: each token is
// converted too, and the tokens the conversion cannot decide go to the host: 0.0 in weight[] and
// (edge index, token offset) appended through an integer counter (counts[2]), so weight[] stays
// a pure function of the text and the list is one up to its order.
template <bool WEIGHTED, bool WRITE>
__global__ void __launch_bounds__(PARSE_BLOCK)
    k_parse(const uint8_t *__restrict__ text, int64_t n, int64_t n_seg,
            const int64_t *__restrict__ lines_incl, const uint32_t *__restrict__ lines_cnt,
            int64_t skip_lines, uint32_t *__restrict__ data_cnt,
            const int64_t *__restrict__ data_incl, ParseOut<WEIGHTED> o,
            unsigned long long *err_line, int32_t *status) {
    __shared__ uint32_t stage[PARSE_LDS_BYTES / 4];
    const Text t = stage_text(text, n, stage);
    const int64_t s = blockIdx.x * static_cast<int64_t>(PARSE_BLOCK) + threadIdx.x;
    if (s >= n_seg) return;
    const int64_t lo = s * PARSE_SEG;
    const int64_t hi = lo + PARSE_SEG < n ? lo + PARSE_SEG : n;
    int64_t line = lines_incl[s] - lines_cnt[s];
    int64_t out = 0;
    if (WRITE) out = data_incl[s] - data_cnt[s];
    uint32_t c = 0;
    for (uint64_t starts = line_starts(t, lo, hi); starts != 0; starts &= starts - 1) {
        const int64_t p = lo + (__ffsll(static_cast<unsigned long long>(starts)) - 1);
        const int64_t this_line = line++;
        if (this_line < skip_lines) continue;
        int64_t a = 0, b = 0;
        WeightToken w{0, {0, 0, false, false}};
        const int kind = parse_line<WEIGHTED>(t, p, a, b, w);
        if (kind == LINE_DATA) {
            if (WRITE) {
                if (out < o.capacity) {
                    uint64_t bits = 0;
                    bool decided = true;
                    if constexpr (WEIGHTED) decided = dw::strtod::scan_bits(w.scan, o.pow5, &bits);
                    o.src[out] = a;
                    o.dst[out] = b;
                    if constexpr (WEIGHTED) {
                        o.weight[out] = __longlong_as_double(static_cast<long long>(bits));
                        if (!decided) {
                            const unsigned long long slot = atomicAdd(o.n_undecided, 1ull);
                            if (slot < static_cast<unsigned long long>(o.undecided_capacity)) {
                                o.undecided[2 * slot] = out;
                                o.undecided[2 * slot + 1] = w.at;
                            }
                        }
                    }
                } else {
                    dw::status_or(status, DW_S_RECORDS_FULL);
                }
                ++out;
            }
            ++c;
        } else if (kind == LINE_BAD && !WRITE) {
            dw::status_or(status, DW_S_BAD_TEXT);
            atomicMin(err_line, static_cast<unsigned long long>(this_line));
        }
    }
    if (!WRITE) data_cnt[s] = c;
}

__global__ void k_parse_totals(const int64_t *__restrict__ data_incl,
                               const int64_t *__restrict__ lines_incl, int64_t n_seg,
                               int64_t *__restrict__ counts) {
    counts[0] = data_incl[n_seg - 1];
    counts[1] = lines_incl[n_seg - 1];
}

// ---- canonical form ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    k_endpoints(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, int64_t m,
                int32_t id_bits, uint64_t *__restrict__ keys, uint32_t *__restrict__ pos,
                int32_t *status) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= m) return;
    const uint64_t u = static_cast<uint64_t>(src[i]), v = static_cast<uint64_t>(dst[i]);
    if ((u >> id_bits) != 0 || (v >> id_bits) != 0) dw::status_or(status, DW_S_BAD_INDEX);
    keys[2 * i] = u;
    keys[2 * i + 1] = v;
    pos[2 * i] = static_cast<uint32_t>(2 * i);
    pos[2 * i + 1] = static_cast<uint32_t>(2 * i + 1);
}

__global__ void __launch_bounds__(256)
    k_run_heads(const uint64_t *__restrict__ keys, int64_t n, uint32_t *__restrict__ head) {
    const int64_t j = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (j < n) head[j] = (j == 0 || keys[j - 1] != keys[j]) ? 1u : 0u;
}

// rank = (heads at or before j) - 1, scattered back to the endpoint's raw position.
__global__ void __launch_bounds__(256)
    k_ranks(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ pos,
            const uint32_t *__restrict__ head, const uint32_t *__restrict__ head_incl, int64_t n,
            uint32_t *__restrict__ rank_of, int64_t *__restrict__ node_ids,
            int64_t *__restrict__ counts) {
    const int64_t j = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = head_incl[j] - 1u;
    rank_of[pos[j]] = r;
    if (head[j]) node_ids[r] = static_cast<int64_t>(keys[j]);
    if (j == n - 1) counts[0] = static_cast<int64_t>(r) + 1;
}

__global__ void __launch_bounds__(256)
    k_edge_keys(const uint32_t *__restrict__ rank_of, int64_t m, int32_t rank_bits,
                uint64_t *__restrict__ keys, uint32_t *__restrict__ idx,
                uint64_t *__restrict__ packed) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= m) return;
    const uint64_t u = rank_of[2 * i], v = rank_of[2 * i + 1];
    keys[i] = ((u < v ? u : v) << rank_bits) | (u < v ? v : u);
    idx[i] = static_cast<uint32_t>(i);
    packed[i] = (u << 32) | v;
}

// Runs of equal keys are in raw order (stable sort): the head is the first occurrence.
__global__ void __launch_bounds__(256)
    k_edge_heads(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, int64_t m,
                 uint8_t *__restrict__ keep, uint32_t *__restrict__ head_pos) {
    const int64_t j = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (j >= m) return;
    const bool head = j == 0 || keys[j - 1] != keys[j];
    keep[idx[j]] = head ? 1 : 0;
    if (head_pos) head_pos[j] = head ? static_cast<uint32_t>(j) : 0u;
}

// The run's tail is the last occurrence: its weight goes to the run's head (the kept edge).
__global__ void __launch_bounds__(256)
    k_tail_weights(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                   const uint32_t *__restrict__ head_pos, const double *__restrict__ weights,
                   int64_t m, double *__restrict__ w_first) {
    const int64_t j = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (j >= m) return;
    if (j == m - 1 || keys[j + 1] != keys[j]) w_first[idx[head_pos[j]]] = weights[idx[j]];
}

// ---- CSR with self-loops and weights -------------------------------------------------------------
// Entry 2i = (u -> v), entry 2i+1 = (v -> u); a self-loop's second entry (and a bad edge) gets
// the key n_nodes, which sorts past every row and is never gathered.
__global__ void __launch_bounds__(256)
    k_entries_loops(const uint64_t *__restrict__ edges, int64_t m, int64_t n_nodes,
                    uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= m) return;
    const uint64_t e = edges[i];
    const uint64_t u = e >> 32, v = e & 0xFFFFFFFFull;
    const uint32_t none = static_cast<uint32_t>(n_nodes);
    const bool bad = u >= static_cast<uint64_t>(n_nodes) || v >= static_cast<uint64_t>(n_nodes);
    keys[2 * i] = bad ? none : static_cast<uint32_t>(u);
    vals[2 * i] = static_cast<uint32_t>(2 * i);
    keys[2 * i + 1] = (bad || u == v) ? none : static_cast<uint32_t>(v);
    vals[2 * i + 1] = static_cast<uint32_t>(2 * i + 1);
}

__global__ void __launch_bounds__(256)
    k_gather_entries(const uint64_t *__restrict__ edges, const double *__restrict__ weights,
                     const uint32_t *__restrict__ entry, const int64_t *__restrict__ nnz_dev,
                     int64_t n_entries, int32_t *__restrict__ col, double *__restrict__ w_col) {
    const int64_t j = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (j >= n_entries || j >= *nnz_dev) return;
    const uint32_t en = entry[j];
    const uint64_t e = edges[en >> 1];
    const uint32_t other = (en & 1u) ? static_cast<uint32_t>(e >> 32) : static_cast<uint32_t>(e);
    col[j] = static_cast<int32_t>(other + 1u);
    if (w_col) w_col[j] = weights[en >> 1];
}

// ---- workspace plans (one size serves the three calls) ------------------------------------------
struct ParseBufs {
    uint32_t *lines_cnt;
    int64_t *lines_incl;
    uint32_t *data_cnt;
    int64_t *data_incl;
    char *scan_tmp;
    size_t scan_tmp_bytes;
};

int plan_parse(Arena &a, int64_t n_bytes, ParseBufs *p) {
    const int64_t n_seg = (n_bytes + PARSE_SEG - 1) / PARSE_SEG > 0
                              ? (n_bytes + PARSE_SEG - 1) / PARSE_SEG : 1;
    DW_HIP_OK(rocprim::inclusive_scan(nullptr, p->scan_tmp_bytes,
                                      static_cast<const uint32_t *>(nullptr),
                                      static_cast<int64_t *>(nullptr),
                                      static_cast<size_t>(n_seg), rocprim::plus<int64_t>()),
              "dw_edgelist_parse: scan size query");
    p->lines_cnt = a.take<uint32_t>(n_seg);
    p->lines_incl = a.take<int64_t>(n_seg);
    p->data_cnt = a.take<uint32_t>(n_seg);
    p->data_incl = a.take<int64_t>(n_seg);
    p->scan_tmp = a.take<char>(p->scan_tmp_bytes);
    return DW_OK;
}

struct CanonBufs {
    uint64_t *keys0, *keys1;
    uint32_t *pos0, *pos1, *head, *head_incl, *rank_of;
    uint64_t *packed;
    uint8_t *keep;
    double *w_first;
    uint32_t *head_pos, *head_pos_incl;
    int64_t *w_count;   // the weight select's count
    char *tmp;
    size_t tmp_bytes;
    int rank_bits;   // bits of a rank: n <= 2 m, so the edge sort reads 2 * rank_bits key bits
};

int plan_canon(Arena &a, int64_t m, CanonBufs *p) {
    const size_t n2 = 2 * static_cast<size_t>(m);
    p->rank_bits = bits_for(2 * m);
    size_t s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0;
    rocprim::double_buffer<uint64_t> kb(nullptr, nullptr);
    rocprim::double_buffer<uint32_t> vb(nullptr, nullptr);
    DW_HIP_OK(rocprim::radix_sort_pairs(nullptr, s1, kb, vb, n2, 0, 60),
              "dw_edges_canonical: endpoint sort size query");
    DW_HIP_OK(rocprim::radix_sort_pairs(nullptr, s2, kb, vb, static_cast<size_t>(m), 0,
                                        2 * p->rank_bits),
              "dw_edges_canonical: edge sort size query");
    DW_HIP_OK(rocprim::inclusive_scan(nullptr, s3, static_cast<const uint32_t *>(nullptr),
                                      static_cast<uint32_t *>(nullptr), n2,
                                      rocprim::plus<uint32_t>()),
              "dw_edges_canonical: rank scan size query");
    DW_HIP_OK(rocprim::inclusive_scan(nullptr, s4, static_cast<const uint32_t *>(nullptr),
                                      static_cast<uint32_t *>(nullptr), static_cast<size_t>(m),
                                      rocprim::maximum<uint32_t>()),
              "dw_edges_canonical: head scan size query");
    DW_HIP_OK(rocprim::select(nullptr, s5, static_cast<const uint64_t *>(nullptr),
                              static_cast<const uint8_t *>(nullptr),
                              static_cast<uint64_t *>(nullptr), static_cast<int64_t *>(nullptr),
                              static_cast<size_t>(m)),
              "dw_edges_canonical: edge select size query");
    DW_HIP_OK(rocprim::select(nullptr, s6, static_cast<const double *>(nullptr),
                              static_cast<const uint8_t *>(nullptr),
                              static_cast<double *>(nullptr), static_cast<int64_t *>(nullptr),
                              static_cast<size_t>(m)),
              "dw_edges_canonical: weight select size query");
    size_t tmp = s1;
    for (size_t s : {s2, s3, s4, s5, s6}) tmp = s > tmp ? s : tmp;
    p->tmp_bytes = tmp;
    p->keys0 = a.take<uint64_t>(n2);
    p->keys1 = a.take<uint64_t>(n2);
    p->pos0 = a.take<uint32_t>(n2);
    p->pos1 = a.take<uint32_t>(n2);
    p->head = a.take<uint32_t>(n2);
    p->head_incl = a.take<uint32_t>(n2);
    p->rank_of = a.take<uint32_t>(n2);
    p->packed = a.take<uint64_t>(m);
    p->keep = a.take<uint8_t>(m);
    p->w_first = a.take<double>(m);
    p->head_pos = a.take<uint32_t>(m);
    p->head_pos_incl = a.take<uint32_t>(m + 2);   // + 8 bytes: the weight select's count
    p->w_count = a.last<int64_t>();
    p->tmp = a.take<char>(tmp);
    return DW_OK;
}

struct LoopCsrBufs {
    uint32_t *keys0, *keys1, *vals0, *vals1, *deg;
    char *tmp;
    size_t tmp_bytes;
};

int plan_loop_csr(Arena &a, int64_t m, int64_t n_nodes, LoopCsrBufs *p) {
    const size_t n2 = 2 * static_cast<size_t>(m);
    size_t s1 = 0, s2 = 0;
    rocprim::double_buffer<uint32_t> kb(nullptr, nullptr), vb(nullptr, nullptr);
    DW_HIP_OK(rocprim::radix_sort_pairs(nullptr, s1, kb, vb, n2, 0, bits_for(n_nodes + 1)),
              "dw_csr_from_edges_loops: sort size query");
    DW_HIP_OK(rocprim::inclusive_scan(nullptr, s2, static_cast<const uint32_t *>(nullptr),
                                      static_cast<int64_t *>(nullptr),
                                      static_cast<size_t>(n_nodes), rocprim::plus<int64_t>()),
              "dw_csr_from_edges_loops: scan size query");
    p->tmp_bytes = s1 > s2 ? s1 : s2;
    p->keys0 = a.take<uint32_t>(n2);
    p->keys1 = a.take<uint32_t>(n2);
    p->vals0 = a.take<uint32_t>(n2);
    p->vals1 = a.take<uint32_t>(n2);
    p->deg = a.take<uint32_t>(n_nodes);
    p->tmp = a.take<char>(p->tmp_bytes);
    return DW_OK;
}

constexpr int64_t LIMIT_31 = int64_t(1) << 31;

// The launcher of both text entry points: plan, count lines, scan, count data lines, scan,
// write, totals. counts: edges, lines, WEIGHTED: and the undecided tokens (o.n_undecided).
#define PARSE_MSG(tail) (WEIGHTED ? "dw_edgelist_parse_weighted" tail : "dw_edgelist_parse" tail)
template <bool WEIGHTED>
int parse_text(const uint8_t *text, int64_t n_bytes, int64_t skip_lines,
               const ParseOut<WEIGHTED> &o, int64_t *counts, int64_t *err_line, int32_t *status,
               void *workspace, size_t workspace_bytes, void *stream) {
    Arena a{static_cast<char *>(workspace)};
    ParseBufs p;
    int rc = plan_parse(a, n_bytes, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off, PARSE_MSG(": workspace too small (%zu < %zu)"),
               workspace_bytes, a.off);
    hipStream_t st = dw::as_stream(stream);
    DW_HIP_OK(hipMemsetAsync(err_line, 0xFF, 8, st), PARSE_MSG(": memset"));   // -1: none
    DW_HIP_OK(hipMemsetAsync(counts, 0, WEIGHTED ? 24 : 16, st), PARSE_MSG(": memset"));
    if (n_bytes == 0) return DW_OK;
    const int64_t n_seg = (n_bytes + PARSE_SEG - 1) / PARSE_SEG;
    DW_REQUIRE((n_seg + 255) / 256 < LIMIT_31, PARSE_MSG(": chunk too large"));
    unsigned long long *err = reinterpret_cast<unsigned long long *>(err_line);
    const dim3 grid(grid_of(n_seg)), block(PARSE_BLOCK);   // (grid_of: blocks of 256)
    hipLaunchKernelGGL(k_count_lines, grid, block, 0, st, text, n_bytes, n_seg, p.lines_cnt);
    DW_LAUNCH_CHECK(PARSE_MSG("/lines"));
    DW_HIP_OK(rocprim::inclusive_scan(p.scan_tmp, p.scan_tmp_bytes,
                                      static_cast<const uint32_t *>(p.lines_cnt), p.lines_incl,
                                      static_cast<size_t>(n_seg), rocprim::plus<int64_t>(), st),
              PARSE_MSG(": line scan"));
    hipLaunchKernelGGL((k_parse<WEIGHTED, false>), grid, block, 0, st, text, n_bytes, n_seg,
                       p.lines_incl, p.lines_cnt, skip_lines, p.data_cnt, p.data_incl, o, err,
                       status);
    DW_LAUNCH_CHECK(PARSE_MSG("/count"));
    DW_HIP_OK(rocprim::inclusive_scan(p.scan_tmp, p.scan_tmp_bytes,
                                      static_cast<const uint32_t *>(p.data_cnt), p.data_incl,
                                      static_cast<size_t>(n_seg), rocprim::plus<int64_t>(), st),
              PARSE_MSG(": data scan"));
    hipLaunchKernelGGL((k_parse<WEIGHTED, true>), grid, block, 0, st, text, n_bytes, n_seg,
                       p.lines_incl, p.lines_cnt, skip_lines, p.data_cnt, p.data_incl, o, err,
                       status);
    DW_LAUNCH_CHECK(PARSE_MSG("/write"));
    hipLaunchKernelGGL(k_parse_totals, dim3(1), dim3(1), 0, st, p.data_incl, p.lines_incl, n_seg,
                       counts);
    DW_LAUNCH_CHECK(PARSE_MSG("/totals"));
    return DW_OK;
}
#undef PARSE_MSG

}  // namespace

extern "C" {

int dw_edgelist_workspace_bytes(int64_t n_text_bytes, int64_t n_edges, size_t *bytes) {
    DW_REQUIRE(bytes && n_text_bytes >= 0 && n_edges >= 0,
               "dw_edgelist_workspace_bytes: bad arguments");
    DW_REQUIRE(n_edges < LIMIT_31, "dw_edgelist_workspace_bytes: n_edges must be below 2^31");
    Arena ta{nullptr}, ca{nullptr}, ra{nullptr};
    ParseBufs t;
    CanonBufs c;
    LoopCsrBufs r;
    const int64_t m = n_edges > 0 ? n_edges : 1;
    // (the CSR's node count is not known before dw_edges_canonical: at most min(2 m, 2^31 - 2))
    const int64_t n_max = 2 * m < LIMIT_31 - 2 ? 2 * m : LIMIT_31 - 2;
    int rc = plan_parse(ta, n_text_bytes, &t);
    if (rc != DW_OK) return rc;
    rc = plan_canon(ca, m, &c);
    if (rc != DW_OK) return rc;
    rc = plan_loop_csr(ra, m, n_max, &r);
    if (rc != DW_OK) return rc;
    size_t b = ta.off > ca.off ? ta.off : ca.off;
    *bytes = b > ra.off ? b : ra.off;
    return DW_OK;
}

int dw_edgelist_parse(const uint8_t *text, int64_t n_bytes, int64_t skip_lines, int64_t *src,
                      int64_t *dst, int64_t capacity, int64_t *counts, int64_t *err_line,
                      int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    DW_REQUIRE(n_bytes >= 0 && skip_lines >= 0 && capacity >= 0,
               "dw_edgelist_parse: bad sizes");
    DW_REQUIRE(counts && err_line && status && workspace && (n_bytes == 0 || text) &&
                   (capacity == 0 || (src && dst)),
               "dw_edgelist_parse: null pointer");
    return parse_text<false>(text, n_bytes, skip_lines, {src, dst, capacity}, counts, err_line,
                             status, workspace, workspace_bytes, stream);
}

int dw_edgelist_parse_weighted(const uint8_t *text, int64_t n_bytes, int64_t skip_lines,
                               const uint64_t *pow5, int64_t *src, int64_t *dst, double *weight,
                               int64_t capacity, int64_t *undecided, int64_t undecided_capacity,
                               int64_t *counts, int64_t *err_line, int32_t *status,
                               void *workspace, size_t workspace_bytes, void *stream) {
    DW_REQUIRE(n_bytes >= 0 && skip_lines >= 0 && capacity >= 0 && undecided_capacity >= 0,
               "dw_edgelist_parse_weighted: bad sizes");
    DW_REQUIRE(counts && err_line && status && workspace && pow5 && (n_bytes == 0 || text) &&
                   (capacity == 0 || (src && dst && weight)) &&
                   (undecided_capacity == 0 || undecided),
               "dw_edgelist_parse_weighted: null pointer");
    return parse_text<true>(text, n_bytes, skip_lines,
                            {pow5, src, dst, weight, capacity, undecided, undecided_capacity,
                             reinterpret_cast<unsigned long long *>(counts + 2)},
                            counts, err_line, status, workspace, workspace_bytes, stream);
}

int dw_edges_canonical(const int64_t *src, const int64_t *dst, const double *weights,
                       int64_t n_edges, int32_t id_bits, int64_t *node_ids, uint64_t *edges,
                       double *edge_weights, int64_t *counts, int32_t *status, void *workspace,
                       size_t workspace_bytes, void *stream) {
    DW_REQUIRE(n_edges >= 1 && n_edges < LIMIT_31, "dw_edges_canonical: 1 <= n_edges < 2^31");
    DW_REQUIRE(id_bits >= 1 && id_bits <= 60, "dw_edges_canonical: id_bits must be in [1, 60]");
    DW_REQUIRE(src && dst && node_ids && edges && counts && status && workspace &&
                   (!weights || edge_weights),
               "dw_edges_canonical: null pointer");
    Arena a{static_cast<char *>(workspace)};
    CanonBufs p;
    int rc = plan_canon(a, n_edges, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off, "dw_edges_canonical: workspace too small (%zu < %zu)",
               workspace_bytes, a.off);
    hipStream_t st = dw::as_stream(stream);
    const int64_t m = n_edges, n2 = 2 * n_edges;
    size_t tmp_bytes = p.tmp_bytes;

    // 1. nodes: sort the 2m endpoints with their positions, rank the runs, scatter ranks back
    hipLaunchKernelGGL(k_endpoints, dim3(grid_of(m)), dim3(256), 0, st, src, dst, m, id_bits,
                       p.keys0, p.pos0, status);
    DW_LAUNCH_CHECK("dw_edges_canonical/endpoints");
    rocprim::double_buffer<uint64_t> kb(p.keys0, p.keys1);
    rocprim::double_buffer<uint32_t> vb(p.pos0, p.pos1);
    DW_HIP_OK(rocprim::radix_sort_pairs(p.tmp, tmp_bytes, kb, vb, static_cast<size_t>(n2), 0,
                                        id_bits, st),
              "dw_edges_canonical: endpoint sort");
    hipLaunchKernelGGL(k_run_heads, dim3(grid_of(n2)), dim3(256), 0, st, kb.current(), n2,
                       p.head);
    DW_LAUNCH_CHECK("dw_edges_canonical/heads");
    tmp_bytes = p.tmp_bytes;
    DW_HIP_OK(rocprim::inclusive_scan(p.tmp, tmp_bytes, static_cast<const uint32_t *>(p.head),
                                      p.head_incl, static_cast<size_t>(n2),
                                      rocprim::plus<uint32_t>(), st),
              "dw_edges_canonical: rank scan");
    hipLaunchKernelGGL(k_ranks, dim3(grid_of(n2)), dim3(256), 0, st, kb.current(), vb.current(),
                       p.head, p.head_incl, n2, p.rank_of, node_ids, counts);
    DW_LAUNCH_CHECK("dw_edges_canonical/ranks");

    // 2. edges: key (min rank, max rank), stable sort with the raw index, keep every run's head
    hipLaunchKernelGGL(k_edge_keys, dim3(grid_of(m)), dim3(256), 0, st, p.rank_of, m,
                       p.rank_bits, p.keys0, p.pos0, p.packed);   // (the endpoint buffers: free)
    DW_LAUNCH_CHECK("dw_edges_canonical/keys");
    rocprim::double_buffer<uint64_t> eb(p.keys0, p.keys1);
    rocprim::double_buffer<uint32_t> ib(p.pos0, p.pos1);
    tmp_bytes = p.tmp_bytes;
    DW_HIP_OK(rocprim::radix_sort_pairs(p.tmp, tmp_bytes, eb, ib, static_cast<size_t>(m), 0,
                                        2 * p.rank_bits, st),
              "dw_edges_canonical: edge sort");
    hipLaunchKernelGGL(k_edge_heads, dim3(grid_of(m)), dim3(256), 0, st, eb.current(),
                       ib.current(), m, p.keep, weights ? p.head_pos : nullptr);
    DW_LAUNCH_CHECK("dw_edges_canonical/first");
    tmp_bytes = p.tmp_bytes;
    DW_HIP_OK(rocprim::select(p.tmp, tmp_bytes, static_cast<const uint64_t *>(p.packed),
                              static_cast<const uint8_t *>(p.keep), edges, counts + 1,
                              static_cast<size_t>(m), st),
              "dw_edges_canonical: edge select");
    if (weights) {
        tmp_bytes = p.tmp_bytes;
        DW_HIP_OK(rocprim::inclusive_scan(p.tmp, tmp_bytes,
                                          static_cast<const uint32_t *>(p.head_pos),
                                          p.head_pos_incl, static_cast<size_t>(m),
                                          rocprim::maximum<uint32_t>(), st),
                  "dw_edges_canonical: head scan");
        hipLaunchKernelGGL(k_tail_weights, dim3(grid_of(m)), dim3(256), 0, st, eb.current(),
                           ib.current(), p.head_pos_incl, weights, m, p.w_first);
        DW_LAUNCH_CHECK("dw_edges_canonical/weights");
        tmp_bytes = p.tmp_bytes;
        DW_HIP_OK(rocprim::select(p.tmp, tmp_bytes, static_cast<const double *>(p.w_first),
                                  static_cast<const uint8_t *>(p.keep), edge_weights, p.w_count,
                                  static_cast<size_t>(m), st),
                  "dw_edges_canonical: weight select");
    }
    return DW_OK;
}

int dw_csr_from_edges_loops(const uint64_t *edges, const double *edge_weights, int64_t n_edges,
                            int64_t n_nodes, int64_t *row_ptr, int32_t *col, double *weights,
                            int32_t *status, void *workspace, size_t workspace_bytes,
                            void *stream) {
    DW_REQUIRE(n_edges >= 0 && n_nodes >= 1 && n_nodes < LIMIT_31 - 1 && 2 * n_edges < LIMIT_31,
               "dw_csr_from_edges_loops: bad sizes");
    DW_REQUIRE(row_ptr && status && workspace && (n_edges == 0 || (edges && col)) &&
                   (!edge_weights || weights || n_edges == 0),
               "dw_csr_from_edges_loops: null pointer");
    Arena a{static_cast<char *>(workspace)};
    LoopCsrBufs p;
    int rc = plan_loop_csr(a, n_edges > 0 ? n_edges : 1, n_nodes, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off,
               "dw_csr_from_edges_loops: workspace too small (%zu < %zu)", workspace_bytes,
               a.off);
    hipStream_t st = dw::as_stream(stream);
    DW_HIP_OK(hipMemsetAsync(p.deg, 0, n_nodes * 4, st), "dw_csr_from_edges_loops: memset");
    hipLaunchKernelGGL(k_row_ptr_head, dim3(1), dim3(1), 0, st, row_ptr);
    DW_LAUNCH_CHECK("dw_csr_from_edges_loops/head");
    const int64_t n2 = 2 * n_edges;
    rocprim::double_buffer<uint32_t> kb(p.keys0, p.keys1), vb(p.vals0, p.vals1);
    if (n_edges > 0) {
        hipLaunchKernelGGL(k_degree<true>, dim3(grid_of(n_edges)), dim3(256), 0, st, edges,
                           n_edges, n_nodes, p.deg, status);
        DW_LAUNCH_CHECK("dw_csr_from_edges_loops/degree");
        hipLaunchKernelGGL(k_entries_loops, dim3(grid_of(n_edges)), dim3(256), 0, st, edges,
                           n_edges, n_nodes, p.keys0, p.vals0);
        DW_LAUNCH_CHECK("dw_csr_from_edges_loops/entries");
        size_t tmp_bytes = p.tmp_bytes;
        DW_HIP_OK(rocprim::radix_sort_pairs(p.tmp, tmp_bytes, kb, vb, static_cast<size_t>(n2), 0,
                                            bits_for(n_nodes + 1), st),
                  "dw_csr_from_edges_loops: sort");
    }
    size_t tmp_bytes = p.tmp_bytes;
    DW_HIP_OK(rocprim::inclusive_scan(p.tmp, tmp_bytes, static_cast<const uint32_t *>(p.deg),
                                      row_ptr + 2, static_cast<size_t>(n_nodes),
                                      rocprim::plus<int64_t>(), st),
              "dw_csr_from_edges_loops: scan");
    if (n_edges > 0) {
        hipLaunchKernelGGL(k_gather_entries, dim3(grid_of(n2)), dim3(256), 0, st, edges,
                           edge_weights, vb.current(), row_ptr + n_nodes + 1, n2, col,
                           edge_weights ? weights : nullptr);
        DW_LAUNCH_CHECK("dw_csr_from_edges_loops/gather");
    }
    return DW_OK;
}

}  // extern "C"
