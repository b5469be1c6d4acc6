// Word2vec text ("key v_0 .. v_{d-1}\n" lines, already in HBM) to embedding rows on the device,
// the inverse of dw_embtext.hip, in two passes: dw_embread_lines indexes the lines (count the
// '\n' of every 64-byte segment, scan, write the line starts), dw_embread_parse converts them.
//
// Pass 2 splits the work by tokens, not by lines: a line at d = 128 is ~1.5 KB, so one lane per
// line would serialise 128 conversions and put the lanes' reads 1.5 KB apart. A wave owns a line
// and takes it in tiles of TILE bytes staged in its own LDS slice with 16-byte loads; a lane
// marks the token starts among its LANE_BYTES bytes (a non-blank byte behind a blank or the line
// start), a wave prefix sum of the marks numbers the tokens across tiles, and the lane that owns
// a token's start converts it (dw_embread.h), reading on through LDS, or through memory where
// the token runs off the staged bytes. Token 0 is the key, token j >= 1 goes to column j - 1.
// A first sweep over the tiles counts the tokens, so that nothing of a line with another count
// than dim + 1 is stored; a line of one tile (every line of the usual d = 128 file) is staged
// once for both sweeps.
//
// LDS: 4 padding bytes behind every 128 staged ones put the lanes' byte reads, which start
// LANE_BYTES = 32 bytes apart, on distinct banks while they move in step (lane l starts at bank
// 8 l + l / 4 of 32); the staging stores are four dword stores for that, which cost what one
// 16-byte store costs. A block holds 4 waves' slices, 8.6 KiB, so LDS allows 18 blocks a CU and
// the register count, not LDS, sets the occupancy.
//
// Every output is a pure function of the input: the only atomics are integer ones, over the
// undecided counter, the smallest bad line and the status word. Reruns are bit-identical, except
// for the order of the undecided list.
#include <rocprim/device/device_scan.hpp>

#include "dw_common.h"
#include "dw_embread.h"
#include "dw_ingest.h"

namespace {

namespace er = dw::embread;
using dw::ingest::Arena;

// ---- pass 1: the line index ------------------------------------------------------------------
constexpr int SEG = 64;        // bytes a lane indexes: four 16-byte loads
constexpr int BLOCK = 256;

// The 16 bytes at the 16-byte aligned address text + g (g may be negative): one vector load
// where they all lie in the text, byte loads of those that do (the others read as 0) otherwise.
// No byte outside text[0, n) is touched.
__device__ __forceinline__ uint4 load16(const uint8_t *__restrict__ text, int64_t n, int64_t g) {
    if (g >= 0 && g + 16 <= n) return *reinterpret_cast<const uint4 *>(text + g);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int i = 0; i < 16; ++i)
        if (g + i >= 0 && g + i < n) w[i >> 2] |= static_cast<uint32_t>(text[g + i]) << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// 0x80 in every byte of w that is '\n'.
__device__ __forceinline__ uint32_t newline_bytes(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// Segment s is the 64 bytes at text - a + 64 s, a = the text's address mod 16, so that its
// loads are aligned; bit k of the result: byte k of it is a '\n' of the text.
__device__ __forceinline__ uint64_t segment_newlines(const uint8_t *__restrict__ text, int64_t n,
                                                     int64_t g) {
    uint64_t m = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint4 v = load16(text, n, g + 16 * c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // gather the four 0x80 marks of a word into four neighbouring bits
            const uint32_t b = newline_bytes(w[k]) >> 7;
            const uint32_t nib = (b | (b >> 7) | (b >> 14) | (b >> 21)) & 0xFu;
            m |= static_cast<uint64_t>(nib) << (16 * c + 4 * k);
        }
    }
    return m;
}

__global__ void __launch_bounds__(BLOCK)
    k_embread_count(const uint8_t *__restrict__ text, int64_t n, int64_t n_seg,
                    uint32_t *__restrict__ cnt) {
    const int64_t s = blockIdx.x * static_cast<int64_t>(BLOCK) + threadIdx.x;
    if (s >= n_seg) return;
    const int64_t a = static_cast<int64_t>(reinterpret_cast<uintptr_t>(text) & 15u);
    cnt[s] = static_cast<uint32_t>(__popcll(segment_newlines(text, n, s * SEG - a)));
}

// line_off[0] = 0, line_off[r + 1] = one behind the r-th '\n'; a last line without its '\n' ends
// at n. Entries past `capacity` lines are not written. counts[0] = lines.
__global__ void __launch_bounds__(BLOCK)
    k_embread_index(const uint8_t *__restrict__ text, int64_t n, int64_t n_seg,
                    const uint32_t *__restrict__ cnt, const int64_t *__restrict__ incl,
                    int64_t *__restrict__ line_off, int64_t capacity,
                    int64_t *__restrict__ counts) {
    const int64_t s = blockIdx.x * static_cast<int64_t>(BLOCK) + threadIdx.x;
    if (s >= n_seg) return;
    const int64_t a = static_cast<int64_t>(reinterpret_cast<uintptr_t>(text) & 15u);
    const int64_t g = s * SEG - a;
    int64_t r = incl[s] - cnt[s];
    if (s == 0) line_off[0] = 0;
    for (uint64_t m = segment_newlines(text, n, g); m != 0; m &= m - 1) {
        const int64_t p = g + (__ffsll(static_cast<unsigned long long>(m)) - 1);
        ++r;
        if (r <= capacity) line_off[r] = p + 1;
    }
    if (s == n_seg - 1) {   // (r = every '\n' of the text)
        const bool open = text[n - 1] != '\n';
        if (open && r + 1 <= capacity) line_off[r + 1] = n;
        counts[0] = r + (open ? 1 : 0);
    }
}

// ---- pass 2: the tokens -------------------------------------------------------------------------
constexpr int WAVES = 4;                 // lines per block
constexpr int LANE_BYTES = 32;           // a lane's bytes of a tile: two 16-byte chunks
constexpr int TILE = 64 * LANE_BYTES;    // 2 KiB
constexpr int OVER = 80;                 // staged behind the tile: a MAX_TOKEN token, rounded up
constexpr int STAGED = TILE + OVER;
constexpr int SLICE = STAGED + (STAGED >> 7) * 4 + 4;   // with the padding

__device__ __forceinline__ uint32_t phys(uint32_t o) { return o + (o >> 7) * 4u; }

// A line's bytes by their offset in the text: staged ones from LDS, the others from memory.
struct Line {
    const uint8_t *__restrict__ t;
    const uint8_t *lds;
    int64_t base, end;   // text[base, end) is staged, text[base + o] at lds[phys(o)]
    __device__ __forceinline__ uint8_t operator[](int64_t q) const {
        if (q >= base && q < end) return lds[phys(static_cast<uint32_t>(q - base))];
        return t[q];
    }
};

// The staged bytes alone, for the tokens that end among them: no choice per byte.
struct Staged {
    const uint8_t *lds;
    int64_t base;
    __device__ __forceinline__ uint8_t operator[](int64_t q) const {
        return lds[phys(static_cast<uint32_t>(q - base))];
    }
};

// Stages text[tb, min(tb + STAGED, le)) in the wave's slice, whole 16-byte chunks at a time
// (text + tb is 16-byte aligned; tb may be negative in the line's first tile).
__device__ __forceinline__ void stage_tile(const uint8_t *__restrict__ text, int64_t n, int64_t tb,
                                           int64_t le, uint32_t *slice, int lane) {
    dw::wave_lds_sync();   // the reads of the tile before are done
    for (int c = lane; c < STAGED / 16; c += 64) {
        const int64_t g = tb + 16 * c;
        if (g >= le) break;
        const uint4 v = load16(text, n, g);
        uint32_t *d = slice + (phys(16u * c) >> 2);
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
    dw::wave_lds_sync();
}

struct ParseArgs {
    const uint8_t *__restrict__ text;
    int64_t n;
    const int64_t *__restrict__ line_off;
    int64_t n_lines;
    int32_t dim;
    const uint64_t *__restrict__ pow5;
    float *__restrict__ table;
    int64_t row0;
    int64_t *__restrict__ key_off, *__restrict__ key_len, *__restrict__ key_i64;
    int64_t *__restrict__ undecided;
    int64_t undecided_capacity;
    unsigned long long *n_undecided;
    unsigned long long *err_line;
    int32_t *status;
};

__global__ void __launch_bounds__(64 * WAVES) k_embread_parse(ParseArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_slice[WAVES][SLICE / 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t line = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    if (line >= a.n_lines) return;
    const int64_t ls = a.line_off[line];
    int64_t le = a.line_off[line + 1];
    if (ls < 0 || le > a.n || ls > le) return;   // (a line_off that is no index: touch nothing)
    if (le > ls && a.text[le - 1] == '\n') --le;
    uint32_t *slice = s_slice[wave];
    const int64_t g0 = ls - static_cast<int64_t>((reinterpret_cast<uintptr_t>(a.text) +
                                                  static_cast<uintptr_t>(ls)) & 15u);
    const int n_tiles = static_cast<int>((le - g0 + TILE - 1) / TILE);
    const int64_t row = a.row0 + line;

    uint32_t starts = 0;   // bit i: a token starts at the lane's byte i of the tile
    for (int sweep = 0; sweep < 2; ++sweep) {
        int32_t seen = 0;            // tokens in the tiles before
        bool after_blank = true;     // of the byte in front of the tile
        for (int k = 0; k < n_tiles; ++k) {
            const int64_t tb = g0 + static_cast<int64_t>(k) * TILE;
            const int64_t mine = tb + lane * LANE_BYTES;
            if (sweep == 0 || n_tiles > 1) {
                stage_tile(a.text, a.n, tb, le, slice, lane);
                uint32_t text_bytes = 0;   // bit i: byte i is a non-blank byte of the line
#pragma unroll
                for (int w = 0; w < LANE_BYTES / 4; ++w) {
                    const uint32_t v = slice[phys(lane * LANE_BYTES + 4 * w) >> 2];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int64_t q = mine + 4 * w + i;
                        const bool in = q >= ls && q < le;
                        if (in && !er::is_blank(static_cast<uint8_t>(v >> (8 * i))))
                            text_bytes |= 1u << (4 * w + i);
                    }
                }
                const uint32_t before = __shfl_up(text_bytes, 1, 64);
                const bool prev_text = lane == 0 ? !after_blank : (before >> 31) != 0;
                starts = text_bytes & ~((text_bytes << 1) | (prev_text ? 1u : 0u));
                after_blank = (__shfl(text_bytes, 63, 64) >> 31) == 0;
            }
            const int32_t cnt = __popc(starts);
            int32_t incl = cnt;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int32_t t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            if (sweep == 1) {
                const Line text{a.text, reinterpret_cast<const uint8_t *>(slice), tb,
                                tb + STAGED < le ? tb + STAGED : le};
                const Staged near{text.lds, tb};
                int32_t j = seen + incl - cnt;
                for (uint32_t m = starts; m != 0; m &= m - 1, ++j) {
                    const int64_t p = mine + (__ffs(m) - 1);
                    int64_t e;
                    if (j == 0) {
                        const int64_t v = er::key_token(text, p, le, &e);
                        a.key_off[row] = p;
                        a.key_len[row] = e - p;
                        a.key_i64[row] = v;
                        if (v < 0) dw::status_or(a.status, DW_S_TEXT_KEY);
                    } else {
                        uint32_t bits;
                        const int kind = er::value_token(near, text.end, text, p, le, a.pow5, &e,
                                                        &bits);
                        a.table[row * a.dim + (j - 1)] = __uint_as_float(bits);
                        if (kind == er::TOKEN_UNDECIDED) {
                            const unsigned long long slot = atomicAdd(a.n_undecided, 1ull);
                            if (slot < static_cast<unsigned long long>(a.undecided_capacity)) {
                                int64_t *u = a.undecided + er::UNDECIDED_WORDS * slot;
                                u[0] = row;
                                u[1] = j - 1;
                                u[2] = p;
                                u[3] = e - p;
                            }
                        }
                    }
                }
            }
            seen += __shfl(incl, 63, 64);
        }
        if (sweep == 0 && seen != a.dim + 1) {   // a bad line: nothing of it is stored
            if (lane == 0) {
                dw::status_or(a.status, DW_S_BAD_TEXT);
                atomicMin(a.err_line, static_cast<unsigned long long>(line));
            }
            return;
        }
    }
}

struct Plan {
    uint32_t *cnt;
    int64_t *incl;
    char *scan_tmp;
    size_t scan_tmp_bytes;
};

int64_t segments(int64_t n_bytes) {   // (+ 1: the text may start up to 15 bytes into segment 0)
    return n_bytes / SEG + 2;
}

int plan(Arena &a, int64_t n_bytes, Plan *p) {
    const int64_t n_seg = segments(n_bytes);
    DW_HIP_OK(rocprim::inclusive_scan(nullptr, p->scan_tmp_bytes,
                                      static_cast<const uint32_t *>(nullptr),
                                      static_cast<int64_t *>(nullptr),
                                      static_cast<size_t>(n_seg), rocprim::plus<int64_t>()),
              "dw_embread_lines: scan size query");
    p->cnt = a.take<uint32_t>(n_seg);
    p->incl = a.take<int64_t>(n_seg);
    p->scan_tmp = a.take<char>(p->scan_tmp_bytes);
    return DW_OK;
}

}  // namespace

extern "C" {

int dw_embread_workspace_bytes(int64_t n_bytes, size_t *bytes) {
    DW_REQUIRE(bytes && n_bytes >= 0, "dw_embread_workspace_bytes: bad arguments");
    Arena a{nullptr};
    Plan p;
    const int rc = plan(a, n_bytes, &p);
    if (rc != DW_OK) return rc;
    *bytes = a.off;
    return DW_OK;
}

int dw_embread_lines(const uint8_t *text, int64_t n_bytes, int64_t *line_off, int64_t capacity,
                     int64_t *counts, int64_t *err_line, void *workspace, size_t workspace_bytes,
                     void *stream) {
    DW_REQUIRE(n_bytes >= 0 && capacity >= 0, "dw_embread_lines: bad sizes");
    DW_REQUIRE(line_off && counts && err_line && workspace && (n_bytes == 0 || text),
               "dw_embread_lines: null pointer");
    Arena a{static_cast<char *>(workspace)};
    Plan p;
    const int rc = plan(a, n_bytes, &p);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(workspace_bytes >= a.off, "dw_embread_lines: workspace too small (%zu < %zu)",
               workspace_bytes, a.off);
    hipStream_t st = dw::as_stream(stream);
    DW_HIP_OK(hipMemsetAsync(err_line, 0xFF, 8, st), "dw_embread_lines: memset");   // -1: none
    DW_HIP_OK(hipMemsetAsync(counts, 0, 16, st), "dw_embread_lines: memset");
    DW_HIP_OK(hipMemsetAsync(line_off, 0, 8, st), "dw_embread_lines: memset");
    if (n_bytes == 0) return DW_OK;
    const int64_t n_seg = segments(n_bytes);
    DW_REQUIRE((n_seg + BLOCK - 1) / BLOCK < (int64_t(1) << 31), "dw_embread_lines: chunk too large");
    const dim3 grid(dw::ingest::grid_of(n_seg)), block(BLOCK);
    hipLaunchKernelGGL(k_embread_count, grid, block, 0, st, text, n_bytes, n_seg, p.cnt);
    DW_LAUNCH_CHECK("dw_embread_lines/count");
    DW_HIP_OK(rocprim::inclusive_scan(p.scan_tmp, p.scan_tmp_bytes,
                                      static_cast<const uint32_t *>(p.cnt), p.incl,
                                      static_cast<size_t>(n_seg), rocprim::plus<int64_t>(), st),
              "dw_embread_lines: scan");
    hipLaunchKernelGGL(k_embread_index, grid, block, 0, st, text, n_bytes, n_seg, p.cnt, p.incl,
                       line_off, capacity, counts);
    DW_LAUNCH_CHECK("dw_embread_lines/index");
    return DW_OK;
}

int dw_embread_parse(const uint8_t *text, int64_t n_bytes, const int64_t *line_off,
                     int64_t n_lines, int32_t dim, const uint64_t *pow5, float *table,
                     int64_t n_rows, int64_t row0, int64_t *key_off, int64_t *key_len,
                     int64_t *key_i64, int64_t *undecided, int64_t undecided_capacity,
                     int64_t *counts, int64_t *err_line, int32_t *status, void *stream) {
    DW_REQUIRE(dim >= 1, "dw_embread_parse: dim must be >= 1");
    if (dim > er::MAX_DIM) {
        dw::set_error("dw_embread_parse: dim %d > %d is not supported", dim, er::MAX_DIM);
        return DW_E_UNSUPPORTED;
    }
    DW_REQUIRE(n_bytes >= 0 && n_lines >= 0 && undecided_capacity >= 0 && row0 >= 0 &&
                   n_lines <= n_bytes && row0 + n_lines <= n_rows,
               "dw_embread_parse: bad sizes (lines [%lld, %lld) of %lld rows, %lld bytes)",
               (long long)row0, (long long)(row0 + n_lines), (long long)n_rows,
               (long long)n_bytes);
    DW_REQUIRE(line_off && pow5 && counts && err_line && status && (n_bytes == 0 || text) &&
                   (n_lines == 0 || (table && key_off && key_len && key_i64)) &&
                   (undecided_capacity == 0 || undecided),
               "dw_embread_parse: null pointer");
    if (n_lines == 0) return DW_OK;
    DW_REQUIRE((n_lines + WAVES - 1) / WAVES < (int64_t(1) << 31), "dw_embread_parse: chunk too large");
    const ParseArgs a{text, n_bytes, line_off, n_lines, dim, pow5, table, row0, key_off, key_len,
                      key_i64, undecided, undecided_capacity,
                      reinterpret_cast<unsigned long long *>(counts + 1),
                      reinterpret_cast<unsigned long long *>(err_line), status};
    const unsigned grid = static_cast<unsigned>((n_lines + WAVES - 1) / WAVES);
    hipLaunchKernelGGL(k_embread_parse, dim3(grid), dim3(64 * WAVES), 0, dw::as_stream(stream), a);
    DW_LAUNCH_CHECK("dw_embread_parse");
    return DW_OK;
}

}  // extern "C"
