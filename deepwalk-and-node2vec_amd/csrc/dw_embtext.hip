// Embedding rows to word2vec text ("key v_0 .. v_{d-1}\n" lines) on the device, in two passes:
// dw_embtext_sizes measures every line and scans the lengths into line_off, dw_embtext_write
// writes the lines of a row range at their offsets. Both run dw_f32text.h's exact shortest-decimal
// conversion per value; pass 2 recomputes the digits instead of reading them back from a
// workspace of 8 B per value.
//
// A wave owns a row. Lane l converts values l, l + 64, .. of it; a wave scan of the token lengths
// places each token in the wave's LDS line, which starts at the same offset mod 16 as its place
// in `out`, so the line leaves as aligned 16-byte vector stores with byte stores only for the
// ragged head and tail. Every output is a pure function of the input: no atomics order anything
// (the status word alone is OR-ed).
#include <hipcub/hipcub.hpp>

#include "dw_common.h"
#include "dw_f32text.h"

namespace {

namespace ft = dw::f32text;

constexpr int WAVES = 4;       // rows per block
constexpr int MAX_DIM = 512;

struct Keys {
    const int64_t *i64;     // [n_rows], or NULL:
    const uint8_t *bytes;   // the keys' bytes, key r at [off[r], off[r + 1])
    const int64_t *off;
};

struct RowHead {
    int64_t src;    // the table row, -1 when out of range (its values print as 0.0)
    int64_t key;    // the integer key (0 when negative)
    int64_t klen;   // bytes of the key
    int32_t st;
};

__device__ __forceinline__ RowHead row_head(int64_t r, const int64_t *__restrict__ rows,
                                            int64_t vocab_size, const Keys &k) {
    RowHead h;
    h.st = 0;
    h.src = rows ? rows[r] : r;
    if (h.src < 0 || h.src >= vocab_size) {
        h.src = -1;
        h.st |= DW_S_BAD_INDEX;
    }
    h.key = 0;
    if (k.i64) {
        h.key = k.i64[r];
        if (h.key < 0) {
            h.key = 0;
            h.st |= DW_S_BAD_INDEX;
        }
        h.klen = ft::key_digits(h.key);
    } else {
        h.klen = k.off[r + 1] - k.off[r];
        if (h.klen < 0) {
            h.klen = 0;
            h.st |= DW_S_BAD_INDEX;
        }
    }
    return h;
}

__device__ __forceinline__ void load_table(uint64_t *s_tab, const uint64_t *__restrict__ tab) {
    if (threadIdx.x < ft::TABLE_WORDS) s_tab[threadIdx.x] = tab[threadIdx.x];
    __syncthreads();
}

// lens[r] = bytes of line r (r < n_rows), lens[n_rows] = 0: the scan's input.
__global__ void __launch_bounds__(64 * WAVES)
    k_embtext_sizes(const float *__restrict__ table, int64_t vocab_size, int32_t dim,
                    const int64_t *__restrict__ rows, int64_t n_rows, Keys keys,
                    const uint64_t *__restrict__ tab, int64_t *__restrict__ lens,
                    int32_t *status) {
    __shared__ uint64_t s_tab[ft::TABLE_WORDS];
    load_table(s_tab, tab);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    if (r == n_rows && lane == 0) lens[n_rows] = 0;
    if (r >= n_rows) return;
    const RowHead h = row_head(r, rows, vocab_size, keys);
    int32_t len = 0, st = h.st;
    for (int32_t c = lane; c < dim; c += 64) {
        const uint32_t bits = h.src >= 0 ? __float_as_uint(table[h.src * dim + c]) : 0u;
        const ft::Dec d = ft::shortest(bits, s_tab);
        if (d.kind != ft::FINITE) st |= DW_S_NONFINITE;
        len += 1 + ft::token_len(d);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        len += __shfl_xor(len, off, 64);
        st |= __shfl_xor(st, off, 64);
    }
    if (lane == 0) {
        lens[r] = h.klen + 1 + len;
        if (st) dw::status_or(status, st);
    }
}

// CAP: the largest dim the wave's LDS line holds (20 bytes a value, the line end, and up to 15
// bytes in front to match the destination's alignment).
template <int CAP>
__global__ void __launch_bounds__(64 * WAVES)
    k_embtext_write(const float *__restrict__ table, int64_t vocab_size, int32_t dim,
                    const int64_t *__restrict__ rows, Keys keys, const uint64_t *__restrict__ tab,
                    const int64_t *__restrict__ line_off, int64_t r0, int64_t r1,
                    uint8_t *__restrict__ out, int64_t capacity, int32_t *status) {
    constexpr int LINE = 16 + CAP * (ft::MAX_TOKEN + 1) + 16;
    __shared__ uint64_t s_tab[ft::TABLE_WORDS];
    __shared__ __attribute__((aligned(16))) uint8_t s_line[WAVES][LINE];
    load_table(s_tab, tab);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = line_off[r0], span = line_off[r1] - base;
    if (span < 0 || span > capacity) {   // the range does not fit: nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0) dw::status_or(status, DW_S_RECORDS_FULL);
        return;
    }
    const int64_t r = r0 + static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    if (r >= r1) return;
    const RowHead h = row_head(r, rows, vocab_size, keys);
    const int64_t start = line_off[r] - base;
    int64_t lim = line_off[r + 1] - base;   // no store of this line at or past lim
    lim = lim < span ? lim : span;
    if (start < 0 || start > lim) return;    // (a line_off that is no scan: write nothing)

    for (int64_t j = lane; j < h.klen; j += 64) {   // the key, straight to memory
        uint8_t b;
        if (keys.i64) {
            uint64_t v = static_cast<uint64_t>(h.key);
            for (int64_t t = h.klen - 1 - j; t > 0; --t) v /= 10u;
            b = static_cast<uint8_t>('0' + v % 10u);
        } else {
            b = keys.bytes[keys.off[r] + j];
        }
        if (start + j < lim) out[start + j] = b;
    }

    const int64_t vstart = start + h.klen;
    const int32_t a = static_cast<int32_t>((reinterpret_cast<uintptr_t>(out) +
                                            static_cast<uintptr_t>(vstart)) & 15u);
    uint8_t *line = s_line[wave];
    int32_t pos = a;
    for (int32_t c0 = 0; c0 < dim; c0 += 64) {
        const int32_t c = c0 + lane;
        ft::Dec d = {};
        int32_t len = 0;
        if (c < dim) {
            const uint32_t bits = h.src >= 0 ? __float_as_uint(table[h.src * dim + c]) : 0u;
            d = ft::shortest(bits, s_tab);
            len = 1 + ft::token_len(d) + (c == dim - 1 ? 1 : 0);
        }
        int32_t incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (c < dim) {
            uint8_t *w = line + pos + incl - len;
            *w++ = ' ';
            ft::token_emit(d, [&w](uint8_t b) { *w++ = b; });
            if (c == dim - 1) *w = '\n';
        }
        pos += __shfl(incl, 63, 64);
    }
    dw::wave_lds_sync();

    // LDS byte i of the line goes to out[gbase + i]; out + gbase is 16-byte aligned
    const int64_t gbase = vstart - a;
    const int32_t n_chunks = (pos + 15) >> 4;
    for (int32_t ch = lane; ch < n_chunks; ch += 64) {
        const int32_t lo = ch << 4, hi = lo + 16;
        if (lo >= a && hi <= pos && gbase + hi <= lim) {
            *reinterpret_cast<uint4 *>(out + gbase + lo) =
                *reinterpret_cast<const uint4 *>(line + lo);
        } else {
            const int32_t b0 = lo > a ? lo : a, b1 = hi < pos ? hi : pos;
            for (int32_t b = b0; b < b1; ++b)
                if (gbase + b < lim) out[gbase + b] = line[b];
        }
    }
}

// lens int64 [n_rows + 1], then hipcub's scan storage.
struct Plan {
    int64_t *lens;
    void *cub;
    size_t cub_bytes;
};

int plan(dw::Arena &a, int64_t n_rows, void *stream, Plan *p) {
    p->lens = a.take<int64_t>(static_cast<size_t>(n_rows) + 1);
    p->cub_bytes = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, p->cub_bytes, (int64_t *)nullptr,
                                                    (int64_t *)nullptr, (int)(n_rows + 1),
                                                    dw::as_stream(stream));
    if (e != hipSuccess) {
        dw::set_error("dw_embtext: hipcub scan size: %s", hipGetErrorString(e));
        return DW_E_HIP;
    }
    p->cub = a.take<char>(p->cub_bytes);
    return DW_OK;
}

int check_shape(const char *who, const float *table, int64_t vocab_size, int32_t dim,
                int64_t n_rows, const int64_t *keys_i64, const uint8_t *key_bytes,
                const int64_t *key_off, const uint64_t *tab) {
    DW_REQUIRE(dim >= 1, "%s: dim must be >= 1", who);
    if (dim > MAX_DIM) {
        dw::set_error("%s: dim %d > %d is not supported", who, dim, MAX_DIM);
        return DW_E_UNSUPPORTED;
    }
    DW_REQUIRE(vocab_size >= 1 && n_rows >= 0 && n_rows < (int64_t(1) << 31) - 1,
               "%s: vocab_size must be >= 1 and n_rows in [0, 2^31 - 1)", who);
    DW_REQUIRE(table && tab, "%s: null pointer", who);
    DW_REQUIRE((keys_i64 != nullptr) != (key_bytes != nullptr && key_off != nullptr),
               "%s: give keys_i64 or (key_bytes, key_off), not both", who);
    return DW_OK;
}

}  // namespace

extern "C" {

int dw_embtext_workspace_bytes(int64_t n_rows, int32_t dim, size_t *bytes) {
    DW_REQUIRE(bytes, "dw_embtext_workspace_bytes: null pointer");
    DW_REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 31) - 1 && dim >= 1,
               "dw_embtext_workspace_bytes: bad sizes");
    dw::Arena a{nullptr};
    Plan p;
    const int rc = plan(a, n_rows, nullptr, &p);
    if (rc != DW_OK) return rc;
    *bytes = a.off;
    return DW_OK;
}

int dw_embtext_sizes(const float *table, int64_t vocab_size, int32_t dim, const int64_t *rows,
                     int64_t n_rows, const int64_t *keys_i64, const uint8_t *key_bytes,
                     const int64_t *key_off, const uint64_t *tab, int64_t *line_off,
                     int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    const int rc = check_shape("dw_embtext_sizes", table, vocab_size, dim, n_rows, keys_i64,
                               key_bytes, key_off, tab);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(line_off && workspace, "dw_embtext_sizes: null pointer");
    dw::Arena a{static_cast<char *>(workspace)};
    Plan p;
    const int prc = plan(a, n_rows, stream, &p);
    if (prc != DW_OK) return prc;
    DW_REQUIRE(a.off <= workspace_bytes, "dw_embtext_sizes: workspace too small (%zu < %zu)",
               workspace_bytes, a.off);
    const unsigned grid = static_cast<unsigned>((n_rows + 1 + WAVES - 1) / WAVES);
    k_embtext_sizes<<<grid, 64 * WAVES, 0, dw::as_stream(stream)>>>(
        table, vocab_size, dim, rows, n_rows, Keys{keys_i64, key_bytes, key_off}, tab, p.lens,
        status);
    DW_LAUNCH_CHECK("dw_embtext_sizes");
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(p.cub, p.cub_bytes, p.lens, line_off,
                                                    (int)(n_rows + 1), dw::as_stream(stream));
    if (e != hipSuccess) {
        dw::set_error("dw_embtext_sizes: hipcub scan: %s", hipGetErrorString(e));
        return DW_E_HIP;
    }
    return DW_OK;
}

int dw_embtext_write(const float *table, int64_t vocab_size, int32_t dim, const int64_t *rows,
                     int64_t n_rows, const int64_t *keys_i64, const uint8_t *key_bytes,
                     const int64_t *key_off, const uint64_t *tab, const int64_t *line_off,
                     int64_t r0, int64_t r1, uint8_t *out, int64_t capacity, int32_t *status,
                     void *stream) {
    const int rc = check_shape("dw_embtext_write", table, vocab_size, dim, n_rows, keys_i64,
                               key_bytes, key_off, tab);
    if (rc != DW_OK) return rc;
    DW_REQUIRE(line_off && out, "dw_embtext_write: null pointer");
    DW_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= n_rows, "dw_embtext_write: bad row range");
    DW_REQUIRE(capacity >= 0, "dw_embtext_write: negative capacity");
    if (r0 == r1) return DW_OK;
    const unsigned grid = static_cast<unsigned>((r1 - r0 + WAVES - 1) / WAVES);
    const Keys keys{keys_i64, key_bytes, key_off};
    if (dim <= 128)
        k_embtext_write<128><<<grid, 64 * WAVES, 0, dw::as_stream(stream)>>>(
            table, vocab_size, dim, rows, keys, tab, line_off, r0, r1, out, capacity, status);
    else
        k_embtext_write<MAX_DIM><<<grid, 64 * WAVES, 0, dw::as_stream(stream)>>>(
            table, vocab_size, dim, rows, keys, tab, line_off, r0, r1, out, capacity, status);
    DW_LAUNCH_CHECK("dw_embtext_write");
    return DW_OK;
}

}  // extern "C"
