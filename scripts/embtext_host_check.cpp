// Stand-alone sanitizer check of dw_embtext_host (csrc/dw_host.cpp with csrc/dw_f32text.h): the
// hard values of the shortest-decimal conversion, formatted into heap buffers of exactly the
// announced size so that AddressSanitizer sees any byte written past a line. Build and run from
// the repository root, as a plain executable:
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I include scripts/embtext_host_check.cpp \
//       deepwalk-and-node2vec_amd/csrc/dw_host.cpp deepwalk-and-node2vec_amd/csrc/dw_abi.cpp \
//       -o /tmp/embtext_host_check && /tmp/embtext_host_check
//
// Every token must read back (strtof) as the float it came from, hold at most 19 bytes, and the
// row-range writes must concatenate to the whole text.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dw_hip.h"

static uint32_t bits_of(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}

static float float_of(uint32_t b) {
    float x;
    memcpy(&x, &b, 4);
    return x;
}

#define CHECK(cond, ...)              \
    do {                              \
        if (!(cond)) {                \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");    \
            return 1;                 \
        }                             \
    } while (0)

int main() {
    std::vector<uint32_t> bits;
    for (int k = -149; k <= 127; ++k) {
        const uint32_t p = bits_of(ldexpf(1.0f, k));
        bits.insert(bits.end(), {p - 1, p, p + 1});
    }
    for (int k = -45; k <= 38; ++k) {
        char buf[16];
        snprintf(buf, sizeof(buf), "1e%d", k);
        const uint32_t p = bits_of(strtof(buf, nullptr));
        for (int o = -2; o <= 2; ++o)
            if (static_cast<int64_t>(p) + o >= 0 && p + o < 0x7F800000u) bits.push_back(p + o);
    }
    for (float v : {1e-4f, 1e16f, 1e-5f, 1e15f, 9999999e9f, 16777216.0f})
        for (int o = -3; o <= 3; ++o) bits.push_back(bits_of(v) + o);
    bits.insert(bits.end(), {1u, 0x007FFFFFu, 0x00800000u, 0x7F7FFFFFu});
    const size_t n_pos = bits.size();
    for (size_t i = 0; i < n_pos; ++i) bits.push_back(bits[i] | 0x80000000u);
    bits.insert(bits.end(), {0u, 0x80000000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00000u,
                             0x7F800001u, 0xFFFFFFFFu});
    uint32_t x = 12345u;   // and pseudo-random patterns
    for (int i = 0; i < 200000; ++i) {
        x = x * 1664525u + 1013904223u;
        bits.push_back(x);
    }

    const int32_t dim = 7;
    const int64_t n = static_cast<int64_t>(bits.size()) / dim;
    std::vector<float> table(static_cast<size_t>(n) * dim);
    memcpy(table.data(), bits.data(), table.size() * 4);
    std::vector<int64_t> keys(n), line_off(n + 1);
    for (int64_t i = 0; i < n; ++i) keys[i] = i * 1000003;
    int32_t status = 0;
    int rc = dw_embtext_host(table.data(), n, dim, nullptr, n, keys.data(), nullptr, nullptr,
                             line_off.data(), 0, n, nullptr, 0, &status);
    CHECK(rc == DW_OK, "sizes: %s", dw_last_error_string());
    CHECK(status == DW_S_NONFINITE, "status %d", status);

    std::string whole;
    for (int64_t r0 = 0; r0 < n;) {   // ranges of 1, 2, 3, .. rows, each in a buffer of its own
        const int64_t r1 = r0 + 1 + (r0 % 97) < n ? r0 + 1 + (r0 % 97) : n;
        const int64_t size = line_off[r1] - line_off[r0];
        uint8_t *buf = static_cast<uint8_t *>(malloc(static_cast<size_t>(size)));
        rc = dw_embtext_host(table.data(), n, dim, nullptr, n, keys.data(), nullptr, nullptr,
                             line_off.data(), r0, r1, buf, size, &status);
        CHECK(rc == DW_OK, "write: %s", dw_last_error_string());
        whole.append(reinterpret_cast<char *>(buf), static_cast<size_t>(size));
        rc = dw_embtext_host(table.data(), n, dim, nullptr, n, keys.data(), nullptr, nullptr,
                             line_off.data(), r0, r1, buf, size - 1, &status);
        CHECK(rc == DW_E_INVALID_ARG, "a buffer one byte short was accepted");
        free(buf);
        r0 = r1;
    }
    CHECK(static_cast<int64_t>(whole.size()) == line_off[n], "total size");

    size_t pos = 0;
    int64_t checked = 0;
    for (int64_t r = 0; r < n; ++r) {
        const size_t end = whole.find('\n', pos);
        CHECK(end != std::string::npos && static_cast<int64_t>(end + 1) == line_off[r + 1],
              "line %lld does not end at its offset", (long long)r);
        std::string line = whole.substr(pos, end - pos);
        size_t p = line.find(' ');
        CHECK(line.substr(0, p) == std::to_string(keys[r]), "key of line %lld", (long long)r);
        for (int c = 0; c < dim; ++c) {
            CHECK(p != std::string::npos, "line %lld is short", (long long)r);
            const size_t q = line.find(' ', p + 1);
            const std::string tok = line.substr(p + 1, q == std::string::npos ? q : q - p - 1);
            const float v = float_of(bits[r * dim + c]);
            CHECK(!tok.empty() && tok.size() <= 19, "token '%s'", tok.c_str());
            if (isnan(v)) {
                CHECK(tok == "nan", "token '%s' for a NaN", tok.c_str());
            } else {
                CHECK(bits_of(strtof(tok.c_str(), nullptr)) == bits[r * dim + c],
                      "token '%s' does not read back as %08x", tok.c_str(), bits[r * dim + c]);
            }
            ++checked;
            p = q;
        }
        CHECK(p == std::string::npos, "line %lld is long", (long long)r);
        pos = end + 1;
    }
    printf("embtext_host_check: %lld tokens in %lld lines, %zu bytes: ok\n", (long long)checked,
           (long long)n, whole.size());
    return 0;
}
