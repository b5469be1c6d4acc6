// The float64 MFMA rate one MI355X sustains: a bare loop of v_mfma_f64_16x16x4_f64 over eight
// independent accumulators per wave, nothing else in flight. It is the yardstick
// scripts/microbench/nodeclf.py holds dw_node_softmax's FLOP/s against, in the role
// dw_stream_copy plays for bytes.
//
//   hipcc --offload-arch=gfx950 -O3 -o scripts/microbench/mfma_f64_peak scripts/microbench/mfma_f64_peak.hip
//   ./scripts/microbench/mfma_f64_peak [iterations]
//
// Prints one JSON line: FLOP/s (2 * 16 * 16 * 4 per instruction), median of 7 timed launches
// after 2 warm-up launches, for 1, 2 and 4 waves per SIMD.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t e = (x);                                                       \
        if (e != hipSuccess) {                                                    \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int CHAINS = 8;

__global__ void __launch_bounds__(256) k_mfma_f64(double *out, int iters) {
    d4 acc[CHAINS];
#pragma unroll
    for (int j = 0; j < CHAINS; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
    const double a = 1e-3 * (threadIdx.x & 63), b = 1e-3 * (threadIdx.x >> 6) + 1e-6;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int j = 0; j < CHAINS; ++j)
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < CHAINS; ++j) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
    out[blockIdx.x * (int64_t)blockDim.x + threadIdx.x] = s;
}

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 1000;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    double *out;
    CHECK(hipMalloc(&out, sizeof(double) * 256 * cus * 4));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    printf("{\"part\": \"mfma_f64_peak\", \"cus\": %d, \"iterations\": %d", cus, iters);
    double best = 0.0;
    for (int per_cu = 1; per_cu <= 4; per_cu *= 2) {   // blocks of 4 waves per CU
        const int blocks = cus * per_cu;
        float ms[7];
        for (int r = -2; r < 7; ++r) {
            CHECK(hipEventRecord(e0));
            hipLaunchKernelGGL(k_mfma_f64, dim3(blocks), dim3(256), 0, 0, out, iters);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            CHECK(hipGetLastError());
            if (r >= 0) CHECK(hipEventElapsedTime(&ms[r], e0, e1));
        }
        std::sort(ms, ms + 7);
        const double flop = 2.0 * 16 * 16 * 4 * CHAINS * (double)iters * 4.0 * blocks;
        const double rate = flop / (ms[3] * 1e-3);
        best = std::max(best, rate);
        printf(", \"waves_per_simd_%d_flops\": %.6g, \"waves_per_simd_%d_ms\": %.4f", per_cu, rate,
               per_cu, ms[3]);
    }
    printf(", \"flops\": %.6g}\n", best);
    CHECK(hipFree(out));
    return 0;
}
