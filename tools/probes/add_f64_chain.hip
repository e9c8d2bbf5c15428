// add_f64_chain.hip - the latency of a dependent float64 addition on one wave (gfx950): the floor of every "blocks in order"
// summation of this project (the estimate's finish walks one addition per 256-particle block, csrc/cluster.hip).
//
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o /tmp/addchain tools/probes/add_f64_chain.hip && /tmp/addchain
//
// One workgroup of one wave; every lane adds the same register operand to its accumulator `adds` times, each addition waiting
// for the one before it (no fast-math: the compiler may not reassociate).  Reported: shader clocks and nanoseconds per addition
// from the wave's own counters (s_memtime, s_memrealtime at 100 MHz), and from device events around the launch for the two
// lengths (their difference removes the launch).
#include <hip/hip_runtime.h>

#include <cstdio>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

__global__ __launch_bounds__(64) void k_chain(const double* __restrict__ in, double* __restrict__ out, long long* __restrict__ clk, int trips) {
    const double d = in[threadIdx.x];
    double r = in[64 + threadIdx.x];
    const long long w0 = wall_clock64(), c0 = clock64();
    for (int i = 0; i < trips; ++i) {
#pragma unroll
        for (int j = 0; j < 64; ++j) r = r + d;
    }
    const long long c1 = clock64(), w1 = wall_clock64();
    out[threadIdx.x] = r;
    if (threadIdx.x == 0) { clk[0] = c1 - c0; clk[1] = w1 - w0; }
}

int main() {
    double *in, *out;
    long long* clk;
    CK(hipMalloc(&in, 128 * sizeof(double)));
    CK(hipMalloc(&out, 64 * sizeof(double)));
    CK(hipMalloc(&clk, 2 * sizeof(long long)));
    double h[128];
    for (int i = 0; i < 128; ++i) h[i] = 1.0 + i * 1e-3;
    CK(hipMemcpy(in, h, sizeof(h), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    float ms[2] = {0, 0};
    const int trips[2] = {64, 1024};  // 4096 and 65536 dependent additions
    for (int rep = 0; rep < 4; ++rep) {
        for (int v = 0; v < 2; ++v) {
            CK(hipEventRecord(e0, 0));
            hipLaunchKernelGGL(k_chain, dim3(1), dim3(64), 0, 0, in, out, clk, trips[v]);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms[v], e0, e1));
            long long c[2];
            CK(hipMemcpy(c, clk, sizeof(c), hipMemcpyDeviceToHost));
            const double adds = 64.0 * trips[v];
            if (rep) printf("adds %6.0f  shader clocks/add %.3f  ns/add (100 MHz counter) %.3f  launch %.2f us\n", adds, c[0] / adds, c[1] * 10.0 / adds, ms[v] * 1e3);
        }
        if (rep) printf("  events: ns/add from the difference of the two lengths %.3f\n", (ms[1] - ms[0]) * 1e6 / (64.0 * (trips[1] - trips[0])));
    }
    return 0;
}
