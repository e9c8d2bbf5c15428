// mfma_f64_probe.hip - what v_mfma_f64_16x16x4_f64 computes, bit for bit, and how fast (sets k_score_mfma_f64's k-slot mapping).
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o mfma_f64_probe mfma_f64_probe.hip ; run on the GPU box
//  1. layout: small integers (exact), D = A B + C against the host with C/D at col = lane & 15, row = (lane >> 4) + 4 reg,
//     A[lane & 15][k = lane >> 4], B[k = lane >> 4][lane & 15].
//  2. arithmetic: per output, which model the result equals bit for bit - the k-ordered fma chain
//     fma(a3,b3, fma(a2,b2, fma(a1,b1, fma(a0,b0,c)))), the reversed chain, the pairwise sum c + ((p0 + p1) + (p2 + p3)) with exact
//     products, or the exactly rounded five-term sum (cases built so that only one rounding can give the answer) - over
//     cancellation-heavy, wide-exponent and random data, with A and B rows chosen per k-slot so that every output sees its own case.
//  3. subnormals: subnormal A / B inputs, subnormal products of normal inputs, subnormal C and results.
//  4. rate: back-to-back independent MFMAs with operands in registers, 1 / 2 / 4 / 8 accumulators, one and two waves per SIMD.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using f64x4 = __attribute__((ext_vector_type(4))) double;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// one tile per block of 64 threads: a[t][lane], b[t][lane], c[t][lane][4] -> d[t][lane][4]
__global__ void k_one(const double* a, const double* b, const double* c, double* d, int ntiles) {
    const int t = blockIdx.x, l = threadIdx.x;
    if (t >= ntiles) return;
    f64x4 acc = {c[(t * 64 + l) * 4 + 0], c[(t * 64 + l) * 4 + 1], c[(t * 64 + l) * 4 + 2], c[(t * 64 + l) * 4 + 3]};
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t * 64 + l], b[t * 64 + l], acc, 0, 0, 0);
    for (int r = 0; r < 4; ++r) d[(t * 64 + l) * 4 + r] = acc[r];
}

template <int NACC>
__global__ __launch_bounds__(512) void k_rate(double* out, int iters, double a0, double b0) {
    f64x4 acc[NACC];
    for (int t = 0; t < NACC; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    double a = a0 + threadIdx.x, b = b0;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < NACC; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
    }
    double s = 0.0;
    for (int t = 0; t < NACC; ++t) s += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3];
    if (s == 12345.678) out[0] = s;
}

// host models of one output: c, a[4], b[4]
static double m_chain(double c, const double* a, const double* b) { for (int k = 0; k < 4; ++k) c = std::fma(a[k], b[k], c); return c; }
static double m_rchain(double c, const double* a, const double* b) { for (int k = 3; k >= 0; --k) c = std::fma(a[k], b[k], c); return c; }
static double m_pair(double c, const double* a, const double* b) { return c + ((a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3])); }
static bool bits_eq(double x, double y) { uint64_t p, q; memcpy(&p, &x, 8); memcpy(&q, &y, 8); return p == q; }

int main() {
    // ---- 1. layout ----
    {
        std::vector<double> A(16 * 4), Bm(4 * 16), Cm(16 * 16), a(64), b(64), c(256), d(256);
        for (int m = 0; m < 16; ++m) for (int k = 0; k < 4; ++k) A[m * 4 + k] = m * 4 + k + 1;
        for (int k = 0; k < 4; ++k) for (int n = 0; n < 16; ++n) Bm[k * 16 + n] = (k + 1) * 100 + n * 7;  // asymmetric
        for (int m = 0; m < 16; ++m) for (int n = 0; n < 16; ++n) Cm[m * 16 + n] = 1000000 * m + 1000 * n;
        for (int l = 0; l < 64; ++l) {
            a[l] = A[(l & 15) * 4 + (l >> 4)];
            b[l] = Bm[(l >> 4) * 16 + (l & 15)];
            for (int r = 0; r < 4; ++r) c[l * 4 + r] = Cm[((l >> 4) + 4 * r) * 16 + (l & 15)];
        }
        double *da, *db, *dc, *dd;
        CK(hipMalloc(&da, 64 * 8)); CK(hipMalloc(&db, 64 * 8)); CK(hipMalloc(&dc, 256 * 8)); CK(hipMalloc(&dd, 256 * 8));
        CK(hipMemcpy(da, a.data(), 64 * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(db, b.data(), 64 * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(dc, c.data(), 256 * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, 0, da, db, dc, dd, 1);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(d.data(), dd, 256 * 8, hipMemcpyDeviceToHost));
        int bad = 0;
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 4; ++r) {
                const int m = (l >> 4) + 4 * r, n = l & 15;
                double want = Cm[m * 16 + n];
                for (int k = 0; k < 4; ++k) want += A[m * 4 + k] * Bm[k * 16 + n];
                bad += d[l * 4 + r] != want;
            }
        printf("layout: C/D col = lane&15, row = (lane>>4) + 4 reg; A[lane&15][lane>>4], B[lane>>4][lane&15]: %d of 256 wrong\n", bad);
        CK(hipFree(da)); CK(hipFree(db)); CK(hipFree(dc)); CK(hipFree(dd));
    }
    // ---- 2. / 3. arithmetic ----
    // Every output (m, n) gets its own four products: A row m and B column n are free per k, but an output shares A row m with
    // 15 others.  So each tile uses B[k][n] = 1 (or a power of two) and puts the case in A[m][k] and C[m][n]: 16 cases a tile
    // (the outputs of one row m repeat them with scaled B - still exact cases since powers of two scale exactly).
    const int NT = 20000;
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<double> a(NT * 64), b(NT * 64), c(NT * 256), d(NT * 256);
    std::vector<int> kind(NT);
    const char* kinds[] = {"random", "cancellation", "wide exponents", "ties (1 + 2^-53 + 2^-53)", "subnormal inputs",
                           "subnormal products", "subnormal C / results"};
    const int NK = 7;
    for (int t = 0; t < NT; ++t) {
        const int kd = t % NK;
        kind[t] = kd;
        for (int l = 0; l < 64; ++l) {
            const int k = l >> 4, i = l & 15;
            double av = U(rng), bv = std::ldexp(1.0, (int)(rng() % 5) - 2) * ((rng() & 1) ? 1 : -1);
            switch (kd) {
                case 1: av = (k == 1 || k == 2) ? std::ldexp(U(rng), 60) : U(rng); if (k == 2) av = -a[t * 64 + 16 + i] + std::ldexp(U(rng), 5); break;
                case 2: av = std::ldexp(U(rng), (int)(rng() % 200) - 100); break;
                case 3: av = k < 2 ? std::ldexp(1.0, -53) : (k == 2 ? std::ldexp(1.0, -54) * ((rng() & 1) ? 1 : -1) : 0.0); bv = 1.0; break;
                case 4: av = std::ldexp(U(rng), -1030 - (int)(rng() % 40)); bv = std::ldexp(1.0, (int)(rng() % 60)); break;
                case 5: av = std::ldexp(U(rng), -540); bv = std::ldexp(1.0 + 0.5 * U(rng), -500 - (int)(rng() % 30)); break;
                case 6: av = std::ldexp(U(rng), -1040); bv = 1.0; break;
            }
            a[t * 64 + l] = av;
            b[t * 64 + l] = bv;
        }
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 4; ++r) {
                double cv = U(rng);
                if (kd == 1) cv = std::ldexp(U(rng), 2);
                if (kd == 2) cv = std::ldexp(U(rng), (int)(rng() % 200) - 100);
                if (kd == 3) cv = 1.0;
                if (kd == 4 || kd == 5) cv = std::ldexp(U(rng), -1045);
                if (kd == 6) cv = std::ldexp(U(rng), -1050);
                c[(t * 64 + l) * 4 + r] = cv;
            }
    }
    double *da, *db, *dc, *dd;
    CK(hipMalloc(&da, a.size() * 8)); CK(hipMalloc(&db, b.size() * 8)); CK(hipMalloc(&dc, c.size() * 8)); CK(hipMalloc(&dd, d.size() * 8));
    CK(hipMemcpy(da, a.data(), a.size() * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(db, b.data(), b.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, c.data(), c.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_one, dim3(NT), dim3(64), 0, 0, da, db, dc, dd, NT);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(d.data(), dd, d.size() * 8, hipMemcpyDeviceToHost));
    long n[NK] = {}, chain[NK] = {}, rchain[NK] = {}, pair[NK] = {}, only_chain[NK] = {}, sub_out[NK] = {}, sub_kept[NK] = {};
    for (int t = 0; t < NT; ++t)
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 4; ++r) {
                const int m = (l >> 4) + 4 * r, nn = l & 15;
                double av[4], bv[4];
                for (int k = 0; k < 4; ++k) { av[k] = a[t * 64 + k * 16 + m]; bv[k] = b[t * 64 + k * 16 + nn]; }
                const double cv = c[(t * 64 + nn + 16 * (m & 3)) * 4 + (m >> 2)];  // C[m][n] sits in lane (m & 3) * 16 + n, reg m >> 2
                const double got = d[(t * 64 + l) * 4 + r];
                const int kd = kind[t];
                const double x0 = m_chain(cv, av, bv), x1 = m_rchain(cv, av, bv), x2 = m_pair(cv, av, bv);
                ++n[kd];
                chain[kd] += bits_eq(got, x0);
                rchain[kd] += bits_eq(got, x1);
                pair[kd] += bits_eq(got, x2);
                only_chain[kd] += bits_eq(got, x0) && !bits_eq(x0, x1) && !bits_eq(x0, x2);
                if (x0 != 0.0 && std::fabs(x0) < 2.2250738585072014e-308) { ++sub_out[kd]; sub_kept[kd] += bits_eq(got, x0); }
            }
    printf("arithmetic (outputs equal to each model, bit for bit):\n");
    for (int k = 0; k < NK; ++k)
        printf("  %-28s %8ld outputs: k-ordered fma chain %8ld, reversed chain %8ld, pairwise %8ld; chain only %7ld; subnormal results %7ld kept %7ld\n",
               kinds[k], n[k], chain[k], rchain[k], pair[k], only_chain[k], sub_out[k], sub_kept[k]);
    {   // the single-rounding discriminator by hand: 1 + 2^-53 + 2^-53 (chain: 1, one rounding: 1 + 2^-52)
        long ones = 0, wide = 0;
        for (int t = 3; t < NT; t += NK)
            for (int l = 0; l < 64; ++l) {
                const double got = d[(t * 64 + l) * 4 + 0];
                ones += got == 1.0;
                wide += got == 1.0 + std::ldexp(1.0, -52);
            }
        printf("  1 + 2^-53 + 2^-53 (+- 2^-54): results exactly 1.0: %ld, exactly 1 + 2^-52: %ld\n", ones, wide);
    }
    CK(hipFree(da)); CK(hipFree(db)); CK(hipFree(dc)); CK(hipFree(dd));
    // ---- 4. rate ----
    double* out;
    CK(hipMalloc(&out, 8));
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    auto run = [&](auto kern, int nacc, int threads, int iters) {
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        const int blocks = prop.multiProcessorCount;
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, 0, out, iters, 1.0, 2.0);
        (void)hipDeviceSynchronize();
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, 0, out, iters, 1.0, 2.0);
        (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1);
        const double per_simd = (double)(threads / 64) / 4.0 * iters * 4.0 * nacc;  // MFMAs issued per SIMD
        const double mfmas = (double)blocks * (threads / 64) * iters * 4.0 * nacc;
        printf("rate: %d accumulators, %d waves/SIMD: %.1f us, %.1f TFLOP/s, %.1f ns per MFMA per SIMD\n", nacc, threads / 256,
               ms * 1e3, mfmas * 2048.0 / (ms * 1e-3) / 1e12, ms * 1e6 / per_simd);
    };
    run(k_rate<1>, 1, 256, 4096);
    run(k_rate<2>, 2, 256, 2048);
    run(k_rate<4>, 4, 256, 1024);
    run(k_rate<8>, 8, 256, 512);
    run(k_rate<4>, 4, 512, 512);
    run(k_rate<16>, 16, 256, 256);
    CK(hipFree(out));
    return 0;
}
