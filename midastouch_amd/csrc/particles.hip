// particles.hip - stand-alone per-particle operators: SE(3) propagate (K2), 6-d pose feature (K3), pose checks and rmse.
// One lane owns one particle; workgroups are single waves (64 threads) to spread the N/64 waves evenly over the 256 CUs.
// (The trees and their search operators: tree.hip; the fused fronts of the step: front*.hip.)
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "pose.hpp"

namespace midas {

__global__ __launch_bounds__(64) void k_propagate(int64_t N, const float* __restrict__ in, float* __restrict__ out,
                                                  const float* __restrict__ odom, const float* __restrict__ tn,
                                                  const float* __restrict__ rot, float std_t, float std_r,
                                                  uint64_t seed, uint64_t step) {
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    float P[16], O[16], R[16];
    load_pose(in + n * 16, P);
#pragma unroll
    for (int i = 0; i < 16; ++i) O[i] = odom[i];
    propagate_one(n, n, P, O, tn, rot, std_t, std_r, seed, step, R);
    store_pose(out + n * 16, R);
}

__global__ __launch_bounds__(64) void k_feature(int64_t N, const float* __restrict__ poses, float wt, float wr,
                                                float* __restrict__ feat) {
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    float P[16], f[6];
    load_pose(poses + n * 16, P);
    se3_feature(P, wt, wr, f);
#pragma unroll
    for (int j = 0; j < 6; ++j) feat[n * 6 + j] = f[j];
}

// check_quats (modules/particle_filter.py:347-357): flag poses whose rotation yields a NaN or
// zero-norm quaternion.  theseus' to_quaternion is derived from trace / off-diagonal terms; a pose
// is flagged when any rotation entry is non-finite or the quaternion's squared norm
// (1 + tr)/4 + |axis|^2-style reconstruction collapses to 0 - in practice only NaN/Inf poses.
__global__ __launch_bounds__(256) void k_check_poses(int64_t N, const float* __restrict__ poses,
                                                     uint8_t* __restrict__ flag, int32_t* __restrict__ count) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (n < N) {
        const float* P = poses + n * 16;
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc += P[i * 4 + j] * P[i * 4 + j];
        bad = !(acc > 0.0f) || !(acc < INFINITY);  // NaN, Inf or all-zero rotation
        flag[n] = bad ? 1 : 0;
    }
    unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (int32_t)__popcll(m));
}

__global__ __launch_bounds__(64) void k_rmse_part(int64_t N, const float* __restrict__ poses,
                                                  const float* __restrict__ gt, double* __restrict__ part) {
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    double a = 0.0, b = 0.0;
    if (n < N) {
        float P[16], G[16];
        load_pose(poses + n * 16, P);
#pragma unroll
        for (int i = 0; i < 16; ++i) G[i] = gt[i];
        rmse_terms(P, G, a, b);
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = a; part[2 * blockIdx.x + 1] = b; }
}

__global__ __launch_bounds__(256) void k_rmse_final(int64_t N, int nb, const double* __restrict__ part,
                                                    double* __restrict__ out2) {
    __shared__ double sa[4], sb[4];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) { a += part[2 * i]; b += part[2 * i + 1]; }
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) { sa[threadIdx.x >> 6] = a; sb[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = (sa[0] + sa[1]) + (sa[2] + sa[3]);
        b = (sb[0] + sb[1]) + (sb[2] + sb[3]);
        out2[0] = __builtin_sqrt(a / (double)N);
        out2[1] = __builtin_sqrt(b / (double)N);
    }
}

// =================================================================================================
// launchers
// =================================================================================================
int launch_se3_feature(midas_ctx* ctx, int64_t N, const float* poses, float w, float* feat6) {
    if (N == 0) return MIDAS_OK;
    // (1.0 - w) * t is a python-float times a float32 tensor in the reference: the scalar is rounded to float32
    const float wt = (float)(1.0 - (double)w), wr = w;
    hipLaunchKernelGGL(k_feature, dim3((unsigned)ceil_div(N, 64)), dim3(64), 0, ctx->stream, N, poses, wt, wr, feat6);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_propagate(midas_ctx* ctx, int64_t N, const float* in, float* out, const float* odom, const float* tn,
                     const float* rot, float std_t, float std_r, uint64_t seed, uint64_t step) {
    if (N == 0) return MIDAS_OK;
    hipLaunchKernelGGL(k_propagate, dim3((unsigned)ceil_div(N, 64)), dim3(64), 0, ctx->stream, N, in, out, odom, tn,
                       rot, std_t, std_r, seed, step);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_check_poses(midas_ctx* ctx, int64_t N, const float* poses, uint8_t* flag, int32_t* count) {
    MIDAS_HIP_CHECK(ctx, hipMemsetAsync(count, 0, sizeof(int32_t), ctx->stream));
    if (N == 0) return MIDAS_OK;
    hipLaunchKernelGGL(k_check_poses, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, poses, flag, count);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_rmse(midas_ctx* ctx, int64_t N, const float* poses, const float* gt16, double* out2) {
    MIDAS_REQUIRE(ctx, N > 0);
    const int nb = (int)ceil_div(N, 64);
    void* part;
    int rc = midas_scratch(ctx, (size_t)nb * 2 * sizeof(double), &part);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rmse_part, dim3(nb), dim3(64), 0, ctx->stream, N, poses, gt16, (double*)part);
    hipLaunchKernelGGL(k_rmse_final, dim3(1), dim3(256), 0, ctx->stream, N, nb, (const double*)part, out2);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int particle_update_blocks(int64_t N) { return (int)ceil_div(N, 64); }

// (the units cut out of this one are loaded with it: midas_ctx_create warms "particles")
MIDAS_WARM_DECL(tree) MIDAS_WARM_DECL(front) MIDAS_WARM_DECL(front_folded) MIDAS_WARM_DECL(front_batch)
int warm_particles() {
    hipFuncAttributes attr;
    int rc = (int)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&k_propagate));
    for (int (*w)() : {warm_tree, warm_front, warm_front_folded, warm_front_batch}) rc = rc ? rc : w();
    return rc;
}

}  // namespace midas
