// pose.hpp - per-lane pose arithmetic of the particle kernels: load / store, the motion model, rmse terms, wave reductions.
#pragma once
#include "midas_internal.hpp"
#include "midas_math.hpp"

namespace midas {

MD void load_pose(const float* p, float* P) {
    const float4* v = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float4 r = v[i];
        P[i * 4 + 0] = r.x; P[i * 4 + 1] = r.y; P[i * 4 + 2] = r.z; P[i * 4 + 3] = r.w;
    }
}
MD void store_pose(float* p, const float* P) {
    float4* v = reinterpret_cast<float4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = make_float4(P[i * 4 + 0], P[i * 4 + 1], P[i * 4 + 2], P[i * 4 + 3]);
}

// the part of the motion model that does not depend on the particle's pose: NO = O @ Tn(noise of slot n) - in two halves (the draws;
// the noise transform and the product), so that a caller may put a round trip of its own under each
MD void noise_draws(int64_t n, int64_t n_global, const float* tn_arr, const float* rot_arr, float std_t, float std_r, uint64_t seed,
                    uint64_t step, float* tn, float* rot) {
    if (tn_arr) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { tn[j] = tn_arr[n * 3 + j]; rot[j] = rot_arr[n * 3 + j]; }
        // (the host draws are consumed inside this branch: values still "in flight" at the join make the compiler wait
        // for every outstanding load there, including ones the caller issued to travel during the arithmetic below)
#pragma unroll
        for (int j = 0; j < 3; ++j) asm volatile("" : "+v"(tn[j]), "+v"(rot[j]));
    } else {
        float z[6];
        philox_normals6((uint64_t)n_global, seed, step, z);
#pragma unroll
        for (int j = 0; j < 3; ++j) { tn[j] = z[j] * std_t; rot[j] = z[3 + j] * std_r; }
    }
}
MD void noise_apply(const float* O, const float* tn, const float* rot, float* NO) {
    float Tn[16];
    noise_transform(tn, rot, Tn);
    mat4_mul(O, Tn, NO);
}
MD void noise_odom(int64_t n, int64_t n_global, const float* O, const float* tn_arr, const float* rot_arr, float std_t,
                   float std_r, uint64_t seed, uint64_t step, float* NO) {
    float tn[3], rot[3];
    noise_draws(n, n_global, tn_arr, rot_arr, std_t, std_r, seed, step, tn, rot);
    noise_apply(O, tn, rot, NO);
}

MD void propagate_one(int64_t n, int64_t n_global, const float* P, const float* O, const float* tn_arr,
                      const float* rot_arr, float std_t, float std_r, uint64_t seed, uint64_t step, float* out) {
    float NO[16];
    noise_odom(n, n_global, O, tn_arr, rot_arr, std_t, std_r, seed, step, NO);
    mat4_mul(P, NO, out);
}

// rmse partials: per-wave (sum e_t^2, sum ang^2) in float64
MD void rmse_terms(const float* P, const float* G, double& et2, double& ang2) {
    float dx = G[3] - P[3], dy = G[7] - P[7], dz = G[11] - P[11];
    float e2 = fmaf_(dz, dz, fmaf_(dy, dy, dx * dx));
    float tr = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float acc = G[i * 4] * P[i * 4];
        acc = fmaf_(G[i * 4 + 1], P[i * 4 + 1], acc);
        acc = fmaf_(G[i * 4 + 2], P[i * 4 + 2], acc);
        tr += acc;
    }
    float ang = acosf((tr - 1.0f) * 0.5f) * 57.2957795130823209f;
    if (ang != ang) ang = 0.0f;
    if (ang > 180.0f) ang -= 360.0f;
    if (ang < -180.0f) ang += 360.0f;
    et2 = (double)e2;
    ang2 = (double)ang * (double)ang;
}

MD double wave_sum(double v) { return wave_sum_ordered(v); }  // (the xor butterfly 32 .. 1 of the spec, by register moves: midas_math.hpp)
MD double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { double t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}
MD double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { double t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}

}  // namespace midas
