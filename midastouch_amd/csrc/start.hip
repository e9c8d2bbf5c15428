// start.hip - the start of B particle sets on the device: init_filter (modules/particle_filter.py:129-145) and the projection onto
// the codebook that follows it (filter/filter.py:159-160), each as ONE launch with the row as grid.y and one lane per particle.
// The frame kernels are not involved: these two write the poses and hints a first frame reads.
#include "start.hpp"

#include "list_scan.hpp"  // nn6_wave
#include "pose.hpp"

namespace midas {

// Tn = [R | t] of init_filter: scipy's extrinsic "zyx" rotation of the float32 degrees (rot[0] about z first, then rot[1] about y,
// then rot[2] about x: R = Rx(rot[2]) Ry(rot[1]) Rz(rot[0])), evaluated in float64 and rounded to float32 - the reference stores
// the float64 matrix into a float32 Tn before the product.
MD void start_transform(const float* tn, const float* rot, float* Tn) {
    const double D2R = 0.017453292519943295;
    double sa, ca, sb, cb, sc, cc;
    sincos((double)rot[0] * D2R, &sa, &ca);
    sincos((double)rot[1] * D2R, &sb, &cb);
    sincos((double)rot[2] * D2R, &sc, &cc);
    Tn[0] = (float)(cb * ca);                 Tn[1] = (float)(-(cb * sa));              Tn[2] = (float)sb;           Tn[3] = tn[0];
    Tn[4] = (float)(cc * sa + sc * sb * ca);  Tn[5] = (float)(cc * ca - sc * sb * sa);  Tn[6] = (float)(-(sc * cb));  Tn[7] = tn[1];
    Tn[8] = (float)(sc * sa - cc * sb * ca);  Tn[9] = (float)(sc * ca + cc * sb * sa);  Tn[10] = (float)(cc * cb);    Tn[11] = tn[2];
    Tn[12] = 0.f; Tn[13] = 0.f; Tn[14] = 0.f; Tn[15] = 1.f;
}

// Row b = blockIdx.y: slots [0, n_rows[b]) of poses[b] := gt[b] @ Tn(slot); the slots behind are left alone.  The row's gt, sigmas
// and count sit at addresses that depend on blockIdx alone.  Draws (tn == nullptr): philox_normals6 keyed seed + b, slot keys from
// 0, scaled as the motion noise is (pose.hpp noise_draws), at the step word of this start.
__global__ __launch_bounds__(64) void k_init_particles_batch(int64_t cap, const int32_t* __restrict__ n_rows, const float* __restrict__ gt16,
                                                             const float* __restrict__ sig, uint64_t seed, uint64_t step,
                                                             const float* __restrict__ tn_arr, const float* __restrict__ rot_arr,
                                                             float* __restrict__ poses) {
    const int64_t b = blockIdx.y, i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t n = n_rows[b];
    if (i >= n || i >= cap) return;
    float G[16], tn[3], rot[3], Tn[16], P[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) G[k] = gt16[b * 16 + k];
    const float std_t = sig[b * 2], std_r = sig[b * 2 + 1];
    const int64_t slot = b * cap + i;
    noise_draws(slot, i, tn_arr, rot_arr, std_t, std_r, seed + (uint64_t)b, step, tn, rot);
    start_transform(tn, rot, Tn);
    mat4_mul(G, Tn, P);
    store_pose(poses + slot * 16, P);
}

// Row b: slots [0, n_rows[b]) of poses[b] := the codebook pose nearest to each, hint[b] := its index - the feature of k_feature, the
// search of k_nn6 without a hint and the rows k_gather_rows copies, on the row's own object.  A wave holds the 64 slots a wave of
// those launches on the row's slice holds, so the search runs lane for lane as theirs.
template <bool SET>
__global__ __launch_bounds__(64) void k_project_batch(const ObjectRecord* __restrict__ recs, const int32_t* __restrict__ row_object,
                                                      TreeView<Kd6> tv1, const float* __restrict__ cb1, int64_t cap,
                                                      const int32_t* __restrict__ n_rows, float wt, float wr, float* __restrict__ poses,
                                                      int32_t* __restrict__ hint) {
    __shared__ float s_cd[KD_MAX_LEVELS * 64];
    const int64_t b = blockIdx.y, i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    int64_t n = n_rows[b];
    n = n < cap ? n : cap;
    if ((int64_t)blockIdx.x * 64 >= n) return;  // (the whole wave)
    const bool live = i < n;
    const int64_t slot = b * cap + i;
    float f[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
        float P[16];
        load_pose(poses + slot * 16, P);
        se3_feature(P, wt, wr, f);
    }
    int32_t bi;
    float bd;
    const float* cbp;
    if (SET) {
        const ObjectRecord& r = recs[row_object[b]];
        cbp = r.cb_poses;
        nn6_wave(r.t6, f, live, -1, bi, bd, s_cd);
    } else {
        cbp = cb1;
        nn6_wave(tv1, f, live, -1, bi, bd, s_cd);
    }
    if (live) {
        const float4* src = reinterpret_cast<const float4*>(cbp + (int64_t)bi * 16);
        float4* dst = reinterpret_cast<float4*>(poses + slot * 16);
        const float4 r0 = src[0], r1 = src[1], r2 = src[2], r3 = src[3];
        dst[0] = r0; dst[1] = r1; dst[2] = r2; dst[3] = r3;
        hint[slot] = bi;
    }
}

// the rows' counts in the context's scratch (one small upload; nothing comes back) and the largest of them
static int upload_counts(midas_ctx* ctx, int32_t B, const int32_t* n_host, const int32_t** n_dev, int64_t* n_max) {
    void* p;
    if (int rc = midas_scratch(ctx, (size_t)B * sizeof(int32_t), &p)) return rc;
    MIDAS_HIP_CHECK(ctx, hipMemcpyAsync(p, n_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    int64_t m = 0;
    for (int32_t b = 0; b < B; ++b) m = n_host[b] > m ? n_host[b] : m;
    *n_dev = (const int32_t*)p;
    *n_max = m;
    return MIDAS_OK;
}

int launch_init_particles_batch(midas_ctx* ctx, int32_t B, int64_t cap, const int32_t* n_host, const float* gt16, const float* sig,
                                uint64_t seed, uint64_t step, const float* tn, const float* rot, float* poses) {
    const int32_t* n_dev;
    int64_t n_max;
    if (int rc = upload_counts(ctx, B, n_host, &n_dev, &n_max)) return rc;
    hipLaunchKernelGGL(k_init_particles_batch, dim3((unsigned)ceil_div(n_max, 64), (unsigned)B), dim3(64), 0, ctx->stream, cap, n_dev, gt16,
                       sig, seed, step, tn, rot, poses);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

int launch_project_batch(midas_ctx* ctx, const midas_object_set* set, const midas_tree* tree6, const float* cb_poses, int32_t B,
                         int64_t cap, const int32_t* n_host, float* poses, int32_t* hint) {
    const int32_t* n_dev;
    int64_t n_max;
    if (int rc = upload_counts(ctx, B, n_host, &n_dev, &n_max)) return rc;
    // the weights of midas_se3_feature at its default w = 0.01 (particles.hip launch_se3_feature)
    const float w = 0.01f, wt = (float)(1.0 - (double)w), wr = w;
    const dim3 grid((unsigned)ceil_div(n_max, 64), (unsigned)B);
    if (set)
        hipLaunchKernelGGL((k_project_batch<true>), grid, dim3(64), 0, ctx->stream, set->recs, set->row_object, TreeView<Kd6>(), nullptr, cap,
                           n_dev, wt, wr, poses, hint);
    else
        hipLaunchKernelGGL((k_project_batch<false>), grid, dim3(64), 0, ctx->stream, nullptr, nullptr, view_of<Kd6>(tree6), cb_poses, cap,
                           n_dev, wt, wr, poses, hint);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

}  // namespace midas
