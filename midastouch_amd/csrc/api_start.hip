// api_start.hip - the entry points of the device start: midas_init_particles_batch and midas_project_batch (start.hip).  Every check
// stands in front of the first enqueue: a refused call leaves the stream as it was.
#include "api_entry.hpp"
#include "start.hpp"

using namespace midas;

// 1 <= n_host[b] <= cap for every row
static bool counts_ok(int32_t B, int64_t cap, const int32_t* n_host) {
    if (!n_host) return false;
    for (int32_t b = 0; b < B; ++b)
        if (n_host[b] < 1 || n_host[b] > cap) return false;
    return true;
}

extern "C" {

MIDAS_EXPORT int midas_init_particles_batch(midas_ctx* ctx, int32_t B, int64_t cap, const int32_t* n_host, const float* gt16_dev,
                                            const float* sig_dev, uint64_t seed, uint32_t draw, const float* tn_dev, const float* rot_dev,
                                            float* poses_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, B >= 1 && B <= 65535 && cap >= 1 && (int64_t)B * cap <= ((int64_t)1 << 31));
    MIDAS_REQUIRE(ctx, counts_ok(B, cap, n_host));
    MIDAS_REQUIRE(ctx, gt16_dev && sig_dev && poses_dev && (uintptr_t)poses_dev % 16 == 0);
    MIDAS_REQUIRE(ctx, (tn_dev == nullptr) == (rot_dev == nullptr));
    // frames count their Philox step words up from 0: starts count theirs down from the top of the word
    return launch_init_particles_batch(ctx, B, cap, n_host, gt16_dev, sig_dev, seed, (uint64_t)(0xFFFFFFFFu - draw), tn_dev, rot_dev, poses_dev);
}

MIDAS_EXPORT int midas_project_batch(midas_ctx* ctx, const midas_object_set* set, const midas_codebook* cb, const midas_tree* tree6,
                                     const float* cb_poses_dev, int32_t B, int64_t cap, const int32_t* n_host, float* poses_dev,
                                     int32_t* hint_out_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, B >= 1 && B <= 65535 && cap >= 1 && (int64_t)B * cap <= ((int64_t)1 << 31));
    MIDAS_REQUIRE(ctx, counts_ok(B, cap, n_host));
    MIDAS_REQUIRE(ctx, poses_dev && hint_out_dev && (uintptr_t)poses_dev % 16 == 0);
    if (set) {  // (the set's creation checked every object's codebook, tree and poses)
        MIDAS_REQUIRE(ctx, set->ctx == ctx && set->B == B);
    } else {
        MIDAS_REQUIRE(ctx, cb && tree6 && tree6->dim == 6 && tree6->K == cb->K);
        MIDAS_REQUIRE(ctx, cb_poses_dev && (uintptr_t)cb_poses_dev % 16 == 0);
    }
    return launch_project_batch(ctx, set, tree6, cb_poses_dev, B, cap, n_host, poses_dev, hint_out_dev);
}

}  // extern "C"
