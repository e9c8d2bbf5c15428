// start.hpp - the launchers of start.hip (the device start of B particle sets), as api_start.hip calls them.
#pragma once
#include "midas_internal.hpp"

namespace midas {

// init_filter for B rows in one launch.  n_host[b] in [1, cap], checked by the caller; step: the Philox step word of this start.
int launch_init_particles_batch(midas_ctx* ctx, int32_t B, int64_t cap, const int32_t* n_host, const float* gt16, const float* sig,
                                uint64_t seed, uint64_t step, const float* tn, const float* rot, float* poses);

// SE3_NN for B rows in one launch: set != nullptr: row b on object set->row_object[b]; else every row on (tree6, cb_poses).
int launch_project_batch(midas_ctx* ctx, const midas_object_set* set, const midas_tree* tree6, const float* cb_poses, int32_t B,
                         int64_t cap, const int32_t* n_host, float* poses, int32_t* hint);

}  // namespace midas
