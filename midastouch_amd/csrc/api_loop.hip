// api_loop.hip - the loop engine's entry points: the whole loop body on a variable-size particle set, for one trajectory
// (midas_loop_step) and for B per launch (midas_loop_step_batch, midas_loop_step_batch_draws, midas_loop_step_batch_wide).  One
// argument check for the four.
#include "api_entry.hpp"

using namespace midas;

// single: any capacity the blocked scan takes, a bound below it (grid_n), any draws, any selection.
// batch: the small-set regime with device draws and ties by index; batch_draws: that regime with host draws and either tie rule
// (include/midas_hip.h).
// batch_wide: batch's draws and tie rule for up to MIDAS_LOOP_BATCH_WIDE_MAX_CAP particles a trajectory, B * cap <= 2^24.
enum class LoopRegime { single, batch, batch_draws, batch_wide };

static int loop_args_check(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                           const midas_loop_args* args, int32_t phases, LoopRegime regime, int32_t B = 1, int64_t log_stride = 0) {
    MIDAS_REQUIRE(ctx, args != nullptr && phases != 0 && (phases & ~15) == 0);
    const midas_loop_args& s = *args;
    const bool batch = regime != LoopRegime::single;
    MIDAS_REQUIRE(ctx, B >= 1 && B <= 65535);
    MIDAS_REQUIRE(ctx, s.cap > 0 && s.ctl_i_dev && s.ctl_d_dev);
    if (regime == LoopRegime::batch_wide)
        MIDAS_REQUIRE(ctx, s.cap <= MIDAS_LOOP_BATCH_WIDE_MAX_CAP && (int64_t)B * s.cap <= ((int64_t)1 << 24));
    else if (batch)
        MIDAS_REQUIRE(ctx, s.cap <= MIDAS_LOOP_BATCH_MAX_CAP);
    else
        MIDAS_REQUIRE(ctx, ceil_div(s.cap, SCAN_BLOCK) <= LAZY_MAX_BLOCKS);
    MIDAS_REQUIRE(ctx, s.poses_dev && s.poses_prop_dev && s.poses_dev != s.poses_prop_dev && s.hint_dev && s.nn_idx_dev && s.valid_dev &&
                           s.x_dev && s.e_dev && s.weights_dev && s.weights_out_dev && s.labels_dev && s.labels_out_dev &&
                           s.labels_dev != s.labels_out_dev && s.src_dev && s.ridx_dev && s.scores_dev && s.cluster_poses_dev &&
                           s.cluster_stds_dev);
    MIDAS_REQUIRE(ctx, (uintptr_t)s.poses_dev % 16 == 0 && (uintptr_t)s.poses_prop_dev % 16 == 0);
    if (regime == LoopRegime::batch || regime == LoopRegime::batch_wide) {
        MIDAS_REQUIRE(ctx, s.tn_dev == nullptr && s.rot_dev == nullptr && s.u_dev == nullptr);
        MIDAS_REQUIRE(ctx, s.topk_ties == MIDAS_TOPK_TIES_INDEX);
    } else if (regime == LoopRegime::batch_draws) {
        MIDAS_REQUIRE(ctx, (s.tn_dev == nullptr) == (s.rot_dev == nullptr));
        MIDAS_REQUIRE(ctx, s.topk_ties == MIDAS_TOPK_TIES_INDEX || s.topk_ties == MIDAS_TOPK_TIES_ATEN_CPU);
    }
    if (batch) {
        MIDAS_REQUIRE(ctx, s.grid_n == 0 && s.anneal_frozen == 0);
        MIDAS_REQUIRE(ctx, s.log_dev == nullptr || log_stride >= MIDAS_LOOP_LOG_DOUBLES || B == 1);
    }
    if (phases & MIDAS_LOOP_FRONT) {
        MIDAS_REQUIRE(ctx, cb && tree6 && tree3 && tree6->dim == 6 && tree3->dim == 3 && tree6->K == cb->K);
        MIDAS_REQUIRE(ctx, s.odom16_dev && s.code_dev && s.cb_poses_dev && (uintptr_t)s.cb_poses_dev % 16 == 0);
        if (batch) {  // every trajectory's particle waves score the rows they need from its own code
            MIDAS_REQUIRE(ctx, sparse_score_ok(cb, s.code_dev));
            MIDAS_REQUIRE(ctx, s.score_stamps_dev != nullptr && s.score_epoch != 0);
        } else {
            MIDAS_REQUIRE(ctx, (s.tn_dev == nullptr) == (s.rot_dev == nullptr));
        }
    }
    if (phases & MIDAS_LOOP_DBSCAN) MIDAS_REQUIRE(ctx, s.eps > 0.0);
    // one DBSCAN pass for the batch: the batch entries only, within the cell tables' bound (a call without the phase does not look)
    MIDAS_REQUIRE(ctx, s.dbscan_batched == 0 || s.dbscan_batched == 1);
    if (s.dbscan_batched) MIDAS_REQUIRE(ctx, batch && (int64_t)B * s.cap <= MIDAS_DBSCAN_BATCH_MAX_POINTS);
    if (phases & MIDAS_LOOP_RESAMPLE)
        MIDAS_REQUIRE(ctx, s.resample_mode == MIDAS_RESAMPLE_MULTINOMIAL || s.resample_mode == MIDAS_RESAMPLE_SYSTEMATIC);
    return MIDAS_OK;
}

extern "C" {

MIDAS_EXPORT int midas_loop_step(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                                 const midas_loop_args* args, int32_t phases) {
    MIDAS_ENTER(ctx);
    if (int rc = loop_args_check(ctx, cb, tree6, tree3, args, phases, LoopRegime::single)) return rc;
    return launch_loop_step(ctx, cb, tree6, tree3, *args, phases);
}

MIDAS_EXPORT int midas_loop_step_batch(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                                       const midas_loop_args* args, int32_t phases, int32_t B, int64_t log_stride) {
    MIDAS_ENTER(ctx);
    if (int rc = loop_args_check(ctx, cb, tree6, tree3, args, phases, LoopRegime::batch, B, log_stride)) return rc;
    return launch_loop_step_batch(ctx, cb, tree6, tree3, *args, phases, B, log_stride);
}

MIDAS_EXPORT int midas_loop_step_batch_draws(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                                             const midas_loop_args* args, int32_t phases, int32_t B, int64_t log_stride) {
    MIDAS_ENTER(ctx);
    if (int rc = loop_args_check(ctx, cb, tree6, tree3, args, phases, LoopRegime::batch_draws, B, log_stride)) return rc;
    return launch_loop_step_batch(ctx, cb, tree6, tree3, *args, phases, B, log_stride);
}

MIDAS_EXPORT int midas_loop_step_batch_wide(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                                            const midas_loop_args* args, int32_t phases, int32_t B, int64_t log_stride) {
    MIDAS_ENTER(ctx);
    if (int rc = loop_args_check(ctx, cb, tree6, tree3, args, phases, LoopRegime::batch_wide, B, log_stride)) return rc;
    return launch_loop_step_batch(ctx, cb, tree6, tree3, *args, phases, B, log_stride, true);
}

}  // extern "C"
