// api_loop.hip - the loop engine's entry points: the whole loop body on a variable-size particle set, for one trajectory
// (midas_loop_step) and for B per launch (midas_loop_step_batch, midas_loop_step_batch_draws, midas_loop_step_batch_wide; with every row on an
// object of its own: midas_object_set_create / _destroy and midas_loop_step_batch_objects; with the filter's parameters per row as
// well: midas_loop_step_batch_rows).  One argument check for the six.
#include <new>
#include <vector>

#include "api_entry.hpp"
#include "tree_search.hpp"  // view_of: the trees as an object record holds them

using namespace midas;

// single: any capacity the blocked scan takes, a bound below it (grid_n), any draws, any selection.
// batch: the small-set regime with device draws and ties by index; batch_draws: that regime with host draws and either tie rule
// (include/midas_hip.h).
// batch_wide: batch's draws and tie rule for up to MIDAS_LOOP_BATCH_WIDE_MAX_CAP particles a trajectory, B * cap <= 2^24.
enum class LoopRegime { single, batch, batch_draws, batch_wide };

static int loop_args_check(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                           const midas_loop_args* args, int32_t phases, LoopRegime regime, int32_t B = 1, int64_t log_stride = 0,
                           const midas_object_set* objects = nullptr) {  // objects: in place of cb, the trees and args->cb_poses_dev
    // the four phases; beyond them only the form of the centres, which belongs to the phase that takes them: alone, or beside other
    // phases only, it selects nothing (one condition: a refused mask names the phases' rule it broke)
    MIDAS_REQUIRE(ctx, args != nullptr && phases != 0 &&
                           ((phases & ~15) == 0 || ((phases & ~15) == MIDAS_LOOP_CENTERS_LOGMAP && (phases & MIDAS_LOOP_ANNEAL))));
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
    if (objects) MIDAS_REQUIRE(ctx, batch && objects->ctx == ctx && objects->B == B);
    if (phases & MIDAS_LOOP_FRONT) {
        if (!objects) {
            MIDAS_REQUIRE(ctx, cb && tree6 && tree3 && tree6->dim == 6 && tree3->dim == 3 && tree6->K == cb->K);
            MIDAS_REQUIRE(ctx, s.odom16_dev && s.code_dev && s.cb_poses_dev && (uintptr_t)s.cb_poses_dev % 16 == 0);
        } else {  // (the set's creation checked every object's codebook, trees and poses; args->cb_poses_dev is not read)
            MIDAS_REQUIRE(ctx, s.odom16_dev && s.code_dev);
        }
        if (batch) {  // every trajectory's particle waves score the rows they need from its own code
            MIDAS_REQUIRE(ctx, objects ? (uintptr_t)s.code_dev % 16 == 0 : sparse_score_ok(cb, s.code_dev));
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

// ---- rows on different objects ------------------------------------------------------------------------------------------------
MIDAS_EXPORT int midas_object_set_create(midas_ctx* ctx, int32_t n_obj, const midas_codebook* const* cbs, const midas_tree* const* tree6s,
                                         const midas_tree* const* tree3s, const float* const* cb_poses_devs, int32_t B,
                                         const int32_t* row_object, midas_object_set** out) {
    MIDAS_ENTER(ctx);
    const auto refuse = [&](const char* why) { return midas_set_error(ctx, MIDAS_ERR_INVALID, "midas_object_set_create", why); };
    if (!out) return refuse("no place for the handle");
    if (n_obj < 1 || !cbs || !tree6s || !tree3s || !cb_poses_devs) return refuse("an empty object set");
    if (B < 1 || B > 65535 || !row_object) return refuse("1 .. 65535 rows, each with its object");
    for (int32_t b = 0; b < B; ++b)
        if (row_object[b] < 0 || row_object[b] >= n_obj) return refuse("a row's object index outside [0, n_obj)");
    std::vector<ObjectRecord> recs((size_t)n_obj);
    int64_t K_max = 0;
    for (int32_t i = 0; i < n_obj; ++i) {
        const midas_codebook* cb = cbs[i];
        const midas_tree *t6 = tree6s[i], *t3 = tree3s[i];
        if (!cb || !t6 || !t3 || !cb_poses_devs[i]) return refuse("an object without codebook, trees or poses");
        if (cb->dtype != MIDAS_F32) return refuse("a codebook that is not float32");
        if (!(cb->D == 128 || cb->D == 256 || cb->D == 512 || cb->D == 1024)) return refuse("a codebook whose D is not 128, 256, 512 or 1024");
        if (cb->D != cbs[0]->D) return refuse("codebooks of different D");
        if ((uintptr_t)cb->emb % 16 != 0) return refuse("misaligned codebook rows");
        if (t6->dim != 6 || t3->dim != 3) return refuse("a tree of the wrong dimension");
        if (t6->K != cb->K) return refuse("a 6-d index whose K differs from its codebook's");
        if ((uintptr_t)cb_poses_devs[i] % 16 != 0) return refuse("misaligned codebook poses");
        ObjectRecord& r = recs[(size_t)i];
        r.t6 = view_of<Kd6>(t6);
        r.t3 = view_of<Kd3>(t3);
        r.vlist = (t6->vlist && t6->vlist_mesh == t3) ? (const MeshRec*)t6->vlist : nullptr;  // as fill_particle_update
        r.vscr = r.vlist ? (const MeshScr*)t6->vscr : nullptr;
        r.field = t3->field;
        r.emb = (const float*)cb->emb; r.norms = cb->norms; r.K = cb->K; r.cb_poses = cb_poses_devs[i];
        K_max = cb->K > K_max ? cb->K : K_max;
    }
    std::vector<const float*> rows((size_t)B);
    for (int32_t b = 0; b < B; ++b) rows[(size_t)b] = cb_poses_devs[row_object[b]];
    const size_t rec_bytes = recs.size() * sizeof(ObjectRecord), row_bytes = rows.size() * sizeof(const float*);
    midas_object_set* set = new (std::nothrow) midas_object_set();
    if (!set) return midas_set_error(ctx, MIDAS_ERR_NOMEM, "new midas_object_set", "");
    if (hipMalloc(&set->dev, rec_bytes + row_bytes + (size_t)B * sizeof(int32_t)) != hipSuccess) {
        delete set;
        return midas_set_error(ctx, MIDAS_ERR_NOMEM, "hipMalloc(object set)", "");
    }
    char* d = (char*)set->dev;
    hipError_t e = hipMemcpy(d, recs.data(), rec_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + rec_bytes, rows.data(), row_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + rec_bytes + row_bytes, row_object, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(set->dev);
        delete set;
        return midas_set_error(ctx, MIDAS_ERR_HIP, "hipMemcpy(object set)", hipGetErrorString(e));
    }
    set->ctx = ctx; set->n_obj = n_obj; set->B = B; set->D = cbs[0]->D; set->K_max = K_max;
    set->recs = (const ObjectRecord*)d;
    set->cb_poses_rows = (const float* const*)(d + rec_bytes);
    set->row_object = (const int32_t*)(d + rec_bytes + row_bytes);
    set->cb_poses_row0 = rows[0];
    *out = set;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_object_set_destroy(midas_object_set* set) {
    if (!set) return MIDAS_OK;
    (void)hipStreamSynchronize(set->ctx->stream);
    (void)hipFree(set->dev);
    delete set;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_loop_step_batch_objects(midas_ctx* ctx, const midas_object_set* set, const midas_loop_args* args, int32_t phases,
                                               int32_t B, int64_t log_stride, int32_t wide) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, set != nullptr && (wide == 0 || wide == 1));
    const LoopRegime regime = wide ? LoopRegime::batch_wide : LoopRegime::batch_draws;
    if (int rc = loop_args_check(ctx, nullptr, nullptr, nullptr, args, phases, regime, B, log_stride, set)) return rc;
    return launch_loop_step_batch_objects(ctx, set, *args, phases, log_stride, wide != 0);
}

// ---- ... and the filter's parameters per row -------------------------------------------------------------------------------------
MIDAS_EXPORT int midas_loop_step_batch_rows(midas_ctx* ctx, const midas_object_set* set, const midas_loop_args* args,
                                            const midas_loop_row_params* rows_dev, int32_t phases, int32_t B, int64_t log_stride,
                                            int32_t wide) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, set != nullptr && (wide == 0 || wide == 1));
    MIDAS_REQUIRE(ctx, rows_dev != nullptr && (uintptr_t)rows_dev % 8 == 0);
    // device draws and ties by index: the counted draw of a seeded frame carries one std per segment, the ATen walk stays shared-parameter
    const LoopRegime regime = wide ? LoopRegime::batch_wide : LoopRegime::batch;
    if (int rc = loop_args_check(ctx, nullptr, nullptr, nullptr, args, phases, regime, B, log_stride, set)) return rc;
    MIDAS_REQUIRE(ctx, args->stream_draws == 0);
    return launch_loop_step_batch_objects(ctx, set, *args, phases, log_stride, wide != 0, rows_dev);
}

}  // extern "C"
