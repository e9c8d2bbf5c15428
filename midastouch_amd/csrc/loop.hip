// loop.hip - the reference's whole loop body on a variable-size particle set (midas_loop_step).
//
// filter/filter.py:150-190 changes the particle count every frame between the measurement update and the resample
// (particle_filter.annealing, modules/particle_filter.py:405-447).  Here the count lives in device memory
// (ctl_i[LOOP_I_N]); every kernel is launched over the capacity of the arrays and reads the live count itself, so a frame
// needs no host round trip:
//
//   FRONT     k_frame_front (front.hip, live count from the control block; sets up to 16 384: k_front_small) ->
//             loop_weights.hip: k_loop_xe (scores gathered, softmax numerators, per-block sums in the spec order) -> k_loop_weights
//             (S, isclose guard, masked weights, drift re-projection, rmse; loop_weights.hpp - in frames without DBSCAN this
//             work sits at the head of the cluster-moment launch instead, k_loop_weights_moments in cluster.hip)
//   DBSCAN    dbscan.hip
//   ANNEAL    k_loop_cluster_* (cluster.hip) -> loop_anneal_phase in one of four regimes: sets up to 16 384, anneal_small.hip:
//             k_loop_anneal_small (decision + selection by one workgroup, the centres' rotations by a second); larger, anneal.hip:
//             k_loop_decide (labels present, var = mean(stds), the annealing rule in float32 as torch evaluates it) ->
//             k_loop_select x 6 (radix select of the k-th smallest / largest weight) -> k_loop_compact_count / k_loop_compact
//             (the annealed set as an index list) -> k_loop_sort_chunks / k_loop_sort_rank (the duplicates in topk's output
//             order); the ATen tie rule: k_loop_std_two_pass -> k_loop_decide -> topk_aten.hip; frozen: k_loop_decide alone
//   RESAMPLE  loop_resample.hip: k_loop_scan (blocked prefix sums of (e * valid)[src]) -> k_loop_resample (n_set draws, exact
//             inverse search on cdf_i = (BP_b + lp_i) / total, gathers through src)
//   A frame whose uniforms come from a caller's stream (stream_draws) is split in front of RESAMPLE; its first call ends with
//   k_loop_scan -> k_loop_ndraw: ctl_i[NDRAW], the uniforms the reference's resampler draws - none on all-zero or NaN weights.
// Every phase is launched by the unit that holds its kernels (declared in midas_internal.hpp beside LoopGrid, what the phases are
// launched over); this unit holds what is left: the two frames, the single call and the batch, as the phases they run.
//
// Spec (oracle/oracle.py OracleLoop): identical to midas_filter_step where the two overlap; ties of the top-k selection go
// to the smaller index (torch's CUDA rule), or - midas_loop_args.topk_ties = MIDAS_TOPK_TIES_ATEN_CPU, the mode that replays a
// seeded run of the reference - to the members ATen's CPU kernel takes (topk_aten.hip).
#include <cstdlib>

#include "midas_internal.hpp"
#include "loop_weights.hpp"   // LoopWeightsRowsArgs: the merged weights travel from the front to the cluster-moment launch
#include "anneal_decide.hpp"  // LOOP_SMALL_MAX

namespace midas {

// ANNEAL, first half: the clusters' moments (with the merged weights at their head) into scratch the selection reads
static int loop_cluster_phase(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, const LoopWeightsParamRowsArgs* merged, LoopMoments& m) {
    const size_t Bz = (size_t)g.B;
    void *part, *cen, *sd, *cnt, *rot;
    int rc;
    if ((rc = midas_scratch(ctx, Bz * LOOP_MAX_CLUSTERS * 10 * sizeof(double), &rot))) return rc;
    if ((rc = midas_scratch(ctx, Bz * (size_t)ceil_div(g.cap, 256) * LOOP_MAX_CLUSTERS * 36 * sizeof(double), &part))) return rc;
    if ((rc = midas_scratch(ctx, Bz * LOOP_MAX_CLUSTERS * 16 * sizeof(float), &cen))) return rc;
    if ((rc = midas_scratch(ctx, Bz * LOOP_MAX_CLUSTERS * 3 * sizeof(float), &sd))) return rc;
    if ((rc = midas_scratch(ctx, Bz * LOOP_MAX_CLUSTERS * sizeof(int64_t), &cnt))) return rc;
    m = LoopMoments{(float*)cen, (float*)sd, (int64_t*)cnt, (double*)rot};
    return launch_loop_cluster(ctx, g.cap, s.ctl_i_dev, s.poses_prop_dev, s.weights_dev, s.labels_dev, (double*)part, m.cen, m.sd, m.cnt, m.rot,
                               merged, g.B, g.logmap, s.cluster_poses_dev);
}

int launch_loop_step(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* t6, const midas_tree* t3,
                     const midas_loop_args& s, int32_t phases) {
    // the grids cover `cap` particles: the capacity, or the caller's upper bound of the live count
    const int64_t cap = (s.grid_n > 0 && s.grid_n < s.cap) ? s.grid_n : s.cap;
    LoopGrid g;
    g.cap = cap;
    g.logmap = (phases & MIDAS_LOOP_CENTERS_LOGMAP) != 0;
#ifdef MIDAS_ANNEAL_CLOCKS
    g.clocks = s.ctl_d_dev;
#endif
    int rc;
    LoopWeightsParamRowsArgs wa{};
    bool weights_merged = false;
    if (phases & MIDAS_LOOP_FRONT) {
        ParticleUpdateArgs pa;
        fill_particle_update(pa, s, t6, t3, cap, s.poses_dev, s.hint_dev, s.valid_dev, s.score_stamps_dev,
                             (s.gt16_dev && s.part_rmse_dev) ? s.gt16_dev : nullptr, s.part_rmse_dev);
        pa.n_live = s.ctl_i_dev + LOOP_I_N;
        pa.scores = nullptr;  // deferred: k_loop_xe gathers the scores
        bool fused = false;
        if (ctx->overlap)
            if ((rc = launch_frame_front(ctx, t6, t3, pa, cb, s.code_dev, s.scores_dev, &fused))) return rc;
        if (!fused) {
            if ((rc = launch_score(ctx, cb, 1, s.code_dev, s.scores_dev))) return rc;
            pa.sp.stamps = nullptr;  // scored densely just above
            if ((rc = launch_particle_update(ctx, t6, t3, pa))) return rc;
        }
        static const bool merge_env = !(getenv("MIDAS_LOOP_MERGE") && atoi(getenv("MIDAS_LOOP_MERGE")) == 0);
        weights_merged = merge_env && loop_weights_mergeable(phases);
        if ((rc = loop_weights_phase(ctx, s, g, cb->K, pa.gt16 != nullptr, weights_merged, wa))) return rc;
    }
    if (phases & MIDAS_LOOP_DBSCAN) {
        if ((rc = launch_dbscan(ctx, cap, s.ctl_i_dev + LOOP_I_N, s.poses_prop_dev, s.eps, -1, s.labels_dev,
                                s.ctl_i_dev + LOOP_I_NCL, s.ctl_i_dev + LOOP_I_ERR, LOOP_MAX_CLUSTERS - 1)))  // (the frame's cluster arrays hold that many)
            return rc;
    }
    if (phases & MIDAS_LOOP_ANNEAL) {
        LoopMoments m;
        if ((rc = loop_cluster_phase(ctx, s, g, weights_merged ? &wa : nullptr, m))) return rc;
        const LoopAnneal regime = loop_anneal_regime(s.anneal_frozen != 0, s.topk_ties == MIDAS_TOPK_TIES_ATEN_CPU,
                                                     s.anneal_small && cap <= LOOP_SMALL_MAX);
        if ((rc = loop_anneal_phase(ctx, s, g, m, regime))) return rc;
    }
    // the annealed set may be a third larger than the particle set the bound was given for
    const int64_t cap2 = cap + cap / 3 + 1 < s.cap ? cap + cap / 3 + 1 : s.cap;
    if (phases & MIDAS_LOOP_RESAMPLE) {
        if ((rc = loop_resample_phase(ctx, s, g, cap2))) return rc;
    } else if (s.stream_draws) {
        if ((rc = loop_ndraw_phase(ctx, s, g, cap2))) return rc;
    }
    return MIDAS_OK;
}

// B trajectories per launch (midas_loop_step_batch): the launches of the small-set frame above with the trajectory as grid.y,
// every array - the caller's and the scratch - (B, ...) contiguous.  The arguments are the regime the entry point checked:
// cap <= LOOP_SMALL_MAX, no bound below the capacity, sparse scoring; through midas_loop_step_batch device draws and ties by index,
// through midas_loop_step_batch_draws also host draws (tn / rot (B, cap, 3), u (B, cap)) and the ATen tie rule, any subset of phases
// (the decision by k_loop_decide per trajectory and launch_topk_aten's B walks in place of k_loop_anneal_small).  One path each: the
// single call's `anneal_small` field and its MIDAS_LOOP_MERGE / MIDAS_FRONT_SMALL switches (which pick between bit-identical
// paths there) are not consulted - k_front_small, the merged weights launch and k_loop_anneal_small always run.
// wide (midas_loop_step_batch_wide, cap <= MIDAS_LOOP_BATCH_WIDE_MAX_CAP, device draws and ties by index): a capacity beyond
// LOOP_SMALL_MAX takes k_front_small over as many waves as it has, and - one trajectory's keys no longer fit one workgroup - the
// single call's decision and radix selection with the trajectory as grid.y (launch_select).  Up to LOOP_SMALL_MAX the launches above.
// objects (midas_loop_step_batch_objects): every row on the object the set names for it - the front takes trees, lists, field and
// codebook from the set's records (k_front_small_objects; cb, t6 and t3 are null) and the weights re-project a drifted row onto its
// own object's poses; the score rows are K_max apart.  Every other phase works on the (B, ...) arrays and never sees a codebook.
// rows (midas_loop_step_batch_rows; objects only, device draws, ties by index): B records of the filter's parameters - the front, the
// weights and the annealing decision are launched as the instantiations that take std, threshold, softmax, unit_weights and floor
// from row blockIdx.y's record (g.rows) where their twins take them from `s`; launch for launch the frame above.
static int loop_step_batch_frame(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* t6, const midas_tree* t3,
                                 const midas_object_set* objects, const midas_loop_args& s, int32_t phases, int32_t B, int64_t log_stride,
                                 bool wide, const midas_loop_row_params* rows = nullptr) {
    const int64_t cap = s.cap;
    const bool large = wide && cap > LOOP_SMALL_MAX;
    LoopGrid g;
    g.cap = cap; g.B = B; g.slice = (int32_t)cap; g.log_stride = log_stride;
    g.lp_stride = (int32_t)(cap + SCAN_CHUNK);  // (the resample reads whole chunks)
    g.rows = rows;
    g.logmap = (phases & MIDAS_LOOP_CENTERS_LOGMAP) != 0;
    int rc;
    LoopWeightsParamRowsArgs wa{};
    bool weights_merged = false;
    if (phases & MIDAS_LOOP_FRONT) {
        static const midas_tree no_tree{};  // (objects: the kernel takes the lists and the field from the row's record)
        ParticleUpdateArgs pa;
        fill_particle_update(pa, s, objects ? &no_tree : t6, objects ? &no_tree : t3, cap, s.poses_dev, s.hint_dev, s.valid_dev,
                             s.score_stamps_dev, (s.gt16_dev && s.part_rmse_dev) ? s.gt16_dev : nullptr, s.part_rmse_dev);
        pa.n_live = s.ctl_i_dev + LOOP_I_N;
        if (objects) rc = launch_front_small_objects(ctx, objects, pa, s.code_dev, s.scores_dev, large, rows);
        else rc = launch_front_small_batch(ctx, t6, t3, pa, cb, s.code_dev, s.scores_dev, B, large);
        if (rc) return rc;
        weights_merged = loop_weights_mergeable(phases);
        if ((rc = loop_weights_phase(ctx, s, g, objects ? objects->K_max : cb->K, pa.gt16 != nullptr, weights_merged, wa, objects))) return rc;
    }
    if ((phases & MIDAS_LOOP_DBSCAN) && s.dbscan_batched) {
        // all trajectories in one set of launches, each in its own region of the cell tables (dbscan.hip): the labels of the passes below
        if ((rc = launch_dbscan_batch(ctx, B, cap, s.ctl_i_dev + LOOP_I_N, LOOP_CTL_I, s.poses_prop_dev, s.eps, -1, s.labels_dev,
                                      s.ctl_i_dev + LOOP_I_NCL, s.ctl_i_dev + LOOP_I_ERR, LOOP_CTL_I, LOOP_MAX_CLUSTERS - 1)))
            return rc;
    } else if (phases & MIDAS_LOOP_DBSCAN) {
        // one trajectory after the other on the stream, each on its slices; the passes take the same scratch (one set of cell tables)
        const midas_scratch_pos pos = midas_scratch_mark(ctx);
        for (int32_t b = 0; b < B; ++b) {
            midas_scratch_rewind(ctx, pos);
            int32_t* ci = s.ctl_i_dev + (size_t)b * LOOP_CTL_I;
            if ((rc = launch_dbscan(ctx, cap, ci + LOOP_I_N, s.poses_prop_dev + (size_t)b * cap * 16, s.eps, -1, s.labels_dev + (size_t)b * cap,
                                    ci + LOOP_I_NCL, ci + LOOP_I_ERR, LOOP_MAX_CLUSTERS - 1)))
                return rc;
        }
    }
    if (phases & MIDAS_LOOP_ANNEAL) {
        LoopMoments m;
        if ((rc = loop_cluster_phase(ctx, s, g, weights_merged ? &wa : nullptr, m))) return rc;
        // (the ATen tie rule: the decision alone per trajectory, then B walks side by side; large: every trajectory's decision clears
        // its own histograms and state, then the selection's launches once)
        if ((rc = loop_anneal_phase(ctx, s, g, m, loop_anneal_regime(false, s.topk_ties == MIDAS_TOPK_TIES_ATEN_CPU, !large)))) return rc;
    }
    if (phases & MIDAS_LOOP_RESAMPLE) {
        if ((rc = loop_resample_phase(ctx, s, g, cap))) return rc;  // (the annealed set never exceeds the capacity)
    } else if (s.stream_draws) {
        if ((rc = loop_ndraw_phase(ctx, s, g, cap))) return rc;
    }
    return MIDAS_OK;
}

int launch_loop_step_batch(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* t6, const midas_tree* t3,
                           const midas_loop_args& s, int32_t phases, int32_t B, int64_t log_stride, bool wide) {
    return loop_step_batch_frame(ctx, cb, t6, t3, nullptr, s, phases, B, log_stride, wide);
}

int launch_loop_step_batch_objects(midas_ctx* ctx, const midas_object_set* set, const midas_loop_args& s, int32_t phases,
                                   int64_t log_stride, bool wide, const midas_loop_row_params* rows) {
    return loop_step_batch_frame(ctx, nullptr, nullptr, nullptr, set, s, phases, set->B, log_stride, wide, rows);
}

// (the units cut out of this one are loaded with it: midas_ctx_create warms "loop")
MIDAS_WARM_DECL(loop_weights) MIDAS_WARM_DECL(anneal) MIDAS_WARM_DECL(anneal_small) MIDAS_WARM_DECL(loop_resample)
int warm_loop() {
    int rc = 0;
    for (int (*w)() : {warm_loop_weights, warm_anneal, warm_anneal_small, warm_loop_resample}) rc = rc ? rc : w();
    return rc;
}

}  // namespace midas
