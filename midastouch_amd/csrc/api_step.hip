// api_step.hip - the fixed-N engines' entry points: the eager step and its batch, the pipelined step, run and flush with their
// batch forms, the score-list seed, the table and guide size queries and the pose estimate.
#include "api_entry.hpp"

using namespace midas;

// ---- profiling bracket of a step ------------------------------------------------------------------
static void prof_begin(midas_ctx* ctx) {  // calibration: an empty event pair measures the bracket overhead itself
    if (!(ctx->prof && ctx->ev_ready)) return;
    (void)hipEventRecord(ctx->ev[6], ctx->stream);
    (void)hipEventRecord(ctx->ev[7], ctx->stream);
}
// reads slots lo .. hi - 1 of the step just enqueued (prof_only: that slot alone; a slot the step does not have: only the wait
// for the calibration pair), then the calibration pair.  skip_slot0: no separate scoring kernel ran (the fused front)
static int prof_end(midas_ctx* ctx, int lo, int hi, bool skip_slot0) {
    if (!(ctx->prof && ctx->ev_ready)) return MIDAS_OK;
    const int first = ctx->prof_only >= 0 ? ctx->prof_only : lo, last = ctx->prof_only >= 0 ? ctx->prof_only + 1 : hi;
    if (first >= lo && last <= hi) {
        MIDAS_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev[last]));
        for (int i = first; i < last; ++i) {
            float ms = 0.f;
            if (i == 0 && skip_slot0) continue;
            MIDAS_HIP_CHECK(ctx, hipEventElapsedTime(&ms, ctx->ev[i], ctx->ev[i + 1]));
            ctx->prof_ms[i] += (double)ms;
        }
    } else {
        MIDAS_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev[7]));
    }
    float cal = 0.f;
    MIDAS_HIP_CHECK(ctx, hipEventElapsedTime(&cal, ctx->ev[6], ctx->ev[7]));
    ctx->prof_ms[7] += (double)cal;
    ctx->prof_calls += 1;
    return MIDAS_OK;
}

extern "C" {

// ---- eager step ----------------------------------------------------------------------------------
static int filter_step_impl(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                            const midas_step_args* args, int32_t B) {
    MIDAS_REQUIRE(ctx, cb && tree6 && tree3 && args && tree6->dim == 6 && tree3->dim == 3);
    const midas_step_args& s = *args;
    MIDAS_REQUIRE(ctx, s.N > 0 && s.poses_in_dev && s.poses_prop_dev && s.poses_out_dev && s.weights_dev &&
                           s.weights_out_dev && s.nn_idx_dev && s.hint_out_dev && s.ridx_dev && s.odom16_dev &&
                           s.code_dev && s.status_dev);
    MIDAS_REQUIRE(ctx, s.poses_prop_dev != s.poses_in_dev && s.poses_prop_dev != s.poses_out_dev);
    MIDAS_REQUIRE(ctx, (s.tn_dev == nullptr) == (s.rot_dev == nullptr));
    MIDAS_REQUIRE(ctx, tree6->K == cb->K);
    const int64_t N = s.N;
    const int npart = particle_update_blocks(N);
    void *scores, *x, *e, *valid, *pmax, *pmin, *prm = nullptr, *cdf;
    int rc;
    const size_t Bz = (size_t)B;
    if ((rc = midas_scratch(ctx, Bz * cb->K * sizeof(double), &scores))) return rc;
    if ((rc = midas_scratch(ctx, Bz * N * sizeof(double), &x))) return rc;
    if ((rc = midas_scratch(ctx, Bz * N * sizeof(double), &e))) return rc;
    if ((rc = midas_scratch(ctx, Bz * N, &valid))) return rc;
    if ((rc = midas_scratch(ctx, Bz * npart * sizeof(double), &pmax))) return rc;
    if ((rc = midas_scratch(ctx, Bz * npart * sizeof(double), &pmin))) return rc;
    if (s.gt16_dev && s.rmse_dev)
        if ((rc = midas_scratch(ctx, Bz * npart * 2 * sizeof(double), &prm))) return rc;
    if ((rc = midas_scratch(ctx, Bz * N * sizeof(double), &cdf))) return rc;
    // Single trajectory: the codebook scoring and the particle update share one launch (k_frame_front); the
    // tail then gathers the scores.  Other layouts / batches: scoring, then the particle update with the scores.
    void* lp_raw = nullptr;
    // a batch scores all its codes in one pass over the codebook on the matrix cores when the layout allows it
    // (float64 batch precision: k_score_mfma_f64, which takes every embedding dtype and D)
    const bool mfma = B > 1 && (cb->batch_precision == MIDAS_F64 ||
                                (cb->dtype == MIDAS_F32 && cb->D % 16 == 0 && (uintptr_t)cb->emb % 16 == 0));
    // Batch: that pass (a separate kernel shape: 1024-thread workgroups, 132 KB of LDS) runs on a side stream
    // concurrently with the particle update, which does not need the scores; the fork / join events cost ~8 us,
    // the overlap saves the ~60 us of the scoring.
    const bool defer_batch = mfma && ctx->overlap;
    if ((B == 1 && ctx->overlap) || defer_batch || (B > 1 && s.score_stamps_dev))
        if ((rc = midas_scratch(ctx, Bz * N * sizeof(double), &lp_raw))) return rc;
    if (defer_batch && !ctx->side) {
        MIDAS_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
        MIDAS_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        MIDAS_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    }

    prof_begin(ctx);
    ParticleUpdateArgs pa;
    fill_particle_update(pa, s, tree6, tree3, N, s.poses_in_dev, s.hint_in_dev, (uint8_t*)valid, B == 1 ? s.score_stamps_dev : nullptr,
                         prm ? s.gt16_dev : nullptr, (double*)prm);
    pa.batch = B;
    pa.score_stride = cb->K;
    pa.scores = (const double*)scores;
    pa.x = (double*)x;
    pa.e = (double*)e;
    pa.status_reset = s.status_dev;
    pa.part_max = (double*)pmax;
    pa.part_min = (double*)pmin;
    bool defer = false;
    // a batch with stamps (B x K of them): every trajectory's particle waves score the rows they need from its own code -
    // the float64 arithmetic of the single-trajectory step, no matrix-core pass, no side stream
    const bool sparse_batch = B > 1 && s.score_stamps_dev && s.score_epoch && sparse_score_ok(cb, s.code_dev);
    if (sparse_batch) {
        pa.sp.stamps = s.score_stamps_dev; pa.sp.epoch = s.score_epoch;
        pa.sp.emb = (const float*)cb->emb; pa.sp.norms = cb->norms; pa.sp.code = s.code_dev; pa.sp.scores = (double*)scores;
        pa.sp.nj = cb->D / 64;
        pa.scores = nullptr;  // deferred: the tail gathers the scores
        prof_mark(ctx, 1);
        if ((rc = launch_particle_update(ctx, tree6, tree3, pa))) return rc;
        defer = true;
    }
    if (B == 1 && ctx->overlap) {
        prof_mark(ctx, 1);  // fused front: reported in the particle_update slot, the score slot stays empty
        if ((rc = launch_frame_front(ctx, tree6, tree3, pa, cb, s.code_dev, (double*)scores, &defer))) return rc;
    }
    if (defer_batch && !sparse_batch) {
        hipStream_t main_stream = ctx->stream;
        MIDAS_HIP_CHECK(ctx, hipEventRecord(ctx->ev_fork, main_stream));  // the codes, and last frame's readers of `scores`
        MIDAS_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
        ctx->stream = ctx->side;
        rc = launch_score_dense_batch(ctx, cb, B, s.code_dev, (double*)scores);
        ctx->stream = main_stream;
        if (rc) return rc;
        MIDAS_HIP_CHECK(ctx, hipEventRecord(ctx->ev_join, ctx->side));
        prof_mark(ctx, 1);
        pa.scores = nullptr;  // deferred: the tail gathers the scores
        if ((rc = launch_particle_update(ctx, tree6, tree3, pa))) return rc;
        MIDAS_HIP_CHECK(ctx, hipStreamWaitEvent(main_stream, ctx->ev_join, 0));
        defer = true;
    } else if (!defer) {
        prof_mark(ctx, 0);
        if ((rc = mfma ? launch_score_dense_batch(ctx, cb, B, s.code_dev, (double*)scores)
                       : launch_score(ctx, cb, B, s.code_dev, (double*)scores)))
            return rc;
        prof_mark(ctx, 1);
        pa.sp.stamps = nullptr;  // scored densely just above
        if ((rc = launch_particle_update(ctx, tree6, tree3, pa))) return rc;
    }
    prof_mark(ctx, 2);

    StepTailArgs ta;
    fill_step_tail(ta, s);
    ta.batch = B;
    ta.npart = npart;
    ta.x = defer ? nullptr : (const double*)x;
    ta.scores = (const double*)scores;
    ta.score_stride = cb->K;
    ta.x_raw = (double*)x;
    ta.lp_raw = (double*)lp_raw;
    ta.e = (double*)e;
    ta.valid = (const uint8_t*)valid;
    ta.part_max = (const double*)pmax;
    ta.part_min = (const double*)pmin;
    ta.cdf = (double*)cdf;
    ta.part_rmse = (const double*)prm;
    if ((rc = launch_step_tail(ctx, ta, 2))) return rc;
    return prof_end(ctx, 0, 4, defer);
}

MIDAS_EXPORT int midas_filter_step(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6,
                                   const midas_tree* tree3, const midas_step_args* args) {
    MIDAS_ENTER(ctx);
    return filter_step_impl(ctx, cb, tree6, tree3, args, 1);
}

MIDAS_EXPORT int midas_filter_step_batch(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6,
                                         const midas_tree* tree3, const midas_step_args* args, int32_t B) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, B >= 1 && B <= 65535);
    return filter_step_impl(ctx, cb, tree6, tree3, args, B);
}

// ---- pipelined single-trajectory step ----------------------------------------------------------------
static int lazy_step_impl(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                          const midas_lazy_args& s, double* rmse_out, int32_t B = 1, int64_t tstride = 0) {
    MIDAS_REQUIRE(ctx, s.N > 0 && ceil_div(s.N, SCAN_BLOCK) <= LAZY_MAX_BLOCKS && s.poses_prop_dev && s.nn_idx_dev && s.valid_dev &&
                           s.status_dev && s.tables_dev && (uintptr_t)s.tables_dev % 128 == 0 && s.scores_dev && s.odom16_dev && s.code_dev);
    MIDAS_REQUIRE(ctx, s.resample_prev ? (s.poses_prop_prev_dev && s.nn_idx_prev_dev && s.status_prev_dev &&
                                          s.poses_prop_prev_dev != s.poses_prop_dev && s.nn_idx_prev_dev != s.nn_idx_dev &&
                                          s.status_prev_dev != s.status_dev)
                                       : (s.poses_in_dev && s.poses_in_dev != s.poses_prop_dev));
    MIDAS_REQUIRE(ctx, (s.tn_dev == nullptr) == (s.rot_dev == nullptr));
    MIDAS_REQUIRE(ctx, s.resample_mode == MIDAS_RESAMPLE_MULTINOMIAL || s.resample_mode == MIDAS_RESAMPLE_SYSTEMATIC);
    const int64_t N = s.N;
    TailTables tb = tables_of(s.tables_dev, N);
    // guide tables of the summation blocks (GUIDE_BINS, midas_internal.hpp): softmax variant | raw variant
    if (s.guide_dev && B == 1) {
        MIDAS_REQUIRE(ctx, (uintptr_t)s.guide_dev % 16 == 0);
        tb.guide = reinterpret_cast<guide_t*>(s.guide_dev);
        tb.guide_raw = tb.guide + ceil_div(N, SCAN_BLOCK) * GUIDE_STRIDE;
    }
    ParticleUpdateArgs pa;
    fill_particle_update(pa, s, tree6, tree3, N, s.poses_in_dev, s.hint_in_dev, s.valid_dev, s.score_stamps_dev,
                         (s.gt16_dev && s.part_rmse_dev) ? s.gt16_dev : nullptr, s.part_rmse_dev);
    pa.batch = B;
    pa.score_stride = cb->K;
    pa.scores = nullptr;
    pa.status_reset = s.status_dev;
    ScorePredict predict;
    if (pa.sp.stamps && s.score_list_dev && B == 1 && s.score_epoch >= 2 && N >= SCAN_CHUNK) {
        MIDAS_REQUIRE(ctx, s.score_epoch < MIDAS_EPOCH_LIMIT);  // (bit 31 of a stamp flags a listed row's second chance)
        predict = wire_score_list(pa.sp, s.score_list_dev, cb->K);
    }
    if (s.resample_prev) {
        LazyResample& r = pa.rs;
        r.enabled = true;
        r.e = tb.e; r.x_raw = tb.x_raw; r.lp = tb.lp; r.lp_raw = tb.lp_raw; r.gend = tb.gend; r.gend_raw = tb.gend_raw;
        r.ggend = tb.ggend; r.ggend_raw = tb.ggend_raw;
        r.guide = tb.guide; r.guide_raw = tb.guide_raw;
        r.bsum_e = tb.bsum_e; r.btot = tb.btot; r.btot_raw = tb.btot_raw; r.bmax = tb.bmax; r.bmin = tb.bmin;
        r.poses_prev = s.poses_prop_prev_dev; r.nn_prev = s.nn_idx_prev_dev; r.status_prev = s.status_prev_dev;
        r.ridx_out = s.ridx_dev;
        r.nb = (int)ceil_div(N, SCAN_BLOCK); r.ng = (int)ceil_div(N, SCAN_CHUNK);
        r.softmax = s.softmax; r.mode = s.resample_mode; r.u = s.u_prev_dev; r.u32 = s.u32_prev;
        r.seed = s.seed; r.step = s.step_prev;
        r.tstride = tstride;
    }
    prof_begin(ctx);
    prof_mark(ctx, 1);
    bool launched = false;
    int rc;
    if (B > 1 && !s.resample_prev) {
        // a batch's first frame (nothing to fold in yet): the plain particle update over grid.y, sparse scoring per trajectory
        MIDAS_REQUIRE(ctx, pa.sp.stamps && sparse_score_ok(cb, s.code_dev));
        pa.sp.emb = (const float*)cb->emb; pa.sp.norms = cb->norms; pa.sp.code = s.code_dev; pa.sp.scores = s.scores_dev; pa.sp.nj = cb->D / 64;
        if ((rc = launch_particle_update(ctx, tree6, tree3, pa))) return rc;
    } else {
        if ((rc = launch_frame_front(ctx, tree6, tree3, pa, cb, s.code_dev, s.scores_dev, &launched))) return rc;
        if (!launched)
            return midas_set_error(ctx, MIDAS_ERR_INVALID, "codebook", B > 1 ? "the pipelined batch step needs a float32 codebook with D in {128,256,512,1024}, score stamps and N <= 262144"
                                                                              : "the pipelined step needs a float32 codebook with D in {128,256,512,1024}");
    }
    prof_mark(ctx, 2);
    if ((rc = launch_tail_a2(ctx, N, s.scores_dev, s.nn_idx_dev, s.valid_dev, s.softmax, tb, s.status_dev, B, cb->K, true,
                             pa.gt16 ? s.part_rmse_dev : nullptr, rmse_out, B > 1 ? tstride : 0, predict.stamps ? &predict : nullptr)))
        return rc;
    prof_mark(ctx, 3);
    return prof_end(ctx, 1, 3, false);
}

MIDAS_EXPORT int midas_lazy_step(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                                 const midas_lazy_args* args) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, cb && tree6 && tree3 && args && tree6->dim == 6 && tree3->dim == 3 && tree6->K == cb->K);
    return lazy_step_impl(ctx, cb, tree6, tree3, *args, (args->gt16_dev && args->part_rmse_dev) ? args->rmse_dev : nullptr);
}

// ---- pose estimate of a fixed-N frame (filter/filter.py:184-186) ----------------------------------------
static int pose_estimate_impl(midas_ctx* ctx, const midas_estimate_args& s) {
    MIDAS_REQUIRE(ctx, s.N > 0 && s.B >= 1 && s.B <= 65535 && s.poses_prop_dev && s.centers_dev && s.stds_dev &&
                           (uintptr_t)s.poses_prop_dev % 16 == 0);
    MIDAS_REQUIRE(ctx, (s.weights_dev == nullptr) != (s.tables_dev == nullptr));
    if (s.weights_dev)
        return launch_pose_estimate(ctx, s.N, s.B, s.poses_prop_dev, s.weights_dev, nullptr, 0, nullptr, s.softmax, s.centers_dev,
                                    s.stds_dev);
    MIDAS_REQUIRE(ctx, s.valid_dev && (uintptr_t)s.tables_dev % 128 == 0 && ceil_div(s.N, SCAN_BLOCK) <= LAZY_MAX_BLOCKS);
    const TailTables tb = tables_of(const_cast<double*>(s.tables_dev), s.N);
    return launch_pose_estimate(ctx, s.N, s.B, s.poses_prop_dev, nullptr, &tb, tables_doubles(s.N), s.valid_dev, s.softmax,
                                s.centers_dev, s.stds_dev);
}

MIDAS_EXPORT int midas_pose_estimate(midas_ctx* ctx, const midas_estimate_args* args) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, args != nullptr);
    return pose_estimate_impl(ctx, *args);
}

// the frame loop of midas_lazy_run and midas_lazy_run_estimate (est_centers / est_stds: NULL, or every frame's estimate)
static int lazy_run_impl(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                         const midas_lazy_args* first, int32_t T, double* rmse_log_dev, float* est_centers, float* est_stds) {
    MIDAS_REQUIRE(ctx, cb && tree6 && tree3 && first && tree6->dim == 6 && tree3->dim == 3 && tree6->K == cb->K && T >= 1);
    MIDAS_REQUIRE(ctx, first->poses_prop_prev_dev && first->nn_idx_prev_dev && first->status_prev_dev && !first->tn_dev &&
                           !first->rot_dev && !first->u_prev_dev);
    MIDAS_REQUIRE(ctx, !rmse_log_dev || (first->gt16_dev && first->part_rmse_dev));
    midas_lazy_args a = *first;
    if (a.score_stamps_dev) {  // every epoch of the run is checked BEFORE anything is enqueued (the last frame uses first + inc (T - 1));
                               // the caller restarts the epochs (and zeroes the stamps) long before the limit
        const uint64_t inc = a.score_list_dev ? 2u : 1u;
        MIDAS_REQUIRE(ctx, (uint64_t)a.score_epoch + inc * (uint64_t)(T - 1) < (a.score_list_dev ? (uint64_t)MIDAS_EPOCH_LIMIT : 0xFFFFFFF0ull));
    }
    for (int32_t f = 0; f < T; ++f) {
        int rc = f ? scratch_reset(ctx) : MIDAS_OK;  // frames are ordered on the stream: each may reuse the scratch
        if (rc) return rc;
        rc = lazy_step_impl(ctx, cb, tree6, tree3, a, rmse_log_dev ? rmse_log_dev + 3 * f : nullptr);
        if (rc) return rc;
        if (est_centers) {  // behind this frame's tail: the next front only reads these tables, its tail rewrites them afterwards
            midas_estimate_args e;
            e.N = a.N; e.B = 1; e.poses_prop_dev = a.poses_prop_dev; e.weights_dev = nullptr; e.tables_dev = a.tables_dev;
            e.valid_dev = a.valid_dev; e.softmax = a.softmax;
            e.centers_dev = est_centers + 16 * (size_t)f; e.stds_dev = est_stds + 3 * (size_t)f;
            if ((rc = pose_estimate_impl(ctx, e))) return rc;
        }
        // next frame: the buffer sets swap, the resample of this frame is folded in, the inputs advance
        float* pp = const_cast<float*>(a.poses_prop_prev_dev);
        int32_t* np = const_cast<int32_t*>(a.nn_idx_prev_dev);
        int32_t* sp = const_cast<int32_t*>(a.status_prev_dev);
        a.poses_prop_prev_dev = a.poses_prop_dev; a.nn_idx_prev_dev = a.nn_idx_dev; a.status_prev_dev = a.status_dev;
        a.poses_prop_dev = pp; a.nn_idx_dev = np; a.status_dev = sp;
        a.resample_prev = 1;
        a.u32_prev = -1.0f;
        a.step_prev = a.step;
        a.step += 1;
        if (a.score_stamps_dev) {  // never 0; two per frame with a prediction list (the tag between two epochs marks its rows)
            a.score_epoch += a.score_list_dev ? 2u : 1u;  // (range checked above, for the whole run)
        }
        a.odom16_dev += 16;
        a.code_dev += cb->D;
        if (a.gt16_dev) a.gt16_dev += 16;
    }
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_lazy_run(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                                const midas_lazy_args* first, int32_t T, double* rmse_log_dev) {
    MIDAS_ENTER(ctx);
    return lazy_run_impl(ctx, cb, tree6, tree3, first, T, rmse_log_dev, nullptr, nullptr);
}

MIDAS_EXPORT int midas_lazy_run_estimate(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                                         const midas_lazy_args* first, int32_t T, double* rmse_log_dev, float* est_centers_dev,
                                         float* est_stds_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, est_centers_dev && est_stds_dev);
    return lazy_run_impl(ctx, cb, tree6, tree3, first, T, rmse_log_dev, est_centers_dev, est_stds_dev);
}

static int lazy_flush_impl(midas_ctx* ctx, const midas_lazy_flush_args& s, int32_t B, int64_t tstride) {
    MIDAS_REQUIRE(ctx, s.N > 0 && s.tables_dev && s.valid_dev && s.nn_idx_dev && s.poses_prop_dev && s.status_dev && s.weights_dev &&
                           s.ridx_dev && s.poses_out_dev && s.weights_out_dev && s.hint_out_dev && s.poses_out_dev != s.poses_prop_dev);
    MIDAS_REQUIRE(ctx, s.resample_mode == MIDAS_RESAMPLE_MULTINOMIAL || s.resample_mode == MIDAS_RESAMPLE_SYSTEMATIC);
    const TailTables tb = tables_of(const_cast<double*>(s.tables_dev), s.N);
    StepTailArgs ta;
    fill_step_tail(ta, s);
    ta.batch = B;
    ta.tstride = B > 1 ? tstride : 0;
    ta.npart = 0;
    ta.x = nullptr; ta.e = nullptr; ta.cdf = nullptr; ta.part_max = nullptr; ta.part_min = nullptr;
    ta.valid = s.valid_dev;
    ta.part_rmse = (s.part_rmse_dev && s.rmse_dev) ? s.part_rmse_dev : nullptr;
    return launch_tail_b2(ctx, ta, tb);
}

MIDAS_EXPORT int midas_lazy_flush(midas_ctx* ctx, const midas_lazy_flush_args* args) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, args != nullptr);
    return lazy_flush_impl(ctx, *args, 1, 0);
}

MIDAS_EXPORT int midas_score_list_seed(midas_ctx* ctx, int64_t K, uint32_t* score_stamps_dev, uint32_t score_epoch, int32_t* score_list_dev,
                                       int64_t N, const int32_t* nn_idx_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, K > 0 && score_stamps_dev && score_epoch >= 2 && score_epoch < MIDAS_EPOCH_LIMIT && score_list_dev && N > 0 && nn_idx_dev);
    return launch_predict_seed(ctx, N, nn_idx_dev, next_score_list(score_stamps_dev, score_epoch, score_list_dev, K));
}

// ---- pipelined batch (config 5): B trajectories, grid.y, one table block per trajectory -------------------------------
MIDAS_EXPORT int64_t midas_lazy_tables_doubles(int64_t N) { return N > 0 ? tables_doubles(N) : 0; }
MIDAS_EXPORT int midas_lazy_guide_layout(int32_t* bins_out, int32_t* unit_out, int32_t* stride_out) {
    if (bins_out) *bins_out = GUIDE_BINS;
    if (unit_out) *unit_out = GUIDE_UNIT;
    if (stride_out) *stride_out = GUIDE_STRIDE;
    return MIDAS_OK;
}
MIDAS_EXPORT int64_t midas_lazy_guide_bytes(int64_t N) { return N > 0 ? 2 * ceil_div(N, SCAN_BLOCK) * (int64_t)GUIDE_STRIDE * (int64_t)sizeof(guide_t) : 0; }

MIDAS_EXPORT int midas_lazy_step_batch(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                                       const midas_lazy_args* args, int32_t B) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, cb && tree6 && tree3 && args && tree6->dim == 6 && tree3->dim == 3 && tree6->K == cb->K && B >= 1);
    MIDAS_REQUIRE(ctx, args->score_stamps_dev && args->score_epoch && ceil_div(args->N, SCAN_BLOCK) <= 64 && args->N >= SCAN_CHUNK);
    return lazy_step_impl(ctx, cb, tree6, tree3, *args, (args->gt16_dev && args->part_rmse_dev) ? args->rmse_dev : nullptr, B,
                          tables_doubles(args->N));
}

MIDAS_EXPORT int midas_lazy_flush_batch(midas_ctx* ctx, const midas_lazy_flush_args* args, int32_t B) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, args != nullptr && B >= 1);
    return lazy_flush_impl(ctx, *args, B, tables_doubles(args->N));
}

}  // extern "C"
