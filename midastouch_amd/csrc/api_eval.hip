// api_eval.hip - single-touch evaluation on the whole codebook: the top-n pose error, the self-similarity panels and their
// top-n pipelines (float32 and float64), and the one-dimensional t-SNE (host drivers over tsne.hip).
#include <cfloat>
#include <cmath>
#include <cstdlib>

#include "api_entry.hpp"

using namespace midas;

extern "C" {

MIDAS_EXPORT int midas_topn_pose_error(midas_ctx* ctx, int32_t B, int64_t K, const double* scores_dev, int64_t row0, int32_t n,
                                       const double* feat_dev, int32_t d, double* err_dev, int32_t* idx_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, B >= 1 && K >= 1 && scores_dev && feat_dev && err_dev && n >= 1 && n <= 256 && d >= 1 && d <= 16);
    MIDAS_REQUIRE(ctx, row0 >= 0 && row0 + B <= K);
    return launch_topn_pose_error(ctx, B, K, scores_dev, row0, n, feat_dev, d, err_dev, idx_dev);
}

MIDAS_EXPORT int midas_selfsim_panel(midas_ctx* ctx, const midas_codebook* cb, int64_t i0, int64_t R, float* panel_dev, int64_t ldo) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, cb && cb->dtype == MIDAS_F32 && cb->D % 32 == 0 && (uintptr_t)cb->emb % 16 == 0 && panel_dev && (uintptr_t)panel_dev % 16 == 0);
    MIDAS_REQUIRE(ctx, i0 >= 0 && R >= 1 && i0 + R <= cb->K && ldo >= ceil_div(cb->K, 128) * 128 && ldo % 4 == 0);
    return launch_selfsim_panel(ctx, cb, i0, R, panel_dev, ldo);
}

MIDAS_EXPORT int midas_selfsim_topn(midas_ctx* ctx, const midas_codebook* cb, int32_t n, const double* feat_dev, int32_t d,
                                    int64_t rows_per_panel, double* err_dev, int32_t* idx_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, cb && cb->dtype == MIDAS_F32 && cb->D % 32 == 0 && (uintptr_t)cb->emb % 16 == 0 && feat_dev && err_dev);
    MIDAS_REQUIRE(ctx, n >= 1 && n <= 256 && d >= 1 && d <= 16 && rows_per_panel >= 128);
    const int64_t K = cb->K, ldo = ceil_div(K, 128) * 128;
    const int64_t R = ceil_div(rows_per_panel < K ? rows_per_panel : K, 128) * 128;
    const int64_t npanels = ceil_div(K, R);
    // Two panels: the selection of panel p (bound by its reads of the panel and by LDS sorts) runs on a side stream beside
    // the GEMM of panel p + 1 (bound by the matrix pipe).  Events hand the panels back and forth.
    const int nbuf = npanels > 1 ? 2 : 1;
    void* panel;
    int rc = midas_scratch(ctx, ((size_t)nbuf * R + 1) * ldo * sizeof(float), &panel);  // + one row: float32 reciprocal norms (the selection's screen)
    if (rc) return rc;
    float* rinv = (float*)panel + (size_t)nbuf * R * ldo;
    rc = launch_topn_rinv(ctx, K, ldo, cb->norms, rinv);
    if (rc) return rc;
    const char* stream_env = getenv("MIDAS_TOPN_STREAM");  // 1: the streaming selection kernel for every row (A/B runs and tests)
    if (stream_env && stream_env[0] == '1') rinv = nullptr;
    if (!ctx->side) MIDAS_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    hipEvent_t ev_gemm[2] = {nullptr, nullptr}, ev_sel[2] = {nullptr, nullptr};
    hipStream_t main_stream = ctx->stream;
    // every exit goes through `finish`: the side stream is joined behind the main stream again (the scratch panels may be handed
    // to the next API call) and the events are destroyed, whatever failed on the way
    auto finish = [&](int code) {
        ctx->stream = main_stream;
        hipEvent_t join = nullptr;
        if (hipEventCreateWithFlags(&join, hipEventDisableTiming) == hipSuccess) {
            if (hipEventRecord(join, ctx->side) == hipSuccess) (void)hipStreamWaitEvent(main_stream, join, 0);
            (void)hipEventDestroy(join);
        }
        for (int k = 0; k < 2; ++k) {
            if (ev_gemm[k]) (void)hipEventDestroy(ev_gemm[k]);
            if (ev_sel[k]) (void)hipEventDestroy(ev_sel[k]);
        }
        return code;
    };
#define TOPN_CHECK(expr)                                                                                              \
    do {                                                                                                              \
        hipError_t _e = (expr);                                                                                       \
        if (_e != hipSuccess) return finish(midas_set_error(ctx, MIDAS_ERR_HIP, #expr, hipGetErrorString(_e)));       \
    } while (0)
    for (int k = 0; k < nbuf; ++k) {
        TOPN_CHECK(hipEventCreateWithFlags(&ev_gemm[k], hipEventDisableTiming));
        TOPN_CHECK(hipEventCreateWithFlags(&ev_sel[k], hipEventDisableTiming));
    }
    // the side stream starts behind whatever the main stream holds (the caller's inputs)
    TOPN_CHECK(hipEventRecord(ev_sel[0], main_stream));
    TOPN_CHECK(hipStreamWaitEvent(ctx->side, ev_sel[0], 0));
    for (int64_t p = 0; p < npanels; ++p) {
        const int k = (int)(p % nbuf);
        const int64_t i0 = p * R, rows = K - i0 < R ? K - i0 : R;
        float* pan = (float*)panel + (size_t)k * R * ldo;
        if (p >= nbuf) TOPN_CHECK(hipStreamWaitEvent(main_stream, ev_sel[k], 0));  // the panel's previous tenant has been consumed
        rc = launch_selfsim_panel(ctx, cb, i0, rows, pan, ldo);
        if (rc) return finish(rc);
        TOPN_CHECK(hipEventRecord(ev_gemm[k], main_stream));
        TOPN_CHECK(hipStreamWaitEvent(ctx->side, ev_gemm[k], 0));
        ctx->stream = ctx->side;  // the launcher enqueues on ctx->stream
        rc = launch_topn_pose_error_dots(ctx, (int32_t)rows, K, pan, ldo, cb->norms, rinv, i0, n, feat_dev, d, err_dev + i0,
                                         idx_dev ? idx_dev + i0 * n : nullptr);
        ctx->stream = main_stream;
        if (rc) return finish(rc);
        TOPN_CHECK(hipEventRecord(ev_sel[k], ctx->side));
    }
#undef TOPN_CHECK
    return finish(MIDAS_OK);  // the results are ordered behind the main stream again
}

MIDAS_EXPORT int midas_selfsim_panel_f64(midas_ctx* ctx, const midas_codebook* cb, int64_t i0, int64_t R, double* panel_dev, int64_t ldo) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, cb && panel_dev && i0 >= 0 && R >= 1 && i0 + R <= cb->K && ldo >= cb->K);
    return launch_selfsim_panel_f64(ctx, cb, i0, R, panel_dev, ldo);
}

// midas_selfsim_topn's pipeline on float64 panels of final cosines (k_selfsim_mfma_f64, bit-identical to midas_score) and the
// streaming selection of midas_topn_pose_error: the errors and indices of the default exact path, for any embedding dtype and D.
// Scratch: two panels of rows_per_panel x K doubles (rows_per_panel <= 0: MIDAS_SELFSIM_F64_ROWS).
MIDAS_EXPORT int midas_selfsim_topn_f64(midas_ctx* ctx, const midas_codebook* cb, int32_t n, const double* feat_dev, int32_t d,
                                        int64_t rows_per_panel, double* err_dev, int32_t* idx_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, cb && feat_dev && err_dev && n >= 1 && n <= 256 && d >= 1 && d <= 16);
    const int64_t K = cb->K, ldo = K;
    const int64_t want = rows_per_panel > 0 ? rows_per_panel : MIDAS_SELFSIM_F64_ROWS;
    const int64_t R = want < K ? want : K;
    const int64_t npanels = ceil_div(K, R);
    // two panels: the selection of panel p runs on the side stream beside the GEMM of panel p + 1, events hand them over
    const int nbuf = npanels > 1 ? 2 : 1;
    void* panel;
    int rc = midas_scratch(ctx, (size_t)nbuf * R * ldo * sizeof(double), &panel);
    if (rc) return rc;
    if (!ctx->side) MIDAS_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    hipEvent_t ev_gemm[2] = {nullptr, nullptr}, ev_sel[2] = {nullptr, nullptr};
    hipStream_t main_stream = ctx->stream;
    // every exit goes through `finish` (as midas_selfsim_topn): the side stream joined behind the main stream, the events destroyed
    auto finish = [&](int code) {
        ctx->stream = main_stream;
        hipEvent_t join = nullptr;
        if (hipEventCreateWithFlags(&join, hipEventDisableTiming) == hipSuccess) {
            if (hipEventRecord(join, ctx->side) == hipSuccess) (void)hipStreamWaitEvent(main_stream, join, 0);
            (void)hipEventDestroy(join);
        }
        for (int k = 0; k < 2; ++k) {
            if (ev_gemm[k]) (void)hipEventDestroy(ev_gemm[k]);
            if (ev_sel[k]) (void)hipEventDestroy(ev_sel[k]);
        }
        return code;
    };
#define TOPN_CHECK(expr)                                                                                              \
    do {                                                                                                              \
        hipError_t _e = (expr);                                                                                       \
        if (_e != hipSuccess) return finish(midas_set_error(ctx, MIDAS_ERR_HIP, #expr, hipGetErrorString(_e)));       \
    } while (0)
    for (int k = 0; k < nbuf; ++k) {
        TOPN_CHECK(hipEventCreateWithFlags(&ev_gemm[k], hipEventDisableTiming));
        TOPN_CHECK(hipEventCreateWithFlags(&ev_sel[k], hipEventDisableTiming));
    }
    TOPN_CHECK(hipEventRecord(ev_sel[0], main_stream));  // the side stream starts behind the caller's inputs
    TOPN_CHECK(hipStreamWaitEvent(ctx->side, ev_sel[0], 0));
    for (int64_t p = 0; p < npanels; ++p) {
        const int k = (int)(p % nbuf);
        const int64_t i0 = p * R, rows = K - i0 < R ? K - i0 : R;
        double* pan = (double*)panel + (size_t)k * R * ldo;
        if (p >= nbuf) TOPN_CHECK(hipStreamWaitEvent(main_stream, ev_sel[k], 0));  // the panel's previous tenant has been consumed
        rc = launch_selfsim_panel_f64(ctx, cb, i0, rows, pan, ldo);
        if (rc) return finish(rc);
        TOPN_CHECK(hipEventRecord(ev_gemm[k], main_stream));
        TOPN_CHECK(hipStreamWaitEvent(ctx->side, ev_gemm[k], 0));
        ctx->stream = ctx->side;  // the launcher enqueues on ctx->stream
        rc = launch_topn_pose_error(ctx, (int32_t)rows, K, pan, ldo, i0, n, feat_dev, d, err_dev + i0, idx_dev ? idx_dev + i0 * n : nullptr);
        ctx->stream = main_stream;
        if (rc) return finish(rc);
        TOPN_CHECK(hipEventRecord(ev_sel[k], ctx->side));
    }
#undef TOPN_CHECK
    return finish(MIDAS_OK);  // the results are ordered behind the main stream again
}

// ---- one-dimensional t-SNE (tsne.hip) ----

MIDAS_EXPORT int midas_tsne_knn(midas_ctx* ctx, const void* X_dev, int32_t dtype, int64_t K, int64_t F, int64_t ld, int32_t nan_to_num,
                                int32_t k, int64_t rows_per_panel, int32_t* idx_dev, double* d2_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, X_dev && idx_dev && d2_dev && (dtype == MIDAS_F32 || dtype == MIDAS_F64) && K >= 2 && F >= 1 && ld >= F);
    MIDAS_REQUIRE(ctx, k >= 1 && k <= 256 && k <= K - 1 && K < INT32_MAX);
    const int64_t want = rows_per_panel > 0 ? rows_per_panel : MIDAS_TSNE_KNN_ROWS;
    const int64_t rows = want < K ? want : K;
    void* scratch;
    const int rc = midas_scratch(ctx, (size_t)(K + rows * K) * sizeof(double), &scratch);
    if (rc) return rc;
    return launch_tsne_knn(ctx, X_dev, dtype, K, F, ld, nan_to_num, k, rows, (double*)scratch, idx_dev, d2_dev);
}

MIDAS_EXPORT int midas_tsne_perplexity(midas_ctx* ctx, const float* d2_dev, int64_t K, int32_t k, float perplexity, double* P_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, d2_dev && P_dev && K >= 1 && k >= 1 && k <= 256 && perplexity > 0.0f);
    return launch_tsne_perplexity(ctx, d2_dev, K, k, log((double)perplexity), P_dev);
}

MIDAS_EXPORT int midas_tsne_gradient(midas_ctx* ctx, int64_t K, const float* y_dev, const int64_t* crow_dev, const int32_t* col_dev,
                                     const float* val_dev, float* grad_dev, double* kl_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, K >= 2 && y_dev && crow_dev && col_dev && val_dev && grad_dev);
    void* work;
    const int rc = midas_scratch(ctx, tsne_grad_scratch_doubles(K) * sizeof(double), &work);
    if (rc) return rc;
    const int r1 = launch_tsne_objective(ctx, K, y_dev, crow_dev, col_dev, val_dev, (double*)work, kl_dev);
    if (r1) return r1;
    return launch_tsne_update(ctx, K, nullptr, (double*)work, 0, grad_dev, nullptr, nullptr, 0.0, 0.0, 0.0f, nullptr);
}

MIDAS_EXPORT int midas_tsne_optimize(midas_ctx* ctx, int64_t K, float* y_dev, const int64_t* crow_dev, const int32_t* col_dev,
                                     const float* val_dev, int32_t it, int32_t max_iter, double momentum, double learning_rate,
                                     int32_t lr_float32, int32_t n_iter_check, int32_t n_iter_without_progress, double min_grad_norm,
                                     double* result) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, K >= 2 && y_dev && crow_dev && col_dev && val_dev && result && it >= 0 && n_iter_check >= 1);
    const size_t nw = tsne_grad_scratch_doubles(K);
    void* scratch;
    const int rc = midas_scratch(ctx, (nw + 2 * (size_t)K + 8) * sizeof(double) + (size_t)K * sizeof(float), &scratch);
    if (rc) return rc;
    double* work = (double*)scratch;
    double* update = work + nw;
    double* gsq = update + K;
    double* rec = gsq + K;  // {KL, sum grad^2}
    float* gains = (float*)(rec + 8);
    int r = launch_tsne_reset(ctx, K, gains, update);
    if (r) return r;
    const int mode = lr_float32 ? 2 : 1;
    const float min_gain = 0.01f;
    double error = DBL_MAX, best_error = DBL_MAX, hrec[2];
    int64_t best_iter = it, i = it;
    bool broke = false, last_err = false;
    for (i = it; i < max_iter; ++i) {
        const bool check = (i + 1) % n_iter_check == 0, want_err = check || i == max_iter - 1;
        if ((r = launch_tsne_objective(ctx, K, y_dev, crow_dev, col_dev, val_dev, work, want_err ? rec : nullptr))) return r;
        if ((r = launch_tsne_update(ctx, K, y_dev, work, mode, nullptr, gains, update, momentum, learning_rate, min_gain, gsq))) return r;
        last_err = want_err;
        if (!want_err) error = 0.0;  // the objective reports no error on these iterations
        if (check) {
            if ((r = launch_tsne_sum(ctx, gsq, K, rec + 1))) return r;
            MIDAS_HIP_CHECK(ctx, hipMemcpyAsync(hrec, rec, sizeof(hrec), hipMemcpyDeviceToHost, ctx->stream));
            MIDAS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            error = hrec[0];
            const double grad_norm = sqrt(hrec[1]);
            if (error < best_error) {
                best_error = error;
                best_iter = i;
            } else if (i - best_iter > n_iter_without_progress) {
                broke = true;
                break;
            }
            if (grad_norm <= min_grad_norm) {
                broke = true;
                break;
            }
        }
    }
    if (!broke && i > it) {
        i -= 1;  // the last iteration run (Python's loop variable)
        if (last_err && (i + 1) % n_iter_check != 0) {
            MIDAS_HIP_CHECK(ctx, hipMemcpyAsync(hrec, rec, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            MIDAS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            error = hrec[0];
        }
    }
    result[0] = error;
    result[1] = (double)i;
    return MIDAS_OK;
}

}  // extern "C"
