// api.hip - context, scratch, errors, profiling read-out, the codebook and tree handles and the single-operator entry points of
// libmidas_hip.so's extern "C" surface: check the arguments, call one launcher.  The engines' entry points are in api_step.hip
// (eager and pipelined step), api_shard.hip (sharded step), api_loop.hip (loop step) and api_eval.hip (single-touch evaluation).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "api_entry.hpp"

using namespace midas;

namespace midas {
int tree_build_impl(midas_ctx* ctx, int32_t dim, int64_t K, const void* points_dev, midas_tree* out);
int attach_mesh_impl(midas_ctx* ctx, midas_tree* t6, const midas_tree* t3, const float* cb_poses_dev);
void tree_free_host(midas_tree* t);
}

// ---- scratch: bump allocator over library-owned device chunks, reset at every API entry ----------
// The chunks live as long as the context: a reset only rewinds to the first one, a request that does not fit the current
// chunk moves on to the next, and only a request that fits none allocates (at least twice the largest chunk so far).  The first
// form freed and re-allocated one consolidated chunk whenever a call had needed more than one - a stream synchronisation,
// hipFree and hipMalloc of tens of MB in the middle of a run: the 5 - 30 ms frames the loop showed now and then whenever a
// phase combination asked for more than any frame before it (MIDAS_SCRATCH_LOG=1 reports every new chunk).
struct ScratchChunk { void* p; size_t cap; };
struct ScratchState {
    std::vector<ScratchChunk> chunks;
    size_t cur = 0;    // chunk in use
    size_t used = 0;   // bytes taken from chunks[cur]
    size_t total = 0;  // bytes requested since the last reset
};
static ScratchState* scratch_of(midas_ctx* ctx) { return reinterpret_cast<ScratchState*>(ctx->scratch); }

int scratch_reset(midas_ctx* ctx) {
    ScratchState* s = scratch_of(ctx);
    s->cur = 0;
    s->used = 0;
    s->total = 0;
    return MIDAS_OK;
}

int midas_scratch(midas_ctx* ctx, size_t bytes, void** out) {
    ScratchState* s = scratch_of(ctx);
    bytes = (bytes + 255) & ~(size_t)255;
    s->total += bytes;
    while (s->cur < s->chunks.size() && s->used + bytes > s->chunks[s->cur].cap) { ++s->cur; s->used = 0; }
    if (s->cur == s->chunks.size()) {
        size_t cap = bytes > (size_t)(1 << 20) ? bytes : (size_t)(1 << 20);
        size_t largest = 0;
        for (const auto& c : s->chunks) largest = c.cap > largest ? c.cap : largest;
        cap = cap > 2 * largest ? cap : 2 * largest;
        void* p = nullptr;
        if (hipMalloc(&p, cap) != hipSuccess) {
            cap = bytes > (size_t)(1 << 20) ? bytes : (size_t)(1 << 20);  // not the generous size then: what is needed
            if (hipMalloc(&p, cap) != hipSuccess) return midas_set_error(ctx, MIDAS_ERR_NOMEM, "hipMalloc(scratch)", "out of device memory");
        }
        static const bool log = getenv("MIDAS_SCRATCH_LOG") != nullptr;
        if (log) fprintf(stderr, "[midas] scratch: chunk %zu of %zu bytes\n", s->chunks.size(), cap);
        s->chunks.push_back({p, cap});
        s->used = 0;
    }
    *out = (char*)s->chunks[s->cur].p + s->used;
    s->used += bytes;
    return MIDAS_OK;
}

midas_scratch_pos midas_scratch_mark(midas_ctx* ctx) {
    const ScratchState* s = scratch_of(ctx);
    return {s->cur, s->used, s->total};
}

void midas_scratch_rewind(midas_ctx* ctx, const midas_scratch_pos& pos) {
    ScratchState* s = scratch_of(ctx);
    s->cur = pos.cur; s->used = pos.used; s->total = pos.total;
}

int midas_set_error(midas_ctx* ctx, int code, const char* what, const char* detail) {
    if (ctx) {
        ctx->last_error = std::string(midas_strerror(code)) + ": " + (what ? what : "") + " (" + (detail ? detail : "") + ")";
    }
    return code;
}

namespace midas {
void prof_mark(midas_ctx* ctx, int slot) {
    if (!ctx->prof || !ctx->ev_ready || slot > MIDAS_PROF_SLOTS) return;
    // prof_only >= 0: bracket a single kernel (events slot and slot+1 only) so that the other kernels run
    // back to back as in an untimed frame
    if (ctx->prof_only >= 0 && slot != ctx->prof_only && slot != ctx->prof_only + 1) return;
    (void)hipEventRecord(ctx->ev[slot], ctx->stream);
}
}  // namespace midas

static const char* kSlotNames[MIDAS_PROF_SLOTS] = {
    "score_codebook", "particle_update", "tail_a", "tail_b", "", "", "", "event_pair_overhead"};

extern "C" {

MIDAS_EXPORT const char* midas_version(void) { return "midas-hip 0.1 (gfx950)"; }

MIDAS_EXPORT const char* midas_strerror(int code) {
    switch (code) {
        case MIDAS_OK: return "ok";
        case MIDAS_ERR_INVALID: return "invalid argument";
        case MIDAS_ERR_HIP: return "HIP runtime error";
        case MIDAS_ERR_NOMEM: return "out of device memory";
        case MIDAS_ERR_NODEVICE: return "no usable HIP device";
        default: return "unknown error";
    }
}

MIDAS_EXPORT const char* midas_last_error(const midas_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

MIDAS_EXPORT int midas_ctx_create(int device, void* hip_stream, midas_ctx** out) {
    if (!out) return MIDAS_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return MIDAS_ERR_NODEVICE;
    if (hipSetDevice(device) != hipSuccess) return MIDAS_ERR_NODEVICE;
    midas_ctx* ctx = new (std::nothrow) midas_ctx();
    if (!ctx) return MIDAS_ERR_NOMEM;
    ctx->device = device;
    ctx->scratch = new (std::nothrow) ScratchState();
    // NULL selects the device's default (null) stream - torch's default stream on ROCm - so that
    // kernels stay ordered with the caller's other work.  The only stream the library creates is the side stream of
    // the batch step, forked from and joined back into this stream by events inside midas_filter_step_batch.
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
    if (const char* ov = getenv("MIDAS_OVERLAP")) ctx->overlap = atoi(ov) != 0;
    // every translation unit's code object is loaded now, not by the first frame that happens to need it (midas_internal.hpp)
    const char* lazy = getenv("MIDAS_LAZY_MODULES");
    if (!(lazy && lazy[0] == '1')) {
        int (*const warm[])() = {warm_score, warm_particles, warm_resample, warm_cluster, warm_topn, warm_selfsim, warm_loop,
                                 warm_dbscan, warm_dbscan_nd, warm_index_build, warm_mt19937, warm_topk_aten, warm_score_f64,
                                 warm_selfsim_f64, warm_tsne};
        for (auto w : warm)
            if (w() != 0) { (void)hipGetLastError(); }  // not fatal: the unit then loads at its first launch, as before
    }
    // hand-over records of the grouped tail (4 KB per 4096 particles; without them the tail takes its one-workgroup-per-block form)
    {
        void* p = nullptr;
        const int blocks = midas::TAIL_GROUP_MAX_BLOCKS;
        // (hipMemset is not ordered against a non-blocking caller stream: the device is drained before anybody can launch on the records)
        if (hipMalloc(&p, (size_t)blocks * midas::TAIL_GROUP_BLOCK_BYTES) == hipSuccess && hipMemset(p, 0, (size_t)blocks * midas::TAIL_GROUP_BLOCK_BYTES) == hipSuccess &&
            hipDeviceSynchronize() == hipSuccess) {
            ctx->tail_rec = (unsigned long long*)p;
            ctx->tail_rec_blocks = blocks;
        } else {
            if (p) (void)hipFree(p);
            (void)hipGetLastError();
        }
    }
    *out = ctx;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_scratch_reserve(midas_ctx* ctx, int64_t bytes) {
    if (!ctx || bytes < 0) return MIDAS_ERR_INVALID;
    MIDAS_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ScratchState* s = scratch_of(ctx);
    size_t have = 0;
    for (const auto& c : s->chunks) have = c.cap > have ? c.cap : have;
    const size_t want = ((size_t)bytes + 255) & ~(size_t)255;
    if (s->chunks.size() == 1 && have >= want) return MIDAS_OK;
    if (s->chunks.size() >= 1 && have >= want && s->chunks[0].cap == have) return MIDAS_OK;  // the first chunk already holds it
    // one chunk that holds everything, in front of the others (a call takes the first chunk its request fits): nothing in
    // flight may still use the old ones when they are freed
    MIDAS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->side) MIDAS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->side));
    void* p = nullptr;
    const size_t cap = want > have ? want : have;
    if (hipMalloc(&p, cap) != hipSuccess) return midas_set_error(ctx, MIDAS_ERR_NOMEM, "hipMalloc(scratch reserve)", "out of device memory");
    for (auto& c : s->chunks) (void)hipFree(c.p);
    s->chunks.clear();
    s->chunks.push_back({p, cap});
    s->cur = 0; s->used = 0; s->total = 0;
    static const bool log = getenv("MIDAS_SCRATCH_LOG") != nullptr;
    if (log) fprintf(stderr, "[midas] scratch: reserved one chunk of %zu bytes\n", cap);
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_ctx_destroy(midas_ctx* ctx) {
    if (!ctx) return MIDAS_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ScratchState* s = scratch_of(ctx);
    for (auto& c : s->chunks) (void)hipFree(c.p);
    delete s;
    if (ctx->tail_rec) (void)hipFree(ctx->tail_rec);
    if (ctx->ev_ready)
        for (auto& e : ctx->ev) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->side) {
        (void)hipStreamSynchronize(ctx->side);
        (void)hipEventDestroy(ctx->ev_fork);
        (void)hipEventDestroy(ctx->ev_join);
        (void)hipStreamDestroy(ctx->side);
    }
    delete ctx;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_ctx_set_stream(midas_ctx* ctx, void* hip_stream) {
    if (!ctx) return MIDAS_ERR_INVALID;
    MIDAS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream) {
        (void)hipStreamDestroy(ctx->stream);
        ctx->own_stream = false;
    }
    ctx->stream = (hipStream_t)hip_stream;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_sync(midas_ctx* ctx) {
    if (!ctx) return MIDAS_ERR_INVALID;
    MIDAS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MIDAS_OK;
}

// ---- codebook ------------------------------------------------------------------------------------
MIDAS_EXPORT int midas_codebook_create(midas_ctx* ctx, int64_t K, int32_t D, const void* emb_dev, int32_t dtype,
                                       midas_codebook** out) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, out && emb_dev && K > 0 && D > 0 && (dtype == MIDAS_F32 || dtype == MIDAS_F64));
    midas_codebook* cb = new (std::nothrow) midas_codebook();
    if (!cb) return midas_set_error(ctx, MIDAS_ERR_NOMEM, "new midas_codebook", "");
    cb->ctx = ctx; cb->K = K; cb->D = D; cb->dtype = dtype; cb->emb = emb_dev; cb->norms = nullptr;
    if (hipMalloc((void**)&cb->norms, (size_t)K * sizeof(double)) != hipSuccess) {
        delete cb;
        return midas_set_error(ctx, MIDAS_ERR_NOMEM, "hipMalloc(norms)", "");
    }
    int rc = launch_row_norms(ctx, K, D, emb_dev, dtype, cb->norms);
    if (rc) { (void)hipFree(cb->norms); delete cb; return rc; }
    *out = cb;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_codebook_destroy(midas_codebook* cb) {
    if (!cb) return MIDAS_OK;
    (void)hipStreamSynchronize(cb->ctx->stream);
    (void)hipFree(cb->norms);
    delete cb;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_score(midas_ctx* ctx, const midas_codebook* cb, int32_t B, const double* codes_dev,
                             double* scores_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, cb && B >= 1 && codes_dev && scores_dev);
    return launch_score(ctx, cb, B, codes_dev, scores_dev);
}

MIDAS_EXPORT int midas_score_batch(midas_ctx* ctx, const midas_codebook* cb, int32_t B, const double* codes_dev,
                                   double* scores_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, cb && B >= 1 && codes_dev && scores_dev);
    return launch_score_batch(ctx, cb, B, codes_dev, scores_dev);
}

MIDAS_EXPORT int midas_score_batch_f64(midas_ctx* ctx, const midas_codebook* cb, int32_t B, const double* codes_dev,
                                       double* scores_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, cb && B >= 1 && codes_dev && scores_dev);
    return launch_score_batch_f64(ctx, cb, B, codes_dev, scores_dev);
}

MIDAS_EXPORT int midas_codebook_set_batch_precision(midas_codebook* cb, int32_t dtype) {
    if (!cb) return MIDAS_ERR_INVALID;
    midas_ctx* ctx = cb->ctx;
    MIDAS_REQUIRE(ctx, dtype == MIDAS_F32 || dtype == MIDAS_F64);
    cb->batch_precision = dtype;
    return MIDAS_OK;
}

// ---- features / trees ----------------------------------------------------------------------------
MIDAS_EXPORT int midas_se3_feature(midas_ctx* ctx, int64_t N, const float* poses_dev, float w, float* feat6_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N >= 0 && (N == 0 || (poses_dev && feat6_dev)));
    return launch_se3_feature(ctx, N, poses_dev, w, feat6_dev);
}

MIDAS_EXPORT int midas_tree_build(midas_ctx* ctx, int32_t dim, int64_t K, const void* points_dev, midas_tree** out) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, out && points_dev && K > 0 && K < ((int64_t)1 << 30) && (dim == 6 || dim == 3));
    midas_tree* t = new (std::nothrow) midas_tree();
    if (!t) return midas_set_error(ctx, MIDAS_ERR_NOMEM, "new midas_tree", "");
    std::memset(t, 0, sizeof(*t));
    t->ctx = ctx;
    t->dim = dim;
    int rc = tree_build_impl(ctx, dim, K, points_dev, t);
    if (rc) { midas_tree_destroy(t); return rc; }
    *out = t;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_tree_attach_mesh(midas_ctx* ctx, midas_tree* tree6, const midas_tree* tree3,
                                        const float* cb_poses_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, tree6 && tree3 && cb_poses_dev && tree6->dim == 6 && tree3->dim == 3);
    return attach_mesh_impl(ctx, tree6, tree3, cb_poses_dev);
}

MIDAS_EXPORT int midas_tree_export(midas_ctx* ctx, const midas_tree* tree, int32_t what, void* dst_host, int64_t bytes) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, tree && dst_host && bytes >= 0 && what >= 0 && what <= 3);
    const void* src = nullptr;
    int64_t have = 0;
    switch (what) {
        case 0: src = tree->nbrs; have = tree->nbrs ? tree->K * NBR_REC * (int64_t)sizeof(Nbr6) : 0; break;
        case 1: src = tree->rho_out; have = tree->rho_out ? tree->K * (int64_t)sizeof(float) : 0; break;
        case 2: src = tree->twin; have = tree->twin ? tree->K * (int64_t)sizeof(int32_t) : 0; break;
        default: src = tree->vlist; have = tree->vlist ? tree->K * MESH_REC * (int64_t)sizeof(MeshRec) : 0; break;
    }
    MIDAS_REQUIRE(ctx, src && bytes == have);
    MIDAS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    MIDAS_HIP_CHECK(ctx, hipMemcpy(dst_host, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_tree_destroy(midas_tree* t) {
    if (!t) return MIDAS_OK;
    (void)hipStreamSynchronize(t->ctx->stream);
    if (t->boxes) (void)hipFree(t->boxes);
    if (t->pts) (void)hipFree(t->pts);
    if (t->inv_perm) (void)hipFree(t->inv_perm);
    if (t->nbrs) (void)hipFree(t->nbrs);
    if (t->rho_out) (void)hipFree(t->rho_out);
    if (t->twin) (void)hipFree(t->twin);
    if (t->vlist) (void)hipFree(t->vlist);
    if (t->vscr) (void)hipFree(t->vscr);
    if (t->field.d) (void)hipFree(const_cast<float*>(t->field.d));
    tree_free_host(t);
    delete t;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_nn6(midas_ctx* ctx, const midas_tree* tree, int64_t N, const float* feat6_dev,
                           const int32_t* hint_dev, int32_t* idx_dev, float* d2_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, tree && tree->dim == 6 && N >= 0 && (N == 0 || (feat6_dev && idx_dev)));
    return launch_nn6(ctx, tree, N, feat6_dev, hint_dev, idx_dev, d2_dev);
}

MIDAS_EXPORT int midas_knn6(midas_ctx* ctx, const midas_tree* tree, int64_t N, const float* feat6_dev, int32_t k,
                            int32_t* idx_dev, float* d2_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, tree && tree->dim == 6 && N >= 0 && k >= 1 && k <= 64 && (int64_t)k <= tree->K &&
                           (N == 0 || (feat6_dev && idx_dev)));
    return launch_knn6(ctx, tree, N, feat6_dev, k, idx_dev, d2_dev);
}

MIDAS_EXPORT int midas_nn6_stats(midas_ctx* ctx, const midas_tree* tree, int64_t N, const float* feat6_dev,
                                 const int32_t* hint_dev, int32_t* leaves_dev, int32_t* nodes_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, tree && tree->dim == 6 && N >= 0 && (N == 0 || (feat6_dev && leaves_dev && nodes_dev)));
    return launch_nn6_stats(ctx, tree, N, feat6_dev, hint_dev, leaves_dev, nodes_dev);
}

MIDAS_EXPORT int midas_nn3(midas_ctx* ctx, const midas_tree* tree, int64_t N, const float* poses_dev, double* dist_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, tree && tree->dim == 3 && N >= 0 && (N == 0 || (poses_dev && dist_dev)));
    return launch_nn3(ctx, tree, N, poses_dev, dist_dev);
}

// ---- motion model --------------------------------------------------------------------------------
MIDAS_EXPORT int midas_propagate(midas_ctx* ctx, int64_t N, const float* poses_in_dev, float* poses_out_dev,
                                 const float* odom16_dev, const float* tn_dev, const float* rot_dev, float std_t,
                                 float std_r, uint64_t seed, uint64_t step) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N >= 0 && odom16_dev && (N == 0 || (poses_in_dev && poses_out_dev)));
    MIDAS_REQUIRE(ctx, (tn_dev == nullptr) == (rot_dev == nullptr));
    return launch_propagate(ctx, N, poses_in_dev, poses_out_dev, odom16_dev, tn_dev, rot_dev, std_t, std_r, seed, step);
}

MIDAS_EXPORT int midas_check_poses(midas_ctx* ctx, int64_t N, const float* poses_dev, uint8_t* flag_dev,
                                   int32_t* count_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N >= 0 && count_dev && (N == 0 || (poses_dev && flag_dev)));
    return launch_check_poses(ctx, N, poses_dev, flag_dev, count_dev);
}

// ---- weights -------------------------------------------------------------------------------------
MIDAS_EXPORT int midas_gather_f64(midas_ctx* ctx, int64_t N, const double* table_dev, const int32_t* idx_dev,
                                  double* out_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N >= 0 && (N == 0 || (table_dev && idx_dev && out_dev)));
    return launch_gather_f64(ctx, N, table_dev, idx_dev, out_dev);
}

MIDAS_EXPORT int midas_softmax(midas_ctx* ctx, int64_t N, const double* x_dev, int32_t softmax, double* w_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N >= 0 && (N == 0 || (x_dev && w_dev)));
    return launch_softmax(ctx, N, x_dev, softmax, w_dev);
}

MIDAS_EXPORT int midas_prune(midas_ctx* ctx, int64_t N, double* w_dev, const double* dist_dev, double thr,
                             int32_t* nvalid_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N >= 0 && nvalid_dev && (N == 0 || (w_dev && dist_dev)));
    return launch_prune(ctx, N, w_dev, dist_dev, thr, nvalid_dev);
}

// ---- resample ------------------------------------------------------------------------------------
MIDAS_EXPORT int midas_cdf(midas_ctx* ctx, int64_t N, const double* w_dev, double* cdf_dev, int32_t* status_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N >= 0 && status_dev && (N == 0 || (w_dev && cdf_dev)));
    return launch_cdf(ctx, N, w_dev, cdf_dev, status_dev);
}

MIDAS_EXPORT int midas_mt19937_seed(midas_ctx* ctx, uint64_t seed, uint32_t* state_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, state_dev != nullptr);
    return launch_mt_seed(ctx, seed, state_dev);
}

MIDAS_EXPORT int midas_mt19937_rand64(midas_ctx* ctx, uint32_t* state_dev, int64_t skip_words, int64_t N, double* out_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, state_dev != nullptr && skip_words >= 0 && N >= 0 && (N == 0 || out_dev != nullptr));
    return launch_mt_rand64(ctx, state_dev, skip_words, N, out_dev, nullptr);
}

MIDAS_EXPORT int midas_mt19937_normal32(midas_ctx* ctx, uint32_t* state_dev, int64_t skip_words, int64_t numel, float mean, float std,
                                        const float* radius_dev, const float* cos_dev, const float* sin_dev, float* out_dev, uint32_t* hist_dev,
                                        const uint32_t* polys_dev, int32_t pieces) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, state_dev != nullptr && skip_words >= 0 && numel >= 16 && radius_dev && cos_dev && sin_dev && out_dev);
    const bool chunked = polys_dev && pieces > 0;
    MIDAS_REQUIRE(ctx, !chunked || (hist_dev != nullptr && pieces <= 1024 && numel >= MIDAS_MT19937_HIST_WORDS));
    return launch_mt_normal32(ctx, state_dev, skip_words, numel, mean, std, radius_dev, cos_dev, sin_dev, out_dev, hist_dev,
                              chunked ? polys_dev : nullptr, chunked ? pieces : 0);
}

MIDAS_EXPORT int midas_mt19937_rand64_chunked(midas_ctx* ctx, uint32_t* state_dev, int64_t skip_words, int64_t N, double* out_dev,
                                              uint32_t* hist_dev, const uint32_t* polys_dev, int32_t pieces) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, state_dev != nullptr && skip_words >= 0 && N >= 0 && (N == 0 || out_dev != nullptr));
    if (!polys_dev || pieces <= 0)  // the sequential walk; leaves the history for a chunked call to follow
        return launch_mt_rand64(ctx, state_dev, skip_words, N, out_dev, hist_dev);
    MIDAS_REQUIRE(ctx, hist_dev != nullptr && N > 0 && pieces <= 1024 && 2 * N >= MIDAS_MT19937_HIST_WORDS);
    return launch_mt_rand64_chunked(ctx, state_dev, N, out_dev, hist_dev, polys_dev, pieces);
}

MIDAS_EXPORT int midas_mt19937_draws(midas_ctx* ctx, uint32_t* state_dev, int64_t skip_words, int32_t nseg, const midas_mt_segment* segs,
                                     const float* radius_dev, const float* cos_dev, const float* sin_dev, uint32_t* hist_dev,
                                     const uint32_t* polys_dev, int32_t pieces) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, state_dev != nullptr && skip_words >= 0 && nseg >= 1 && nseg <= 8 && segs != nullptr);
    int64_t total = 0;
    for (int i = 0; i < nseg; ++i) {
        const midas_mt_segment& g = segs[i];
        MIDAS_REQUIRE(ctx, (g.kind == MIDAS_MT_SEGMENT_RAND64 && g.count >= 0 && (g.count == 0 || g.out_dev)) ||
                               (g.kind == MIDAS_MT_SEGMENT_RAND32 && g.count == 1 && g.out_dev) ||
                               (g.kind == MIDAS_MT_SEGMENT_NORMAL32 && g.count >= 16 && g.out_dev && radius_dev && cos_dev && sin_dev));
        total += g.kind == MIDAS_MT_SEGMENT_RAND64 ? 2 * g.count : g.kind == MIDAS_MT_SEGMENT_RAND32 ? g.count : g.count + ((g.count & 15) ? 16 : 0);
    }
    const bool chunked = polys_dev && pieces > 0;
    MIDAS_REQUIRE(ctx, !chunked || (hist_dev != nullptr && pieces <= 1024 && total >= MIDAS_MT19937_HIST_WORDS));
    return launch_mt_draws(ctx, state_dev, skip_words, nseg, segs, radius_dev, cos_dev, sin_dev, hist_dev, chunked ? polys_dev : nullptr,
                           chunked ? pieces : 0);
}

MIDAS_EXPORT int midas_mt19937_draws_batch(midas_ctx* ctx, int32_t B, uint32_t* states_dev, int64_t skip_words, int32_t nseg,
                                           const midas_mt_segment* segs, const float* radius_dev, const float* cos_dev, const float* sin_dev,
                                           uint32_t* hist_dev, const uint32_t* polys_dev, int32_t pieces) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, B >= 1 && B <= 65535 && states_dev != nullptr && skip_words >= 0 && nseg >= 1 && nseg <= 8 && segs != nullptr);
    int64_t total = 0;
    for (int i = 0; i < nseg; ++i) {
        const midas_mt_segment& g = segs[i];
        MIDAS_REQUIRE(ctx, (g.kind == MIDAS_MT_SEGMENT_RAND64 && g.count >= 0 && (g.count == 0 || g.out_dev)) ||
                               (g.kind == MIDAS_MT_SEGMENT_RAND32 && g.count == 1 && g.out_dev) ||
                               (g.kind == MIDAS_MT_SEGMENT_NORMAL32 && g.count >= 16 && g.out_dev && radius_dev && cos_dev && sin_dev));
        total += g.kind == MIDAS_MT_SEGMENT_RAND64 ? 2 * g.count : g.kind == MIDAS_MT_SEGMENT_RAND32 ? g.count : g.count + ((g.count & 15) ? 16 : 0);
    }
    const bool chunked = polys_dev && pieces > 0;
    MIDAS_REQUIRE(ctx, !chunked || (hist_dev != nullptr && pieces <= 1024 && total >= MIDAS_MT19937_HIST_WORDS));
    return launch_mt_draws_batch(ctx, B, states_dev, skip_words, nseg, segs, radius_dev, cos_dev, sin_dev, hist_dev,
                                 chunked ? polys_dev : nullptr, chunked ? pieces : 0);
}

MIDAS_EXPORT int midas_mt19937_draws_counted(midas_ctx* ctx, uint32_t* state_dev, int64_t skip_words, int32_t nseg,
                                             const midas_mt_counted_segment* segs, const float* radius_dev, const float* cos_dev,
                                             const float* sin_dev, int32_t* status_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, state_dev != nullptr && skip_words >= 0 && nseg >= 1 && nseg <= 8 && segs != nullptr && status_dev != nullptr);
    for (int i = 0; i < nseg; ++i) {
        const midas_mt_counted_segment& g = segs[i];
        MIDAS_REQUIRE(ctx, g.kind == MIDAS_MT_SEGMENT_RAND64 || (g.kind == MIDAS_MT_SEGMENT_RAND32 && g.per == 1) ||
                               (g.kind == MIDAS_MT_SEGMENT_NORMAL32 && radius_dev && cos_dev && sin_dev));
        // (the grids and the scratch are sized by per x bound: up to 2^31 - 1 values a segment)
        MIDAS_REQUIRE(ctx, g.count_dev != nullptr && g.per >= 1 && g.bound >= 0 && g.bound <= 0x7fffffff / g.per && (g.bound == 0 || g.out_dev));
    }
    return launch_mt_draws_counted(ctx, state_dev, skip_words, nseg, segs, radius_dev, cos_dev, sin_dev, status_dev);
}

MIDAS_EXPORT int midas_mt19937_draws_counted_batch(midas_ctx* ctx, int32_t B, uint32_t* states_dev, int64_t skip_words, int32_t nseg,
                                                   const midas_mt_counted_segment* segs, int64_t count_stride, const float* radius_dev,
                                                   const float* cos_dev, const float* sin_dev, int32_t* status_dev, int64_t status_stride) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, B >= 1 && B <= 65535 && states_dev != nullptr && skip_words >= 0 && nseg >= 1 && nseg <= 8 && segs != nullptr &&
                           status_dev != nullptr && count_stride >= 0 && status_stride >= 0);
    MIDAS_REQUIRE(ctx, B == 1 || (count_stride > 0 && status_stride > 0));  // (every stream its own counts and status word)
    for (int i = 0; i < nseg; ++i) {
        const midas_mt_counted_segment& g = segs[i];
        MIDAS_REQUIRE(ctx, g.kind == MIDAS_MT_SEGMENT_RAND64 || (g.kind == MIDAS_MT_SEGMENT_RAND32 && g.per == 1) ||
                               (g.kind == MIDAS_MT_SEGMENT_NORMAL32 && radius_dev && cos_dev && sin_dev));
        MIDAS_REQUIRE(ctx, g.count_dev != nullptr && g.per >= 1 && g.bound >= 0 && g.bound <= 0x7fffffff / g.per && (g.bound == 0 || g.out_dev));
    }
    return launch_mt_draws_counted_batch(ctx, B, states_dev, skip_words, nseg, segs, count_stride, radius_dev, cos_dev, sin_dev, status_dev,
                                         status_stride);
}

MIDAS_EXPORT int midas_resample_search(midas_ctx* ctx, int64_t N, const double* cdf_dev, int64_t M, int32_t mode,
                                       const double* u_dev, float u32, uint64_t seed, uint64_t step, int32_t* idx_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && M >= 0 && cdf_dev && (M == 0 || idx_dev));
    MIDAS_REQUIRE(ctx, mode == MIDAS_RESAMPLE_MULTINOMIAL || mode == MIDAS_RESAMPLE_SYSTEMATIC);
    return launch_search(ctx, N, cdf_dev, M, mode, u_dev, u32, seed, step, idx_dev);
}

MIDAS_EXPORT int midas_gather_rows(midas_ctx* ctx, int64_t M, const int32_t* idx_dev, const void* src_dev, void* dst_dev,
                                   int32_t row_bytes) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, M >= 0 && row_bytes > 0 && (M == 0 || (idx_dev && src_dev && dst_dev)));
    return launch_gather_rows(ctx, M, idx_dev, src_dev, dst_dev, row_bytes);
}

MIDAS_EXPORT int midas_rmse(midas_ctx* ctx, int64_t N, const float* poses_dev, const float* gt16_dev, double* out2_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && poses_dev && gt16_dev && out2_dev);
    return launch_rmse(ctx, N, poses_dev, gt16_dev, out2_dev);
}

// ---- clustering and annealing operators ---------------------------------------------------------
MIDAS_EXPORT int midas_cluster_centers(midas_ctx* ctx, int64_t N, const float* poses_dev, const double* weights64_dev,
                                       const float* weights32_dev, const int64_t* labels_dev, int32_t C,
                                       const int64_t* label_values_dev, float* centers_dev, float* stds_dev,
                                       int64_t* counts_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && poses_dev && labels_dev && label_values_dev && centers_dev && stds_dev && C >= 1 && C <= 65535);
    MIDAS_REQUIRE(ctx, (weights64_dev == nullptr) != (weights32_dev == nullptr));
    MIDAS_REQUIRE(ctx, (uintptr_t)poses_dev % 16 == 0);
    return launch_cluster_centers(ctx, N, poses_dev, weights64_dev, weights32_dev, labels_dev, C, label_values_dev, centers_dev,
                                  stds_dev, counts_dev);
}

MIDAS_EXPORT int midas_cluster_centers_logmap(midas_ctx* ctx, int64_t N, const float* poses_dev, const double* weights64_dev,
                                              const float* weights32_dev, const int64_t* labels_dev, int32_t C,
                                              const int64_t* label_values_dev, float* centers_dev, float* stds_dev,
                                              int64_t* counts_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && poses_dev && labels_dev && label_values_dev && centers_dev && stds_dev && C >= 1 && C <= 65535);
    MIDAS_REQUIRE(ctx, (weights64_dev == nullptr) != (weights32_dev == nullptr));
    MIDAS_REQUIRE(ctx, (uintptr_t)poses_dev % 16 == 0);
    return launch_cluster_centers(ctx, N, poses_dev, weights64_dev, weights32_dev, labels_dev, C, label_values_dev, centers_dev,
                                  stds_dev, counts_dev, true);
}

MIDAS_EXPORT int midas_se3_log(midas_ctx* ctx, int64_t N, const float* poses_dev, double* xi_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && poses_dev && xi_dev && (uintptr_t)poses_dev % 16 == 0);
    return launch_se3_log(ctx, N, poses_dev, xi_dev);
}

MIDAS_EXPORT int midas_anneal_select(midas_ctx* ctx, int64_t N, const double* weights_dev, int32_t mode, int64_t k,
                                     int32_t* src_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && ceil_div(N, SCAN_BLOCK) <= LAZY_MAX_BLOCKS && weights_dev && src_dev && (mode == 1 || mode == 2) &&
                           k >= 0 && k <= N / 3);
    return launch_anneal_select(ctx, N, weights_dev, k == 0 ? 0 : mode, k, MIDAS_TOPK_TIES_INDEX, src_dev, nullptr);
}

MIDAS_EXPORT int midas_anneal_select_ties(midas_ctx* ctx, int64_t N, const double* weights_dev, int32_t mode, int64_t k, int32_t ties,
                                          int32_t* src_dev, int32_t* info_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && ceil_div(N, SCAN_BLOCK) <= LAZY_MAX_BLOCKS && weights_dev && src_dev && (mode == 1 || mode == 2) &&
                           k >= 0 && k <= N / 3 && (ties == MIDAS_TOPK_TIES_INDEX || ties == MIDAS_TOPK_TIES_ATEN_CPU));
    return launch_anneal_select(ctx, N, weights_dev, k == 0 ? 0 : mode, k, ties, src_dev, info_dev);
}

MIDAS_EXPORT int midas_dbscan(midas_ctx* ctx, int64_t N, const float* poses_dev, double eps, int64_t min_samples,
                              int32_t* labels_dev, int32_t* ncl_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && N < ((int64_t)1 << 31) && poses_dev && labels_dev && ncl_dev && eps > 0.0);
    MIDAS_HIP_CHECK(ctx, hipMemsetAsync(ncl_dev, 0, 2 * sizeof(int32_t), ctx->stream));
    return launch_dbscan(ctx, N, nullptr, poses_dev, eps, min_samples, labels_dev, ncl_dev, ncl_dev + 1, 0);
}

MIDAS_EXPORT int midas_dbscan_batch(midas_ctx* ctx, int32_t B, int64_t cap, const int32_t* n_dev, int64_t n_stride, const float* poses_dev,
                                    double eps, int64_t min_samples, int32_t* labels_dev, int32_t* info_dev, int32_t max_clusters) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, B >= 1 && B <= 65535 && cap >= 1 && (int64_t)B * cap <= MIDAS_DBSCAN_BATCH_MAX_POINTS);
    MIDAS_REQUIRE(ctx, poses_dev && labels_dev && info_dev && eps > 0.0 && (n_dev == nullptr || n_stride >= 1));
    MIDAS_REQUIRE(ctx, max_clusters >= 0 && max_clusters < MIDAS_LOOP_MAX_CLUSTERS);
    MIDAS_HIP_CHECK(ctx, hipMemsetAsync(info_dev, 0, (size_t)B * 2 * sizeof(int32_t), ctx->stream));
    return launch_dbscan_batch(ctx, B, cap, n_dev, n_stride, poses_dev, eps, min_samples, labels_dev, info_dev, info_dev + 1, 2, max_clusters);
}

MIDAS_EXPORT int midas_dbscan_points(midas_ctx* ctx, int64_t N, int32_t dim, const double* points_dev, double eps, int64_t min_samples,
                                     int32_t* labels_dev, int32_t* info_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && N < ((int64_t)1 << 31) && dim >= 2 && dim <= 6 && points_dev && labels_dev && info_dev && eps > 0.0);
    MIDAS_HIP_CHECK(ctx, hipMemsetAsync(info_dev, 0, 2 * sizeof(int32_t), ctx->stream));
    return launch_dbscan_points(ctx, N, dim, points_dev, eps, min_samples, labels_dev, info_dev);
}

MIDAS_EXPORT int midas_selftest_wave_sums(midas_ctx* ctx, const double* in64_dev, double* out256_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, in64_dev && out256_dev);
    return midas::launch_selftest_wave_sums(ctx, in64_dev, out256_dev);
}

#ifdef MIDAS_DEBUG_CLOCKS
MIDAS_EXPORT int midas_debug_tb2_clocks(long long* out16) { return midas::debug_tb2_clocks(out16); }
MIDAS_EXPORT int midas_debug_ta_clocks(long long* out16) { return midas::debug_ta_clocks(out16); }
MIDAS_EXPORT int midas_debug_tg_clocks(long long* io64, int reset) { return midas::debug_tg_clocks(io64, reset); }
MIDAS_EXPORT int midas_debug_tg_waves(long long* out4096) { return midas::debug_tg_waves(out4096); }
MIDAS_EXPORT int midas_debug_ff_clocks(long long* io8192, int reset) { return midas::debug_ff_clocks(io8192, reset); }
#endif

// ---- profiling -----------------------------------------------------------------------------------
MIDAS_EXPORT int midas_profile_enable(midas_ctx* ctx, int32_t on) {
    if (!ctx) return MIDAS_ERR_INVALID;
    MIDAS_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (on && !ctx->ev_ready) {
        for (auto& e : ctx->ev) MIDAS_HIP_CHECK(ctx, hipEventCreate(&e));
        ctx->ev_ready = true;
    }
    ctx->prof = on != 0;
    ctx->prof_only = on >= 2 ? on - 2 : -1;  // 1: every kernel of the step; 2 + k: only kernel slot k
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_profile_read(midas_ctx* ctx, double* ms_out, int64_t* calls_out, int32_t reset) {
    if (!ctx || !ms_out || !calls_out) return MIDAS_ERR_INVALID;
    MIDAS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < MIDAS_PROF_SLOTS; ++i) ms_out[i] = ctx->prof_ms[i];
    *calls_out = ctx->prof_calls;
    if (reset) {
        for (auto& v : ctx->prof_ms) v = 0.0;
        ctx->prof_calls = 0;
    }
    return MIDAS_OK;
}

MIDAS_EXPORT const char* midas_profile_slot_name(int32_t slot) {
    return (slot >= 0 && slot < MIDAS_PROF_SLOTS) ? kSlotNames[slot] : "";
}

}  // extern "C"
