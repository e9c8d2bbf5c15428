// api_shard.hip - the sharded engine's entry points: front, tail, route and unpack pieces, peer memory, the frame enqueued by
// one call (midas_shard_step, midas_shard_run) with its pose estimate, and the eager form's resample (midas_tail_resample).
#include <cstdlib>
#include <cstring>

#include "api_entry.hpp"
#include "peer_row.hpp"

using namespace midas;

extern "C" {

// ---- particle-sharded step pieces -------------------------------------------------------------------
// part_rmse_out (C-side frame): the per-wave rmse sums are left in scratch for the tail to add up (no k_reduce_partials launch);
// score_list / predict_out (C-side frame): prediction lists of the sparse scoring as in midas_lazy_args.score_list_dev
// inbox (midas_shard_run, frames after the first): the particles are the rows of the rank's inbox - the previous frame's unpack
// folded into this front (poses_in / hint_in are not read)
static int shard_front_impl(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                            const midas_shard_front_args* args, void** part_rmse_out = nullptr, int32_t* score_list = nullptr,
                            ScorePredict* predict_out = nullptr, const PeerInboxSrc* inbox = nullptr) {
    MIDAS_REQUIRE(ctx, tree6 && tree3 && args && tree6->dim == 6 && tree3->dim == 3);
    const midas_shard_front_args& s = *args;
    MIDAS_REQUIRE(ctx, s.scores_ready || (cb && tree6->K == cb->K && s.code_dev));
    MIDAS_REQUIRE(ctx, s.N > 0 && s.poses_in_dev && s.poses_prop_dev && s.nn_idx_dev && s.valid_dev && s.scores_dev &&
                           s.odom16_dev && s.status_dev && s.flags_dev && s.poses_in_dev != s.poses_prop_dev);
    MIDAS_REQUIRE(ctx, (s.tn_dev == nullptr) == (s.rot_dev == nullptr));
    const int npart = particle_update_blocks(s.N);
    void* prm = nullptr;
    int rc;
    if (s.gt16_dev && s.rmse_sums_dev)
        if ((rc = midas_scratch(ctx, (size_t)npart * 2 * sizeof(double), &prm))) return rc;
    ParticleUpdateArgs pa;
    fill_particle_update(pa, s, tree6, tree3, s.N, s.poses_in_dev, s.hint_in_dev, s.valid_dev, s.scores_ready ? nullptr : s.score_stamps_dev,
                         prm ? s.gt16_dev : nullptr, (double*)prm);
    pa.slot_base = s.slot_base;
    pa.scores = nullptr;  // deferred: midas_shard_tail_a gathers the scores
    pa.status_reset = s.status_dev;
    pa.flags_reset = s.flags_dev;
    if (inbox) pa.inbox = *inbox;
    // (an epoch at the limit is an error here as in lazy_step_impl - bits 31:30 of a stamp are a listed row's age -, not a frame
    // that silently runs without its list)
    MIDAS_REQUIRE(ctx, !(pa.sp.stamps && score_list && predict_out) || s.score_epoch < MIDAS_EPOCH_LIMIT);
    if (pa.sp.stamps && score_list && predict_out && s.score_epoch >= 2 && s.N >= SCAN_CHUNK && cb)
        *predict_out = wire_score_list(pa.sp, score_list, cb->K);
    bool fused = false;
    if (!s.scores_ready && ctx->overlap)
        if ((rc = launch_frame_front(ctx, tree6, tree3, pa, cb, s.code_dev, s.scores_dev, &fused))) return rc;
    if (!fused) {
        pa.sp = SparseScore();  // the unfused form scores every row first
        if (!s.scores_ready)
            if ((rc = launch_score(ctx, cb, 1, s.code_dev, s.scores_dev))) return rc;
        if ((rc = launch_particle_update(ctx, tree6, tree3, pa))) return rc;
    }
    if (!fused && predict_out) *predict_out = ScorePredict();  // the unfused form scored every row: no list for the next frame
    if (part_rmse_out) { *part_rmse_out = prm; return MIDAS_OK; }
    if (prm) return launch_reduce_partials(ctx, npart, nullptr, nullptr, (const double*)prm, nullptr, s.rmse_sums_dev);
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_shard_front(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* tree6,
                                   const midas_tree* tree3, const midas_shard_front_args* args) {
    MIDAS_ENTER(ctx);
    return shard_front_impl(ctx, cb, tree6, tree3, args);
}

// tables block of one shard: the lazy layout without the per-block records (those live in the exchange record r1)
static TailTables shard_tables_of(double* t, int64_t N) { return tables_of(t, N, false); }

MIDAS_EXPORT int midas_shard_tail_a(midas_ctx* ctx, int64_t N, const double* scores_dev, const int32_t* nn_idx_dev,
                                    const uint8_t* valid_dev, int32_t softmax, double* tables_dev, double* r1_dev,
                                    int32_t* status_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && scores_dev && nn_idx_dev && valid_dev && tables_dev && (uintptr_t)tables_dev % 128 == 0 && r1_dev &&
                           status_dev);
    return launch_shard_tail_a(ctx, N, scores_dev, nn_idx_dev, valid_dev, softmax, shard_tables_of(tables_dev, N), r1_dev, status_dev);
}

MIDAS_EXPORT int midas_shard_tail_fin(midas_ctx* ctx, int64_t N, const double* tables_dev, const uint8_t* valid_dev,
                                      double* weights_dev, double* cdf_dev, int32_t G, const double* r1_all_dev, int32_t rank,
                                      int64_t N_total, int32_t softmax, double* rmse_dev, int32_t* status_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && G > 0 && rank >= 0 && rank < G && tables_dev && valid_dev && weights_dev && cdf_dev && r1_all_dev &&
                           N_total >= N && status_dev);
    const int nb = (int)ceil_div(N, SCAN_BLOCK);
    const TailTables tb = shard_tables_of(const_cast<double*>(tables_dev), N);
    return launch_tail_fin(ctx, N, tb.e, tb.x_raw, tb.lp, tb.lp_raw, valid_dev, weights_dev, cdf_dev, G, nb, r1_all_dev, rank,
                           (double)N_total, softmax, rmse_dev, status_dev);
}

static int shard_route(midas_ctx* ctx, const midas_shard_route_args* args, bool pack, const PeerRouteSync* sync = nullptr) {
    MIDAS_REQUIRE(ctx, args != nullptr);
    const midas_shard_route_args& s = *args;
    MIDAS_REQUIRE(ctx, s.N >= 256 && s.G > 0 && s.G <= 64 && s.rank >= 0 && s.rank < s.G && s.r1_all_dev && s.tables_dev &&
                           (uintptr_t)s.tables_dev % 128 == 0 && s.valid_dev && s.nn_idx_dev && s.poses_prop_dev && s.status_dev &&
                           s.counts_dev);
    MIDAS_REQUIRE(ctx, !pack || (s.weights_dev && (s.peers_dev || (s.send_dev && (uintptr_t)s.send_dev % 8 == 0))));
    MIDAS_REQUIRE(ctx, !pack || s.peers_dev || s.fixed_cap == 0 || (s.fixed_cap > 0 && s.ovf_cap > 0 && s.ovf_dev && (uintptr_t)s.ovf_dev % 8 == 0 && s.self_dev && (uintptr_t)s.self_dev % 8 == 0 &&
                                                     s.G * s.fixed_cap < ((int64_t)1 << 31)));
    MIDAS_REQUIRE(ctx, s.resample_mode == MIDAS_RESAMPLE_MULTINOMIAL || s.resample_mode == MIDAS_RESAMPLE_SYSTEMATIC);
    TailTables tb = shard_tables_of(const_cast<double*>(s.tables_dev), s.N);
    if (s.guide_dev) {  // (read only by the peer-mapped form's searches; the table layout of midas_lazy_args.guide_dev)
        MIDAS_REQUIRE(ctx, (uintptr_t)s.guide_dev % 16 == 0);
        tb.guide = reinterpret_cast<guide_t*>(const_cast<uint8_t*>(s.guide_dev));
        tb.guide_raw = tb.guide + ceil_div(s.N, SCAN_BLOCK) * GUIDE_STRIDE;
    }
    return launch_shard_route(ctx, s, tb, pack, sync);
}

MIDAS_EXPORT int midas_shard_route_count(midas_ctx* ctx, const midas_shard_route_args* args) {
    MIDAS_ENTER(ctx);
    return shard_route(ctx, args, false);
}

MIDAS_EXPORT int midas_shard_route_pack(midas_ctx* ctx, const midas_shard_route_args* args) {
    MIDAS_ENTER(ctx);
    return shard_route(ctx, args, true);
}

MIDAS_EXPORT int midas_shard_unpack(midas_ctx* ctx, int64_t N, const void* recv_dev, int32_t* ridx_dev, float* poses_out_dev,
                                    double* weights_out_dev, int32_t* hint_out_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && recv_dev && (uintptr_t)recv_dev % 8 == 0 && ridx_dev && poses_out_dev && weights_out_dev && hint_out_dev);
    return launch_shard_unpack(ctx, N, recv_dev, ridx_dev, poses_out_dev, weights_out_dev, hint_out_dev);
}

MIDAS_EXPORT int midas_shard_unpack_rows(midas_ctx* ctx, int64_t rows, const void* recv_dev, int32_t dest, int32_t* ridx_dev,
                                         float* poses_out_dev, double* weights_out_dev, int32_t* hint_out_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, rows > 0 && recv_dev && (uintptr_t)recv_dev % 8 == 0 && ridx_dev && poses_out_dev && weights_out_dev && hint_out_dev);
    return launch_shard_unpack(ctx, rows, recv_dev, ridx_dev, poses_out_dev, weights_out_dev, hint_out_dev, dest);
}

MIDAS_EXPORT int midas_shard_unpack_fixed(midas_ctx* ctx, int64_t rows_recv, const void* recv_dev, int64_t rows_ovf,
                                          const void* ovf_all_dev, int32_t rank, int64_t rows_self, const void* self_dev,
                                          int32_t* ridx_dev, float* poses_out_dev, double* weights_out_dev, int32_t* hint_out_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, rows_recv >= 0 && rows_ovf >= 0 && rows_self >= 0 && rank >= 0 && ridx_dev && poses_out_dev && weights_out_dev &&
                           hint_out_dev);
    MIDAS_REQUIRE(ctx, (rows_recv == 0 || (recv_dev && (uintptr_t)recv_dev % 8 == 0)) && (rows_ovf == 0 || (ovf_all_dev && (uintptr_t)ovf_all_dev % 8 == 0)) &&
                           (rows_self == 0 || (self_dev && (uintptr_t)self_dev % 8 == 0)));
    int rc = MIDAS_OK;
    if (rows_recv > 0) rc = launch_shard_unpack(ctx, rows_recv, recv_dev, ridx_dev, poses_out_dev, weights_out_dev, hint_out_dev, -1);
    if (rc == MIDAS_OK && rows_ovf > 0) rc = launch_shard_unpack(ctx, rows_ovf, ovf_all_dev, ridx_dev, poses_out_dev, weights_out_dev, hint_out_dev, rank);
    if (rc == MIDAS_OK && rows_self > 0) rc = launch_shard_unpack(ctx, rows_self, self_dev, ridx_dev, poses_out_dev, weights_out_dev, hint_out_dev, -1);
    return rc;
}

MIDAS_EXPORT int midas_shard_unpack_peer(midas_ctx* ctx, int64_t N, const void* inbox_dev, int32_t* ridx_dev, float* poses_out_dev,
                                         double* weights_out_dev, int32_t* hint_out_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && inbox_dev && (uintptr_t)inbox_dev % 8 == 0 && ridx_dev && poses_out_dev && weights_out_dev && hint_out_dev);
    return launch_shard_unpack_peer(ctx, N, inbox_dev, ridx_dev, poses_out_dev, weights_out_dev, hint_out_dev);
}

MIDAS_EXPORT int midas_peer_alloc(midas_ctx* ctx, int64_t bytes, void** ptr_out, void* handle64_out) {
    MIDAS_ENTER(ctx);
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "the interprocess handle is 64 bytes");
    MIDAS_REQUIRE(ctx, bytes > 0 && ptr_out && handle64_out);
    void* p = nullptr;
    MIDAS_HIP_CHECK(ctx, hipExtMallocWithFlags(&p, (size_t)bytes, hipDeviceMallocFinegrained));
    hipIpcMemHandle_t h;
    const hipError_t e = hipIpcGetMemHandle(&h, p);
    if (e != hipSuccess) {
        (void)hipFree(p);
        MIDAS_HIP_CHECK(ctx, e);
    }
    MIDAS_HIP_CHECK(ctx, hipMemsetAsync(p, 0, (size_t)bytes, ctx->stream));
    memcpy(handle64_out, &h, 64);
    *ptr_out = p;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_peer_free(midas_ctx* ctx, void* ptr) {
    MIDAS_ENTER(ctx);
    if (ptr) MIDAS_HIP_CHECK(ctx, hipFree(ptr));
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_peer_open(midas_ctx* ctx, const void* handle64, void** ptr_out) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, handle64 && ptr_out);
    hipIpcMemHandle_t h;
    memcpy(&h, handle64, 64);
    void* p = nullptr;
    MIDAS_HIP_CHECK(ctx, hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
    *ptr_out = p;
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_peer_close(midas_ctx* ctx, void* ptr) {
    MIDAS_ENTER(ctx);
    if (ptr) MIDAS_HIP_CHECK(ctx, hipIpcCloseMemHandle(ptr));
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_peer_probe_write(midas_ctx* ctx, void* const* peers_dev, int32_t G, int32_t rank, int32_t nonce) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, peers_dev && G > 0 && G <= 64 && rank >= 0 && rank < G);
    return launch_peer_probe(ctx, peers_dev, nullptr, G, rank, nonce, nullptr);
}

MIDAS_EXPORT int midas_peer_probe_check(midas_ctx* ctx, const void* inbox_dev, int32_t G, int32_t nonce, int32_t* ok_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, inbox_dev && G > 0 && G <= 64 && ok_dev);
    return launch_peer_probe(ctx, nullptr, inbox_dev, G, 0, nonce, ok_dev);
}

// ---- the sharded frame enqueued by ONE call, on a library-owned RCCL communicator ------------------------------------------
struct midas_comm;
extern "C" int midas_comm_all_gather(midas_comm* c, const void* send_dev, void* recv_dev, int64_t bytes);

// The frame's pose estimate across the ranks (filter/filter.py:184-186; midas_shard_step_estimate / midas_shard_run_estimate)
struct ShardEstimate {
    double* part;      // ceil(N / 256) x 36: this rank's moment partials
    double* part_all;  // G x the same, in rank order
    float* center;     // 16 out
    float* stds;       // 3 out
};
static int64_t estimate_blocks(int64_t N) { return ceil_div(N, (int64_t)256); }

// from_inbox (midas_shard_run): the front takes its particles from the rows of the inbox (the previous frame ran without its
// UNPACK phase; its route kernel ended with the inbox complete)
// est: behind ROUTE (which leaves the masked weights in weights_dev) the rank's moment partials, their all_gather and the finish -
// in front of UNPACK and of the next frame's front, which rewrites poses_prop
static int shard_step_impl(midas_ctx* ctx, midas_comm* comm, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                           const midas_shard_step_args& s, int32_t phases, bool from_inbox = false, const ShardEstimate* est = nullptr) {
    MIDAS_REQUIRE(ctx, phases != 0 && (phases & ~31) == 0);
    MIDAS_REQUIRE(ctx, s.front.N >= 256 && s.G >= 1 && s.G <= 64 && s.rank >= 0 && s.rank < s.G && s.tables_dev && s.r1_dev);
    MIDAS_REQUIRE(ctx, s.r1_all_dev || !(phases & (MIDAS_SHARD_PHASE_GATHER | MIDAS_SHARD_PHASE_ROUTE)));
    const int64_t N = s.front.N;
    const int nb = (int)ceil_div(N, SCAN_BLOCK);
    const int64_t rec = 5 * (int64_t)nb + 4;
    int rc;
    if (phases & MIDAS_SHARD_PHASE_LOCAL) {  // propagate / NN / prune / scoring, then the shard's softmax tables and its record
        void* prm = nullptr;
        ScorePredict predict;
        PeerInboxSrc src;
        if (from_inbox) {
            MIDAS_REQUIRE(ctx, s.inbox_dev && s.flag_offset >= N * PEER_ROW);
            src.rows = (const char*)s.inbox_dev;
        }
        if ((rc = shard_front_impl(ctx, cb, tree6, tree3, &s.front, &prm, s.score_list_dev, &predict, from_inbox ? &src : nullptr))) return rc;
        MIDAS_REQUIRE(ctx, (uintptr_t)s.tables_dev % 128 == 0);
        TailTables tbs = shard_tables_of(s.tables_dev, N);
        if (s.guide_dev) {
            MIDAS_REQUIRE(ctx, (uintptr_t)s.guide_dev % 16 == 0);
            tbs.guide = reinterpret_cast<guide_t*>(s.guide_dev);
            tbs.guide_raw = tbs.guide + nb * GUIDE_STRIDE;
        }
        if ((rc = launch_shard_tail_a(ctx, N, s.front.scores_dev, s.front.nn_idx_dev, s.front.valid_dev, s.softmax,
                                      tbs, s.r1_dev, s.front.status_dev, (const double*)prm,
                                      predict.stamps ? &predict : nullptr)))
            return rc;
    }
    if (phases & MIDAS_SHARD_PHASE_GATHER) {  // one record per rank, in rank order, to every rank
        MIDAS_REQUIRE(ctx, comm != nullptr);
        if ((rc = midas_comm_all_gather(comm, s.r1_dev, s.r1_all_dev, rec * (int64_t)sizeof(double)))) return rc;
    }
    if (phases & (MIDAS_SHARD_PHASE_ROUTE | MIDAS_SHARD_PHASE_UNPACK))
        MIDAS_REQUIRE(ctx, s.peers_dev && s.inbox_dev && s.flag_offset >= N * PEER_ROW && s.flag_offset % 8 == 0 && s.frame_tag != 0 &&
                               s.counts_dev && s.weights_dev && s.ridx_dev && s.poses_out_dev && s.weights_out_dev && s.hint_out_dev);
    if (phases & MIDAS_SHARD_PHASE_ROUTE) {  // owner-side resample into the peers' inboxes, then the completion flags
        midas_shard_route_args r;
        memset(&r, 0, sizeof(r));
        r.N = N; r.G = s.G; r.rank = s.rank;
        r.r1_all_dev = s.r1_all_dev; r.tables_dev = s.tables_dev; r.valid_dev = s.front.valid_dev; r.nn_idx_dev = s.front.nn_idx_dev;
        r.poses_prop_dev = s.front.poses_prop_dev; r.status_dev = s.front.status_dev; r.rmse_dev = s.rmse_dev;
        r.softmax = s.softmax; r.resample_mode = s.resample_mode; r.u_all_dev = s.u_all_dev; r.u32 = s.u32;
        r.seed = s.front.seed; r.step = s.front.step;
        r.counts_dev = s.counts_dev; r.weights_dev = s.weights_dev; r.peers_dev = s.peers_dev;
        r.guide_dev = s.guide_dev;
        // without FLAG the route kernel's last workgroup publishes this rank's flag and waits for every rank's: when the kernel
        // ends the inbox is complete (one polling wave; the word behind the 64 flags is its workgroup counter)
        const PeerRouteSync sync{(const char*)s.inbox_dev, s.flag_offset, s.frame_tag};
        if ((rc = shard_route(ctx, &r, true, (phases & MIDAS_SHARD_PHASE_FLAG) ? nullptr : &sync))) return rc;
        if (phases & MIDAS_SHARD_PHASE_FLAG)  // shards of one process on one stream: the flags must be out before ANY shard waits
            if ((rc = launch_peer_flag_write(ctx, s.peers_dev, s.G, s.rank, s.flag_offset, s.frame_tag))) return rc;
    }
    if (est) {
        const int64_t nbm = estimate_blocks(N);
        if ((rc = launch_shard_estimate_moments(ctx, N, s.front.poses_prop_dev, s.weights_dev, est->part))) return rc;
        if ((rc = midas_comm_all_gather(comm, est->part, est->part_all, nbm * ESTIMATE_PART_DOUBLES * (int64_t)sizeof(double)))) return rc;
        if ((rc = launch_shard_estimate_finish(ctx, s.G * nbm, est->part_all, est->center, est->stds))) return rc;
    }
    if (phases & MIDAS_SHARD_PHASE_UNPACK) {  // inbox -> slots; with FLAG behind a wait for every rank's flag in the own inbox
        if (phases & MIDAS_SHARD_PHASE_FLAG)
            rc = launch_shard_unpack_peer_wait(ctx, N, s.inbox_dev, s.ridx_dev, s.poses_out_dev, s.weights_out_dev, s.hint_out_dev,
                                               s.G, s.flag_offset, s.frame_tag, s.front.status_dev, nullptr, s.rank);
        else
            rc = launch_shard_unpack_peer(ctx, N, s.inbox_dev, s.ridx_dev, s.poses_out_dev, s.weights_out_dev, s.hint_out_dev);
        if (rc) return rc;
    }
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_shard_step(midas_ctx* ctx, midas_comm* comm, const midas_codebook* cb, const midas_tree* tree6,
                                  const midas_tree* tree3, const midas_shard_step_args* args, int32_t phases) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, args != nullptr);
    return shard_step_impl(ctx, comm, cb, tree6, tree3, *args, phases);
}

static bool shard_estimate_ok(const ShardEstimate& e) {
    return e.part && e.part_all && e.center && e.stds && (uintptr_t)e.part % 16 == 0 && (uintptr_t)e.part_all % 16 == 0;
}

MIDAS_EXPORT int midas_shard_estimate_moments(midas_ctx* ctx, int64_t N, const float* poses_prop_dev, const double* weights_dev,
                                              double* part_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, N > 0 && poses_prop_dev && weights_dev && part_dev && (uintptr_t)poses_prop_dev % 16 == 0 &&
                           (uintptr_t)part_dev % 16 == 0);
    return launch_shard_estimate_moments(ctx, N, poses_prop_dev, weights_dev, part_dev);
}

MIDAS_EXPORT int midas_shard_estimate_finish(midas_ctx* ctx, int64_t nblocks, const double* part_all_dev, float* center_dev,
                                             float* stds_dev) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, nblocks > 0 && nblocks <= (int64_t)1 << 24 && part_all_dev && center_dev && stds_dev && (uintptr_t)part_all_dev % 16 == 0);
    return launch_shard_estimate_finish(ctx, nblocks, part_all_dev, center_dev, stds_dev);
}

static const int32_t SHARD_WHOLE_FRAME = MIDAS_SHARD_PHASE_LOCAL | MIDAS_SHARD_PHASE_GATHER | MIDAS_SHARD_PHASE_ROUTE | MIDAS_SHARD_PHASE_UNPACK;

MIDAS_EXPORT int midas_shard_step_estimate(midas_ctx* ctx, midas_comm* comm, const midas_codebook* cb, const midas_tree* tree6,
                                           const midas_tree* tree3, const midas_shard_step_args* args, double* part_dev,
                                           double* part_all_dev, float* center_dev, float* stds_dev) {
    MIDAS_ENTER(ctx);
    const ShardEstimate est{part_dev, part_all_dev, center_dev, stds_dev};
    MIDAS_REQUIRE(ctx, args != nullptr && comm != nullptr && shard_estimate_ok(est));
    return shard_step_impl(ctx, comm, cb, tree6, tree3, *args, SHARD_WHOLE_FRAME, false, &est);
}

// est_log: NULL, or the partial buffers and the T x 16 / T x 3 logs (row f: frame f's estimate)
static int shard_run_impl(midas_ctx* ctx, midas_comm* comm, const midas_codebook* cb, const midas_tree* tree6, const midas_tree* tree3,
                          const midas_shard_step_args* first, int32_t T, const ShardEstimate* est_log) {
    MIDAS_REQUIRE(ctx, first != nullptr && comm != nullptr && cb != nullptr && T >= 1);
    MIDAS_REQUIRE(ctx, !first->front.tn_dev && !first->front.rot_dev && !first->u_all_dev && !first->front.scores_ready);
    midas_shard_step_args a = *first;
    if (a.front.score_stamps_dev)  // every epoch of the run checked before anything is enqueued (see midas_lazy_run)
        MIDAS_REQUIRE(ctx, (uint64_t)a.front.score_epoch + (a.score_list_dev ? 2ull : 1ull) * (uint64_t)(T - 1) < (uint64_t)MIDAS_EPOCH_LIMIT);
    // The unpack of every frame but the last is folded into the NEXT frame's front: the rows other ranks stored into this rank's
    // inbox are read there, behind the same flag wait (MIDAS_SHARD_FOLD=0: every frame unpacks into the particle arrays).
    // Safe with one inbox: a peer stores the rows of frame f + 1 behind its record all_gather of frame f + 1, which completes only
    // when every rank has joined it - and a rank joins behind its own front of frame f + 1, the reader of the rows of frame f.
    static const bool fold = !(getenv("MIDAS_SHARD_FOLD") && getenv("MIDAS_SHARD_FOLD")[0] == '0');
    for (int32_t f = 0; f < T; ++f) {
        int rc = f ? scratch_reset(ctx) : MIDAS_OK;
        if (rc) return rc;
        const bool last = f == T - 1;
        const int32_t phases = MIDAS_SHARD_PHASE_LOCAL | MIDAS_SHARD_PHASE_GATHER | MIDAS_SHARD_PHASE_ROUTE | ((last || !fold) ? MIDAS_SHARD_PHASE_UNPACK : 0);
        ShardEstimate est;
        if (est_log) est = ShardEstimate{est_log->part, est_log->part_all, est_log->center + 16 * (size_t)f, est_log->stds + 3 * (size_t)f};
        if ((rc = shard_step_impl(ctx, comm, cb, tree6, tree3, a, phases, fold && f > 0, est_log ? &est : nullptr))) return rc;
        // next frame: the resampled particles are in poses_out / hint_out (= the front's inputs: the engine passes the same buffers)
        a.front.step += 1;
        a.frame_tag += 1;
        a.u32 = -1.0f;
        if (a.front.score_stamps_dev) a.front.score_epoch += a.score_list_dev ? 2u : 1u;
        a.front.odom16_dev += 16;
        a.front.code_dev += cb->D;
        if (a.front.gt16_dev) a.front.gt16_dev += 16;
    }
    return MIDAS_OK;
}

MIDAS_EXPORT int midas_shard_run(midas_ctx* ctx, midas_comm* comm, const midas_codebook* cb, const midas_tree* tree6,
                                 const midas_tree* tree3, const midas_shard_step_args* first, int32_t T) {
    MIDAS_ENTER(ctx);
    return shard_run_impl(ctx, comm, cb, tree6, tree3, first, T, nullptr);
}

MIDAS_EXPORT int midas_shard_run_estimate(midas_ctx* ctx, midas_comm* comm, const midas_codebook* cb, const midas_tree* tree6,
                                          const midas_tree* tree3, const midas_shard_step_args* first, int32_t T, double* part_dev,
                                          double* part_all_dev, float* est_centers_dev, float* est_stds_dev) {
    MIDAS_ENTER(ctx);
    const ShardEstimate est{part_dev, part_all_dev, est_centers_dev, est_stds_dev};
    MIDAS_REQUIRE(ctx, shard_estimate_ok(est));
    return shard_run_impl(ctx, comm, cb, tree6, tree3, first, T, &est);
}

MIDAS_EXPORT int midas_tail_resample(midas_ctx* ctx, const midas_tail_resample_args* args) {
    MIDAS_ENTER(ctx);
    MIDAS_REQUIRE(ctx, args && args->N > 0 && args->n_per_rank > 0 && args->N_all >= args->N && args->slot_base >= 0 &&
                           args->slot_base + args->N <= args->N_all && args->pack_all_dev &&
                           args->rank_stride >= 84 * args->n_per_rank && args->rank_stride % 16 == 0 &&
                           args->n_per_rank % 2 == 0 && args->status_dev && args->ridx_dev && args->poses_out_dev &&
                           args->weights_out_dev && args->hint_out_dev);
    MIDAS_REQUIRE(ctx, args->mode == MIDAS_RESAMPLE_MULTINOMIAL || args->mode == MIDAS_RESAMPLE_SYSTEMATIC);
    return launch_tail_resample(ctx, *args);
}

}  // extern "C"
