// front_wave.hpp - one particle wave of a frame front (particle_update_wave) with the folded-resample prologue (lazy_*), and
// k_frame_front, the kernel template every single-launch form of the front instantiates: front.hip (no folded resample),
// front_folded.hip (folded, one trajectory), front_batch.hip (folded, a batch of trajectories).
#pragma once
#include <type_traits>

#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "score_body.hpp"
#include "peer_row.hpp"
#include "resample_search.hpp"
#include "list_scan.hpp"
#include "pose.hpp"

namespace midas {

#ifndef MIDAS_SCORE_ROUNDS
#define MIDAS_SCORE_ROUNDS 2  // quads of codebook rows a scoring wave of the fused front streams (dense scoring)
#endif
#ifndef MIDAS_CLAIM_HASH
#define MIDAS_CLAIM_HASH 1  // leaders of the row claims through an LDS hash table (score_body.hpp claim_rows_issue); 0: ballot rounds
#endif

// ---- resample of the previous frame as a prologue of the particle update (LazyResample) -------------------------
// Workgroup part: guard, sequential block prefix, exact cdf at the block ends into LDS (every thread of the
// 256-thread workgroup takes part).  rs_lds: [0, nb) block prefix | [256, 256+nb) block ends | 512: total, 513: S,
// 514: apply | [516, 516+nb) block sums of e | [LAZY_WG_W, +nb) block totals (the guide tables' bin width).  Same arithmetic as
// k_tail_b / k_tail_b2.
constexpr int LAZY_WG_W = 3 * LAZY_MAX_BLOCKS + 8, LAZY_WG_LDS = 4 * LAZY_MAX_BLOCKS + 8;
MD void lazy_tables(const LazyResample& rs, double* rs_lds) {
    __shared__ double s_ex[12];
    const int t = threadIdx.x;
    const int b = t < rs.nb ? t : rs.nb - 1;  // nb <= 256: one block per thread, clamped loads
    const double bt = rs.btot[b], btr = rs.btot_raw[b], bs = rs.bsum_e[b], bx = rs.bmax[b], bn = rs.bmin[b];
    const int32_t status = rs.status_prev[0];  // with the records: read in lazy_source it was a round trip of its own
    const bool in = t < rs.nb;
    double mx = in ? bx : -INFINITY, mn = in ? bn : INFINITY;
    const bool nan = in && ((bx != bx) || (bn != bn));
    mx = wave_max_dpp(mx);  // (DPP moves: midas_math.hpp)
    mn = wave_min_dpp(mn);
    const bool wn = __any(nan);
    if ((t & 63) == 0) { s_ex[t >> 6] = mx; s_ex[4 + (t >> 6)] = mn; s_ex[8 + (t >> 6)] = wn ? 1.0 : 0.0; }
    __syncthreads();
    mx = s_ex[0]; mn = s_ex[4];
    double f = s_ex[8];
    for (int w = 1; w < 4; ++w) { mx = s_ex[w] > mx ? s_ex[w] : mx; mn = s_ex[4 + w] < mn ? s_ex[4 + w] : mn; f += s_ex[8 + w]; }
    if (f != 0.0) { mx = NAN; mn = NAN; }
    const bool apply = rs.softmax && !(__builtin_fabs(mx - mn) <= ISCLOSE_ATOL);
    double* s_bp = rs_lds;
    double* s_w = rs_lds + 256;
    double* s_se = rs_lds + 516;
    if (in) { s_w[t] = apply ? bt : btr; s_se[t] = bs; }
    __syncthreads();
    if (t == 0) {
        double acc = 0.0, S = 0.0;
        for (int i = 0; i < rs.nb; ++i) { s_bp[i] = acc; acc = acc + s_w[i]; S = S + s_se[i]; }
        rs_lds[512] = acc;
        rs_lds[513] = apply ? S : 1.0;
        rs_lds[514] = apply ? 1.0 : 0.0;
        rs_lds[515] = status != 0 ? 1.0 : 0.0;
    }
    __syncthreads();
    const double total = rs_lds[512];
    // exact cdf at the last slot of every block: (BP_b + W_b) / total - the block total IS the block-local prefix at
    // the block's last slot (same additions in the same order); the last block ends at N-1, forced to 1
    const double wb = in ? s_w[t] : 0.0;
    __syncthreads();
    if (in) rs_lds[LAZY_WG_W + t] = wb;
    if (in) s_w[t] = (t == rs.nb - 1) ? 1.0 : (s_bp[t] + wb) / total;
    __syncthreads();
}

// The same tables built by ONE wave for itself (nb <= 64: N <= 262144), split in two so that the pose-independent half of
// the motion model runs between the loads and their use: no workgroup barrier, no serial LDS loop - the sequential block
// prefix is a left fold over lane values read with v_readlane (the same additions in the same order as lazy_tables).
// Layout of the wave's block (LAZY_WAVE_LDS doubles): [0, 64) block prefix | [64, 128) block ends | 128 total | 130 apply |
// 131 status of the previous frame | [132, 196) block totals (the guide table's bin width, GUIDE_BINS).
constexpr int LAZY_WAVE_LD = 64, LAZY_WAVE_LDS = 3 * LAZY_WAVE_LD + 4;
struct LazyRecords { double bt, btr, bx, bn; int32_t status; };
MD LazyRecords lazy_records_load(const LazyResample& rs) {
    const int lane = threadIdx.x & 63;
    const int b = lane < rs.nb ? lane : rs.nb - 1;
    LazyRecords r;
    r.bt = rs.btot[b]; r.btr = rs.btot_raw[b]; r.bx = rs.bmax[b]; r.bn = rs.bmin[b];
    r.status = rs.status_prev[0];
    return r;
}
MD void lazy_tables_wave(const LazyResample& rs, const LazyRecords& r, double* rs_lds) {
    const int lane = threadIdx.x & 63;
    const bool in = lane < rs.nb;
    double mx = in ? r.bx : -INFINITY, mn = in ? r.bn : INFINITY;
    const bool nan = in && ((r.bx != r.bx) || (r.bn != r.bn));
    mx = wave_max_dpp(mx);  // (DPP moves: midas_math.hpp)
    mn = wave_min_dpp(mn);
    if (__any(nan)) { mx = NAN; mn = NAN; }
    const bool apply = rs.softmax && !(__builtin_fabs(mx - mn) <= ISCLOSE_ATOL);
    const double w = in ? (apply ? r.bt : r.btr) : 0.0;
    // The sequential prefix of the block totals: the totals go through LDS (every lane reads the same eight values a round -
    // broadcast reads, all requested before the first addition) and every lane runs the same chain of additions, keeping the
    // value it passes at its own block.  Blocks past nb hold +0.0: adding them changes nothing (the sum never is -0.0).
    // (v_readlane with the block number in a scalar register cost two hazards and a branch per block: 1.4 us of a wave's life)
    double* s_wb = rs_lds + 2 * LAZY_WAVE_LD + 4;
    s_wb[lane] = w;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double acc = 0.0, bp = 0.0;
    for (int i0 = 0; i0 < rs.nb; i0 += 8) {
        double wv[8];
        const double2* p2 = reinterpret_cast<const double2*>(s_wb + i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double2 t = p2[j]; wv[2 * j] = t.x; wv[2 * j + 1] = t.y; }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            bp = lane == i0 + j ? acc : bp;
            acc = acc + wv[j];
        }
    }
    const double total = acc;
    if (in) {
        rs_lds[lane] = bp;
        rs_lds[LAZY_WAVE_LD + lane] = (lane == rs.nb - 1) ? 1.0 : (bp + w) / total;
    }
    if (lane == 0) {
        rs_lds[2 * LAZY_WAVE_LD] = total;
        rs_lds[2 * LAZY_WAVE_LD + 2] = apply ? 1.0 : 0.0;
        rs_lds[2 * LAZY_WAVE_LD + 3] = r.status != 0 ? 1.0 : 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Per-lane part: the source particle of slot n (what k_tail_b2 writes to ridx[n]).
// ld = stride of the table block: 256 (lazy_tables, one block per workgroup) or LAZY_WAVE_LD (lazy_tables_wave)
// gend_lds / lp_lds (both or gend_lds alone): the caller's LDS copies of the chunk-end / per-slot tables
// mid: arithmetic of the caller's that does not depend on the search, run once while the guide entries travel (NoMid: none; a lane
// that leaves the search before that point has not run it - the caller looks at its own flag)
// FU: the twin of a systematic frame with u32 == MIDAS_U32_FROM_U - the trajectory's offset is the first double of its row of `u`
// (midas_math.hpp systematic_draw; front_from_u below picks the twin at the launch).  Every other frame runs FU = false: the code it
// always ran.
template <typename GT = const double*, typename LT = const double*, typename MID = NoMid, bool FU = false>
MD int64_t lazy_source(const LazyResample& rs, const double* rs_lds, int64_t n, int64_t N, int ld = 256, GT gend_lds = nullptr,
                       LT lp_lds = nullptr, MID mid = MID()) {
    const double* s_bp = rs_lds;
    const double* s_end = rs_lds + ld;
    const double total = rs_lds[2 * ld];
    const bool apply = rs_lds[2 * ld + 2] != 0.0;
    const bool bad_total = !(total == total) || total == 0.0;
    if (rs_lds[2 * ld + 3] != 0.0 || bad_total) return n;  // unusable weights: the resampler keeps the particles
    const double* __restrict__ lp = apply ? rs.lp : rs.lp_raw;
    const double* __restrict__ gend = apply ? rs.gend : rs.gend_raw;
    double tq;
    bool upper;
    if (rs.mode == MIDAS_RESAMPLE_MULTINOMIAL) {
        tq = rs.u ? rs.u[n] : philox_uniform53((uint64_t)(n + rs.key_base), rs.seed, rs.step);
        upper = false;
    } else {
        const float r = systematic_draw<FU>(rs.u32, rs.u, rs.seed + (uint64_t)rs.traj, rs.step);
        const float off = r / (float)N;
        tq = (double)n / (double)N + (double)off;
        tq = tq >= 1.0 ? tq - 1.0 : tq;
        upper = true;
    }
    auto left_exact = [&](double c) { return upper ? (c <= tq) : (c < tq); };
    // block: first b whose exact end value is not left of the draw
    int lo = 0, hi = rs.nb;
    while (hi > lo) {
        const int mid = lo + ((hi - lo) >> 1);
        if (left_exact(s_end[mid])) lo = mid + 1; else hi = mid;
    }
    if (lo >= rs.nb) return N - 1;
    if constexpr (__is_same(LT, lds_cdp)) {
        return search_in_block_t<lds_cdp, GT>(lp_lds, gend, apply ? rs.ggend : rs.ggend_raw, lo, N, N - 1, s_bp[lo], total, tq, upper, gend_lds);
    } else {
        // guide table of the block: the unit from one entry pair (the block totals sit behind the tables, per wave or per workgroup)
        const guide_t* guide = apply ? rs.guide : rs.guide_raw;
        return search_in_block_t<const double*, GT, MID>(lp, gend, apply ? rs.ggend : rs.ggend_raw, lo, N, N - 1, s_bp[lo], total, tq, upper, gend_lds,
                                                         guide, guide ? rs_lds[(ld == LAZY_WAVE_LD ? 2 * LAZY_WAVE_LD + 4 : LAZY_WG_W) + lo] : 0.0, mid);
    }
}

// =================================================================================================
// fused particle update of the step
// =================================================================================================
// One wave = 64 consecutive particles of trajectory `traj`; `wave` counts the waves of that trajectory,
// `nwaves` = waves per trajectory (strides of the per-wave partial arrays), s_cd = this wave's LDS columns.
// WT (with rs_lds): the wave builds the resample tables itself (lazy_tables_wave; rs_lds = its own LAZY_WAVE_LDS doubles)
// SCREEN: half-record screening in the list scans (see part4)
// PREF: the vertex list's header and first batch are requested before the sparse-scoring claim (72 more registers: only
// where two waves per SIMD are all the launch needs, N <= 131072 in one-wave workgroups)
// STATS (profiling instantiations only, chosen by MIDAS_ABLATE != 0): per-wave phase clocks, scan statistics and the ablation
// switches; the production instantiations read no clock and test no switch
// PRES: the presorted form (pre_order / pre_src, batch kernels only) is compiled in; elsewhere the arguments are ignored
// NANPART: the per-wave extrema of x carry a NaN score on (k_particle_update alone: the one kernel whose partials a guard reads -
// the eager step's legacy tail, k_tail_a; every other form of the tail gathers the scores itself)
template <bool WT = false, bool SCREEN = false, bool PREF = false, bool STATS = false, bool PRES = false, bool NANPART = false, bool FU = false>
MD void particle_update_wave(const TreeView<Kd6>& t6, const TreeView<Kd3>& t3, ParticleUpdateArgs a, int64_t wave,
                             int nwaves, int traj, double* s_cd, double* rs_lds = nullptr) {
    const int lane = threadIdx.x & 63;
    if (a.n_live) {  // variable particle count: the grid covers the capacity, the waves past the live set leave
        const int64_t nl = *a.n_live;
        a.N = nl < a.N ? nl : a.N;
        if (wave * 64 >= a.N && wave != 0) return;
    }
    if (traj) {  // batch of trajectories: every per-trajectory array is (B, ...) contiguous
        const int64_t b = traj, o = b * a.N;
        a.poses_in += o * 16; a.poses_prop += o * 16; a.odom16 += b * 16;
        if (a.tn) { a.tn += o * 3; a.rot += o * 3; }
        if (a.hint_in) a.hint_in += o;
        a.nn_idx += o; a.valid += o;
        if (a.scores) { a.scores += b * a.score_stride; a.x += o; a.e += o; a.part_max += b * nwaves; a.part_min += b * nwaves; }
        if (a.gt16) { a.gt16 += b * 16; a.part_rmse += 2 * b * nwaves; }
        if (a.status_reset) a.status_reset += 2 * b;
        if (a.sp.stamps) {  // sparse scoring per trajectory: its own stamps, tactile code and score row
            a.sp.stamps += b * a.score_stride; a.sp.scores += b * a.score_stride; a.sp.code += b * (int64_t)(a.sp.nj * 64);
        }
        a.slot_base += o;
        if (a.rs.enabled) {  // pipelined batch: per-trajectory table blocks, previous-frame arrays and draws
            const int64_t ts = b * a.rs.tstride;
            a.rs.e += ts; a.rs.x_raw += ts; a.rs.lp += ts; a.rs.lp_raw += ts; a.rs.gend += ts; a.rs.gend_raw += ts;
            a.rs.ggend += ts; a.rs.ggend_raw += ts; a.rs.bsum_e += ts; a.rs.btot += ts; a.rs.btot_raw += ts; a.rs.bmax += ts; a.rs.bmin += ts;
            a.rs.poses_prev += o * 16; a.rs.nn_prev += o; a.rs.status_prev += 2 * b;
            if (a.rs.ridx_out) a.rs.ridx_out += o;
            if (a.rs.u) a.rs.u += o;
            a.rs.key_base = o;
            a.rs.traj = traj;
        }
        if (a.pre_order) { a.pre_order += o; a.pre_src += o; if (a.pre_rmse_terms) a.pre_rmse_terms += 2 * o; }
    }
    // presorted (wave-uniform): lane `rank` of the launch works on slot order[rank] - slots that start from the same codebook
    // entry sit side by side, so the list records a wave's lanes ask for are mostly the SAME addresses (one look-up, one line)
    const bool presorted = PRES && a.pre_order != nullptr;
    const int64_t rank = wave * 64 + lane;
    const bool live = rank < a.N;
    int64_t n = rank;
    int32_t src_pre = 0;
    if (presorted) {
        n = a.pre_order[live ? rank : 0];
        src_pre = a.pre_src[live ? rank : 0];
    }
    if (wave == 0 && lane == 0) {
        if (a.status_reset) { a.status_reset[0] = 0; a.status_reset[1] = 0; }
        if (a.flags_reset) { a.flags_reset[0] = 0.0; a.flags_reset[1] = 0.0; }
        if (a.sp.next_count) *a.sp.next_count = 0;  // this frame's tail appends the next frame's prediction list
    }
    unsigned long long st_nn = 0, st_mesh = 0, st_scan = 0;
    int st_rows = 0;
    const bool dense_scores = scores_dense(a.sp);  // requested here, looked at after the nearest-neighbour search
    const int ablate = STATS ? a.ablate : 0;
    long long tc[10];  // phase clocks, reported with MIDAS_ABLATE=4
    long long tp[4] = {0, 0, 0, 0};  // ... and inside the first phase (MIDAS_ABLATE=4 + 128: reported in place of phases 4 .. 7)
#define MIDAS_TICK(i) do { if (STATS) tc[i] = clock64(); } while (0)
#define MIDAS_PTICK(i) do { if (STATS) tp[i] = clock64(); } while (0)
    MIDAS_TICK(0);
    const long long wall0 = STATS ? wall_clock64() : 0;  // 100 MHz
    double x = 0.0, et2 = 0.0, ang2 = 0.0;
    float R[16], f[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 16; ++i) R[i] = 0.f;
    // source of the particle: its own slot, or - resample of the previous frame folded in - slot src of the previous
    // frame's propagated poses
    int64_t src = n;
    float NO[16];
    if (WT) {
        // the block records travel while the pose-independent half of the motion model (draws, noise transform,
        // O @ Tn: half of the propagate's arithmetic) is computed; the tables are then built from registers
        // (memory operations come back in order: the odometry is requested BEFORE the records, or waiting for it would
        // be waiting for them)
        float O[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) O[i] = a.odom16[i];
        __builtin_amdgcn_sched_barrier(0);
        LazyRecords rec;
        if (!presorted) rec = lazy_records_load(a.rs);
        __builtin_amdgcn_sched_barrier(0);
        // (the draws under the records' round trip; the noise transform and O @ Tn under the guide entries' - see lazy_source)
        float tnv[3] = {0.f, 0.f, 0.f}, rotv[3] = {0.f, 0.f, 0.f};
        bool no_done = false;
        if (live) noise_draws(n, n + a.slot_base, a.tn, a.rot, a.std_t, a.std_r, a.seed, a.step, tnv, rotv);
        if (!presorted) lazy_tables_wave(a.rs, rec, rs_lds);
        MIDAS_PTICK(0);  // records there, tables built (draws done under their trip)
        auto mid = [&]() { noise_apply(O, tnv, rotv, NO); no_done = true; };
        if (rs_lds && live && !presorted && !(ablate & 8)) {
            src = lazy_source<const double*, const double*, decltype(mid), FU>(a.rs, rs_lds, n, a.N, LAZY_WAVE_LD, (const double*)nullptr,
                                                                               (const double*)nullptr, mid);
            if (a.rs.ridx_out) a.rs.ridx_out[n] = (int32_t)src;
        }
        if (live && !no_done) mid();
        MIDAS_PTICK(1);  // source slot known (guide entries, prefix piece)
    }
    if (rs_lds && live) {
        if (presorted) {
            src = src_pre;  // (ridx_out was written by the presort)
        } else if (!WT) {
            // ablate 8 (profiling): no search, own slot
            src = (ablate & 8) ? n : lazy_source<const double*, const double*, NoMid, FU>(a.rs, rs_lds, n, a.N, 256);
            if (a.rs.ridx_out) a.rs.ridx_out[n] = (int32_t)src;
        }
    }
    const float* pose_src = rs_lds ? a.rs.poses_prev : a.poses_in;
    // the sharded frame with the unpack folded in (midas_shard_run): the particle of slot n is row n of this rank's inbox, stored
    // there by the owner of its source; the rows are complete - the route kernel in front of this launch ended with every
    // rank's completion flag in
    const bool from_inbox = !WT && a.inbox.rows != nullptr;
    PeerRow row;
    if (from_inbox && live) row = peer_row_load(a.inbox.rows, n);
    // the hint travels with the pose (behind the store of the propagated pose it would be a round trip of its own)
    const int32_t hint = !live ? -1 : from_inbox ? (int32_t)(row.head[1] & 0xFFFFFFFFull) : rs_lds ? a.rs.nn_prev[src] : a.hint_in ? a.hint_in[n] : -1;
    if (live) {
        float P[16];
        if (from_inbox) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                P[2 * k] = __int_as_float((int)(row.pose[k] & 0xFFFFFFFFull));
                P[2 * k + 1] = __int_as_float((int)(row.pose[k] >> 32));
            }
        } else {
            load_pose(pose_src + src * 16, P);
        }
        if (WT) {
            mat4_mul(P, NO, R);
            MIDAS_PTICK(2);  // source row there, propagated
        } else {
            float O[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) O[i] = a.odom16[i];
            propagate_one(n, n + a.slot_base, P, O, a.tn, a.rot, a.std_t, a.std_r, a.seed, a.step, R);
        }
        store_pose(a.poses_prop + n * 16, R);
        se3_feature(R, 0.99f, 0.01f, f);
    }
    // the prune's distance-field cell is requested now (it needs the translation only): the answer arrives under the search
    const float tq_f[3] = {R[3], R[7], R[11]};
    const FieldProbe probe = field_fetch(a.field, tq_f, live && !(ablate & 2));
    MIDAS_TICK(1);
    // nearest codebook entry
    int32_t bi = 0;
    float bd;
    if (ablate & 1) {  // profiling only: trust the hint
        bi = hint < 0 ? 0 : hint;
    } else {
        int nscan = 0;
        const bool fb = nn6_wave<false, SCREEN>(t6, f, live, hint, bi, bd, reinterpret_cast<float*>(s_cd), nullptr, nullptr, STATS ? &nscan : nullptr,
                                                STATS ? &tc[2] : nullptr);
        MIDAS_TICK(3);
        if (a.telemetry && (ablate & 4)) {  // MIDAS_ABLATE=4: scan statistics (profiling only), flushed at the end
            st_nn = __ballot(live && nscan >= NN_SOLO - 1);
            st_scan = (unsigned long long)wave_sum((double)nscan);
        }
        if (a.telemetry) {
            const unsigned long long m = __ballot(fb);
            if (lane == 0 && m) atomicAdd(&a.telemetry[0], (unsigned long long)__popcll(m));
        }
    }
    // sparse scoring: the first particle of the frame on an entry has it scored - the exchanges leave here, the answers are
    // looked at after the prune
    // (small-set regime, registers to spare: the vertex list's header and first batch are requested before the claim, whose
    // look at the stamps is a round trip of its own)
    // (of the float32 screening copy; without one the float64 list is read after the claim)
    constexpr bool PRE = PREF;
    // prune, first word: the distance field (1 valid, 0 invalid: certain; -1: the vertex lists / the tree decide)
    int mv = live ? field_decide(a.field, probe, a.thr) : -1;
    const bool lists_needed = __ballot(live && mv < 0) != 0;  // (wave-uniform: a wave whose particles are all decided skips the lists)
    MeshScr pre[PRE ? 1 + MESH_BATCH : 1];
    if (PRE && a.vscr != nullptr && lists_needed) {
        const MeshScr* vs = a.vscr + (size_t)(live ? bi : 0) * MESH_REC;
#pragma unroll
        for (int j = 0; j < (PRE ? 1 + MESH_BATCH : 1); ++j) pre[j] = vs[j];
    }
    RowClaim claim{false, 0u};
    if (a.sp.stamps && !(ablate & 16)) {  // ablate 16 (profiling): nobody scores
        claim = claim_rows_issue(a.sp, live, bi, MIDAS_CLAIM_HASH ? reinterpret_cast<int*>(s_cd) : nullptr);
        st_rows = score_claimed_rows_nj(a.sp, claim, bi, dense_scores);
    }
    MIDAS_TICK(9);
    // prune: valid <=> some mesh vertex within sqrt(t2) of the particle
    double q3[3] = {(double)R[3], (double)R[7], (double)R[11]};
    double best = a.t2;
    int64_t vi = 0;
    if (ablate & 2) mv = 1;
    else if (a.vlist && lists_needed) {
        double lim_lane = 0.0;
        const bool open = live && mv < 0;  // the lanes the field left undecided
        if (a.vscr) {  // first records, per lane: float32 screening copy, the float64 records only for what it cannot decide
            const float tqf[3] = {R[3], R[7], R[11]};
            if (open) mv = mesh_screen_check<PRE>(a.vscr, bi, tqf, a.thr, MESH_SOLO, &lim_lane, pre);
            if (__ballot(mv == -2)) {
                if (mv == -2) mv = mesh_list_check<false>(a.vlist, bi, q3, a.t2, a.thr, MESH_SOLO, &lim_lane);
            }
        } else if (open) {
            mv = mesh_list_check<false>(a.vlist, bi, q3, a.t2, a.thr, MESH_SOLO, &lim_lane);
        }
        MIDAS_TICK(4);
        if (a.telemetry && (ablate & 4)) st_mesh = __ballot(live && mv < 0);
        mesh_coop(a.vlist, bi, q3, a.t2, lim_lane, live && mv < 0, mv);             // the rest, whole wave per lane
    }
    MIDAS_TICK(5);
    bool ok = wave_search<Kd3, true>(t3, q3, best, vi, live && mv < 0, s_cd);
    if (a.telemetry) {
        const unsigned long long m = __ballot(live && mv < 0);
        if (lane == 0 && m) atomicAdd(&a.telemetry[1], (unsigned long long)__popcll(m));
    }
    if (mv >= 0) ok = mv == 1;
    if (a.telemetry && st_rows && lane == 0) atomicAdd(&a.telemetry[2], (unsigned long long)st_rows);  // rows scored by particle waves
    MIDAS_TICK(6);
    if (live) {
        a.nn_idx[n] = bi;
        if (a.scores) {  // nullptr: the scoring runs concurrently, the tail gathers the scores
            x = a.scores[bi];
            a.x[n] = x;
            a.e[n] = exp_spec(x - 1.0);
        }
        a.valid[n] = ok ? 1 : 0;
        if (a.gt16) {
            float G[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) G[i] = a.gt16[i];
            rmse_terms(R, G, et2, ang2);
        }
    }
    MIDAS_TICK(7);
    // per-wave extrema of x over live lanes
    const double NEG = -INFINITY, POS = INFINITY;
    if (a.scores) {
        double mx = wave_max(live ? x : NEG), mn = wave_min(live ? x : POS);
        // NaN never wins a comparison: a wave with a NaN score hands on NaN extrema (torch.max / min propagate it), which is where
        // block_extrema looks for it - the guard is then open and every weight NaN, not the raw scores of a collapsed cloud
        if (NANPART && __any(live && x != x)) { mx = NAN; mn = NAN; }
        if (lane == 0) { a.part_max[wave] = mx; a.part_min[wave] = mn; }
    }
    if (a.gt16) {
        if (presorted && a.pre_rmse_terms) {
            // a presorted wave holds other slots than 64 wave .. 64 wave + 63: its sum would be a different (and, the order inside
            // a group being what the LDS atomics made it, run-dependent) grouping of the same terms.  The terms go out by slot.
            if (live) reinterpret_cast<double2*>(a.pre_rmse_terms)[n] = make_double2(et2, ang2);
        } else {
            et2 = wave_sum(et2);
            ang2 = wave_sum(ang2);
            if (lane == 0) { a.part_rmse[2 * wave] = et2; a.part_rmse[2 * wave + 1] = ang2; }
        }
    }
    if (STATS && a.telemetry && (ablate & 4) && lane == 0) {
        // MIDAS_ABLATE=4: per-wave scan statistics and phase clocks, plain stores into the wave's own 16 slots
        // behind the 16 cumulative counters (the caller sized the buffer 16 + 16 * waves)
        tc[8] = clock64();
        unsigned long long* w = a.telemetry + 16 + 16 * ((size_t)traj * nwaves + wave);
        w[0] += (unsigned long long)st_rows;                 // codebook rows this wave scored (sparse scoring)
        w[1] = (unsigned long long)wall0;                    // start of the wave (100 MHz wall clock, not cumulative)
        w[2] += (unsigned long long)__popcll(st_nn); w[4] += st_nn ? 1 : 0;
        w[3] += (unsigned long long)__popcll(st_mesh); w[5] += st_mesh ? 1 : 0;
        w[6] += st_scan;
        w[7] += (unsigned long long)(wall_clock64() - wall0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            long long d = i == 3 ? tc[9] - tc[3] : i == 4 ? tc[5] - tc[9] : tc[i + 1] - tc[i];  // [3] claim + scoring, [4] prune lists
            // + 128: the first phase in four pieces instead of phases 4 .. 7: records + tables, source slot, source row + product,
            // store + feature + field probe
            if ((ablate & 128) && i >= 4) d = !tp[0] ? 0 : i == 4 ? tp[0] - tc[0] : i == 5 ? tp[1] - tp[0] : i == 6 ? tp[2] - tp[1] : tc[1] - tp[2];  // (frames without a folded resample: nothing)
            w[8 + i] += (unsigned long long)d;
        }
    }
#undef MIDAS_TICK
#undef MIDAS_PTICK
}

// Front kernel of the fused step: the particle update (latency-bound: dependent scattered
// fetches, ~1.5 waves per SIMD) and the codebook scoring (HBM-bound stream) have no dependency on each other -
// the scores are only gathered in the tail - so they share ONE launch: workgroups [0, n_pu) run FW
// particle waves each and start first, workgroups [n_pu, ...) stream codebook rows behind them (all K rows, or the
// prediction list of the sparse scoring) and fill the memory pipes the particle waves leave idle.
// k_frame_front<T, NJ, LAZY, FW, SCR, PREF, STATS> - the one statement of its layout (launch_frame_front, front.hip, picks the form):
// T, NJ: element type of the codebook rows (float) and their length in 64-element pieces (D = 64 NJ: 2, 4, 8 or 16)
// LAZY: 0 the particles are read from the particle arrays (or a shard's inbox); 1 the resample of the previous frame runs as a
// prologue of the particle waves (midas_lazy_step) from tables built per workgroup (more than 64 summation blocks; 256 threads:
// FW = 4); 2 the same with the tables built per wave (nb <= 64), which also frees the workgroup size
// FW: particle waves per workgroup, 1 or 4 (64 FW threads).  With FW = 1 the 1563 particle waves of c2 spread 6 - 7 per CU;
// workgroups of four land 4 or 8 on a CU.  One-wave workgroups are the small-set regime: screened list scans (MIDAS_SCREEN)
// SCR = false (batch of trajectories, grid.y): whole-record list scans - the screen costs the batch step more than it saves - and
// the presorted form compiled in
// PREF: the vertex list's header and first batch are requested before the sparse-scoring claim (see particle_update_wave)
// STATS: the profiling instantiations (MIDAS_ABLATE != 0; D = 512, one-wave workgroups only)
// Launch bounds: 64 FW threads; waves per SIMD MIDAS_BATCH_OCC for the batch form, MIDAS_FRONT4_OCC for LAZY 1, else MIDAS_FRONT_OCC.
#ifndef MIDAS_FRONT_OCC
#define MIDAS_FRONT_OCC 1  // waves per SIMD the single-trajectory forms are compiled for (1 = no register cap: 234 registers, two waves)
#endif
#ifndef MIDAS_FRONT4_OCC
#define MIDAS_FRONT4_OCC 4  // ... and the four-wave workgroups with workgroup-level tables = sets beyond 131 072 particles: several rounds of waves, four a SIMD (c3, N = 1 M: 190 -> 181 us; 3: no gain).  NOT the four-wave form of the dense front at smaller N (per-wave tables): one round of waves, the cap cost it 4 us of 29
#endif
#ifndef MIDAS_BATCH_OCC
#define MIDAS_BATCH_OCC 1  // waves per SIMD the batch form (SCR = false) is compiled for (1 = no register cap)
#endif
// wall-clock span of the front's particle waves [0, 1] and of its scoring waves [2, 3] (tools/tg_clocks.py, tools/diag_early.py).
// The build has no relocatable device code, so a __device__ variable belongs to one translation unit: under MIDAS_DEBUG_CLOCKS
// the stamps are taken by the forms of front_folded.hip only (MIDAS_FRONT_CLOCKS: the pipelined single-trajectory frame, what
// the two tools run), where g_ff_clk and debug_ff_clocks live; the plain and the batch forms take none.
#if defined(MIDAS_DEBUG_CLOCKS) && defined(MIDAS_FRONT_CLOCKS)
__device__ long long g_ff_clk[16384];  // per frame parity and workgroup: start, end
#define FF_T0 const long long ff_t0_ = wall_clock64()
#define FF_END do { if (threadIdx.x == 0 && blockIdx.x < 4096) { long long* c_ = g_ff_clk + (a.step & 1) * 8192; c_[2 * blockIdx.x] = ff_t0_; c_[2 * blockIdx.x + 1] = wall_clock64(); } } while (0)
#else
#define FF_T0 do { } while (0)
#define FF_END do { } while (0)
#endif
template <typename T, int NJ, int LAZY, int FW, bool SCR = true, bool PREF = false, bool STATS = false, bool FU = false>
__global__ __launch_bounds__(64 * FW, (!SCR && FW == 1) ? MIDAS_BATCH_OCC : (FW == 4 && LAZY == 1) ? MIDAS_FRONT4_OCC : MIDAS_FRONT_OCC) void k_frame_front(TreeView<Kd6> t6, TreeView<Kd3> t3, ParticleUpdateArgs a,
                                                         int n_pu, int nwaves, const T* __restrict__ emb,
                                                         const double* __restrict__ norms, const double* __restrict__ code,
                                                         double* __restrict__ scores, int64_t K) {
    static_assert(LAZY != 1 || FW == 4, "the workgroup-level tables take 256 threads");
    FF_T0;
    __shared__ double s_cd[FW][KD_MAX_LEVELS * 64];
    __shared__ alignas(16) double s_rs[LAZY == 1 ? LAZY_WG_LDS : LAZY == 2 ? FW * LAZY_WAVE_LDS : 8];
    const int w = threadIdx.x >> 6;
    // (a batch's trajectories bound to XCDs - XCD c serving the trajectories c mod 8 so that its L2 sees an eighth of the batch's
    // lists - was measured and dropped: 371 against 319 us per c5 batch frame)
    const unsigned bx = blockIdx.x, by = blockIdx.y;
    if ((int)bx < n_pu) {
        if (LAZY == 1) lazy_tables(a.rs, s_rs);
        const int64_t wave = (int64_t)bx * FW + w;
        if (wave < nwaves) {
            // one-wave workgroups = the small-set regime (see launch_frame_front): screened scans
            constexpr bool SCREEN = FW == 1 && MIDAS_SCREEN && SCR;
            const int traj = (int)by;
            if (LAZY == 2) particle_update_wave<true, SCREEN, PREF, STATS, !SCR && !STATS, false, FU>(t6, t3, a, wave, nwaves, traj, s_cd[w], s_rs + w * LAZY_WAVE_LDS);
            else particle_update_wave<false, SCREEN, PREF, STATS, false, false, FU>(t6, t3, a, wave, nwaves, traj, s_cd[w], LAZY ? s_rs : nullptr);
        }
    } else if (a.sp.list) {  // prediction list: the rows the previous frame used, four per wave-instruction
        if ((int)bx == n_pu && threadIdx.x == 0 && a.telemetry) {  // rows scored off the list (cumulative, for the bench's byte count)
            const int c = *a.sp.list_count;
            if (a.sp.dense_thr > 0 && c > a.sp.dense_thr) atomicAdd(&a.telemetry[3], (unsigned long long)a.sp.K);  // all of them
            else if (c > 0) atomicAdd(&a.telemetry[3], (unsigned long long)(c < a.sp.list_cap ? c : a.sp.list_cap));
        }
        if (!(STATS && (a.ablate & 64)))  // ablate 64 (profiling): the list is not scored - what its stream costs the particle waves
            score_list_wave<NJ>(a.sp, (int)(bx - n_pu) * FW + w, ((int)gridDim.x - n_pu) * FW);
    } else {
        // all K rows (the dense K1 beside the particle waves): MIDAS_SCORE_ROUNDS consecutive quads of rows a wave, requested
        // together (score_wave_multi, score_body.hpp)
        const int64_t w0 = ((int64_t)(bx - n_pu) * FW + w) * MIDAS_SCORE_ROUNDS;
        if (w0 * 4 < K) score_wave_multi<T, NJ, MIDAS_SCORE_ROUNDS>(emb, norms, code, scores, K, w0);
    }
    FF_END;
}

// hand-over record of the two-kernel form (front.hip): 6-d feature + hint of a particle
struct alignas(16) PuFeat { float f[6]; int32_t hint; int32_t pad; };
static_assert(sizeof(PuFeat) == 32, "two 16-byte pieces per particle");

// ---- launching a form ---------------------------------------------------------------------------------------------------------
// cb->D -> NJ, the one place: f(std::integral_constant<int, NJ>())
template <class F>
void with_nj(int32_t D, F&& f) {
    switch (D) {
        case 512: f(std::integral_constant<int, 8>()); break;
        case 256: f(std::integral_constant<int, 4>()); break;
        case 128: f(std::integral_constant<int, 2>()); break;
        default: f(std::integral_constant<int, 16>()); break;
    }
}
// the folded resample's systematic offset stands in device memory (MIDAS_U32_FROM_U): the FU twins of the folded forms
inline bool front_from_u(const ParticleUpdateArgs& a) {
    return a.rs.enabled && a.rs.mode == MIDAS_RESAMPLE_SYSTEMATIC && a.rs.u32 == MIDAS_U32_FROM_U;
}
template <int NJ, int LAZY, int FW, bool SCR, bool PREF, bool STATS, bool FU = false>
void launch_front_kernel(const FrontLaunch& L) {
    hipLaunchKernelGGL((k_frame_front<float, NJ, LAZY, FW, SCR, PREF, STATS, FU>), L.grid, dim3(64 * FW), 0, L.ctx->stream, view_of<Kd6>(L.t6),
                       view_of<Kd3>(L.t3), L.a, L.n_pu, L.nwaves, (const float*)L.cb->emb, L.cb->norms, L.code, L.scores, L.cb->K);
}
// launches form f if it is <LAZY, FW, SCR, PREF, STATS> (a unit's launcher lists its forms with this, each once); the profiling
// forms are instantiated for D = 512 alone and launch_frame_front asks for them there only
template <int LAZY, int FW, bool SCR, bool PREF, bool STATS = false>
bool launch_if_form(const FrontLaunch& L, const FrontForm& f) {
    if (f.lazy != LAZY || f.fw != FW || f.scr != SCR || f.pref != PREF || f.stats != STATS) return false;
    if constexpr (STATS) {
        if (front_from_u(L.a)) return false;  // (the profiling forms have no FU twin)
        launch_front_kernel<8, LAZY, FW, SCR, PREF, true>(L);
    } else {
        with_nj(L.cb->D, [&](auto nj) {
            if constexpr (LAZY != 0) {
                if (front_from_u(L.a)) {
                    launch_front_kernel<decltype(nj)::value, LAZY, FW, SCR, PREF, false, true>(L);
                    return;
                }
            }
            launch_front_kernel<decltype(nj)::value, LAZY, FW, SCR, PREF, false>(L);
        });
    }
    return true;
}

}  // namespace midas
