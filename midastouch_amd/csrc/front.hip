// front.hip - the fused front of the step: launch_frame_front (which form of the front a frame takes), the forms of
// k_frame_front without folded resample (the folded ones: front_folded.hip, front_batch.hip), the forms for small particle sets
// (k_frame_front_a + k_particle_nn_prune, k_front_small, k_front_small_objects), and the unfused particle update (k_particle_update) with the reduction
// of its per-wave partials.
// (The small-set kernels share this unit with the plain forms on purpose: in a unit of their own every caller of
// score_claimed_rows_nj passes dense = false, the compiler folds that into the callee before inlining it, and
// k_particle_nn_prune / k_front_small come out with other instructions.)
#include "front_wave.hpp"

namespace midas {

template <bool STATS>
__global__ __launch_bounds__(64) void k_particle_update(TreeView<Kd6> t6, TreeView<Kd3> t3, ParticleUpdateArgs a) {
    __shared__ double s_cd[KD_MAX_LEVELS * 64];  // child-distance columns, reused by both searches
    particle_update_wave<false, false, false, STATS, false, true>(t6, t3, a, blockIdx.x, gridDim.x, blockIdx.y, s_cd);
}

int launch_particle_update(midas_ctx* ctx, const midas_tree* t6, const midas_tree* t3, const ParticleUpdateArgs& a_in) {
    if (a_in.N == 0) return MIDAS_OK;
    ParticleUpdateArgs a = a_in;
    // MIDAS_ABLATE (profiling only, results become wrong): bit 0 skips the NN search, bit 1 the mesh prune
    static const int ablate = getenv("MIDAS_ABLATE") ? atoi(getenv("MIDAS_ABLATE")) : 0;
    a.ablate = ablate;
    const dim3 grid((unsigned)particle_update_blocks(a.N), (unsigned)(a.batch > 1 ? a.batch : 1));
    if (ablate) hipLaunchKernelGGL(k_particle_update<true>, grid, dim3(64), 0, ctx->stream, view_of<Kd6>(t6), view_of<Kd3>(t3), a);
    else hipLaunchKernelGGL(k_particle_update<false>, grid, dim3(64), 0, ctx->stream, view_of<Kd6>(t6), view_of<Kd3>(t3), a);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

// =================================================================================================
// two-kernel form of the front: (A) resample prologue + propagate + feature, beside the codebook scoring;
// (B) nearest neighbour + prune with FOUR lanes per particle
// =================================================================================================
// At N = 100k the particle waves of the single front kernel are 1.5 per SIMD and every one of them walks its whole chain
// of dependent fetches alone.  The chain's second half - list scans - parallelises over records:
// a quad of lanes fetches the 32 solo records of the neighbour list (then the 16 of the vertex list) in ONE round trip
// instead of four (two).  That needs four times the waves, which do not fit beside the 127-register front and the
// scoring stream; as a kernel of its own (no propagate state, no scoring) they do.  The hand-over is 32 bytes per
// particle (6-d feature + hint); the results are the ones of the single-kernel form bit for bit (exact NN with the same
// tie rule, the same "first event in record order" of the prune list).

// part A of a particle wave: what particle_update_wave does before the nearest-neighbour search, plus its rmse epilogue
template <bool FU = false>
MD void particle_front_wave(ParticleUpdateArgs a, int64_t wave, const double* rs_lds, PuFeat* __restrict__ feat) {
    const int lane = threadIdx.x & 63;
    if (a.n_live) {
        const int64_t nl = *a.n_live;
        a.N = nl < a.N ? nl : a.N;
        if (wave * 64 >= a.N && wave != 0) return;
    }
    const int64_t n = wave * 64 + lane;
    const bool live = n < a.N;
    if (wave == 0 && lane == 0) {
        if (a.status_reset) { a.status_reset[0] = 0; a.status_reset[1] = 0; }
        if (a.flags_reset) { a.flags_reset[0] = 0.0; a.flags_reset[1] = 0.0; }
        if (a.sp.next_count) *a.sp.next_count = 0;  // this frame's tail appends the next frame's prediction list
    }
    double et2 = 0.0, ang2 = 0.0;
    int64_t src = n;
    if (rs_lds && live) {
        src = lazy_source<const double*, const double*, NoMid, FU>(a.rs, rs_lds, n, a.N);
        if (a.rs.ridx_out) a.rs.ridx_out[n] = (int32_t)src;
    }
    const float* pose_src = rs_lds ? a.rs.poses_prev : a.poses_in;
    if (live) {
        float P[16], O[16], R[16], f[6];
        load_pose(pose_src + src * 16, P);
        const int32_t hint = rs_lds ? a.rs.nn_prev[src] : a.hint_in ? a.hint_in[n] : -1;
#pragma unroll
        for (int i = 0; i < 16; ++i) O[i] = a.odom16[i];
        propagate_one(n, n + a.slot_base, P, O, a.tn, a.rot, a.std_t, a.std_r, a.seed, a.step, R);
        store_pose(a.poses_prop + n * 16, R);
        se3_feature(R, 0.99f, 0.01f, f);
        float4* o = reinterpret_cast<float4*>(feat + n);
        o[0] = make_float4(f[0], f[1], f[2], f[3]);
        o[1] = make_float4(f[4], f[5], __int_as_float(hint), 0.f);
        if (a.gt16) {
            float G[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) G[i] = a.gt16[i];
            rmse_terms(R, G, et2, ang2);
        }
    }
    if (a.gt16) {
        et2 = wave_sum(et2);
        ang2 = wave_sum(ang2);
        if (lane == 0) { a.part_rmse[2 * wave] = et2; a.part_rmse[2 * wave + 1] = ang2; }
    }
}

template <typename T, int NJ, bool LAZY, bool FU = false>
__global__ __launch_bounds__(256) void k_frame_front_a(ParticleUpdateArgs a, int n_pu, int nwaves, PuFeat* __restrict__ feat,
                                                       const T* __restrict__ emb, const double* __restrict__ norms,
                                                       const double* __restrict__ code, double* __restrict__ scores, int64_t K) {
    __shared__ double s_rs[LAZY ? LAZY_WG_LDS : 8];
    const int w = threadIdx.x >> 6;
    if ((int)blockIdx.x < n_pu) {
        if (LAZY) lazy_tables(a.rs, s_rs);
        const int64_t wave = (int64_t)blockIdx.x * 4 + w;
        if (wave < nwaves) particle_front_wave<FU>(a, wave, LAZY ? s_rs : nullptr, feat);
    } else {
        score_wave<T, NJ, 0>(emb, norms, code, scores, K, (int64_t)(blockIdx.x - n_pu) * 4 + w);
    }
}

template <int CTRL>
MD float dpp_f32(float v) { return __uint_as_float(dpp_u32<CTRL>(__float_as_uint(v))); }

// part B: a wave = 64/LPP particles x LPP lanes (4 or 2); lane g of a group takes records g, g + LPP, ... of its
// particle's lists: with four lanes the 32 solo records of the neighbour list are one round trip of eight records per
// lane, with two lanes two; header + 16 records of the vertex list are one round trip either way.
static_assert(NN_SOLO == 32 && MESH_SOLO == 16, "the group scans fetch 32 / 16 records");
#ifndef MIDAS_NNP_OCC
#define MIDAS_NNP_OCC 2  // the two-kernel form only serves small sets now (launch_frame_front's split_front: a pipelined set of <= 512 particles, a plain one of <= 2048, a live-count set of <= 16 384 - the loop step): registers over occupancy
#endif
template <int LPP>
MD void particle_nn_prune_wg(const TreeView<Kd6>& t6, const TreeView<Kd3>& t3, ParticleUpdateArgs a, const PuFeat* __restrict__ feat) {
    static_assert(LPP == 4 || LPP == 2, "lanes per particle");
    // quad_perm selectors inside a group of LPP lanes: broadcast of its first / last lane
    constexpr int BC_FIRST = LPP == 4 ? 0x00 : 0xA0, BC_LAST = LPP == 4 ? 0xFF : 0xF5;
    constexpr int PPW = 64 / LPP;          // particles per wave
    constexpr int NN_PASSES = 32 / (8 * LPP);  // round trips of eight records per lane
    constexpr int MESH_PER_LANE = 16 / LPP;
    __shared__ double s_cd[4][KD_MAX_LEVELS * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane & (LPP - 1);
    if (a.n_live) {
        const int64_t nl = *a.n_live;
        a.N = nl < a.N ? nl : a.N;
        if ((int64_t)blockIdx.x * 4 * PPW >= a.N) return;  // whole workgroup past the live set
    }
    const int64_t p = ((int64_t)blockIdx.x * 4 + w) * PPW + lane / LPP;
    const bool live = p < a.N, owner = g == 0;
    const int64_t pc = live ? p : (a.N > 0 ? a.N - 1 : 0);
    const float4* fp = reinterpret_cast<const float4*>(feat + pc);
    const float4 f0 = fp[0], f1 = fp[1];
    const float q[6] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y};
    int32_t hint = live ? __float_as_int(f1.z) : -1;
    // the prune's distance-field cell (MeshField) is requested now, under the search: the translation is in the propagated pose
    const float* pr = a.poses_prop + pc * 16;
    const float tq_f[3] = {pr[3], pr[7], pr[11]};
    const FieldProbe probe = field_fetch(a.field, tq_f, live);
    // ---- nearest codebook entry: the solo records of the hinted entry's list ----
    float best = INFINITY, r_lane = 0.f;
    int64_t bi = 0;
    bool done = !live;
    const bool hinted = live && hint >= 0 && (int64_t)hint < t6.K;
    int32_t piv = hinted ? hint : 0;  // the entry whose list is scanned: the hint, or its twin across the angle-pi cut
    int32_t tw = t6.twin[piv];        // (see nn6_hint_scan_screened: a particle far from the hinted entry has crossed the cut)
    const Nbr6* nb = t6.nbrs + (size_t)piv * NBR_REC;
    int pass = 0;                     // group-uniform: the group's next batch of 8 LPP records
#pragma unroll 1
    while (__any(hinted && !done && pass < NN_PASSES)) {
        const int pc_ = pass < NN_PASSES ? pass : NN_PASSES - 1;  // finished groups re-read their last batch (unused)
        Nbr6 e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = nb[pc_ * 8 * LPP + LPP * j + g];
        float d0 = 0.f, ld = INFINITY;
        int li = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            Point6 pt;
#pragma unroll
            for (int c = 0; c < 6; ++c) pt.c[c] = e[j].c[c];
            const float d = dist2(q, pt);
            if (j == 0) d0 = d;  // record 0 (first lane, first pass) is the entry itself: the starting candidate, below
            const bool cand = !(pass == 0 && j == 0 && g == 0);
            if (cand && (d < ld || (d == ld && e[j].idx < li))) { ld = d; li = e[j].idx; }  // NaN never wins
        }
#define MIDAS_GSTEP(CTRL)                                                          \
        {                                                                          \
            const float od = dpp_f32<CTRL>(ld);                                    \
            const int oi = (int)dpp_u32<CTRL>((uint32_t)li);                        \
            if (od < ld || (od == ld && oi < li)) { ld = od; li = oi; }            \
        }
        MIDAS_GSTEP(DPP_XOR1)
        if (LPP == 4) MIDAS_GSTEP(DPP_XOR2)
#undef MIDAS_GSTEP
        d0 = dpp_f32<BC_FIRST>(d0);
        const float rho_last = dpp_f32<BC_LAST>(e[7].rho);  // the largest rho fetched so far
        bool flip = false;
        if (hinted && !done && pass < NN_PASSES) {
            if (pass == 0) {
                best = d0;  // a NaN distance stays, as in the serial scan
                bi = piv;
                r_lane = __builtin_sqrtf(d0);
            }
            if (ld < best || (ld == best && (int64_t)li < bi)) { best = ld; bi = li; }
            // every record behind the last one fetched is at least this far (lower bound with slack for the rounding
            // of r and rho, as in nn6_hint_scan): nothing unseen can beat or tie the best
            const float gg = fmaf_(rho_last - r_lane, 0.9999996f, -8e-7f * r_lane);
            done = gg > 0.0f && gg * gg * 0.99997f > best;
            flip = pass == 0 && !done && r_lane > FLIP_R && tw >= 0;
        }
        if (flip) {  // the twin's list from its start (once: tw = -1)
            piv = tw;
            tw = -1;
            nb = t6.nbrs + (size_t)piv * NBR_REC;
        } else {
            ++pass;
        }
    }
    hint = hinted ? piv : hint;
    nn6_coop(t6, q, hint, r_lane, best, bi, owner && hinted && !done, done);  // the rest of the list, owners = first lanes
    const bool fb = owner && live && !done;
    wave_search<Kd6, false>(t6, q, best, bi, fb, reinterpret_cast<float*>(s_cd[w]));
    if (a.telemetry) {
        const unsigned long long m = __ballot(fb);
        if (lane == 0 && m) atomicAdd(&a.telemetry[0], (unsigned long long)__popcll(m));
    }
    const int32_t nn = (int32_t)dpp_u32<BC_FIRST>((uint32_t)(int32_t)bi);
    // ---- prune: header + records 1 .. 16 of the entry's vertex list in one round trip, requested BEFORE the row claim of the
    // sparse scoring so that the claim's look at the stamps (a round trip of its own) runs beside it ----
    const double q3[3] = {(double)tq_f[0], (double)tq_f[1], (double)tq_f[2]};
    int mv = live ? field_decide(a.field, probe, a.thr) : -1;  // 1 valid, 0 invalid (the distance field: certain), -1 undecided
    const bool lists_needed = __ballot(live && mv < 0) != 0;    // (wave-uniform)
    double lim = 0.0;
    MeshRec hd, e[MESH_PER_LANE];
    if (a.vlist && lists_needed) {
        const MeshRec* vl = a.vlist + (size_t)(live ? nn : 0) * MESH_REC;
        hd = vl[0];
#pragma unroll
        for (int j = 0; j < MESH_PER_LANE; ++j) e[j] = vl[1 + LPP * j + g];
    }
    RowClaim claim{false, 0u};
    if (a.sp.stamps) {
        claim = claim_rows_issue(a.sp, owner && live, nn, MIDAS_CLAIM_HASH ? reinterpret_cast<int*>(s_cd[w]) : nullptr);
        const int nr = score_claimed_rows_nj(a.sp, claim, nn);
        if (a.telemetry && nr && lane == 0) atomicAdd(&a.telemetry[2], (unsigned long long)nr);
    }
    if (a.vlist && lists_needed) {
        Point3 ph;
        ph.c[0] = hd.c[0]; ph.c[1] = hd.c[1]; ph.c[2] = hd.c[2];
        const double delta = __builtin_sqrt(dist2(q3, ph)) * (1.0 + 1e-12);
        lim = a.thr * (1.0 + 1e-9) + delta + 1e-12;  // as mesh_list_check
        unsigned hits = 0, stops = 0;
#pragma unroll
        for (int j = 0; j < MESH_PER_LANE; ++j) {
            Point3 pt;
            pt.c[0] = e[j].c[0]; pt.c[1] = e[j].c[1]; pt.c[2] = e[j].c[2];
            const int pos = LPP * j + g;  // record 1 + pos
            stops |= ((double)e[j].rho * (1.0 - 1e-7) > lim ? 1u : 0u) << pos;
            hits |= (dist2(q3, pt) <= a.t2 ? 1u : 0u) << pos;
        }
        hits |= dpp_u32<DPP_XOR1>(hits); stops |= dpp_u32<DPP_XOR1>(stops);
        if (LPP == 4) { hits |= dpp_u32<DPP_XOR2>(hits); stops |= dpp_u32<DPP_XOR2>(stops); }
        if (live && mv < 0 && (hits | stops)) {  // the first event in record order decides, "provably too far" before "hit"
            const int fh = hits ? __builtin_ctz(hits) : 32, fs = stops ? __builtin_ctz(stops) : 32;
            mv = fh < fs ? 1 : 0;
        }
        mesh_coop(a.vlist, nn, q3, a.t2, lim, owner && live && mv < 0, mv);
    }
    double bestd = a.t2;
    int64_t vi = 0;
    const bool fb3 = owner && live && mv < 0;
    bool ok = wave_search<Kd3, true>(t3, q3, bestd, vi, fb3, s_cd[w]);
    if (a.telemetry) {
        const unsigned long long m = __ballot(fb3);
        if (lane == 0 && m) atomicAdd(&a.telemetry[1], (unsigned long long)__popcll(m));
    }
    if (mv >= 0) ok = mv == 1;
    if (owner && live) {
        a.nn_idx[p] = nn;
        a.valid[p] = ok ? 1 : 0;
    }
}

template <int LPP>
__global__ __launch_bounds__(256, MIDAS_NNP_OCC) void k_particle_nn_prune(TreeView<Kd6> t6, TreeView<Kd3> t3, ParticleUpdateArgs a,
                                                                          const PuFeat* __restrict__ feat) {
    particle_nn_prune_wg<LPP>(t6, t3, a, feat);
}

// Both parts in ONE launch for the loop step's small sets (no folded resample, sparse scoring: no streaming workgroups): a
// workgroup's first wave is part A for the 64 particles the workgroup's four waves then search with four lanes each.  Part A is
// a chain of round trips that one wave per 64 particles carries as well as four waves per 256 did; what goes is a launch
// boundary (~4 us of a frame of 85) and the first touch of the hand-over records by another launch.
// A batch of trajectories (midas_loop_step_batch; trajectory = blockIdx.y): every per-trajectory array is (B, ...) contiguous with
// the launch's capacity a.N as the extent - taken HERE, before the waves clamp a.N to the live count, which every trajectory reads
// from its own control block - its own stamps, tactile code and score row, its own hand-over records, and the Philox key
// seed + trajectory with slot keys from 0: the draws of a single engine built with that seed.
__global__ __launch_bounds__(256, MIDAS_NNP_OCC) void k_front_small(TreeView<Kd6> t6, TreeView<Kd3> t3, ParticleUpdateArgs a, int nwaves,
                                                                    PuFeat* __restrict__ feat) {
    if (blockIdx.y) {
        const int64_t b = blockIdx.y, o = b * a.N;
        a.n_live += b * LOOP_CTL_I;
        a.poses_in += o * 16; a.poses_prop += o * 16; a.odom16 += b * 16;
        if (a.hint_in) a.hint_in += o;
        a.nn_idx += o; a.valid += o;
        if (a.gt16) { a.gt16 += b * 16; a.part_rmse += 2 * b * nwaves; }
        a.sp.stamps += b * a.score_stride; a.sp.scores += b * a.score_stride; a.sp.code += b * (int64_t)(a.sp.nj * 64);
        a.seed += (uint64_t)b;
        if (a.tn) { a.tn += o * 3; a.rot += o * 3; }  // (midas_loop_step_batch_draws: (B, N, 3) host draws)
        feat += o;
    }
    if (threadIdx.x < 64 && (int)blockIdx.x < nwaves) particle_front_wave(a, (int64_t)blockIdx.x, nullptr, feat);
    __syncthreads();  // (drains the first wave's stores of the hand-over records: the other waves read them through the L2)
    particle_nn_prune_wg<4>(t6, t3, a, feat);
}

// k_front_small for a batch whose rows stand on different objects (midas_loop_step_batch_objects): the workgroup takes its row's
// object from the set's row map and that object's record - trees, vertex lists, distance field, embeddings - from the set's
// table.  Both addresses depend on blockIdx.y alone, so the record arrives by scalar loads and stays in SGPRs, where k_front_small
// holds the same values as kernel arguments; nothing is stored before they are read.  Every row takes its offsets, row 0 included
// (its offsets are zero); score and stamp rows are a.score_stride = K_max apart and row b touches the first K_b slots of its own.
// (the body is a file of its own, included here and in the twin that takes std_t, std_r, thr and t2 from the rows' parameter table: the twin then
// shares every statement, and this kernel's token stream - so its code, instruction for instruction - is what it was)
__global__ __launch_bounds__(256, MIDAS_NNP_OCC) void k_front_small_objects(const ObjectRecord* __restrict__ recs,
                                                                            const int32_t* __restrict__ row_object, ParticleUpdateArgs a,
                                                                            int nwaves, PuFeat* __restrict__ feat) {
#include "front_objects_body.hpp"
}

// k_front_small_objects with the motion noise and the prune threshold per row (midas_loop_step_batch_rows): std_t, std_r, thr and t2
// come from row blockIdx.y's record of the parameter table instead of the argument record - four more values by scalar loads through a
// uniform address, in SGPRs where the twin holds kernel arguments (the squared threshold is the host's: no root, no square here);
// no lane loads anything it did not load there.  Behind that head the twin's body.
__global__ __launch_bounds__(256, MIDAS_NNP_OCC) void k_front_small_rows(const ObjectRecord* __restrict__ recs,
                                                                         const int32_t* __restrict__ row_object,
                                                                         const midas_loop_row_params* __restrict__ rows,
                                                                         ParticleUpdateArgs a, int nwaves, PuFeat* __restrict__ feat) {
    const midas_loop_row_params& rp = rows[blockIdx.y];
    a.std_t = rp.std_t; a.std_r = rp.std_r; a.thr = rp.prune_thr; a.t2 = rp.prune_t2;
#include "front_objects_body.hpp"
}

template <int NJ, bool LAZY, bool FU = false>
static void launch_front_a(const FrontLaunch& L, PuFeat* feat) {
    hipLaunchKernelGGL((k_frame_front_a<float, NJ, LAZY, FU>), L.grid, dim3(256), 0, L.ctx->stream, L.a, L.n_pu, L.nwaves, feat,
                       (const float*)L.cb->emb, L.cb->norms, L.code, L.scores, L.cb->K);
}

// the forms without folded resample (the other families: front_folded.hip, front_batch.hip)
bool launch_front_plain(const FrontLaunch& L, const FrontForm& f) {
    return launch_if_form<0, 1, true, true>(L, f) || launch_if_form<0, 1, true, false>(L, f) || launch_if_form<0, 4, true, false>(L, f) ||
           launch_if_form<0, 1, true, false, true>(L, f);
}

// fused front: returns MIDAS_ERR_UNSUPPORTED-like 1 when the codebook layout has no fused instantiation
int launch_frame_front(midas_ctx* ctx, const midas_tree* t6, const midas_tree* t3, const ParticleUpdateArgs& a_in,
                       const midas_codebook* cb, const double* code, double* scores, bool* launched) {
    *launched = false;
    if (a_in.N == 0 || cb->dtype != MIDAS_F32) return MIDAS_OK;
    // a batch of trajectories (grid.y) only in the pipelined form with per-wave tables and sparse scoring (midas_lazy_step_batch)
    if (a_in.batch > 1 && !(a_in.rs.enabled && a_in.rs.nb <= LAZY_WAVE_LD && a_in.sp.stamps)) return MIDAS_OK;
    if ((uintptr_t)cb->emb % 16 != 0 || (uintptr_t)code % 16 != 0) return MIDAS_OK;
    if (cb->D != 512 && cb->D != 256 && cb->D != 128 && cb->D != 1024) return MIDAS_OK;
    if (front_from_u(a_in) && !a_in.rs.u)
        return midas_set_error(ctx, MIDAS_ERR_INVALID, "u32_prev", "MIDAS_U32_FROM_U without the uniforms' pointer");
    ParticleUpdateArgs a = a_in;
    static const int ablate = getenv("MIDAS_ABLATE") ? atoi(getenv("MIDAS_ABLATE")) : 0;
    a.ablate = ablate;
    a.scores = nullptr;  // deferred: the tail gathers the scores
    const int nwaves = particle_update_blocks(a.N), n_pu = (nwaves + 3) / 4;
    if (a.sp.stamps) {  // sparse scoring: the particle waves score the rows they need, no streaming workgroups
        a.sp.emb = (const float*)cb->emb; a.sp.norms = cb->norms; a.sp.code = code; a.sp.scores = scores; a.sp.nj = cb->D / 64;
    }
    // prediction list: scored by streaming workgroups of the single-kernel form only; elsewhere the tags are not honoured
    // (a row stamped pred_tag is then simply stale and gets claimed: same scores)
    static const int list_wgs_env = getenv("MIDAS_LIST_WAVES") ? atoi(getenv("MIDAS_LIST_WAVES")) : 1024;
    const bool use_list = a.sp.stamps && a.sp.list && a.batch <= 1 && list_wgs_env > 0;
    // MIDAS_DENSE_ROWS=<rows>: a frame whose prediction list holds more rows scores the whole codebook with the streaming waves
    // and its particle waves claim nothing (decided on the device, per frame).  Off by default: measured on the frames after a
    // wide start (20k -> 400 distinct rows over the driver's window) it changes nothing (19.2 - 19.5k steps/s either way, thresholds
    // 1500 / 3125 / 6000, 1024 - 4096 streaming waves) - with the prediction lists the claims are no longer what those frames wait for.
    const char* dense_env = getenv("MIDAS_DENSE_ROWS");
    a.sp.K = cb->K;
    a.sp.dense_thr = use_list && dense_env ? atoi(dense_env) : 0;
    const unsigned grid = (unsigned)(n_pu + (a.sp.stamps ? 0 : ceil_div(cb->K, 16)));
    // Two-kernel form (group-parallel list scans, see k_particle_nn_prune) for small particle sets (round 1's rule was "while
    // its N/16 waves fit the chip at once": 65536 particles).  Measured at K = 50k, D = 512 the pipelined frame
    // gains 6 - 15 % for N = 4k .. 40k; when the particle set is materialised every frame the extra launch boundary only pays
    // off for the smallest sets; at N = 100k the four-lane form (two rounds of waves) loses 4 %, the two-lane form (one
    // round, two trips) 8 %, at N = 1M 7 %: there the single kernel stays.
    // MIDAS_SPLIT_FRONT = 0 never, 2 always with 4 lanes per particle, 3 always with 2.
    static const int split_env = getenv("MIDAS_SPLIT_FRONT") ? atoi(getenv("MIDAS_SPLIT_FRONT")) : 1;
    // a live count in device memory (loop engine): the two-kernel form while the caller's bound of the count (a.N here) is small -
    // the set shrinks within a few frames of annealing; a set held at 100k takes the single kernel (42 -> ~22 us at N = 100k)
    // (re-measured after the single kernel's second pass - per-wave tables, one-wave workgroups, screened scans: pipelined,
    // split / single at N = 6k 29.6k / 27.5k steps/s, 8k 29.0k / 27.9k, 12k 28.3k / 28.5k, 20k 25.8k / 27.1k, 65k 21.0k / 22.9k:
    // the two-kernel form now pays up to ~10 000 particles instead of 65 536; the loop step (live count) keeps it: 126 / 138 us)
    // (round 4, with the guide tables in the folded search: the single kernel wins from N = 1000 up - pipelined, split / single at
    // N = 1k 27.4 / 26.4 us a step, 3k 28.8 / 26.8, 8k 28.7 / 26.7, 12k 27.0 / 27.1, 20k 27.5 / 27.5 - so the pipelined form splits no more)
    const bool split_front = a.batch <= 1 && !a.inbox.rows && (split_env >= 2 || (split_env == 1 && ((a.rs.enabled && a.N <= 512) || (!a.rs.enabled && a.N <= 2048) || (a.n_live && a.N <= 16384))));
    const int lpp = split_env == 3 ? 2 : 4;
    if (split_front && !(a.ablate & 7)) {
        a.sp.pred_tag = 0; a.sp.list = nullptr;  // (next_count stays: the tail appends whatever form the front had)
        void* feat;
        int rc = midas_scratch(ctx, (size_t)a.N * sizeof(PuFeat), &feat);
        if (rc) return rc;
        static const bool small_env = !(getenv("MIDAS_FRONT_SMALL") && atoi(getenv("MIDAS_FRONT_SMALL")) == 0);
        if (small_env && !a.rs.enabled && a.sp.stamps && lpp == 4) {  // (no streaming workgroups beside part A: grid == n_pu)
            hipLaunchKernelGGL(k_front_small, dim3((unsigned)ceil_div(a.N, 64)), dim3(256), 0, ctx->stream, view_of<Kd6>(t6), view_of<Kd3>(t3),
                               a, nwaves, (PuFeat*)feat);
        } else {
            const FrontLaunch L{ctx, t6, t3, a, cb, code, scores, dim3(grid), n_pu, nwaves};
            with_nj(cb->D, [&](auto nj) {
                if (front_from_u(a)) launch_front_a<decltype(nj)::value, true, true>(L, (PuFeat*)feat);
                else if (a.rs.enabled) launch_front_a<decltype(nj)::value, true>(L, (PuFeat*)feat);
                else launch_front_a<decltype(nj)::value, false>(L, (PuFeat*)feat);
            });
            if (lpp == 4)
                hipLaunchKernelGGL(k_particle_nn_prune<4>, dim3((unsigned)ceil_div(a.N, 64)), dim3(256), 0, ctx->stream,
                                   view_of<Kd6>(t6), view_of<Kd3>(t3), a, (const PuFeat*)feat);
            else
                hipLaunchKernelGGL(k_particle_nn_prune<2>, dim3((unsigned)ceil_div(a.N, 128)), dim3(256), 0, ctx->stream,
                                   view_of<Kd6>(t6), view_of<Kd3>(t3), a, (const PuFeat*)feat);
        }
        MIDAS_HIP_CHECK(ctx, hipGetLastError());
        *launched = true;
        return MIDAS_OK;
    }
    // the single kernel: workgroup-level tables (more than 64 summation blocks) or per-wave tables, then FW waves per
    // workgroup (MIDAS_FRONT_WAVES = 1 | 4; default 1 with sparse scoring, 4 beside the streaming workgroups)
    static const int fw_env = getenv("MIDAS_FRONT_WAVES") ? atoi(getenv("MIDAS_FRONT_WAVES")) : 0;
    static const int wt_env = getenv("MIDAS_WAVE_TABLES") ? atoi(getenv("MIDAS_WAVE_TABLES")) : 1;
    const bool wave_tables = a.rs.enabled && a.rs.nb <= LAZY_WAVE_LD && wt_env != 0;
    const int fw = a.batch > 1 ? 1 : (a.rs.enabled && !wave_tables) ? 4 : fw_env == 1 || fw_env == 4 ? fw_env : (a.sp.stamps ? 1 : 4);
    const int n_pu_fw = (nwaves + fw - 1) / fw;
    if (!use_list) { a.sp.pred_tag = 0; a.sp.list = nullptr; }
    // presort (see k_presort_search): the batch step (grid.y trajectories), on by default, MIDAS_PRESORT=0 switches it off.
    // Measured at c5 (profiles/r04_c5_presort.txt): grouped and dealt to the waves in runs of 8 (MIDAS_PRESORT_RUN), 298 / 287 us per
    // batch frame against 313 / 303 without - the front itself drops from ~290 to ~237 us, the two launches in front of it cost
    // 53 us (the search they moved out of the front included).  Grouped WITHOUT the deal (a wave = one entry's particles) it loses:
    // a hard entry's particles then share waves, their cooperative continuations (one owner's list per pass) queue up inside a
    // wave instead of spreading over the launch, and the front swings between 180 and 480 us (362 / 331 us).  Compiled into the
    // batch kernels only (SCR = false): tried in the single-trajectory front too, the two launches cost c2 more than the front's
    // whole list phase (14.5k against 23.7k steps/s) and the untaken branches 2 us.
    static const int presort_env = getenv("MIDAS_PRESORT") ? atoi(getenv("MIDAS_PRESORT")) : 1;
    if (wave_tables && fw == 1 && a.batch > 1 && !a.inbox.rows && !a.ablate && !a.n_live && presort_env != 0) {
        const int rc = launch_presort(ctx, a);
        if (rc) return rc;
    }
    const unsigned grid_fw = (unsigned)(n_pu_fw + (a.sp.stamps ? (use_list ? (list_wgs_env + fw - 1) / fw : 0) : ceil_div(cb->K, 4 * fw * MIDAS_SCORE_ROUNDS)));
    // the vertex-list prefetch (PREF) also in the form without folded resample: eager engine 58.8 -> 55.3 us per frame at c2; not
    // where the particles come from a shard's inbox (57.4 - 58.0 us either way: the row's registers are in use there).
    // MIDAS_PREF_PLAIN=0: off
    static const bool pref_env = !(getenv("MIDAS_PREF_PLAIN") && getenv("MIDAS_PREF_PLAIN")[0] == '0');
    const bool pref_plain = pref_env && !a.inbox.rows;
    // the form: k_frame_front's <LAZY, FW, SCR, PREF, STATS> (front_wave.hpp)
    const bool small_set = fw == 1 && a.N <= 131072;  // two waves per SIMD are all the launch needs: registers for the prefetch
    FrontForm form;
    if (a.batch > 1) form = {2, 1, false, false, false};
    else if (!a.rs.enabled) form = {0, fw, true, small_set && pref_plain, false};
    else if (!wave_tables) form = {1, 4, true, false, false};
    else form = {2, fw, true, small_set, false};
    // profiling instantiations (MIDAS_ABLATE != 0; D = 512, one-wave workgroups): phase clocks, scan statistics, ablation switches -
    // of the batch form, of the plain form (without the prefetch) and of the folded form with per-wave tables and the prefetch
    if (a.ablate && cb->D == 512 && fw == 1 && (a.batch > 1 || !a.rs.enabled || form.pref)) {
        form.stats = true;
        if (!a.rs.enabled) form.pref = false;
    }
    const FrontLaunch L{ctx, t6, t3, a, cb, code, scores, dim3(grid_fw, (unsigned)(a.batch > 1 ? a.batch : 1)), n_pu_fw, nwaves};
    if (!(launch_front_batch(L, form) || launch_front_plain(L, form) || launch_front_folded(L, form)))
        return midas_set_error(ctx, MIDAS_ERR_INVALID, "launch_frame_front", "no kernel for this form of the front");
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    *launched = true;
    return MIDAS_OK;
}

int launch_front_small_batch(midas_ctx* ctx, const midas_tree* t6, const midas_tree* t3, const ParticleUpdateArgs& a_in,
                             const midas_codebook* cb, const double* code, double* scores, int32_t B, bool wide) {
    ParticleUpdateArgs a = a_in;
    // wide (midas_loop_step_batch_wide): the same kernel over the ceil(N / 64) waves of a larger capacity - a wave indexes the hand-over
    // records, the per-wave rmse partials and every (B, ...) array in 64 bits, and k_loop_weights sums any number of partials
    if (!(a.n_live && a.N > 0 && (a.N <= 16384 || (wide && a.N <= MIDAS_LOOP_BATCH_WIDE_MAX_CAP)) && a.sp.stamps && !a.rs.enabled && cb->dtype == MIDAS_F32 &&
          (cb->D == 512 || cb->D == 256 || cb->D == 128 || cb->D == 1024) && (uintptr_t)cb->emb % 16 == 0 && (uintptr_t)code % 16 == 0))
        return midas_set_error(ctx, MIDAS_ERR_INVALID, "launch_front_small_batch", "no small-set front for these arguments");
    a.scores = nullptr;  // deferred: k_loop_xe gathers the scores
    a.sp.emb = (const float*)cb->emb; a.sp.norms = cb->norms; a.sp.code = code; a.sp.scores = scores; a.sp.nj = cb->D / 64;
    a.sp.K = cb->K; a.sp.pred_tag = 0; a.sp.list = nullptr;
    a.score_stride = cb->K;
    a.batch = B;
    const int nwaves = particle_update_blocks(a.N);
    void* feat;
    const int rc = midas_scratch(ctx, (size_t)B * a.N * sizeof(PuFeat), &feat);
    if (rc) return rc;
    hipLaunchKernelGGL(k_front_small, dim3((unsigned)ceil_div(a.N, 64), (unsigned)B), dim3(256), 0, ctx->stream, view_of<Kd6>(t6),
                       view_of<Kd3>(t3), a, nwaves, (PuFeat*)feat);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_front_small_objects(midas_ctx* ctx, const midas_object_set* set, const ParticleUpdateArgs& a_in, const double* code,
                               double* scores, bool wide, const midas_loop_row_params* rows) {
    ParticleUpdateArgs a = a_in;
    // (the set's creation checked every codebook: float32, one D of the sparse scoring's, aligned rows)
    if (!(a.n_live && a.N > 0 && (a.N <= 16384 || (wide && a.N <= MIDAS_LOOP_BATCH_WIDE_MAX_CAP)) && a.sp.stamps && !a.rs.enabled &&
          (uintptr_t)code % 16 == 0))
        return midas_set_error(ctx, MIDAS_ERR_INVALID, "launch_front_small_objects", "no small-set front for these arguments");
    a.scores = nullptr;  // deferred: k_loop_xe gathers the scores
    a.sp.code = code; a.sp.scores = scores; a.sp.nj = set->D / 64;
    a.sp.pred_tag = 0; a.sp.list = nullptr;
    a.score_stride = set->K_max;
    a.batch = set->B;
    const int nwaves = particle_update_blocks(a.N);
    void* feat;
    const int rc = midas_scratch(ctx, (size_t)set->B * a.N * sizeof(PuFeat), &feat);
    if (rc) return rc;
    const dim3 grid((unsigned)ceil_div(a.N, 64), (unsigned)set->B);
    if (rows) hipLaunchKernelGGL(k_front_small_rows, grid, dim3(256), 0, ctx->stream, set->recs, set->row_object, rows, a, nwaves, (PuFeat*)feat);
    else hipLaunchKernelGGL(k_front_small_objects, grid, dim3(256), 0, ctx->stream, set->recs, set->row_object, a, nwaves, (PuFeat*)feat);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

// per-wave partials of the particle update -> two extrema and (optionally) two rmse sums
__global__ __launch_bounds__(256) void k_reduce_partials(int np, const double* __restrict__ pmax,
                                                         const double* __restrict__ pmin, const double* __restrict__ prm,
                                                         double* __restrict__ extrema2, double* __restrict__ rmse_sums2) {
    __shared__ double s0[4], s1[4], s2[4], s3[4];
    double a = -INFINITY, b = INFINITY, p = 0.0, q = 0.0;
    bool nan = false;
    for (int i = threadIdx.x; i < np; i += 256) {
        if (pmax) {
            double u = pmax[i], v = pmin[i];
            nan |= (u != u) || (v != v);
            a = u > a ? u : a;
            b = v < b ? v : b;
        }
        if (prm) { p += prm[2 * i]; q += prm[2 * i + 1]; }
    }
    a = wave_max(a);
    b = wave_min(b);
    p = wave_sum(p);
    q = wave_sum(q);
    const bool wnan = __any(nan);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        s0[w] = wnan ? NAN : a; s1[w] = wnan ? NAN : b; s2[w] = p; s3[w] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        bool bad = false;
        for (int i = 0; i < 4; ++i) {
            bad |= s0[i] != s0[i];
            a = s0[i] > a ? s0[i] : a;
            b = s1[i] < b ? s1[i] : b;
        }
        if (extrema2) {
            extrema2[0] = bad ? NAN : a;
            extrema2[1] = bad ? NAN : b;
        }
        if (rmse_sums2) {
            rmse_sums2[0] = (s2[0] + s2[1]) + (s2[2] + s2[3]);
            rmse_sums2[1] = (s3[0] + s3[1]) + (s3[2] + s3[3]);
        }
    }
}

int launch_reduce_partials(midas_ctx* ctx, int np, const double* pmax, const double* pmin, const double* prm,
                           double* extrema2, double* rmse_sums2) {
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, ctx->stream, np, pmax, pmin, prm, extrema2, rmse_sums2);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

MIDAS_WARM_TU(front, k_particle_update<false>)

}  // namespace midas
