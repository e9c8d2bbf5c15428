// loop_resample.hip - RESAMPLE of a loop frame (loop.hip): k_loop_scan (blocked prefix sums of (e * valid)[src] over the annealed set) ->
// k_loop_resample (n_set draws, exact inverse search on cdf_i = (BP_b + lp_i) / total, gathers through src; the frame's bookkeeping).
// A frame whose uniforms come from a caller's stream (stream_draws) is split in front of the resample; its first call ends with
// k_loop_scan -> k_loop_ndraw: ctl_i[NDRAW], the uniforms the reference's resampler draws - none on all-zero or NaN weights.
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "tail_block.hpp"
#include "anneal_clocks.hpp"

namespace midas {

// block-local prefix of (e * valid)[src] (or x * valid when the weights are raw scores) in the spec order
__global__ __launch_bounds__(256) void k_loop_scan(const int32_t* __restrict__ ctl_i, const double* __restrict__ x,
                                                   const double* __restrict__ e, const uint8_t* __restrict__ valid,
                                                   const int32_t* __restrict__ src, double* __restrict__ lp,
                                                   double* __restrict__ btot, int32_t* __restrict__ bnan, int32_t cap = 0,
                                                   int32_t lp_stride = 0) {
    __shared__ double s_gtot[16];
    __shared__ double s_t[LDS_CHUNK_DOUBLES];  // (k_loop_xe: slot-per-lane in memory, chunk-per-thread for the sums)
    if (blockIdx.y) {  // a batch of trajectories (midas_loop_step_batch): `cap` particles, lp_stride prefix values, a launch's block totals each
        const int64_t b = blockIdx.y, o = b * cap, ob = b * gridDim.x;
        ctl_i += b * LOOP_CTL_I; x += o; e += o; valid += o; src += o; lp += b * lp_stride; btot += ob; bnan += ob;
    }
    const int64_t n2 = ctl_i[LOOP_I_NSET];
    const int raw = ctl_i[LOOP_I_RAW];
    const int blk = blockIdx.x, t = threadIdx.x;
    const int64_t bbase = (int64_t)blk * SCAN_BLOCK;
    if (bbase >= n2) return;
    double v[SCAN_CHUNK];
    int32_t sv[SCAN_CHUNK];
    bool nan = false;
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int64_t i = bbase + (int64_t)k * 256 + t;
        sv[k] = src[i < n2 ? i : n2 - 1];
    }
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const bool in = bbase + (int64_t)k * 256 + t < n2;
        const double num = raw ? x[sv[k]] : e[sv[k]];
        const double m = num * (valid[sv[k]] ? 1.0 : 0.0);
        nan |= in && m != m;
        s_t[lds_chunk_pos(k * 256 + t)] = in ? m : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) v[j] = s_t[17 * t + j];
    const double W = block_scan(v, v, s_gtot);
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) s_t[17 * t + j] = v[j];
    const int f = __syncthreads_or(nan ? 1 : 0);
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int64_t i = bbase + (int64_t)k * 256 + t;
        if (i < n2) lp[i] = s_t[lds_chunk_pos(k * 256 + t)];
    }
    if (t == 0) { btot[blk] = W; bnan[blk] = f; }
}

// The status of the annealed set's CDF from the scan's block results, by a 256-thread workgroup (thread t brings block t's total and
// NaN flag; nb <= LAZY_MAX_BLOCKS blocks are alive, the launch was sized for nb_cap): the block totals added one after the other in
// block order - s_bp[b] = the total in front of block b, s_bp[nb] the CDF's - then 2 for a NaN (any block's flag, or the total), 1
// for a total of zero, else 0.  k_loop_resample resamples by it; k_loop_ndraw tells a caller's stream by it, ahead of the resample,
// whether the reference's resampler draws on this frame.
MD int loop_cdf_status(double bt_t, int bn_t, int nb, int nb_cap, double* __restrict__ s_bp, int* __restrict__ s_flag) {
    const int t = threadIdx.x;
    const int nbl = nb < nb_cap ? nb : nb_cap;  // (more alive than the launch was sized for: flagged elsewhere; stay inside the arrays)
    if (t < nbl) s_bp[t + 1] = bt_t;
    if (t == 0) *s_flag = 0;
    __syncthreads();
    if (t < nbl && bn_t) *s_flag = 1;
    if (t == 0) {
        double acc = 0.0;
        s_bp[0] = 0.0;
        for (int b = 0; b < nb; ++b) { const double w = s_bp[b + 1]; acc = acc + w; s_bp[b + 1] = acc; }
    }
    __syncthreads();
    const double total = s_bp[nb];
    return (*s_flag || total != total) ? 2 : (total == 0.0 ? 1 : 0);
}

// ctl_i[NDRAW] = the uniforms the reference's resampler draws on this frame: n_set, or 0 where it returns its input before drawing
// (all-zero or NaN weights, particle_filter.py:237-241) - from the block results of a k_loop_scan over the annealed set, launched
// with the resample's bound cap2.  One workgroup a trajectory (blockIdx.y), behind the frame's phases up to ANNEAL and in front of
// the caller's counted draw (midas_loop_args.stream_draws).
__global__ __launch_bounds__(256) void k_loop_ndraw(int32_t* __restrict__ ctl_i, const double* __restrict__ btot,
                                                    const int32_t* __restrict__ bnan, int32_t cap2) {
    __shared__ double s_bp[LAZY_MAX_BLOCKS + 1];
    __shared__ int s_flag;
    const int nb_cap = (int)(((int64_t)cap2 + SCAN_BLOCK - 1) / SCAN_BLOCK);
    if (blockIdx.y) {
        const int64_t b = blockIdx.y;
        ctl_i += b * LOOP_CTL_I; btot += b * nb_cap; bnan += b * nb_cap;
    }
    const int t = threadIdx.x;
    const int tb = t < nb_cap ? t : nb_cap - 1;
    const double bt_t = btot[tb];
    const int bn_t = bnan[tb];
    const int64_t n2 = ctl_i[LOOP_I_NSET];
    const int nb = (int)((n2 + SCAN_BLOCK - 1) / SCAN_BLOCK);
    const int status = loop_cdf_status(bt_t, bn_t, nb < LAZY_MAX_BLOCKS ? nb : LAZY_MAX_BLOCKS, nb_cap, s_bp, &s_flag);
    if (t == 0) ctl_i[LOOP_I_NDRAW] = status ? 0 : (int32_t)n2;
}

struct LoopResampleArgs {
    int32_t* ctl_i;
    double* ctl_d;
    const double* lp;
    const double* btot;
    const int32_t* bnan;
    const int32_t* src;
    const float* poses_prop;
    const double* w;
    const int32_t* nn_idx;
    const int32_t* labels;
    float* poses_out;
    double* weights_out;
    int32_t* hint_out;
    int32_t* labels_out;
    int32_t* ridx;
    int32_t mode;
    const double* u;
    float u32;
    uint64_t seed, step;
    double* log;
    const float* cluster_poses;
    const float* cluster_stds;
    int32_t* host_mirror;
    int32_t cap2;  // slots the prefix array holds (the launch's bound of the annealed set)
    // a batch of trajectories (midas_loop_step_batch; blockIdx.y): particles per trajectory in the (B, ...) arrays, prefix values
    // between two trajectories' tables, doubles between their log rows
    int32_t cap = 0, lp_stride = 0;
    int64_t log_stride = 0;
    int32_t check_ndraw = 0;  // midas_loop_args.stream_draws: the frame's status against ctl_i[NDRAW]
};

// n_set draws over cdf_i = (BP_b + lp_i) / total (last slot 1): lower bound (multinomial) / upper bound (systematic) by
// bisection on the exact values; the drawn particle's rows are fetched through src.  All-zero or NaN weights: the annealed
// set goes on unresampled (particle_filter.py:240-241).
// FROM_U: the twin a systematic frame with u32 == MIDAS_U32_FROM_U launches - its offset is the first double of the trajectory's row of
// `u` (midas_math.hpp systematic_draw); every other frame launches the kernel it always did.
template <bool FROM_U>
__global__ __launch_bounds__(256) void k_loop_resample(LoopResampleArgs a) {
#ifdef MIDAS_ANNEAL_CLOCKS  // phase clocks of workgroup 0, thread 0 (anneal_clocks.hpp: RCK)
    const long long ck0 = wall_clock64();
    double* ctl_d = a.ctl_d;
#endif
    __shared__ double s_bp[LAZY_MAX_BLOCKS + 1];
    __shared__ int s_flag;
    // Small sets (softmax weights: the prefix sums do not decrease): the prefix at the end of every 16-slot chunk is staged in LDS
    // by the whole workgroup (one batch of loads), a draw's search walks those and finishes inside ONE chunk - one cache line
    // of the prefix array.  The plain bisection is ~14 dependent trips to the L2 (7 of the kernel's 10.7 us at N ~ 10^4); any
    // search finds the same slot in a non-decreasing sequence (the values compared are the same exact quotients).
    constexpr int RS_CHUNKS = 2048;
    __shared__ double s_ce[RS_CHUNKS];
    if (blockIdx.y) {  // trajectory b draws with the key seed + b, slot keys from 0: the draws of a single engine built with that seed
        const int64_t b = blockIdx.y, o = b * a.cap, ob = b * ((a.cap2 + SCAN_BLOCK - 1) / SCAN_BLOCK);
        a.ctl_i += b * LOOP_CTL_I; a.ctl_d += b * LOOP_CTL_D;
        a.lp += b * a.lp_stride; a.btot += ob; a.bnan += ob;
        a.src += o; a.poses_prop += o * 16; a.w += o; a.nn_idx += o; a.labels += o;
        a.poses_out += o * 16; a.weights_out += o; a.hint_out += o; a.labels_out += o; a.ridx += o;
        a.seed += (uint64_t)b;
        if (a.u) a.u += o;  // (midas_loop_step_batch_draws: (B, cap) host draws)
        if (a.log) a.log += b * a.log_stride;
        a.cluster_poses += b * LOOP_MAX_CLUSTERS * 16; a.cluster_stds += b * LOOP_MAX_CLUSTERS * 3;
        if (a.host_mirror) a.host_mirror += 2 * b;
    }
    const int t = threadIdx.x;
    // Chunk ends, block totals and NaN flags leave before the control block is looked at (it is a trip of its own): by position,
    // bounded by what the launch was sized for - what lies behind the live count is not used.
    // The table's stride is 16 slots while the launch's bound fits the table, else the next power of two that does (64 slots at
    // N = 100k: eleven probes of LDS + six of memory instead of seventeen dependent probes of memory with a division each -
    // 17 us of a 99 us frame).
    constexpr int RS_PRE = RS_CHUNKS / 256;
    int ssh = 4;
    while ((((int64_t)a.cap2 + ((int64_t)1 << ssh) - 1) >> ssh) > RS_CHUNKS) ++ssh;
    const int64_t stride = (int64_t)1 << ssh;
    const int nb_cap = (int)(((int64_t)a.cap2 + SCAN_BLOCK - 1) / SCAN_BLOCK);
    double ce[RS_PRE];
    const bool pre = a.cap2 > 0;
    if (pre) {
#pragma unroll
        for (int k = 0; k < RS_PRE; ++k) {
            const int64_t p = stride * (t + 256 * k) + stride - 1;
            ce[k] = a.lp[p < a.cap2 ? p : a.cap2 - 1];
        }
    }
    const int tb = t < nb_cap ? t : nb_cap - 1;  // (nb_cap <= LAZY_MAX_BLOCKS = 256: one block a thread)
    const double bt_t = a.btot[tb];
    const int bn_t = a.bnan[tb];
    const int64_t n2 = a.ctl_i[LOOP_I_NSET];
    const int64_t i = (int64_t)blockIdx.x * 256 + t;
    // The frame's bookkeeping (status, log row, counters, the host's mirror: ~2 us of one thread, loads and stores one after the
    // other) is done by the LAST workgroup of the launch when that one has no draws of its own - the launches are sized for a
    // third more than the set can hold, so it normally has none - instead of by the first behind its gathers: the kernel was as
    // long as workgroup 0.
    const bool last_idle = (int64_t)(gridDim.x - 1) * 256 >= n2 && gridDim.x > 1;
    const bool book = last_idle ? blockIdx.x == gridDim.x - 1 : blockIdx.x == 0;
    if ((int64_t)blockIdx.x * 256 >= n2 && !book) return;
    RCK(16);
    const int nb = (int)((n2 + SCAN_BLOCK - 1) / SCAN_BLOCK);
    const int64_t nch = (n2 + stride - 1) >> ssh;  // (<= RS_CHUNKS while n2 <= cap2)
    const bool two_level = a.ctl_i[LOOP_I_RAW] == 0 && nch <= RS_CHUNKS && n2 > 0;
    if (two_level) {  // (the chunk that straddles the live count ends at slot n2 - 1)
#pragma unroll
        for (int k = 0; k < RS_PRE; ++k) {
            const int c = t + 256 * k;
            if (c < (int)nch) s_ce[c] = stride * c + stride - 1 < n2 ? ce[k] : a.lp[n2 - 1];
        }
    }
    const int status = loop_cdf_status(bt_t, bn_t, nb, nb_cap, s_bp, &s_flag);
    const double total = s_bp[nb];
    RCK(17);
    if (i < n2) {
        int64_t pick = i;
        if (!status) {
            const bool upper = a.mode == MIDAS_RESAMPLE_SYSTEMATIC;
            double uq;
            if (!upper) {
                uq = a.u ? a.u[i] : philox_uniform53((uint64_t)i, a.seed, a.step);
            } else {
                const float r = systematic_draw<FROM_U>(a.u32, a.u, a.seed, a.step);
                const float off = r / (float)n2;
                uq = (double)i / (double)n2 + (double)off;
                uq = uq >= 1.0 ? uq - 1.0 : uq;
            }
            int64_t lo = 0, hi = n2;
            auto left_exact = [&](int64_t m) {
                const double c = m == n2 - 1 ? 1.0 : (s_bp[m >> 12] + a.lp[m]) / total;
                return upper ? c <= uq : c < uq;
            };
            if (two_level) {
                // the first chunk whose end is not left of the draw, then inside it - probed WITHOUT the division (total > 0 here:
                // bp + v against uq total; a float64 division is ~40 dependent instructions, fifteen probes were 3 of the kernel's
                // 10 us), then the exact predicate on the two neighbours of the boundary, walking where the two disagree: the
                // predicate on the quotients is monotone in the slot, so the result is the bisection's (resample_search.hpp does
                // the same for the large sets)
                const double tt = uq * total;
                auto left_fast = [&](int64_t m, double v_) {
                    if (m >= n2 - 1) return false;
                    const double c = s_bp[m >> 12] + v_;
                    return upper ? c <= tt : c < tt;
                };
                int cl = 0, ch = (int)nch;
                while (ch > cl) {
                    const int cm = cl + ((ch - cl) >> 1);
                    if (left_fast(stride * cm + stride - 1, s_ce[cm])) cl = cm + 1; else ch = cm;
                }
                lo = stride * cl;
                hi = lo + stride < n2 ? lo + stride : n2;
                if (cl >= (int)nch) lo = hi = n2;
                // (inside the chunk: four dependent probes of one cache line; its sixteen values fetched together - eight 16-byte
                // loads a lane, every lane a line of its own - made the kernel 1 us slower)
                while (hi > lo) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (left_fast(mid, a.lp[mid])) lo = mid + 1; else hi = mid;
                }
                while (lo > 0 && !left_exact(lo - 1)) --lo;
                while (lo < n2 && left_exact(lo)) ++lo;
            } else {
                while (hi > lo) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (left_exact(mid)) lo = mid + 1; else hi = mid;
                }
            }
            pick = lo < n2 ? lo : n2 - 1;
        }
        RCK(18);
        a.ridx[i] = (int32_t)pick;
        const int32_t s = a.src[pick];
        const float4* s4 = reinterpret_cast<const float4*>(a.poses_prop + (size_t)s * 16);
        float4* d4 = reinterpret_cast<float4*>(a.poses_out + (size_t)i * 16);
        const float4 r0 = s4[0], r1 = s4[1], r2 = s4[2], r3 = s4[3];
        d4[0] = r0; d4[1] = r1; d4[2] = r2; d4[3] = r3;
        a.weights_out[i] = a.w[s];
        a.hint_out[i] = a.nn_idx[s];
        a.labels_out[i] = a.labels[s];
        RCK(19);
    }
    if (book && t == 0) {
        const int32_t n = a.ctl_i[LOOP_I_N];
        a.ctl_i[LOOP_I_STATUS] = status;
        a.ctl_d[LOOP_D_TOTAL] = total;
        // the caller's stream drew ctl_i[NDRAW] uniforms for this frame: what k_loop_ndraw said must be what happens here
        if (a.check_ndraw && a.ctl_i[LOOP_I_NDRAW] != (status ? 0 : (int32_t)n2)) a.ctl_i[LOOP_I_ERR] |= 256;
        if (a.log) {
            double* L = a.log;
            L[0] = (double)a.ctl_i[LOOP_I_FRAME]; L[1] = (double)n; L[2] = (double)n2;
            L[3] = a.ctl_d[LOOP_D_RMSE_T]; L[4] = a.ctl_d[LOOP_D_RMSE_R];
            L[5] = (double)a.ctl_i[LOOP_I_KEPT]; L[6] = (double)a.ctl_i[LOOP_I_DRIFT]; L[7] = (double)status;
            L[8] = (double)a.ctl_i[LOOP_I_MODE]; L[9] = (double)a.ctl_i[LOOP_I_K];
            const int np = a.ctl_i[LOOP_I_NPRES];
            L[10] = (double)np; L[11] = a.ctl_d[LOOP_D_VAR]; L[12] = a.ctl_d[LOOP_D_S]; L[13] = (double)a.ctl_i[LOOP_I_RAW];
            // (with min_samples = n / 5 a frame has at most five clusters + the noise label; the row holds eight: bit 8 says
            // the centres of a frame with more present labels are truncated here - the engine's own arrays hold them all)
            // L[15] = THIS frame's condition bits: the word is cleared once the row holds it (it used to stay set, and every
            // later row repeated the first overflow)
            L[14] = (double)a.ctl_i[LOOP_I_NCL]; L[15] = (double)(a.ctl_i[LOOP_I_ERR] | (np > 8 ? 8 : 0));
            a.ctl_i[LOOP_I_ERR] = 0;
            for (int c = 0; c < 8 && c < np; ++c) {
                for (int k = 0; k < 16; ++k) L[16 + c * 19 + k] = (double)a.cluster_poses[c * 16 + k];
                for (int k = 0; k < 3; ++k) L[16 + c * 19 + 16 + k] = (double)a.cluster_stds[c * 3 + k];
            }
        }
        a.ctl_i[LOOP_I_FRAME] += 1;
        a.ctl_i[LOOP_I_N] = (int32_t)n2;  // the other workgroups read LOOP_I_NSET only
        if (a.host_mirror) {  // pinned host memory: the count first, then the frame number that says it is there
            __hip_atomic_store(&a.host_mirror[1], (int32_t)n2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&a.host_mirror[0], a.ctl_i[LOOP_I_FRAME], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        ctl_d_count(ctl_d, 22);  // launches
    }
    RCK(20);
}

static void fill_loop_resample(LoopResampleArgs& r, const midas_loop_args& s, const void* lp, const void* bt, const void* bn) {
    r.ctl_i = s.ctl_i_dev; r.ctl_d = s.ctl_d_dev;
    r.lp = (const double*)lp; r.btot = (const double*)bt; r.bnan = (const int32_t*)bn;
    r.src = s.src_dev; r.poses_prop = s.poses_prop_dev; r.w = s.weights_dev; r.nn_idx = s.nn_idx_dev; r.labels = s.labels_dev;
    r.poses_out = s.poses_dev; r.weights_out = s.weights_out_dev; r.hint_out = s.hint_dev; r.labels_out = s.labels_out_dev;
    r.ridx = s.ridx_dev; r.mode = s.resample_mode; r.u = s.u_dev; r.u32 = s.u32; r.seed = s.seed; r.step = s.step;
    r.log = s.log_dev; r.cluster_poses = s.cluster_poses_dev; r.cluster_stds = s.cluster_stds_dev;
    r.host_mirror = s.host_mirror;
}

// the scan of the cap2 slots a trajectory's annealed set may take: its prefix values and block results, in scratch
struct LoopScan { void *lp, *bt, *bn; };
static int loop_scan_launch(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, int64_t cap2, LoopScan& sc) {
    const size_t Bz = (size_t)g.B;
    const unsigned nb2 = (unsigned)ceil_div(cap2, SCAN_BLOCK);
    int rc;
    if ((rc = midas_scratch(ctx, Bz * ((size_t)cap2 + SCAN_CHUNK) * sizeof(double), &sc.lp))) return rc;  // (the resample reads whole chunks)
    if ((rc = midas_scratch(ctx, Bz * nb2 * sizeof(double), &sc.bt))) return rc;
    if ((rc = midas_scratch(ctx, Bz * nb2 * sizeof(int32_t), &sc.bn))) return rc;
    hipLaunchKernelGGL(k_loop_scan, dim3(nb2, g.by()), dim3(256), 0, ctx->stream, (const int32_t*)s.ctl_i_dev, (const double*)s.x_dev,
                       (const double*)s.e_dev, (const uint8_t*)s.valid_dev, (const int32_t*)s.src_dev, (double*)sc.lp, (double*)sc.bt,
                       (int32_t*)sc.bn, g.slice, g.lp_stride);
    return MIDAS_OK;
}

// RESAMPLE over the cap2 slots a trajectory the annealed set may take
int loop_resample_phase(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, int64_t cap2) {
    LoopScan sc;
    if (int rc = loop_scan_launch(ctx, s, g, cap2, sc)) return rc;
    LoopResampleArgs r;
    fill_loop_resample(r, s, sc.lp, sc.bt, sc.bn);  // (a batch's u_dev: NULL, or (B, cap) through midas_loop_step_batch_draws)
    r.cap2 = loop_bound(cap2); r.cap = g.slice; r.lp_stride = g.lp_stride; r.log_stride = g.log_stride;
    r.check_ndraw = s.stream_draws;
    const bool from_u = r.mode == MIDAS_RESAMPLE_SYSTEMATIC && r.u32 == MIDAS_U32_FROM_U;
    if (from_u && !r.u) return midas_set_error(ctx, MIDAS_ERR_INVALID, "u32", "MIDAS_U32_FROM_U without u_dev");
    if (from_u)
        hipLaunchKernelGGL(k_loop_resample<true>, dim3((unsigned)ceil_div(cap2, 256), g.by()), dim3(256), 0, ctx->stream, r);
    else
        hipLaunchKernelGGL(k_loop_resample<false>, dim3((unsigned)ceil_div(cap2, 256), g.by()), dim3(256), 0, ctx->stream, r);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// stream_draws, a call that ends in front of the resample: the resample's scan (the caller's draw in between takes the scratch,
// so the resample scans again) and ctl_i[NDRAW] from its block results.  The two launches may be sized by different bounds cap2
// (the resample-only call of a single engine carries no bound of the live count); block b's total does not depend on cap2 and
// both kernels read the ceil(n_set / SCAN_BLOCK) totals that are alive, so the status is the same.
int loop_ndraw_phase(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, int64_t cap2) {
    LoopScan sc;
    if (int rc = loop_scan_launch(ctx, s, g, cap2, sc)) return rc;
    hipLaunchKernelGGL(k_loop_ndraw, dim3(1, g.by()), dim3(256), 0, ctx->stream, s.ctl_i_dev, (const double*)sc.bt, (const int32_t*)sc.bn,
                       loop_bound(cap2));
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

MIDAS_WARM_TU(loop_resample, k_loop_scan)

}  // namespace midas
