// loop_weights.hip - FRONT, second half, of a loop frame (loop.hip): the scores the front left per codebook entry become the
// particles' weights.  k_loop_xe (scores gathered, softmax numerators, per-block sums in the spec order) -> k_loop_weights (S, isclose
// guard, masked weights, drift re-projection, rmse: loop_weights.hpp - in frames without DBSCAN that work sits at the head of the
// cluster-moment launch instead, k_loop_weights_moments in cluster.hip), then loop_weights_phase, which launches them.
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "tail_block.hpp"
#include "loop_weights.hpp"
#include "anneal_clocks.hpp"

namespace midas {

// x = scores[nn], e = exp(x - 1) (or x when the softmax is off); per 4096-slot block the sum of e in the spec order,
// the extrema of x, the particles the prune kept, NaN among the scores.
// (round 6) The block's slots are read and written slot-per-lane - a wave's load is 64 consecutive indices, its stores 64
// consecutive values - and the numerators reach the chunk-per-thread layout the summation spec is written in through LDS
// (lds_chunk_pos, tail_block.hpp).  With sixteen CONSECUTIVE slots per thread every lane of
// every load and store was a cache line of its own: 64 look-ups an instruction, ~80 instructions a wave - the launch's bound.
__global__ __launch_bounds__(256) void k_loop_xe(const int32_t* __restrict__ ctl_i, const double* __restrict__ scores,
                                                 const int32_t* __restrict__ nn_idx, const uint8_t* __restrict__ valid,
                                                 int32_t softmax, int32_t unit, double* __restrict__ x_out, double* __restrict__ e_out,
                                                 double* __restrict__ bsum, double* __restrict__ bmax, double* __restrict__ bmin,
                                                 int32_t* __restrict__ bkept, int32_t* __restrict__ bnan, int32_t cap_n, int64_t K,
                                                 double* __restrict__ clk = nullptr) {
#ifdef MIDAS_ANNEAL_CLOCKS  // phase clocks of workgroup 0, thread 0 (anneal_clocks.hpp: XCK)
    const long long xck0 = wall_clock64();
#endif
    __shared__ double s_gtot[16];
    __shared__ double s_mx[4], s_mn[4];
    __shared__ int s_k[4], s_f[4];
    __shared__ double s_t[LDS_CHUNK_DOUBLES];
    if (blockIdx.y) {  // a batch of trajectories (midas_loop_step_batch): cap_n slots, K scores and a launch's block results per trajectory
        const int64_t b = blockIdx.y, o = b * cap_n, ob = b * gridDim.x;
        ctl_i += b * LOOP_CTL_I; scores += b * K; nn_idx += o; valid += o; x_out += o; e_out += o;
        bsum += ob; bmax += ob; bmin += ob; bkept += ob; bnan += ob;
    }
    const int blk = blockIdx.x, t = threadIdx.x;
    const int64_t bbase = (int64_t)blk * SCAN_BLOCK;
    // batched, unconditional loads on clamped indices (a branch around a load makes hipcc wait for each one in turn); clamped to
    // what the launch was sized for, not to the live count - the control block is a trip of its own, the indices and the scores
    // travel beside it (a slot behind the live count holds anything: its row number is clamped too, its values are masked)
    double v[SCAN_CHUNK];
    int32_t nn[SCAN_CHUNK];
    unsigned okbits = 0;
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int64_t i = bbase + (int64_t)k * 256 + t, ic = i < cap_n ? i : cap_n - 1;
        const int32_t r = nn_idx[ic];
        nn[k] = r < 0 ? 0 : ((int64_t)r >= K ? (int32_t)(K - 1) : r);
        okbits |= valid[ic] != 0 ? (1u << k) : 0u;
    }
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) v[k] = unit ? 1.0 : scores[nn[k]];
    const int64_t n = ctl_i[LOOP_I_N];
    if (bbase >= n) return;
    double mx = -INFINITY, mn = INFINITY;
    XCK(36);
    int kept = 0;
    bool nan = false;
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int64_t i = bbase + (int64_t)k * 256 + t;
        const bool in = i < n;
        const double xv = v[k];
        mx = in && xv > mx ? xv : mx;
        mn = in && xv < mn ? xv : mn;
        kept += in && ((okbits >> k) & 1u) ? 1 : 0;
        nan |= in && xv != xv;
        if (in) x_out[i] = xv;
    }
    XCK(37);  // scores there
    if (softmax) {
#pragma unroll
        for (int k = 0; k < SCAN_CHUNK; ++k) {
            v[k] = exp_spec(v[k] - 1.0);
            // four exponentials interleaved: each is a dependent chain of ~25 fma at ~20 cycles a step, and the workgroup's four
            // waves are alone on their SIMDs
            if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int il = k * 256 + t;
        const bool in = bbase + il < n;
        if (in) e_out[bbase + il] = v[k];
        s_t[lds_chunk_pos(il)] = in ? v[k] : 0.0;
    }
    XCK(38);  // exponentials done, values stored
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) v[j] = s_t[17 * t + j];  // the own chunk: slots 16 t .. 16 t + 15 of the block
    const double W = block_total(v, s_gtot);
    XCK(39);  // block total
    mx = wave_max_dpp(mx);  // (register moves; NaN never wins, as in the shuffle form - flagged beside)
    mn = wave_min_dpp(mn);
    kept = wave_isum_dpp(kept);
    const bool wnan = __any(nan);
    if ((t & 63) == 0) { s_mx[t >> 6] = mx; s_mn[t >> 6] = mn; s_k[t >> 6] = kept; s_f[t >> 6] = wnan ? 1 : 0; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w) {
            mx = s_mx[w] > mx ? s_mx[w] : mx;
            mn = s_mn[w] < mn ? s_mn[w] : mn;
            kept += s_k[w];
        }
        const int f = s_f[0] | s_f[1] | s_f[2] | s_f[3];
        bsum[blk] = W;
        bmax[blk] = f ? NAN : mx;  // NaN propagates, as torch.max / torch.min do
        bmin[blk] = f ? NAN : mn;
        bkept[blk] = kept;
        bnan[blk] = f;
    }
    XCK(40);
    XCK_COUNT(41);
}

// S = blocks summed in order; guard; w = (e or x) / S * valid; every particle back onto its codebook pose when all of them
// were pruned (filter.py:176-179); block 0 finalises the control block and the rmse.  (The arithmetic lives in loop_weights.hpp:
// frames whose cluster moments follow in the same call have it at the head of that launch instead, cluster.hip.)
// (Args: LoopWeightsArgs, or LoopWeightsRowsArgs - rows on different objects, loop_weights.hpp)
template <class Args>
__global__ __launch_bounds__(256) void k_loop_weights(Args a) {
    __shared__ double s_sum[LAZY_MAX_BLOCKS];
    __shared__ double s_red[8], s_ab[8];
    __shared__ int s_ired[8];
    if (blockIdx.y) loop_weights_batch(a, blockIdx.y);  // a batch of trajectories (midas_loop_step_batch)
    const int blk = blockIdx.x, t = threadIdx.x;
    const int64_t bbase = (int64_t)blk * SCAN_BLOCK;
    // Everything this workgroup reads leaves before the live count is looked at (the control block is a trip of its own): the block
    // results of every LAUNCHED block (the ones behind the live count hold stale values and are masked), and the slots'
    // numerators / masks on indices bounded by the launches' cap.
    const LoopWeightsPre pre = loop_weights_prefetch(a, blk == 0);
    double pe[SCAN_CHUNK], px[SCAN_CHUNK];
    uint8_t pv[SCAN_CHUNK];
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = bbase + (int64_t)j * 256 + t, ic = i < a.grid_n ? i : a.grid_n - 1;
        pe[j] = a.e[ic]; px[j] = a.x[ic]; pv[j] = a.valid[ic];
    }
    const int64_t n = a.ctl_i[LOOP_I_N];
    if (bbase >= n && blk != 0) return;
    const LoopWeightsHead h = loop_weights_head(a, pre, n, s_sum, s_red, s_ired);
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = bbase + (int64_t)j * 256 + t;
        if (i < n) {
            loop_weight_store(a, h, i, pe[j], px[j], pv[j]);
            if (h.drifted) {
                const float4* s4 = reinterpret_cast<const float4*>(a.cb_poses + (size_t)a.nn_idx[i] * 16);
                float4* d4 = reinterpret_cast<float4*>(a.poses_prop + (size_t)i * 16);
                d4[0] = s4[0]; d4[1] = s4[1]; d4[2] = s4[2]; d4[3] = s4[3];
            }
        }
    }
    if (blk != 0) return;
    loop_weights_finalise(a, h, pre, s_ab);
}

struct LoopBlockResults { double *bsum, *bmax, *bmin; int32_t *bkept, *bnan; };  // of k_loop_xe, `count` blocks
static int carve_block_results(midas_ctx* ctx, size_t count, LoopBlockResults& br) {
    void* p;
    if (int rc = midas_scratch(ctx, count * (3 * sizeof(double) + 2 * sizeof(int32_t)), &p)) return rc;
    br.bsum = (double*)p;
    br.bmax = br.bsum + count; br.bmin = br.bmax + count;
    br.bkept = (int32_t*)(br.bmin + count);
    br.bnan = br.bkept + count;
    return MIDAS_OK;
}
static void fill_loop_weights(LoopWeightsRowsArgs& wa, const midas_loop_args& s, const LoopBlockResults& br, int32_t grid_n, unsigned nbcap,
                              bool rmse) {
    wa.ctl_i = s.ctl_i_dev; wa.ctl_d = s.ctl_d_dev; wa.grid_n = grid_n; wa.nbl = (int32_t)nbcap;
    wa.bsum = br.bsum; wa.bmax = br.bmax; wa.bmin = br.bmin; wa.bkept = br.bkept; wa.bnan = br.bnan;
    wa.x = (const double*)s.x_dev; wa.e = (const double*)s.e_dev; wa.valid = (const uint8_t*)s.valid_dev;
    wa.nn_idx = (const int32_t*)s.nn_idx_dev; wa.cb_poses = s.cb_poses_dev; wa.poses_prop = s.poses_prop_dev;
    wa.w_out = s.weights_dev; wa.src = s.src_dev; wa.part_rmse = (const double*)(rmse ? s.part_rmse_dev : nullptr);
    wa.softmax = s.softmax;
}

// The weights may run at the head of the cluster-moment launch when that launch follows in this call with nothing in between
// (DBSCAN reads the re-projected poses: frames that cluster keep the launch of their own).
bool loop_weights_mergeable(int32_t phases) { return (phases & MIDAS_LOOP_ANNEAL) && !(phases & MIDAS_LOOP_DBSCAN); }

// behind the front: k_loop_xe, then the weights - launched here, or (merged) left in `wa` for the cluster-moment launch
int loop_weights_phase(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, int64_t K, bool rmse, bool merged,
                       LoopWeightsRowsArgs& wa, const midas_object_set* objects) {
    const unsigned nbcap = g.nbcap();
    LoopBlockResults br;
    if (int rc = carve_block_results(ctx, (size_t)g.B * nbcap, br)) return rc;
    hipLaunchKernelGGL(k_loop_xe, dim3(nbcap, g.by()), dim3(256), 0, ctx->stream, (const int32_t*)s.ctl_i_dev, (const double*)s.scores_dev,
                       (const int32_t*)s.nn_idx_dev, (const uint8_t*)s.valid_dev, s.softmax, s.unit_weights, s.x_dev, s.e_dev, br.bsum, br.bmax,
                       br.bmin, br.bkept, br.bnan, loop_bound(g.cap), K, g.clocks);
    fill_loop_weights(wa, s, br, loop_bound(g.cap), nbcap, rmse);
    wa.cb_poses_rows = nullptr;
    if (objects) {  // (row 0 takes `cb_poses` as it stands: the kernels look at the table for blockIdx.y != 0 only)
        wa.cb_poses = objects->cb_poses_row0;
        wa.cb_poses_rows = objects->cb_poses_rows;
    }
    if (!merged && objects) hipLaunchKernelGGL(k_loop_weights<LoopWeightsRowsArgs>, dim3(nbcap, g.by()), dim3(256), 0, ctx->stream, wa);
    else if (!merged) hipLaunchKernelGGL(k_loop_weights<LoopWeightsArgs>, dim3(nbcap, g.by()), dim3(256), 0, ctx->stream, static_cast<const LoopWeightsArgs&>(wa));
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

MIDAS_WARM_TU(loop_weights, k_loop_xe)

}  // namespace midas
