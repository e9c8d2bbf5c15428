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
// (the body is a file of its own, included here and in the twin that takes softmax and unit from the rows' parameter table: the twin then
// shares every statement, and this kernel's token stream - so its code, instruction for instruction - is what it was)
__global__ __launch_bounds__(256) void k_loop_xe(const int32_t* __restrict__ ctl_i, const double* __restrict__ scores,
                                                 const int32_t* __restrict__ nn_idx, const uint8_t* __restrict__ valid,
                                                 int32_t softmax, int32_t unit, double* __restrict__ x_out, double* __restrict__ e_out,
                                                 double* __restrict__ bsum, double* __restrict__ bmax, double* __restrict__ bmin,
                                                 int32_t* __restrict__ bkept, int32_t* __restrict__ bnan, int32_t cap_n, int64_t K,
                                                 double* __restrict__ clk = nullptr) {
#include "loop_xe_body.hpp"
}

// k_loop_xe with the softmax switch and the unit-weight switch of row blockIdx.y's record (midas_loop_step_batch_rows): two scalar
// loads through a uniform address in place of two kernel arguments; both stay workgroup-uniform, so the branches they guard stay scalar.
__global__ __launch_bounds__(256) void k_loop_xe_rows(const int32_t* __restrict__ ctl_i, const double* __restrict__ scores,
                                                      const int32_t* __restrict__ nn_idx, const uint8_t* __restrict__ valid,
                                                      const midas_loop_row_params* __restrict__ rows, double* __restrict__ x_out,
                                                      double* __restrict__ e_out, double* __restrict__ bsum, double* __restrict__ bmax,
                                                      double* __restrict__ bmin, int32_t* __restrict__ bkept, int32_t* __restrict__ bnan,
                                                      int32_t cap_n, int64_t K) {
    const int32_t softmax = rows[blockIdx.y].softmax, unit = rows[blockIdx.y].unit_weights;
    [[maybe_unused]] double* const clk = nullptr;  // (the phase clocks of a profiling build: the single call only)
#include "loop_xe_body.hpp"
}

// S = blocks summed in order; guard; w = (e or x) / S * valid; every particle back onto its codebook pose when all of them
// were pruned (filter.py:176-179); block 0 finalises the control block and the rmse.  (The arithmetic lives in loop_weights.hpp:
// frames whose cluster moments follow in the same call have it at the head of that launch instead, cluster.hip.)
// (Args: LoopWeightsArgs, LoopWeightsRowsArgs - rows on different objects - or LoopWeightsParamRowsArgs - and their own softmax
// switch: loop_weights.hpp)
template <class Args>
__global__ __launch_bounds__(256) void k_loop_weights(Args a) {
    __shared__ double s_sum[LAZY_MAX_BLOCKS];
    __shared__ double s_red[8], s_ab[8];
    __shared__ int s_ired[8];
    if (blockIdx.y || loop_weights_every_row(a)) loop_weights_batch(a, blockIdx.y);  // a batch of trajectories (midas_loop_step_batch)
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
static void fill_loop_weights(LoopWeightsParamRowsArgs& wa, const midas_loop_args& s, const LoopBlockResults& br, int32_t grid_n, unsigned nbcap,
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
                       LoopWeightsParamRowsArgs& wa, const midas_object_set* objects) {
    const unsigned nbcap = g.nbcap();
    LoopBlockResults br;
    if (int rc = carve_block_results(ctx, (size_t)g.B * nbcap, br)) return rc;
    if (g.rows)  // the rows' own softmax and unit-weight switches (midas_loop_step_batch_rows)
        hipLaunchKernelGGL(k_loop_xe_rows, dim3(nbcap, g.by()), dim3(256), 0, ctx->stream, (const int32_t*)s.ctl_i_dev,
                           (const double*)s.scores_dev, (const int32_t*)s.nn_idx_dev, (const uint8_t*)s.valid_dev, g.rows, s.x_dev, s.e_dev,
                           br.bsum, br.bmax, br.bmin, br.bkept, br.bnan, loop_bound(g.cap), K);
    else
        hipLaunchKernelGGL(k_loop_xe, dim3(nbcap, g.by()), dim3(256), 0, ctx->stream, (const int32_t*)s.ctl_i_dev, (const double*)s.scores_dev,
                           (const int32_t*)s.nn_idx_dev, (const uint8_t*)s.valid_dev, s.softmax, s.unit_weights, s.x_dev, s.e_dev, br.bsum, br.bmax,
                           br.bmin, br.bkept, br.bnan, loop_bound(g.cap), K, g.clocks);
    fill_loop_weights(wa, s, br, loop_bound(g.cap), nbcap, rmse);
    wa.cb_poses_rows = nullptr;
    wa.rows = g.rows;
    if (objects) {  // (row 0 takes `cb_poses` as it stands: the kernels look at the table for blockIdx.y != 0 only)
        wa.cb_poses = objects->cb_poses_row0;
        wa.cb_poses_rows = objects->cb_poses_rows;
    }
    if (!merged && wa.rows) hipLaunchKernelGGL(k_loop_weights<LoopWeightsParamRowsArgs>, dim3(nbcap, g.by()), dim3(256), 0, ctx->stream, wa);
    else if (!merged && objects) hipLaunchKernelGGL(k_loop_weights<LoopWeightsRowsArgs>, dim3(nbcap, g.by()), dim3(256), 0, ctx->stream, static_cast<const LoopWeightsRowsArgs&>(wa));
    else if (!merged) hipLaunchKernelGGL(k_loop_weights<LoopWeightsArgs>, dim3(nbcap, g.by()), dim3(256), 0, ctx->stream, static_cast<const LoopWeightsArgs&>(wa));
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

MIDAS_WARM_TU(loop_weights, k_loop_xe)

}  // namespace midas
