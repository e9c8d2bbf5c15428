// tail_sums.hpp - what the weight operators (resample.hip), the step tail (tail.hip) and the sharded exchange
// (shard_route.hip) share: wave reductions, the extrema of an array of partials, the block limit of the LDS tables.
#pragma once
#include "midas_internal.hpp"
#include "midas_math.hpp"

namespace midas {

constexpr int TB_MAX_BLOCKS = 1024;  // 4 M particles (per GPU in the fused step, in total in the sharded step)

MD double wmax(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { double t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}
MD double wmin(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { double t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}

// The isclose guard of the softmax (particle_filter.py:459-468) over a workgroup's extrema, in two halves with the caller's
// barrier between them.  s_ex: three rows of LDS, STRIDE doubles apart (max, min, "a NaN was seen"), one entry a wave.
// publish: every thread's own max / min / NaN flag -> its wave's entries
template <int STRIDE>
MD void guard_publish(double mx, double mn, bool nan, double* s_ex) {
    mx = wmax(mx);
    mn = wmin(mn);
    const bool wn = __any(nan);
    const int t = threadIdx.x;
    if ((t & 63) == 0) { s_ex[t >> 6] = mx; s_ex[STRIDE + (t >> 6)] = mn; s_ex[2 * STRIDE + (t >> 6)] = wn ? 1.0 : 0.0; }
}
// collect: the four waves' entries in order (NaN propagates, as torch.max / torch.min do).  The decision itself,
// fabs(mx - mn) <= ISCLOSE_ATOL (false on NaN), stays spelled out at the callers: behind a function of its own k_tail_a2 and
// k_tail_b2 compile to other instructions.
struct GuardExtrema { double mx, mn; };
template <int STRIDE>
MD GuardExtrema guard_collect(const double* s_ex) {
    double mx = s_ex[0], mn = s_ex[STRIDE], f = s_ex[2 * STRIDE];
    for (int w = 1; w < 4; ++w) { mx = s_ex[w] > mx ? s_ex[w] : mx; mn = s_ex[STRIDE + w] < mn ? s_ex[STRIDE + w] : mn; f += s_ex[2 * STRIDE + w]; }
    if (f != 0.0) { mx = NAN; mn = NAN; }
    return {mx, mn};
}

}  // namespace midas
