// front_folded.hip - the single-trajectory forms of k_frame_front with the resample of the previous frame folded in
// (LAZY 1: workgroup-level tables, LAZY 2: per-wave tables).
#define MIDAS_FRONT_CLOCKS  // this unit's forms take the MIDAS_DEBUG_CLOCKS stamps (see FF_T0, front_wave.hpp)
#include "front_wave.hpp"

namespace midas {

bool launch_front_folded(const FrontLaunch& L, const FrontForm& f) {
    return launch_if_form<1, 4, true, false>(L, f) || launch_if_form<2, 1, true, true>(L, f) || launch_if_form<2, 1, true, false>(L, f) ||
           launch_if_form<2, 4, true, false>(L, f) || launch_if_form<2, 1, true, true, true>(L, f);
}

#if defined(MIDAS_DEBUG_CLOCKS)
int debug_ff_clocks(long long* io8192, int reset) {
    if (reset) {
        static long long zero[16384];
        return hipMemcpyToSymbol(HIP_SYMBOL(g_ff_clk), zero, sizeof(zero)) == hipSuccess ? 0 : 1;
    }
    return hipMemcpyFromSymbol(io8192, HIP_SYMBOL(g_ff_clk), 16384 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
#endif
MIDAS_WARM_TU(front_folded, (k_frame_front<float, 8, 2, 1, true, true>))

}  // namespace midas
