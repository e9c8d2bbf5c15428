// score_f64.hpp - the float64 spec chains on v_mfma_f64_16x16x4_f64, shared by k_score_mfma_f64 (score_f64.hip) and
// k_selfsim_mfma_f64 (selfsim_f64.hip).  The layouts, the probe's chain model and the tree: score_f64.hip's header, DESIGN.md 4.4.
#pragma once
#include "midas_internal.hpp"
#include "midas_math.hpp"

namespace midas {

using f64x4 = __attribute__((ext_vector_type(4))) double;

// element of chain s, k-slot g at step u (-1 past D)
template <bool REG>
MD int sf_elem(int u, int s, int g, int D) {
    if (REG) return 64 * u + 4 * s + g;
    const int d = 64 * u + 16 * g + s;
    return d < D ? d : -1;
}

// 4 x 4 transpose across the four lane groups (rows of 16 lanes): in: v[c] of group g = A[g][c]; out: v[c] of group g = A[c][g]
MD void sf_transpose4(uint32_t (&v)[4]) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {  // groups {0, 1} <-> {2, 3}
        const auto r = __builtin_amdgcn_permlane32_swap(v[c], v[c + 2], false, false);
        v[c] = r[0]; v[c + 2] = r[1];
    }
#pragma unroll
    for (int c = 0; c < 4; c += 2) {  // groups {0, 2} <-> {1, 3}
        const auto r = __builtin_amdgcn_permlane16_swap(v[c], v[c + 1], false, false);
        v[c] = r[0]; v[c + 1] = r[1];
    }
}

// The row pieces of step u, as loaded (zeros past D).  REG: lane group g reads the 16 bytes of chain s = 4 m + g (its four k-slots)
// for m = 0..3 - an instruction reads 16 rows x 64 contiguous bytes; sf_unpack's 4 x 4 transpose across the groups then hands group g
// the k-slot g of chains 4 m + c.  (Sixteen 4-byte gathers at a stride of 16 bytes instead - an instruction touching 16 rows x 16 B,
// the lines re-read by the next fifteen - thrashed the L1.)  Strided: k-slot g of chain s is element 64 u + 16 g + s.
template <typename T, bool REG>
MD void sf_load(T (&w)[16], const T* __restrict__ rp, int u, int g, int D) {
    if constexpr (REG) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const T* p = rp + 64 * u + 16 * m + 4 * g;
            if constexpr (sizeof(T) == 4) {
                const float4 v = *reinterpret_cast<const float4*>(p);
                w[4 * m + 0] = v.x; w[4 * m + 1] = v.y; w[4 * m + 2] = v.z; w[4 * m + 3] = v.w;
            } else {
                const double2 a = reinterpret_cast<const double2*>(p)[0], b = reinterpret_cast<const double2*>(p)[1];
                w[4 * m + 0] = a.x; w[4 * m + 1] = a.y; w[4 * m + 2] = b.x; w[4 * m + 3] = b.y;
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int d = sf_elem<REG>(u, s, g, D);
            w[s] = d >= 0 ? rp[d] : (T)0;
        }
    }
}

// k-slot g of the sixteen chains, widened to float64, from sf_load's pieces (run when the step is consumed, not when it is loaded:
// the transposes wait for the loads)
template <typename T, bool REG>
MD void sf_unpack(double (&x)[16], const T (&w)[16]) {
    if constexpr (!REG) {
#pragma unroll
        for (int s = 0; s < 16; ++s) x[s] = (double)w[s];
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if constexpr (sizeof(T) == 4) {
                uint32_t v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = __float_as_uint((float)w[4 * m + c]);
                sf_transpose4(v);
#pragma unroll
                for (int c = 0; c < 4; ++c) x[4 * m + c] = (double)__uint_as_float(v[c]);
            } else {
                uint32_t lo[4], hi[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint64_t b = (uint64_t)__double_as_longlong((double)w[4 * m + c]);
                    lo[c] = (uint32_t)b; hi[c] = (uint32_t)(b >> 32);
                }
                sf_transpose4(lo);
                sf_transpose4(hi);
#pragma unroll
                for (int c = 0; c < 4; ++c) x[4 * m + c] = double_of(lo[c], hi[c]);
            }
        }
    }
}

// steps of 64 elements (REG: D / 64, even; strided: rounded up to even - the extra step is zeros, exact as the other padding):
// the main loop takes the steps in pairs, one ring slot each
template <bool REG>
__host__ __device__ inline int sf_steps(int D) { const int nu = (D + 63) / 64; return REG ? nu : nu + (nu & 1); }

MD double sf_tree(const f64x4 (&a)[16], int r) {  // quarter_reduce's tree: ((p0 + p8) + (p4 + p12)) + ((p2 + p10) + (p6 + p14)) + ..
    const double q0 = (a[0][r] + a[8][r]) + (a[4][r] + a[12][r]);
    const double q2 = (a[2][r] + a[10][r]) + (a[6][r] + a[14][r]);
    const double q1 = (a[1][r] + a[9][r]) + (a[5][r] + a[13][r]);
    const double q3 = (a[3][r] + a[11][r]) + (a[7][r] + a[15][r]);
    return (q0 + q2) + (q1 + q3);
}

// one MFMA link of chain s: four fmas (probe: k-ordered fma chain).  MIDAS_SF_ONESLOT: one k-slot an instruction, the others
// zero (exact whatever the instruction's internal order; a quarter of the rate) - the form to use on hardware where the probe
// finds no chain.
#ifndef MIDAS_SF_ONESLOT
#define MIDAS_SF_ONESLOT 0
#endif
MD f64x4 sf_link(double e, double x, f64x4 acc) {
#if MIDAS_SF_ONESLOT
    const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(g == c ? e : 0.0, g == c ? x : 0.0, acc, 0, 0, 0);
    return acc;
#else
    return __builtin_amdgcn_mfma_f64_16x16x4f64(e, x, acc, 0, 0, 0);
#endif
}

}  // namespace midas
