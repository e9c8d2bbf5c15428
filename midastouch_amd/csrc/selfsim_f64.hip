// selfsim_f64.hip - the codebook's self-similarity in float64 on the matrix cores (v_mfma_f64_16x16x4_f64), bit-identical to
// midas_score: panel[r][j] = cos(E[i0 + r], E[j]) for R query rows against all K entries, every value the one midas_score returns
// for code E[i0 + r] (widened to float64) against row j.
//
// Arithmetic (score_f64.hpp): the sixteen spec partial sums, REG layout 64 j + 4 s + c for D in {128, 256, 512,
// 1024} with a 16-byte-aligned codebook (the form midas_score takes for these operands), the strided layout s + 16 t zero-padded
// for any other D; one MFMA is four links of a chain; then the 16-lane butterfly (sf_tree) and tree / (ne_i * norms[j]).  The
// query norm ne_i IS norms[i]: midas_score forms a code's norm with the chain, tree, sqrt and COS_EPS floor that form the
// codebook's row norms (score_body.hpp score_wave / k_score_generic, MODE 0 against MODE 1, same layout), and a widened float32 row
// has the same elements - so zero and degenerate rows come out as midas_score has them.
//
// Both operands are codebook rows, so both go through LDS, in operand order (lane (g, i) of pair p reads one double2: k-slot g of
// chains 2 p, 2 p + 1 of row i - one ds_read_b128 per MFMA pair and operand, no lane transposes):
//   * a workgroup owns QT query tiles of 16 rows, staged once at full D (QT nu 8 KB, nu = ceil(D / 64) steps of 64 elements);
//   * it walks entry groups of EG tiles (blockIdx.x, + gridDim.x, ..), a step at a time: each step's EG x 16 x 64 elements are
//     loaded into registers one step ahead (raw, T as stored), widened into the other of two LDS slots behind the current step's
//     MFMAs, one barrier a step;
//   * QT x EG waves, wave w on query tile w % QT x entry tile w / QT: one 16 x 16 output tile, sixteen f64 accumulator tiles
//     (128 VGPRs: a wave can hold one or two, so the reuse is the LDS's - every staged entry step feeds QT waves, every staged
//     query step all of the block's entry groups).
// Sizes (<= 160 KB of LDS): D <= 128: QT 4, EG 1 (80 KB, two workgroups a CU); D 256: QT 4, EG 1 (144 KB); D 512: QT 2, EG 2;
// D 1024: QT 1, EG 2; up to D 1152: QT 1, EG 1; beyond, the queries are read from memory (two 8-byte gathers per MFMA pair -
// correct, not fast).  MIDAS_SSF_QT=1|2|4 forces a smaller query block where it fits (A/B runs).
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "score_f64.hpp"

#include <cstdlib>

namespace midas {

constexpr size_t SSF_LDS_MAX = 160 * 1024;
constexpr size_t SSF_STEP_BYTES = 16 * 64 * sizeof(double);  // one tile's step, staged

// offset (in doubles) of element o (0 .. 63) of a step of row i inside a staged tile step: chain s, k-slot g, pair s >> 1
template <bool REG>
MD int ssf_lds(int i, int o) {
    const int s = REG ? o >> 2 : o & 15, g = REG ? o & 3 : o >> 4;
    return ((s >> 1) * 64 + g * 16 + i) * 2 + (s & 1);
}

// the four elements d0 .. d0 + 3 of a row, raw (zeros past D).  REG: one 16-byte piece (D % 64 == 0, aligned rows).
template <typename T, bool REG>
MD void ssf_fetch4(T (&w)[4], const T* __restrict__ rp, int d0, int D) {
    if constexpr (REG) {
        if constexpr (sizeof(T) == 4) {
            const float4 v = *reinterpret_cast<const float4*>(rp + d0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
            const double2 a = reinterpret_cast<const double2*>(rp + d0)[0], b = reinterpret_cast<const double2*>(rp + d0)[1];
            w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = d0 + c < D ? rp[d0 + c] : (T)0;
    }
}

// stores four fetched elements (row i of a tile step, elements o .. o + 3), widened exactly; a dead row stores zeros
template <typename T, bool REG>
MD void ssf_put4(double* __restrict__ dst, const T (&w)[4], int i, int o, bool live) {
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[ssf_lds<REG>(i, o + c)] = live ? (double)w[c] : 0.0;
}

// grid (entry-group slots, query blocks); block y holds queries [i0 + 16 QT y, + 16 QT) of the panel [i0, i0 + R).
// LDS: Q_LDS: [QT tiles][nu steps][8 pairs][64 lanes] x double2, then the entry slots [2][EG tiles][8 pairs][64 lanes] x double2.
template <typename T, bool REG, int QT, bool Q_LDS>
__global__ __launch_bounds__(256) void k_selfsim_mfma_f64(const T* __restrict__ emb, const double* __restrict__ norms, int64_t K,
                                                          int D, int64_t i0, int64_t R, int EG, double* __restrict__ out,
                                                          int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) double s_f[];
    constexpr int PER = 4 / QT;  // 4-element pieces a thread stages per step: EG x 16 rows x 16 pieces over 64 QT EG threads
    const int nu = (D + 63) / 64;
    const int tid = (int)threadIdx.x, nthr = 64 * QT * EG, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
    const int qt = wave % QT, et = wave / QT;
    const int64_t qbase = i0 + (int64_t)blockIdx.y * 16 * QT, qend = i0 + R;
    double* s_e = s_f + (Q_LDS ? (size_t)QT * nu * 1024 : 0);
    const int64_t ngroups = (K + 16 * EG - 1) / (16 * EG);
    if ((int64_t)blockIdx.x >= ngroups) return;  // (block-uniform: no barrier behind it is skipped by part of a block)
    const int64_t my_groups = (ngroups - 1 - (int64_t)blockIdx.x) / gridDim.x + 1, stages = my_groups * nu;

    if constexpr (Q_LDS) {  // the block's queries at full D, once
        for (int c = tid; c < QT * 16 * nu * 16; c += nthr) {
            const int row = c / (nu * 16), rem = c - row * nu * 16, u = rem >> 4, o = 4 * (rem & 15);
            const int64_t q = qbase + row;
            T w[4];
            ssf_fetch4<T, REG>(w, emb + (q < qend ? q : i0) * (int64_t)D, 64 * u + o, D);
            ssf_put4<T, REG>(s_f + (size_t)((row >> 4) * nu + u) * 1024, w, row & 15, o, q < qend);
        }
    }
    // stage st = (entry group k of this block, step u): piece c = tid + p nthr is row c >> 4 of the group, elements 4 (c & 15) ..
    T w[PER][4];
    auto fetch = [&](int64_t st) {
        const int64_t k = st / nu, row0 = ((int64_t)blockIdx.x + k * gridDim.x) * 16 * EG;
        const int u = (int)(st - k * nu);
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int c = tid + p * nthr;
            const int64_t j = row0 + (c >> 4);
            ssf_fetch4<T, REG>(w[p], emb + (j < K ? j : K - 1) * (int64_t)D, 64 * u + 4 * (c & 15), D);
        }
    };
    auto put = [&](int64_t st, int slot) {
        const int64_t k = st / nu, row0 = ((int64_t)blockIdx.x + k * gridDim.x) * 16 * EG;
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int c = tid + p * nthr, r = c >> 4;
            ssf_put4<T, REG>(s_e + (size_t)(slot * EG + (r >> 4)) * 1024, w[p], r & 15, 4 * (c & 15), row0 + r < K);
        }
    };
    fetch(0);
    put(0, 0);
    __syncthreads();

    const double2* s_q2 = reinterpret_cast<const double2*>(s_f);
    const double2* s_e2 = reinterpret_cast<const double2*>(s_e);
    const int64_t qa = qbase + 16 * qt;  // the wave's query tile: A rows; the lane's outputs are queries qa + g + 4 r
    double nq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int64_t q = qa + g + 4 * r; nq[r] = norms[q < qend ? q : i0]; }
    const T* qrow = emb + (qa + i < qend ? qa + i : i0) * (int64_t)D;  // (!Q_LDS: the lane's A row)
    int64_t st = 0;
    for (int64_t k = 0; k < my_groups; ++k) {
        f64x4 acc[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int u = 0; u < nu; ++u, ++st) {
            const int64_t nx = st + 1 < stages ? st + 1 : st;  // (the last step re-reads itself: unconditional loads)
            fetch(nx);  // in flight under this step's MFMAs
            const int slot = (int)(st & 1);
            double2 a[8], b[8];
#pragma unroll
            for (int pp = 0; pp < 8; ++pp) {
                if constexpr (Q_LDS) {
                    a[pp] = s_q2[((size_t)(qt * nu + u) * 8 + pp) * 64 + lane];
                } else {
                    const int d0 = sf_elem<REG>(u, 2 * pp, g, D), d1 = sf_elem<REG>(u, 2 * pp + 1, g, D);
                    a[pp].x = d0 >= 0 && qa + i < qend ? (double)qrow[d0] : 0.0;
                    a[pp].y = d1 >= 0 && qa + i < qend ? (double)qrow[d1] : 0.0;
                }
                b[pp] = s_e2[((size_t)(slot * EG + et) * 8 + pp) * 64 + lane];
            }
#pragma unroll
            for (int pp = 0; pp < 8; ++pp) {
                acc[2 * pp] = sf_link(a[pp].x, b[pp].x, acc[2 * pp]);
                acc[2 * pp + 1] = sf_link(a[pp].y, b[pp].y, acc[2 * pp + 1]);
            }
            // the other slot was last read in the previous step (behind its barrier); the widening waits for the loads, so it stays
            // behind this step's MFMAs
            __builtin_amdgcn_sched_barrier(0);
            put(nx, slot ^ 1);
            __syncthreads();
        }
        const int64_t j = ((int64_t)blockIdx.x + k * gridDim.x) * 16 * EG + 16 * et + i;
        if (j < K) {
            const double nr = norms[j];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t q = qa + g + 4 * r;
                if (q < qend) out[(q - i0) * ldo + j] = sf_tree(acc, r) / (nq[r] * nr);
            }
        }
    }
}

struct SsfShape {
    int QT, EG;
    bool q_lds;
    size_t lds;
};

static SsfShape ssf_shape(int D) {
    const size_t tile = (size_t)((D + 63) / 64) * SSF_STEP_BYTES;
    int qt_max = 4;
    if (const char* e = getenv("MIDAS_SSF_QT")) {
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4) qt_max = v;
    }
    for (int QT = qt_max; QT >= 1; QT /= 2)
        for (int EG = 4 / QT; EG >= 1; EG /= 2) {
            const size_t lds = QT * tile + 2 * EG * SSF_STEP_BYTES;
            if (lds <= SSF_LDS_MAX) return {QT, EG, true, lds};
        }
    return {1, 4, false, 2 * 4 * SSF_STEP_BYTES};
}

template <typename T, bool REG, int QT, bool Q_LDS>
static void ssf_launch(midas_ctx* ctx, dim3 grid, const SsfShape& sh, const midas_codebook* cb, int64_t i0, int64_t R, double* out,
                       int64_t ldo) {
    auto kern = k_selfsim_mfma_f64<T, REG, QT, Q_LDS>;
    constexpr int MAXDEV = 64;  // the dynamic-LDS limit, per device (as sf_launch)
    static bool attr_set[MAXDEV] = {};
    const int di = ctx->device >= 0 && ctx->device < MAXDEV ? ctx->device : 0;
    if (!attr_set[di] || ctx->device != di) {
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SSF_LDS_MAX);
        attr_set[di] = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(64 * QT * sh.EG), sh.lds, ctx->stream, (const T*)cb->emb, cb->norms, cb->K, (int)cb->D, i0, R,
                       sh.EG, out, ldo);
}

template <typename T, bool REG>
static void ssf_dispatch(midas_ctx* ctx, dim3 grid, const SsfShape& sh, const midas_codebook* cb, int64_t i0, int64_t R, double* out,
                         int64_t ldo) {
    if (!sh.q_lds) ssf_launch<T, REG, 1, false>(ctx, grid, sh, cb, i0, R, out, ldo);
    else if (sh.QT == 4) ssf_launch<T, REG, 4, true>(ctx, grid, sh, cb, i0, R, out, ldo);
    else if (sh.QT == 2) ssf_launch<T, REG, 2, true>(ctx, grid, sh, cb, i0, R, out, ldo);
    else ssf_launch<T, REG, 1, true>(ctx, grid, sh, cb, i0, R, out, ldo);
}

// rows [i0, i0 + R) of the self-similarity as final float64 cosines: panel[(i - i0) * ldo + j], ldo >= K
int launch_selfsim_panel_f64(midas_ctx* ctx, const midas_codebook* cb, int64_t i0, int64_t R, double* panel, int64_t ldo) {
    const int D = cb->D;
    // the layout midas_score takes for a code that is a codebook row (score.hip dispatch: 16-byte-aligned rows and code - the
    // widened copy of the exact path is a fresh allocation, a float64 row is 16-byte aligned with the codebook)
    const bool reg = (D == 128 || D == 256 || D == 512 || D == 1024) && (uintptr_t)cb->emb % 16 == 0;
    const SsfShape sh = ssf_shape(D);
    constexpr int MAXDEV = 64;
    static int ncu_dev[MAXDEV] = {};
    const int di = ctx->device >= 0 && ctx->device < MAXDEV ? ctx->device : 0;
    if (!ncu_dev[di] || ctx->device != di) {
        hipDeviceProp_t prop;
        ncu_dev[di] = (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    const int ncu = ncu_dev[di];
    const int64_t ngroups = ceil_div(cb->K, (int64_t)16 * sh.EG);
    const int64_t per_cu = std::max<int64_t>(1, (int64_t)(SSF_LDS_MAX / sh.lds));
    const int64_t qrows = (int64_t)16 * sh.QT * 65535;  // grid.y limit: launches of at most 65535 query blocks
    for (int64_t a = 0; a < R; a += qrows) {
        const int64_t Ra = R - a < qrows ? R - a : qrows, gy = ceil_div(Ra, (int64_t)16 * sh.QT);
        // about one round of workgroups over the CUs: each block walks ngroups / gx entry groups against its queries
        const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(ngroups, ceil_div(ncu * per_cu, gy)));
        const dim3 grid((unsigned)gx, (unsigned)gy);
        double* out = panel + a * ldo;
        if (cb->dtype == MIDAS_F32) {
            if (reg) ssf_dispatch<float, true>(ctx, grid, sh, cb, i0 + a, Ra, out, ldo);
            else ssf_dispatch<float, false>(ctx, grid, sh, cb, i0 + a, Ra, out, ldo);
        } else {
            if (reg) ssf_dispatch<double, true>(ctx, grid, sh, cb, i0 + a, Ra, out, ldo);
            else ssf_dispatch<double, false>(ctx, grid, sh, cb, i0 + a, Ra, out, ldo);
        }
        MIDAS_HIP_CHECK(ctx, hipGetLastError());
    }
    return MIDAS_OK;
}

MIDAS_WARM_TU(selfsim_f64, (k_selfsim_mfma_f64<float, true, 4, true>))

}  // namespace midas
