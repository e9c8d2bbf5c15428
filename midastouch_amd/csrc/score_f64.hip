// score_f64.hip - batched float64 cosine scoring on the matrix cores (v_mfma_f64_16x16x4_f64), bit-identical to midas_score.
//
// scores[b K + k] = tree(pd) / (ne_b * norms[k]) for B codes in one pass over the codebook, where pd are the 16 partial sums of
// <code_b, C_k> of the summation spec (oracle/midas_oracle.c MO_SCORE_BODY, score_body.hpp): partial s is a sequential fma chain,
// starting at +0.0, over the elements
//   REG layout (D in {128, 256, 512, 1024}, the 16-byte-aligned operands of k_score_reg):  64 j + 4 s + c   for j, then c = 0..3
//   strided layout (any other D, or the fallback of k_score_generic):                       s + 16 t        for t = 0, 1, ..
// and the tree is the 16-lane xor butterfly (8, 4, 2, 1) of quarter_reduce.
//
// v_mfma_f64_16x16x4_f64 performs, per output element, fma(a3,b3, fma(a2,b2, fma(a1,b1, fma(a0,b0, acc)))) - four correctly
// rounded fmas in k order (tools/probes/mfma_f64_probe.hip) - so one instruction is four links of one chain:
// sixteen accumulator tiles, tile s = partial s, step u feeds tile s the k-slots c = 0..3 of
//   REG: elements 64 u + 4 s + c (chain index t = 4 u + c)       strided: elements s + 16 (4 u + c) = 64 u + 16 c + s, zero past D
// (the zero padding is exact: a chain starting at +0.0 is never -0.0, and fma(0, 0, acc) = acc).  Tile s and tile s ^ 8 hold a
// given output in the same lane and register, so the tree is register adds.
//
// Operands: A = codes (M = 16 codes), B = codebook rows (N = 16 rows); lane (g = l >> 4, i = l & 15) supplies k-slot g of code i
// and of row i.  D[code g + 4 r][row i] comes back in register r of lane (g, i) (the f64 form's own C/D map): a store of register
// r covers 16 consecutive rows of four codes.
//
// Codes stay float64 (64 codes x D 512 x 8 B = 256 KB: more than the CU's 160 KB of LDS).  A workgroup (four waves, one a SIMD)
// stages a BLOCK of up to four code tiles of 16 - as many as fit 128 KB (D 512: 32 codes, D 1024: 16, D <= 256: 64) - in LDS in the
// order the operand reads take them (one conflict-free ds_read_b128 per two tiles and step), sixteen 8-byte loads a thread in flight,
// and forms the block's code norms from the staged copy in the spec order.  D > 1024 (one tile over 128 KB): the operands are
// read from memory instead, two 8-byte gathers per MFMA pair - correct, not fast.  The code blocks are grid.y; a unit of work is
// (16 rows, one code tile), dealt round-robin over all waves of the block's workgroups (balanced to one unit); a wave re-reads its
// rows for every code tile (from the L2: its neighbour in the deal is the same rows' next tile).
// In the wave: the sixteen double4 tiles are the MFMAs' C/D in place (VGPR form, Makefile: the default AGPR form copied every tile
// through one AGPR tile around its MFMA), carried by a plain loop over a unit's steps taken in pairs; the row pieces travel in a
// two-slot ring, raw as loaded (the REG transposes run when a step is consumed), refilled as soon as a slot is read - across unit
// boundaries - and a scheduling barrier keeps a step's unpacking behind the previous step's MFMAs.  Float32 rows are widened exactly
// in registers.  K 50k x D 512 x B 64: 109.6 us, the matrix pipe busy 38 % of the time.
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "score_body.hpp"
#include "score_f64.hpp"

namespace midas {

constexpr int SF_WAVES = 4;                  // one a SIMD: 512 registers for 16 accumulator tiles + the ring
constexpr int SF_MAX_CT = 4;                   // code tiles of 16 per block
constexpr size_t SF_LDS_CODES = 128 * 1024;    // the staged block (the norms behind it)

// grid (gx, code blocks); block y holds codes [16 CT y, + 16 CT).  LDS: [CT tiles][nu steps][8 tile pairs][64 lanes] x double2
// (code 16 t + i, k-slot g of chains 2 p, 2 p + 1 at step u in lane (g, i)), then 16 CT code norms.
template <typename T, bool REG, bool CODES_LDS>
__global__ __launch_bounds__(64 * SF_WAVES) void k_score_mfma_f64(const T* __restrict__ emb, const double* __restrict__ norms,
                                                                  const double* __restrict__ codes, double* __restrict__ out,
                                                                  int64_t K, int D, int B, int CT) {
    extern __shared__ __attribute__((aligned(16))) double s_f[];
    const int nu = sf_steps<REG>(D);
    const int nc = 16 * CT;                       // codes of a block
    const int b0 = (int)blockIdx.y * nc;
    const int nb = B - b0 < nc ? B - b0 : nc;     // real codes of this block
    double* s_ne = s_f + (CODES_LDS ? (size_t)CT * nu * 1024 : 0);
    const int tid = (int)threadIdx.x, lane = tid & 63, g = lane >> 4, i = lane & 15;
    if constexpr (CODES_LDS) {
        // sixteen 8-byte loads a thread in flight per round, then their LDS stores
        const int Dp = 64 * nu, total = nc * Dp;
        for (int base = 0; base < total; base += 16 * 64 * SF_WAVES) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int e = base + k * 64 * SF_WAVES + tid, c = e / Dp, d = e - c * Dp;
                v[k] = (e < total && c < nb && d < D) ? codes[(int64_t)(b0 + c) * D + d] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int e = base + k * 64 * SF_WAVES + tid, c = e / Dp, d = e - c * Dp;
                const int u = d >> 6, r = d & 63;
                const int s = REG ? r >> 2 : r & 15, gs = REG ? r & 3 : r >> 4;
                if (e < total) s_f[(((size_t)((c >> 4) * nu + u) * 8 + (s >> 1)) * 64 + gs * 16 + (c & 15)) * 2 + (s & 1)] = v[k];
            }
        }
        __syncthreads();
    }
    // code norms: a quarter-wave per code, lane s over its chain (score_wave / k_score_generic's ne2) - from the staged copy when
    // there is one - then the 16-lane tree
    for (int c0 = 0; c0 < nc; c0 += 4 * SF_WAVES) {  // (wave-uniform trip count: the tree's moves need the whole row of lanes)
        const int c = c0 + (tid >> 4), s = tid & 15;
        const bool real = c < nb;
        const double* cp = codes + (int64_t)(b0 + (real ? c : 0)) * D;
        double ne2 = 0.0;
        const int nt = REG ? D / 16 : (D + 15) / 16;
#pragma unroll 8
        for (int t = 0; t < nt; ++t) {
            const int d = REG ? 64 * (t >> 2) + 4 * s + (t & 3) : s + 16 * t;
            if (d < D) {
                double v;
                if constexpr (CODES_LDS) {  // element d of code c: step d >> 6, chain sc, k-slot gs (as staged above)
                    const int r = d & 63, sc = REG ? r >> 2 : r & 15, gs = REG ? r & 3 : r >> 4;
                    v = real ? s_f[(((size_t)((c >> 4) * nu + (d >> 6)) * 8 + (sc >> 1)) * 64 + gs * 16 + (c & 15)) * 2 + (sc & 1)] : 0.0;
                } else {
                    v = cp[d];
                }
                ne2 = fma_(v, v, ne2);
            }
        }
        ne2 = quarter_reduce(ne2);
        if (c < nc && s == 0) {
            double ne = __builtin_sqrt(ne2);
            ne = ne < COS_EPS ? COS_EPS : ne;
            s_ne[c] = real ? ne : 1.0;
        }
    }
    __syncthreads();

    const int G = (int)((K + 15) / 16);            // (the launch checks units x nu < 2^31)
    const int ct_real = (nb + 15) / 16;           // code tiles of this block with a code in them
    const int units = G * ct_real;
    const int nw = (int)gridDim.x * SF_WAVES, q0 = (int)blockIdx.x * SF_WAVES + (tid >> 6);
    if (q0 >= units) return;  // (no barrier behind this point)
    const double2* s_c2 = reinterpret_cast<const double2*>(s_f);
    // Row pieces SF_PF steps ahead of the multiplies, raw as loaded, in a shift register ring; the fetch cursor (qf, uf) runs
    // through the wave's units (q0, q0 + nw, ..) in step order, so a unit's first pieces leave during the previous unit's last
    // steps.  The accumulators are carried by a plain loop over the unit's steps (zeroed in front of it, read behind it): MFMA C/D
    // in place, no copies between register files.
    int qf = q0, uf = 0;
    auto fetch = [&](T (&w)[16]) {
        const int q = qf < units ? qf : q0;  // (past the last unit: re-read the first one, nobody uses it)
        const int64_t row0 = (int64_t)(q / ct_real) * 16, row = row0 + i < K ? row0 + i : K - 1;  // (surplus rows: dropped)
        sf_load<T, REG>(w, emb + row * (int64_t)D, uf, g, D);
        if (++uf == nu) { uf = 0; qf += nw; }
    };
    T ring[2][16];
    fetch(ring[0]);
    fetch(ring[1]);
    for (int q = q0; q < units; q += nw) {
        const int64_t row0 = (int64_t)(q / ct_real) * 16;
        const int ct = q % ct_real;
        const double nr = norms[row0 + i < K ? row0 + i : K - 1];  // (needed behind the unit's steps)
        f64x4 acc[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int u0 = 0; u0 < nu; u0 += 2) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {  // step u0 + p from ring slot p, which then takes the pieces of two steps on
                const int u = u0 + p;
                double2 e[8];
#pragma unroll
                for (int pp = 0; pp < 8; ++pp) {
                    if constexpr (CODES_LDS) {
                        e[pp] = s_c2[((size_t)(ct * nu + u) * 8 + pp) * 64 + lane];
                    } else {  // (D > 1024: two 8-byte gathers from memory per MFMA pair - correct, not fast)
                        const int b = 16 * ct + i;
                        const double* cp = codes + (int64_t)(b0 + (b < nb ? b : 0)) * D;
                        const int d0 = sf_elem<REG>(u, 2 * pp, g, D), d1 = sf_elem<REG>(u, 2 * pp + 1, g, D);
                        e[pp].x = (b < nb && d0 >= 0) ? cp[d0] : 0.0;
                        e[pp].y = (b < nb && d1 >= 0) ? cp[d1] : 0.0;
                    }
                }
                double x[16];
                sf_unpack<T, REG>(x, ring[p]);
                fetch(ring[p]);
#pragma unroll
                for (int pp = 0; pp < 8; ++pp) {
                    acc[2 * pp] = sf_link(e[pp].x, x[2 * pp], acc[2 * pp]);
                    acc[2 * pp + 1] = sf_link(e[pp].y, x[2 * pp + 1], acc[2 * pp + 1]);
                }
                // (the next step's transposes stay behind this step's MFMAs: hoisted, they wait for pieces still in flight)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (row0 + i < K) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * ct + g + 4 * r;
                if (c < nb) out[(int64_t)(b0 + c) * K + row0 + i] = sf_tree(acc, r) / (s_ne[c] * nr);
            }
        }
    }
}

template <typename T, bool REG, bool CODES_LDS>
static void sf_attr(midas_ctx* ctx) {
    (void)hipFuncSetAttribute((const void*)k_score_mfma_f64<T, REG, CODES_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
}

template <typename T>
static int sf_launch(midas_ctx* ctx, const midas_codebook* cb, int32_t B, const double* codes, double* scores, bool reg) {
    const int D = cb->D, nu = reg ? sf_steps<true>(D) : sf_steps<false>(D);
    const size_t tile_bytes = (size_t)nu * 1024 * sizeof(double);  // one code tile, staged
    const bool codes_lds = tile_bytes <= SF_LDS_CODES;
    int CT = codes_lds ? (int)(SF_LDS_CODES / tile_bytes) : 1;
    CT = CT > SF_MAX_CT ? SF_MAX_CT : CT;
    const int need = (int)ceil_div(B, 16);
    CT = CT > need ? need : CT;
    const int nblk = (int)ceil_div(B, 16 * CT);
    const size_t lds = (codes_lds ? (size_t)CT * tile_bytes : 0) + (size_t)16 * CT * sizeof(double);
    // the dynamic-LDS limit, per device (as launch_score_batch)
    constexpr int MAXDEV = 64;
    static bool attr_set[MAXDEV] = {};
    static int ncu_dev[MAXDEV] = {};
    const int di = ctx->device >= 0 && ctx->device < MAXDEV ? ctx->device : 0;
    if (!attr_set[di] || ctx->device != di) {
        sf_attr<T, true, true>(ctx); sf_attr<T, false, true>(ctx); sf_attr<T, true, false>(ctx); sf_attr<T, false, false>(ctx);
        hipDeviceProp_t prop;
        ncu_dev[di] = (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
        attr_set[di] = true;
    }
    // one workgroup a CU over all code blocks (a 128 KB block leaves room for one), fewer when there are fewer units than waves
    const int64_t units = ceil_div(cb->K, 16) * CT;
    if (units * nu >= (int64_t)1 << 31)
        return midas_set_error(ctx, MIDAS_ERR_INVALID, "midas_score_batch_f64", "ceil(K / 16) x code tiles x ceil(D / 64) >= 2^31");
    const int64_t want = ceil_div(ncu_dev[di], nblk);
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, ceil_div(units, SF_WAVES)));
    const dim3 grid(gx, (unsigned)nblk), block(64 * SF_WAVES);
    const T* emb = (const T*)cb->emb;
    if (reg && codes_lds)
        hipLaunchKernelGGL((k_score_mfma_f64<T, true, true>), grid, block, lds, ctx->stream, emb, cb->norms, codes, scores, cb->K, D, B, CT);
    else if (codes_lds)
        hipLaunchKernelGGL((k_score_mfma_f64<T, false, true>), grid, block, lds, ctx->stream, emb, cb->norms, codes, scores, cb->K, D, B, CT);
    else if (reg)
        hipLaunchKernelGGL((k_score_mfma_f64<T, true, false>), grid, block, lds, ctx->stream, emb, cb->norms, codes, scores, cb->K, D, B, CT);
    else
        hipLaunchKernelGGL((k_score_mfma_f64<T, false, false>), grid, block, lds, ctx->stream, emb, cb->norms, codes, scores, cb->K, D, B, CT);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_score_batch_f64(midas_ctx* ctx, const midas_codebook* cb, int32_t B, const double* codes, double* scores) {
    if (B < 1) return midas_set_error(ctx, MIDAS_ERR_INVALID, "midas_score_batch_f64", "B >= 1");
    // the layout midas_score takes for these operands (score.hip dispatch: the register form needs 16-byte-aligned rows and code)
    const int D = cb->D;
    const bool reg = (D == 128 || D == 256 || D == 512 || D == 1024) && (uintptr_t)cb->emb % 16 == 0 && (uintptr_t)codes % 16 == 0;
    if (cb->dtype == MIDAS_F32) return sf_launch<float>(ctx, cb, B, codes, scores, reg);
    return sf_launch<double>(ctx, cb, B, codes, scores, reg);
}

// the dense batch pass of midas_filter_step_batch at the codebook's batch precision
int launch_score_dense_batch(midas_ctx* ctx, const midas_codebook* cb, int32_t B, const double* codes, double* scores) {
    return cb->batch_precision == MIDAS_F64 ? launch_score_batch_f64(ctx, cb, B, codes, scores)
                                            : launch_score_batch(ctx, cb, B, codes, scores);
}

MIDAS_WARM_TU(score_f64, (k_score_mfma_f64<float, true, true>))

}  // namespace midas
