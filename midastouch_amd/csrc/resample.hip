// resample.hip - weights (K5), float64 CDF in the fixed blocked order (K6), inverse-CDF search (K7) and
// gather-resample (K8) as operators of their own.  The fused tail of the per-frame step: tail.hip (its TA is
// at the end of this unit), the sharded engine's exchange: shard_route.hip.
//
// Summation order (DESIGN.md "Summation order", oracle/midas_oracle.c mo_blocked_scan): 16 values =
// chunk (one lane), 16 chunks = group (a quarter-wave), 16 groups = block (one 256-thread workgroup,
// 4096 values); every level is a sequential float64 sum in index order starting from +0.0.
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "tail_block.hpp"
#include "tail_sums.hpp"

namespace midas {

MD double wsum_shuffles(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// self-check of the register-move sums against the shuffle butterflies: 64 doubles in, per lane {shuffle wave sum, ordered wave
// sum, shuffle quarter sum, ordered quarter sum} out (256 doubles)
__global__ __launch_bounds__(64) void k_debug_wave_sum(const double* __restrict__ in, double* __restrict__ out) {
    const int l = threadIdx.x;
    const double v = in[l];
    double q = v;
    q += __shfl_xor(q, 8); q += __shfl_xor(q, 4); q += __shfl_xor(q, 2); q += __shfl_xor(q, 1);
    out[4 * l] = wsum_shuffles(v);
    out[4 * l + 1] = wave_sum_ordered(v);
    out[4 * l + 2] = q;
    out[4 * l + 3] = quarter_sum_ordered(v);
}
int launch_selftest_wave_sums(midas_ctx* ctx, const double* in64, double* out256) {
    hipLaunchKernelGGL(k_debug_wave_sum, dim3(1), dim3(64), 0, ctx->stream, in64, out256);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

// sequential sum of per-block totals part[0..nb), exclusive prefix up to `b` returned in bp
MD void seq_totals(const double* __restrict__ part, int nb, int b, double& bp, double& total) {
    double acc = 0.0, pre = 0.0;
    for (int i = 0; i < nb; ++i) {
        if (i == b) pre = acc;
        acc = acc + part[i];
    }
    bp = pre;
    total = acc;
}

// block-wide max/min over an array of partials
MD void block_extrema(const double* __restrict__ pmax, const double* __restrict__ pmin, int np, int stride,
                      double* s_red, double& mx, double& mn) {
    double a = -INFINITY, b = INFINITY;
    bool nan = false;
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        double u = pmax[(int64_t)i * stride], v = pmin[(int64_t)i * stride];
        nan |= (u != u) || (v != v);
        a = u > a ? u : a;
        b = v < b ? v : b;
    }
    a = wmax(a);
    b = wmin(b);
    const bool wnan = __any(nan);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_red[w] = a; s_red[8 + w] = b; s_red[16 + w] = wnan ? 1.0 : 0.0; }
    __syncthreads();
    a = s_red[0]; b = s_red[8];
    double f = s_red[16];
    for (int i = 1; i < nw; ++i) {
        a = s_red[i] > a ? s_red[i] : a;
        b = s_red[8 + i] < b ? s_red[8 + i] : b;
        f += s_red[16 + i];
    }
    __syncthreads();
    if (f != 0.0) { a = NAN; b = NAN; }  // torch.max/min propagate NaN
    mx = a;
    mn = b;
}

// ------------------------------------------------------------------------------------------------
// standalone kernels
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gather_f64(int64_t N, const double* __restrict__ table,
                                                    const int32_t* __restrict__ idx, double* __restrict__ out) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n < N) out[n] = table[idx[n]];
}
int launch_gather_f64(midas_ctx* ctx, int64_t N, const double* table, const int32_t* idx, double* out) {
    if (N == 0) return MIDAS_OK;
    hipLaunchKernelGGL(k_gather_f64, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, table, idx, out);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// per-block extrema of x (4096 values per block)
__global__ __launch_bounds__(256) void k_extrema(int64_t N, const double* __restrict__ x, double* __restrict__ pmax,
                                                 double* __restrict__ pmin) {
    __shared__ double s_red[24];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK;
    double a = -INFINITY, b = INFINITY;
    bool nan = false;
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = base + (int64_t)j * 256 + threadIdx.x;
        if (i < N) {
            double v = x[i];
            nan |= v != v;
            a = v > a ? v : a;
            b = v < b ? v : b;
        }
    }
    a = wmax(a);
    b = wmin(b);
    const bool wnan = __any(nan);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_red[w] = a; s_red[8 + w] = b; s_red[16 + w] = wnan ? 1.0 : 0.0; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double f = 0.0;
        for (int i = 0; i < 4; ++i) {
            a = s_red[i] > a ? s_red[i] : a;
            b = s_red[8 + i] < b ? s_red[8 + i] : b;
            f += s_red[16 + i];
        }
        pmax[blockIdx.x] = f != 0.0 ? NAN : a;
        pmin[blockIdx.x] = f != 0.0 ? NAN : b;
    }
}

// e = exp(x - max) (or x when the softmax is skipped) ; per-block totals of e in the spec order.
// valid (nullable) is NOT applied here.  flag_out[0] = 1 when the softmax is applied.
__global__ __launch_bounds__(256) void k_exp_partial(int64_t N, const double* __restrict__ x, int np,
                                                     const double* __restrict__ pmax, const double* __restrict__ pmin,
                                                     int32_t softmax, double* __restrict__ e_out,
                                                     double* __restrict__ part_sum, int32_t* __restrict__ flag_out) {
    __shared__ double s_red[24];
    __shared__ double s_gtot[16];
    double mx, mn;
    block_extrema(pmax, pmin, np, 1, s_red, mx, mn);
    // not isclose(max - min, 0): |max-min| > atol, or NaN (isclose(NaN, 0) is False)
    const double spread = mx - mn;
    const bool apply = softmax && !(__builtin_fabs(spread) <= ISCLOSE_ATOL);
    if (blockIdx.x == 0 && threadIdx.x == 0 && flag_out) flag_out[0] = apply ? 1 : 0;
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_CHUNK;
    double v[SCAN_CHUNK], l[SCAN_CHUNK];
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = base + j;
        double e = 0.0;
        if (i < N) {
            const double xi = x[i];
            e = apply ? exp_spec(xi - mx) : xi;
            e_out[i] = e;
        }
        v[j] = e;
    }
    const double W = block_scan(v, l, s_gtot);
    if (threadIdx.x == 0) part_sum[blockIdx.x] = W;
}

// w = e / S with S = sequential sum of the block totals (only when flag[0])
__global__ __launch_bounds__(256) void k_normalise(int64_t N, double* __restrict__ w, int nb,
                                                   const double* __restrict__ part_sum,
                                                   const int32_t* __restrict__ flag) {
    if (!flag[0]) return;
    double bp, S;
    seq_totals(part_sum, nb, 0, bp, S);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) w[i] = w[i] / S;
}
int launch_softmax(midas_ctx* ctx, int64_t N, const double* x, int32_t softmax, double* w) {
    if (N == 0) return MIDAS_OK;
    const int nb = (int)ceil_div(N, SCAN_BLOCK);
    void* sc;
    int rc = midas_scratch(ctx, (size_t)nb * 3 * sizeof(double) + 64, &sc);
    if (rc) return rc;
    double* pmax = (double*)sc;
    double* pmin = pmax + nb;
    double* psum = pmin + nb;
    int32_t* flag = (int32_t*)(psum + nb);
    hipLaunchKernelGGL(k_extrema, dim3(nb), dim3(256), 0, ctx->stream, N, x, pmax, pmin);
    hipLaunchKernelGGL(k_exp_partial, dim3(nb), dim3(256), 0, ctx->stream, N, x, nb, pmax, pmin, softmax, w, psum, flag);
    hipLaunchKernelGGL(k_normalise, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, w, nb, psum, flag);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

__global__ __launch_bounds__(256) void k_prune(int64_t N, double* __restrict__ w, const double* __restrict__ dist,
                                               double thr, int32_t* __restrict__ nvalid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < N) {
        keep = !(dist[i] > thr);
        w[i] = w[i] * (keep ? 1.0 : 0.0);
    }
    unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(nvalid, (int32_t)__popcll(m));
}
int launch_prune(midas_ctx* ctx, int64_t N, double* w, const double* dist, double thr, int32_t* nvalid) {
    MIDAS_HIP_CHECK(ctx, hipMemsetAsync(nvalid, 0, sizeof(int32_t), ctx->stream));
    if (N == 0) return MIDAS_OK;
    hipLaunchKernelGGL(k_prune, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, w, dist, thr, nvalid);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// block-local prefix of w (spec order) -> lp ; block totals -> part ; NaN detection -> status[0] |= 2
__global__ __launch_bounds__(256) void k_scan_local(int64_t N, const double* __restrict__ w, double* __restrict__ lp,
                                                    double* __restrict__ part, int32_t* __restrict__ status) {
    __shared__ double s_gtot[16];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_CHUNK;
    double v[SCAN_CHUNK], l[SCAN_CHUNK];
    bool nan = false;
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = base + j;
        double t = 0.0;
        if (i < N) { t = w[i]; nan |= t != t; }
        v[j] = t;
    }
    const double W = block_scan(v, l, s_gtot);
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j)
        if (base + j < N) lp[base + j] = l[j];
    if (threadIdx.x == 0) part[blockIdx.x] = W;
    const bool wnan = __any(nan);
    if (wnan && (threadIdx.x & 63) == 0) atomicOr(status, 2);
}

// cdf_i = (BP_b + lp_i) / total ; cdf_{N-1} = 1 ; status[0] = 1 when total == 0 (2 already set on NaN)
__global__ __launch_bounds__(256) void k_cdf_final(int64_t N, double* __restrict__ cdf, int nb,
                                                   const double* __restrict__ part, int32_t* __restrict__ status) {
    double bp, total;
    seq_totals(part, nb, blockIdx.x, bp, total);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (total != total) atomicOr(status, 2);
        else if (total == 0.0) atomicOr(status, 1);
    }
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK;
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = base + (int64_t)j * 256 + threadIdx.x;
        if (i < N) cdf[i] = (i == N - 1) ? 1.0 : (bp + cdf[i]) / total;
    }
}
int launch_cdf(midas_ctx* ctx, int64_t N, const double* w, double* cdf, int32_t* status) {
    MIDAS_HIP_CHECK(ctx, hipMemsetAsync(status, 0, sizeof(int32_t), ctx->stream));
    if (N == 0) return MIDAS_OK;
    const int nb = (int)ceil_div(N, SCAN_BLOCK);
    void* sc;
    int rc = midas_scratch(ctx, (size_t)nb * sizeof(double), &sc);
    if (rc) return rc;
    hipLaunchKernelGGL(k_scan_local, dim3(nb), dim3(256), 0, ctx->stream, N, w, cdf, (double*)sc, status);
    hipLaunchKernelGGL(k_cdf_final, dim3(nb), dim3(256), 0, ctx->stream, N, cdf, nb, (const double*)sc, status);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

MD int32_t search_lower(const double* __restrict__ cdf, int64_t N, double u) {
    int64_t lo = 0, hi = N;
    while (hi > lo) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] < u) lo = mid + 1; else hi = mid;
    }
    return (int32_t)(lo < N ? lo : N - 1);
}
MD int32_t search_upper(const double* __restrict__ cdf, int64_t N, double u) {
    int64_t lo = 0, hi = N;
    while (hi > lo) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
    }
    return (int32_t)(lo < N ? lo : N - 1);
}

static_assert(MIDAS_U32_FROM_U == -2.0f, "midas_math.hpp systematic_draw");
template <bool FROM_U = false>
MD int32_t resample_slot(const double* __restrict__ cdf, int64_t N, int64_t M, int64_t i, int32_t mode,
                         const double* __restrict__ u, float u32, uint64_t seed, uint64_t step) {
    if (mode == MIDAS_RESAMPLE_MULTINOMIAL) {
        const double ui = u ? u[i] : philox_uniform53((uint64_t)i, seed, step);
        return search_lower(cdf, N, ui);
    }
    const float r = systematic_draw<FROM_U>(u32, u, seed, step);
    const float off = r / (float)M;
    double loc = (double)i / (double)M + (double)off;
    loc = loc >= 1.0 ? loc - 1.0 : loc;  // fmod(loc, 1) for loc in [0, 2)
    return search_upper(cdf, N, loc);
}

template <bool FROM_U>
__global__ __launch_bounds__(256) void k_search(int64_t N, const double* __restrict__ cdf, int64_t M, int32_t mode,
                                                const double* __restrict__ u, float u32, uint64_t seed, uint64_t step,
                                                int32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < M) idx[i] = resample_slot<FROM_U>(cdf, N, M, i, mode, u, u32, seed, step);
}
int launch_search(midas_ctx* ctx, int64_t N, const double* cdf, int64_t M, int32_t mode, const double* u, float u32,
                  uint64_t seed, uint64_t step, int32_t* idx) {
    if (M == 0) return MIDAS_OK;
    const bool from_u = mode == MIDAS_RESAMPLE_SYSTEMATIC && u32 == MIDAS_U32_FROM_U;
    if (from_u && !u) return midas_set_error(ctx, MIDAS_ERR_INVALID, "u32", "MIDAS_U32_FROM_U without u_dev");
    if (from_u)
        hipLaunchKernelGGL(k_search<true>, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, N, cdf, M, mode, u, u32, seed, step, idx);
    else
        hipLaunchKernelGGL(k_search<false>, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, N, cdf, M, mode, u, u32, seed, step, idx);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// rows of 16-byte multiples: one lane per 16-byte piece ; other sizes: one lane per byte group of 4/8/1
template <typename V>
__global__ __launch_bounds__(256) void k_gather_rows(int64_t M, const int32_t* __restrict__ idx,
                                                     const V* __restrict__ src, V* __restrict__ dst, int per_row) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = t / per_row;
    const int k = (int)(t - i * per_row);
    if (i < M) dst[i * per_row + k] = src[(int64_t)idx[i] * per_row + k];
}
int launch_gather_rows(midas_ctx* ctx, int64_t M, const int32_t* idx, const void* src, void* dst, int32_t row_bytes) {
    if (M == 0) return MIDAS_OK;
    const bool a16 = row_bytes % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
    const bool a8 = row_bytes % 8 == 0 && (uintptr_t)src % 8 == 0 && (uintptr_t)dst % 8 == 0;
    const bool a4 = row_bytes % 4 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0;
    if (a16) {
        const int per = row_bytes / 16;
        hipLaunchKernelGGL((k_gather_rows<float4>), dim3((unsigned)ceil_div(M * per, 256)), dim3(256), 0, ctx->stream, M,
                           idx, (const float4*)src, (float4*)dst, per);
    } else if (a8) {
        const int per = row_bytes / 8;
        hipLaunchKernelGGL((k_gather_rows<double>), dim3((unsigned)ceil_div(M * per, 256)), dim3(256), 0, ctx->stream, M,
                           idx, (const double*)src, (double*)dst, per);
    } else if (a4) {
        const int per = row_bytes / 4;
        hipLaunchKernelGGL((k_gather_rows<float>), dim3((unsigned)ceil_div(M * per, 256)), dim3(256), 0, ctx->stream, M,
                           idx, (const float*)src, (float*)dst, per);
    } else {
        hipLaunchKernelGGL((k_gather_rows<uint8_t>), dim3((unsigned)ceil_div(M * row_bytes, 256)), dim3(256), 0,
                           ctx->stream, M, idx, (const uint8_t*)src, (uint8_t*)dst, row_bytes);
    }
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// TA, the first half of the eager step tail (tail.hip, launch_step_tail: k_tail_b is the second), lives here: it shares
// block_extrema with k_exp_partial, and a unit whose only caller passes stride 1 compiles k_exp_partial differently.
// TA: e = exp(x - 1) comes from the particle update (x replaces it when the isclose guard skips the softmax);
//     em = e * valid ;
//     block-local prefix of em -> lp_out ; local block totals of e (softmax denominator) and of em
//     (CDF total) ; status[0] = 2 on NaN ; status[1] = particles kept.
//     The CDF is built from e*valid directly: the softmax normalisation cancels in prefix / total.
__global__ __launch_bounds__(256) void k_tail_a(int64_t N, const double* __restrict__ x, const uint8_t* __restrict__ valid,
                                                int np, int pstride, const double* __restrict__ pmax_all,
                                                const double* __restrict__ pmin_all, int32_t softmax,
                                                double* __restrict__ e_io, double* __restrict__ lp_out,
                                                double* __restrict__ block_sums_e, double* __restrict__ block_totals_em,
                                                double* __restrict__ flags_out, int32_t* __restrict__ flag,
                                                int32_t* __restrict__ status) {
    __shared__ double s_red[24];
    __shared__ double s_gtot[16];
    if (blockIdx.y) {  // batch of trajectories
        const int64_t b = blockIdx.y, o = b * N;
        x += o; valid += o; e_io += o; lp_out += o;
        pmax_all += b * np; pmin_all += b * np;
        block_sums_e += b * gridDim.x; block_totals_em += b * gridDim.x;
        flag += b; status += 2 * b;
    }
    double mx, mn;
    block_extrema(pmax_all, pmin_all, np, pstride, s_red, mx, mn);
    const bool apply = softmax && !(__builtin_fabs(mx - mn) <= ISCLOSE_ATOL);
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[0] = apply ? 1 : 0;
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_CHUNK;
    double v[SCAN_CHUNK], vm[SCAN_CHUNK], l[SCAN_CHUNK];
    bool nan = false;
    int kept = 0;
    // unconditional loads on clamped slots (conditional ones are issued one round trip at a time)
    const double* __restrict__ src = apply ? e_io : x;
    uint8_t okv[SCAN_CHUNK];
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = base + j, ic = i < N ? i : N - 1;
        v[j] = src[ic];
        okv[j] = valid[ic];
    }
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = base + j;
        double e = 0.0, em = 0.0;
        if (i < N) {
            e = v[j];
            if (!apply) e_io[i] = e;
            const bool ok = okv[j] != 0;
            em = e * (ok ? 1.0 : 0.0);
            kept += ok ? 1 : 0;
            nan |= em != em;
        }
        v[j] = e;
        vm[j] = em;
    }
    const double We = block_scan(v, l, s_gtot);
    __syncthreads();
    const double Wm = block_scan(vm, l, s_gtot);
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j)
        if (base + j < N) lp_out[base + j] = l[j];
    if (threadIdx.x == 0) { block_sums_e[blockIdx.x] = We; block_totals_em[blockIdx.x] = Wm; }
    const bool wnan = __any(nan);
    if (wnan && (threadIdx.x & 63) == 0) {
        atomicOr(&status[0], 2);
        if (flags_out) atomicAdd(&flags_out[0], 1.0);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    if ((threadIdx.x & 63) == 0 && kept) {
        atomicAdd(&status[1], kept);
        if (flags_out) atomicAdd(&flags_out[1], (double)kept);  // exact: integers far below 2^53
    }
}
int launch_tail_a(midas_ctx* ctx, int64_t N, const double* x, const uint8_t* valid, int np, int pstride,
                  const double* pmax_all, const double* pmin_all, int32_t softmax, double* e_io, double* lp_out,
                  double* block_sums_e, double* block_totals_em, double* flags_out, int32_t* flag, int32_t* status,
                  int batch) {
    hipLaunchKernelGGL(k_tail_a, dim3((unsigned)ceil_div(N, SCAN_BLOCK), (unsigned)(batch > 1 ? batch : 1)), dim3(256), 0, ctx->stream, N, x, valid, np, pstride,
                       pmax_all, pmin_all, softmax, e_io, lp_out, block_sums_e, block_totals_em, flags_out, flag, status);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// (the units cut out of this one are loaded with it: midas_ctx_create warms "resample")
MIDAS_WARM_DECL(tail) MIDAS_WARM_DECL(shard_route)
int warm_resample() {
    hipFuncAttributes attr;
    int rc = (int)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&k_gather_f64));
    for (int (*w)() : {warm_tail, warm_shard_route}) rc = rc ? rc : w();
    return rc;
}

}  // namespace midas
