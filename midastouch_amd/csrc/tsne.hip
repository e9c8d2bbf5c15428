// tsne.hip - one-dimensional t-SNE on the device (eval/viz_codebook.py -> modules/misc.py color_tsne): sklearn's TSNE(n_components=1)
// affinities and optimiser schedule, with the EXACT O(K^2) gradient in place of Barnes-Hut.  DESIGN.md 4.6.
//
//   k_tsne_norms      |x_i|^2 in float64 (nan_to_num applied on the fly when asked: the caller's matrix is read, never rewritten)
//   k_tsne_knn_f64    d2[i][j] = max(-2 x_i.x_j + |x_i|^2 + |x_j|^2, 0) for a panel of query rows against all K rows, the dot
//                     products on v_mfma_f64_16x16x4_f64 (float32 widened exactly)
//   k_tsne_select     the k smallest (d2, j) of a panel row, j != i, in ascending (d2, j) order - a running top-k list in LDS,
//                     candidates below its k-th entry buffered and merged by a bitonic sort
//   k_tsne_perplexity sklearn _utils._binary_search_perplexity, one wave per row, float64 arithmetic on float32 distances
//   k_tsne_rep        the repulsive O(K^2) sweep: per (row, slice of columns) sum_j q_ij and sum_j q_ij^2 (y_i - y_j), float32 pair
//                     terms, float32 sums over 64 columns flushed into float64
//   k_tsne_attr       the attractive term over P's row (wave per row) and the fixed-order sum of the slices
//   k_tsne_kl         sum_j p_ij log(max(p_ij, FLT_MIN) / max(q_ij / Z, FLT_MIN)) per row (compute_gradient_positive's error)
//   k_tsne_sum        one-block fixed-order sum of a float64 vector (Z, KL, |grad|^2)
//   k_tsne_update     grad = 4 (pos - neg / Z), then _gradient_descent's gains / momentum / step with numpy 2's promotion
// No float atomics anywhere: every sum has a fixed order, so a run is bit-reproducible.
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "score_f64.hpp"

#include <cfloat>
#include <cmath>

namespace midas {

template <typename T>
MD T tsne_ntn(T x) {  // np.nan_to_num: NaN -> 0, +-inf -> +-max of the dtype
    if (x != x) return (T)0;
    if (x == (T)INFINITY) return sizeof(T) == 4 ? (T)FLT_MAX : (T)DBL_MAX;
    if (x == -(T)INFINITY) return sizeof(T) == 4 ? (T)-FLT_MAX : (T)-DBL_MAX;
    return x;
}

MD double tsne_wave_sum(double v) {  // xor butterfly: every lane ends with the same bits
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---- kNN -------------------------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(256) void k_tsne_norms(const T* __restrict__ X, int64_t K, int64_t F, int64_t ld, int ntn,
                                                    double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= K) return;
    const T* row = X + i * ld;
    double s = 0.0;
    for (int64_t f = lane; f < F; f += 64) {
        const double x = (double)(ntn ? tsne_ntn(row[f]) : row[f]);
        s = fma(x, x, s);
    }
    s = tsne_wave_sum(s);
    if (lane == 0) out[i] = s;
}

// Block tile 128 query rows x 128 entry rows, four waves of 64 x 64 (4 x 4 MFMA tiles of 16 x 16, sixteen f64x4 accumulators).
// A step stages KC = 16 columns of both row blocks in LDS, k-major ([k][row]: lane (g, i) of an MFMA reads k-slot g of row i);
// the next step is loaded into registers under the current step's MFMAs.  MFMA C/D: element r of lane (g, i) = row g + 4 r,
// column i (score_f64.hpp).
constexpr int KNN_BT = 128, KNN_KC = 16;

template <typename T>
__global__ __launch_bounds__(256) void k_tsne_knn_f64(const T* __restrict__ X, int64_t K, int64_t F, int64_t ld, int ntn,
                                                      const double* __restrict__ nrm, int64_t i0, int64_t R,
                                                      double* __restrict__ panel, int64_t ldo) {
    __shared__ double sa[KNN_KC][KNN_BT];
    __shared__ double sb[KNN_KC][KNN_BT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t qb = i0 + (int64_t)blockIdx.y * KNN_BT, eb = (int64_t)blockIdx.x * KNN_BT, qend = i0 + R;
    // loader: thread t stages row t >> 1, columns 8 (t & 1) .. + 8 of both blocks
    const int lr = tid >> 1, lc = 8 * (tid & 1);
    const int64_t qrow = qb + lr, erow = eb + lr;
    const T* qp = X + (qrow < qend ? qrow : i0) * ld;
    const T* ep = X + (erow < K ? erow : 0) * ld;
    const bool qlive = qrow < qend, elive = erow < K;
    double ra[8], rb[8];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int64_t f = k0 + lc + c;
            T a = (T)0, b = (T)0;
            if (f < F) {
                a = qp[f];
                b = ep[f];
            }
            if (ntn) { a = tsne_ntn(a); b = tsne_ntn(b); }
            ra[c] = qlive ? (double)a : 0.0;
            rb[c] = elive ? (double)b : 0.0;
        }
    };
    f64x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int64_t nsteps = (F + KNN_KC - 1) / KNN_KC;
    fetch(0);
    for (int64_t s = 0; s < nsteps; ++s) {
        __syncthreads();  // the previous step's reads are done
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            sa[lc + c][lr] = ra[c];
            sb[lc + c][lr] = rb[c];
        }
        __syncthreads();
        if (s + 1 < nsteps) fetch((s + 1) * KNN_KC);
#pragma unroll
        for (int kk = 0; kk < KNN_KC / 4; ++kk) {
            double av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                av[t] = sa[4 * kk + g][64 * wm + 16 * t + i];
                bv[t] = sb[4 * kk + g][64 * wn + 16 * t + i];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int64_t j = eb + 64 * wn + 16 * b + i;
        if (j >= K) continue;
        const double nj = nrm[j];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t q = qb + 64 * wm + 16 * a + g + 4 * r;
                if (q < qend) {
                    const double d = (-2.0 * acc[a][b][r] + nrm[q]) + nj;
                    panel[(q - i0) * ldo + j] = d > 0.0 ? d : 0.0;
                }
            }
    }
}

// One block a panel row.  LDS: SEL_N (d2, j) slots; [0, 256) the running list (ascending after each merge, +inf past what it
// holds), [256, 256 + cnt) the candidates of the chunks since the last merge.  A chunk is 1024 columns (four a thread); a merge
// sorts all SEL_N slots (bitonic) and runs when the buffer could not take another chunk, and at the end.
constexpr int SEL_N = 2048, SEL_LIST = 256, SEL_CHUNK = 1024;

MD bool sel_less(double da, int ja, double db, int jb) { return da < db || (da == db && ja < jb); }

__global__ __launch_bounds__(256) void k_tsne_select(const double* __restrict__ panel, int64_t ldo, int64_t K, int64_t i0,
                                                     int k, int32_t* __restrict__ idx_out, double* __restrict__ d2_out) {
    __shared__ double sd[SEL_N];
    __shared__ int sj[SEL_N];
    __shared__ int s_cnt;
    __shared__ double s_td;
    __shared__ int s_tj;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x, gi = i0 + row;
    const double* pr = panel + row * ldo;
    for (int t = tid; t < SEL_N; t += 256) { sd[t] = INFINITY; sj[t] = INT32_MAX; }
    if (tid == 0) { s_cnt = 0; s_td = INFINITY; s_tj = INT32_MAX; }
    __syncthreads();
    auto merge = [&]() {
        const int cnt = s_cnt;
        for (int t = SEL_LIST + cnt + tid; t < SEL_N; t += 256) { sd[t] = INFINITY; sj[t] = INT32_MAX; }
        __syncthreads();
        for (int size = 2; size <= SEL_N; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int p = tid; p < SEL_N / 2; p += 256) {
                    const int lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    const double dl = sd[lo], dh = sd[hi];
                    const int jl = sj[lo], jh = sj[hi];
                    if (sel_less(dh, jh, dl, jl) == up) { sd[lo] = dh; sd[hi] = dl; sj[lo] = jh; sj[hi] = jl; }
                }
                __syncthreads();
            }
        if (tid == 0) {
            s_cnt = 0;
            s_td = sd[k - 1];  // +inf until the list holds k entries
            s_tj = sj[k - 1];
        }
        __syncthreads();
    };
    for (int64_t c0 = 0; c0 < K; c0 += SEL_CHUNK) {
        const double td = s_td;
        const int tj = s_tj;
#pragma unroll
        for (int q = 0; q < SEL_CHUNK / 256; ++q) {
            const int64_t j = c0 + q * 256 + tid;
            if (j < K && j != gi) {
                const double d = pr[j];
                if (sel_less(d, (int)j, td, tj)) {
                    const int pos = atomicAdd(&s_cnt, 1);
                    sd[SEL_LIST + pos] = d;
                    sj[SEL_LIST + pos] = (int)j;
                }
            }
        }
        __syncthreads();
        const int cnt = s_cnt;
        __syncthreads();  // (every thread has read the count before the next chunk adds to it)
        if (cnt > SEL_N - SEL_LIST - SEL_CHUNK || c0 + SEL_CHUNK >= K) merge();
    }
    for (int t = tid; t < k; t += 256) {
        idx_out[gi * k + t] = sj[t];
        d2_out[gi * k + t] = sd[t];
    }
}

// ---- conditional affinities ------------------------------------------------------------------------------------------------

// sklearn _binary_search_perplexity on one row per wave: lane l holds columns l, l + 64, .. (k <= 256).  beta from 1, at most 100
// steps, sum_Pi floored at (double)1e-8f, tolerance (double)1e-5f, entropy = log(sum_Pi) + beta sum_j d_j p_j.
__global__ __launch_bounds__(256) void k_tsne_perplexity(const float* __restrict__ d2, int64_t K, int k, double desired_entropy,
                                                         double* __restrict__ P) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= K) return;
    const float* dr = d2 + row * k;
    double d[4], p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = lane + 64 * q < k ? (double)dr[lane + 64 * q] : 0.0;
    const double eps_sum = (double)1e-8f, tol = (double)1e-5f;
    double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY;
    for (int l = 0; l < 100; ++l) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            p[q] = lane + 64 * q < k ? exp(-d[q] * beta) : 0.0;
            s += p[q];
        }
        double sum_p = tsne_wave_sum(s);
        if (sum_p == 0.0) sum_p = eps_sum;
        double sd = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            p[q] /= sum_p;
            sd += d[q] * p[q];
        }
        const double sum_dp = tsne_wave_sum(sd);
        const double entropy = log(sum_p) + beta * sum_dp;
        const double diff = entropy - desired_entropy;
        if (fabs(diff) <= tol) break;
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (lane + 64 * q < k) P[row * k + lane + 64 * q] = p[q];
}

// ---- gradient --------------------------------------------------------------------------------------------------------------

constexpr int REP_TPB = 256, REP_FLUSH = 64;

// grid (ceil(K / 256), S): thread i of block x sweeps columns [s slice, (s + 1) slice) of slice s = blockIdx.y.  The row's own
// column adds q = 1 (d = 0, rcp(1) = 1 exactly) and 0 to the repulsion; the 1 is taken off the float64 sum.
__global__ __launch_bounds__(REP_TPB) void k_tsne_rep(const float* __restrict__ y, int64_t K, int64_t slice,
                                                      double* __restrict__ part_neg, double* __restrict__ part_z) {
    __shared__ float sy[REP_TPB];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * REP_TPB + tid;
    const int64_t j0 = (int64_t)blockIdx.y * slice, j1 = j0 + slice < K ? j0 + slice : K;
    const float yi = y[i < K ? i : K - 1];
    double zn = 0.0, zz = 0.0;
    for (int64_t c = j0; c < j1; c += REP_TPB) {
        const int n = (int)(j1 - c < REP_TPB ? j1 - c : REP_TPB);
        __syncthreads();
        if (tid < n) sy[tid] = y[c + tid];
        __syncthreads();
        for (int t0 = 0; t0 < n; t0 += REP_FLUSH) {
            const int t1 = t0 + REP_FLUSH < n ? t0 + REP_FLUSH : n;
            float an = 0.f, az = 0.f, bn = 0.f, bz = 0.f;
            int t = t0;
            for (; t + 1 < t1; t += 2) {
                const float d0 = yi - sy[t], d1 = yi - sy[t + 1];
                const float q0 = __builtin_amdgcn_rcpf(fmaf(d0, d0, 1.f)), q1 = __builtin_amdgcn_rcpf(fmaf(d1, d1, 1.f));
                az += q0;
                bz += q1;
                an = fmaf(q0 * q0, d0, an);
                bn = fmaf(q1 * q1, d1, bn);
            }
            if (t < t1) {
                const float d0 = yi - sy[t];
                const float q0 = __builtin_amdgcn_rcpf(fmaf(d0, d0, 1.f));
                az += q0;
                an = fmaf(q0 * q0, d0, an);
            }
            zn += (double)an + (double)bn;
            zz += (double)az + (double)bz;
        }
    }
    if (i < K) {
        if (i >= j0 && i < j1) zz -= 1.0;
        part_neg[blockIdx.y * K + i] = zn;
        part_z[blockIdx.y * K + i] = zz;
    }
}

// one wave a row: pos_i = sum over P's row of p_ij q_ij (y_i - y_j) (compute_gradient_positive's float32 terms, float64 sum), and the
// slices of k_tsne_rep summed in slice order
__global__ __launch_bounds__(256) void k_tsne_attr(const float* __restrict__ y, int64_t K, const int64_t* __restrict__ crow,
                                                   const int32_t* __restrict__ col, const float* __restrict__ val, int S,
                                                   const double* __restrict__ part_neg, const double* __restrict__ part_z,
                                                   double* __restrict__ pos, double* __restrict__ neg, double* __restrict__ zrow) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= K) return;
    const float yi = y[i];
    double s = 0.0;
    for (int64_t e = crow[i] + lane; e < crow[i + 1]; e += 64) {
        const float d = yi - y[col[e]];
        const float q = 1.f / (1.f + d * d);
        s += (double)(val[e] * q) * (double)d;
    }
    s = tsne_wave_sum(s);
    if (lane == 0) {
        double n = 0.0, z = 0.0;
        for (int k = 0; k < S; ++k) { n += part_neg[k * K + i]; z += part_z[k * K + i]; }
        pos[i] = s;
        neg[i] = n;
        zrow[i] = z;
    }
}

__global__ __launch_bounds__(256) void k_tsne_kl(const float* __restrict__ y, int64_t K, const int64_t* __restrict__ crow,
                                                 const int32_t* __restrict__ col, const float* __restrict__ val,
                                                 const double* __restrict__ Z, double* __restrict__ kl_row) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= K) return;
    const float yi = y[i];
    const double z = Z[0];
    double s = 0.0;
    for (int64_t e = crow[i] + lane; e < crow[i + 1]; e += 64) {
        const float d = yi - y[col[e]];
        const float q = 1.f / (1.f + d * d);
        const float p = val[e], qz = (float)((double)q / z);
        const float ratio = fmaxf(p, FLT_MIN) / fmaxf(qz, FLT_MIN);
        s += (double)p * log((double)ratio);
    }
    s = tsne_wave_sum(s);
    if (lane == 0) kl_row[i] = s;
}

// one block of 1024: out[0] = sum of x[0 .. n) in a fixed order (strided per thread, then a tree)
__global__ __launch_bounds__(1024) void k_tsne_sum(const double* __restrict__ x, int64_t n, double* __restrict__ out) {
    __shared__ double s[1024];
    double a = 0.0;
    for (int64_t t = threadIdx.x; t < n; t += 1024) a += x[t];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s[0];
}

// grad_i = float32(pos - neg / Z) * 4 (tot_force, then `grad *= c`).  mode 0: write it and stop (midas_tsne_gradient).  Otherwise
// one step of _gradient_descent: gains +0.2 / x0.8 (float32), clipped at min_gain, grad *= gains, update = momentum update - lr grad,
// p += update.  mode 1: the learning rate is a numpy float64 scalar (learning_rate="auto"), so update is float64 and p is rounded
// from float64(p) + update; mode 2: a Python float learning rate, everything float32.  gsq[i] = grad_i^2 (after the gains).
__global__ __launch_bounds__(256) void k_tsne_update(int64_t K, float* __restrict__ y, const double* __restrict__ pos,
                                                     const double* __restrict__ neg, const double* __restrict__ Z, int mode,
                                                     float* __restrict__ grad_out, float* __restrict__ gains,
                                                     double* __restrict__ update, double momentum, double lr, float min_gain,
                                                     double* __restrict__ gsq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    float g = (float)(pos[i] - neg[i] / Z[0]);
    g = g * 4.0f;
    if (mode == 0) {
        grad_out[i] = g;
        return;
    }
    const double u = update[i];
    const bool inc = mode == 1 ? (u * (double)g < 0.0) : ((float)u * g < 0.0f);
    float gn = gains[i];
    gn = inc ? gn + 0.2f : gn * 0.8f;
    gn = gn < min_gain ? min_gain : gn;
    gains[i] = gn;
    g = g * gn;
    if (mode == 1) {
        const double un = momentum * u - lr * (double)g;
        update[i] = un;
        y[i] = (float)((double)y[i] + un);
    } else {
        const float un = (float)momentum * (float)u - (float)lr * g;
        update[i] = (double)un;
        y[i] = y[i] + un;
    }
    gsq[i] = (double)g * (double)g;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------

int launch_tsne_knn(midas_ctx* ctx, const void* X, int32_t dtype, int64_t K, int64_t F, int64_t ld, int32_t ntn, int32_t k,
                    int64_t rows, double* scratch, int32_t* idx_out, double* d2_out) {
    double* nrm = scratch;
    double* panel = scratch + K;
    const unsigned nb = (unsigned)ceil_div(K, (int64_t)4);
    if (dtype == MIDAS_F32) hipLaunchKernelGGL(k_tsne_norms<float>, dim3(nb), dim3(256), 0, ctx->stream, (const float*)X, K, F, ld, ntn, nrm);
    else hipLaunchKernelGGL(k_tsne_norms<double>, dim3(nb), dim3(256), 0, ctx->stream, (const double*)X, K, F, ld, ntn, nrm);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    for (int64_t i0 = 0; i0 < K; i0 += rows) {
        const int64_t R = K - i0 < rows ? K - i0 : rows;
        const dim3 grid((unsigned)ceil_div(K, (int64_t)KNN_BT), (unsigned)ceil_div(R, (int64_t)KNN_BT));
        if (dtype == MIDAS_F32)
            hipLaunchKernelGGL(k_tsne_knn_f64<float>, grid, dim3(256), 0, ctx->stream, (const float*)X, K, F, ld, ntn, nrm, i0, R, panel, K);
        else
            hipLaunchKernelGGL(k_tsne_knn_f64<double>, grid, dim3(256), 0, ctx->stream, (const double*)X, K, F, ld, ntn, nrm, i0, R, panel, K);
        MIDAS_HIP_CHECK(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_tsne_select, dim3((unsigned)R), dim3(256), 0, ctx->stream, panel, K, K, i0, k, idx_out, d2_out);
        MIDAS_HIP_CHECK(ctx, hipGetLastError());
    }
    return MIDAS_OK;
}

int launch_tsne_perplexity(midas_ctx* ctx, const float* d2, int64_t K, int32_t k, double desired_entropy, double* P) {
    hipLaunchKernelGGL(k_tsne_perplexity, dim3((unsigned)ceil_div(K, (int64_t)4)), dim3(256), 0, ctx->stream, d2, K, k,
                       desired_entropy, P);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

// slices of the repulsive sweep: enough (row block, slice) pairs to fill the chip, slices of at least 1024 columns
static int tsne_slices(int64_t K) {
    int64_t s = K / 1024;
    return (int)(s < 1 ? 1 : s > 32 ? 32 : s);
}

size_t tsne_grad_scratch_doubles(int64_t K) { return (size_t)(2 * tsne_slices(K) + 6) * (size_t)K + 8; }

// the objective at y: fills pos / neg / Z (work: tsne_grad_scratch_doubles), and the KL into kl_out (device) when asked
int launch_tsne_objective(midas_ctx* ctx, int64_t K, const float* y, const int64_t* crow, const int32_t* col, const float* val,
                          double* work, double* kl_out) {
    const int S = tsne_slices(K);
    const int64_t slice = ceil_div(K, (int64_t)S);
    double* part_neg = work;
    double* part_z = part_neg + (size_t)S * K;
    double* pos = part_z + (size_t)S * K;
    double* neg = pos + K;
    double* zrow = neg + K;
    double* klr = zrow + K;
    double* Z = klr + K;
    hipLaunchKernelGGL(k_tsne_rep, dim3((unsigned)ceil_div(K, (int64_t)REP_TPB), (unsigned)S), dim3(REP_TPB), 0, ctx->stream, y, K,
                       slice, part_neg, part_z);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    const unsigned nw = (unsigned)ceil_div(K, (int64_t)4);
    hipLaunchKernelGGL(k_tsne_attr, dim3(nw), dim3(256), 0, ctx->stream, y, K, crow, col, val, S, part_neg, part_z, pos, neg, zrow);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_tsne_sum, dim3(1), dim3(1024), 0, ctx->stream, zrow, K, Z);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    if (kl_out) {
        hipLaunchKernelGGL(k_tsne_kl, dim3(nw), dim3(256), 0, ctx->stream, y, K, crow, col, val, Z, klr);
        MIDAS_HIP_CHECK(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_tsne_sum, dim3(1), dim3(1024), 0, ctx->stream, klr, K, kl_out);
        MIDAS_HIP_CHECK(ctx, hipGetLastError());
    }
    return MIDAS_OK;
}

// pos / neg / Z of the last launch_tsne_objective on `work`
int launch_tsne_update(midas_ctx* ctx, int64_t K, float* y, double* work, int mode, float* grad_out, float* gains, double* update,
                       double momentum, double lr, float min_gain, double* gsq) {
    const int S = tsne_slices(K);
    const double* pos = work + (size_t)2 * S * K;
    const double* neg = pos + K;
    const double* Z = neg + 3 * K;
    hipLaunchKernelGGL(k_tsne_update, dim3((unsigned)ceil_div(K, (int64_t)256)), dim3(256), 0, ctx->stream, K, y, pos, neg, Z, mode,
                       grad_out, gains, update, momentum, lr, min_gain, gsq);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

__global__ __launch_bounds__(256) void k_tsne_reset(int64_t K, float* __restrict__ gains, double* __restrict__ update) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < K) { gains[i] = 1.0f; update[i] = 0.0; }
}

int launch_tsne_reset(midas_ctx* ctx, int64_t K, float* gains, double* update) {
    hipLaunchKernelGGL(k_tsne_reset, dim3((unsigned)ceil_div(K, (int64_t)256)), dim3(256), 0, ctx->stream, K, gains, update);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_tsne_sum(midas_ctx* ctx, const double* x, int64_t n, double* out) {
    hipLaunchKernelGGL(k_tsne_sum, dim3(1), dim3(1024), 0, ctx->stream, x, n, out);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

MIDAS_WARM_TU(tsne, k_tsne_rep)

}  // namespace midas
