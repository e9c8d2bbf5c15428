// cluster.hip - K9: cluster centres of the labelled particle set.
//
// particle_filter.get_cluster_centers(method="quat_avg") (modules/particle_filter.py:153-206) with
// pose.xyz_quat_averaged (modules/pose.py:112-147): per cluster label the weights (float32) are flattened to 1 when
// isclose(max - min, 0); the rotation is Markley's quaternion mean = principal eigenvector of sum w q q^T / sum w over
// sign-fixed quaternions (qw >= 0), the translation the weighted mean, the spread sqrt(sum w (t - mean)^2 / sum w).
// The reference walks the clusters in a Python loop of ~25 small torch ops each; here one pass over the particles
// accumulates every cluster's moments (both the weighted and the flattened set, the choice needs the cluster's
// extrema) and one small kernel finishes each cluster (4x4 symmetric eigenproblem: the top eigenvector by repeated squaring in float64, cluster_rot.hpp).
//
// Summation order (deterministic): per particle wave a shuffle tree, per 256-thread block the four waves in order,
// then the blocks in order.
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "cluster_rot.hpp"
#include "cluster_logmap.hpp"
#include "loop_weights.hpp"

namespace midas {

// (the moments' layout - CL_MOM, M_* - and the closed forms made of them: cluster_rot.hpp)

// unit quaternion (x, y, z, w) of a rotation matrix, float64, branch on the largest diagonal term (Shepperd)
MD void quat_of(const float* P, double* q) {
    const double r00 = P[0], r01 = P[1], r02 = P[2], r10 = P[4], r11 = P[5], r12 = P[6], r20 = P[8], r21 = P[9], r22 = P[10];
    const double tr = r00 + r11 + r22;
    double x, y, z, w;
    if (tr > 0.0) {
        const double s = __builtin_sqrt(tr + 1.0) * 2.0;
        w = 0.25 * s; x = (r21 - r12) / s; y = (r02 - r20) / s; z = (r10 - r01) / s;
    } else if (r00 > r11 && r00 > r22) {
        const double s = __builtin_sqrt(1.0 + r00 - r11 - r22) * 2.0;
        w = (r21 - r12) / s; x = 0.25 * s; y = (r01 + r10) / s; z = (r02 + r20) / s;
    } else if (r11 > r22) {
        const double s = __builtin_sqrt(1.0 + r11 - r00 - r22) * 2.0;
        w = (r02 - r20) / s; x = (r01 + r10) / s; y = 0.25 * s; z = (r12 + r21) / s;
    } else {
        const double s = __builtin_sqrt(1.0 + r22 - r00 - r11) * 2.0;
        w = (r10 - r01) / s; x = (r02 + r20) / s; y = (r12 + r21) / s; z = 0.25 * s;
    }
    const double n = __builtin_sqrt(x * x + y * y + z * z + w * w);
    const double sg = w < 0.0 ? -1.0 : 1.0;  // antipodal fix (pose.py:126)
    q[0] = sg * x / n; q[1] = sg * y / n; q[2] = sg * z / n; q[3] = sg * w / n;
}

MD double cl_wsum(double v) { return wave_sum_ordered(v); }  // (the xor butterfly 32 .. 1 of the spec, by register moves: midas_math.hpp)
MD double cl_wmax(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}
MD double cl_wmin(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}

// part[(c * nbs + block) * CL_MOM + m] (nbs = the launch's blocks: a cluster's partials lie together, whoever sums them can ask
// for them without knowing how many clusters there are); label_value(c) = the label cluster slot c stands for.  In two steps: what a particle
// contributes (pose rows, label, float32-rounded weight) and the accumulation, so that the loop step can compute the weight in
// the same launch (k_loop_weights_moments).
struct MomIn {
    float P[12];
    int64_t lab;
    double w;
};
MD void moments_load_pose(int64_t nc, const float* __restrict__ poses, MomIn& in) {
    const float4* p4 = reinterpret_cast<const float4*>(poses + nc * 16);
#pragma unroll
    for (int i = 0; i < 3; ++i) { const float4 r = p4[i]; in.P[4 * i] = r.x; in.P[4 * i + 1] = r.y; in.P[4 * i + 2] = r.z; in.P[4 * i + 3] = r.w; }
}
template <typename LabelT>
MD MomIn moments_load(int64_t nc, const float* __restrict__ poses, const double* __restrict__ w64, const float* __restrict__ w32,
                      const LabelT* __restrict__ labels) {
    MomIn in;
    moments_load_pose(nc, poses, in);
    in.lab = (int64_t)labels[nc];
    // particles.weights.float() (:161): the reference averages with float32 weights
    in.w = w64 ? (double)(float)w64[nc] : w32 ? (double)w32[nc] : 0.0;  // (neither: the caller computes the weight itself)
    return in;
}

// skip: a cluster NONE of the workgroup's particles belongs to is not summed (34 wave sums and two barriers each: with six
// clusters alive and one or two of them in a workgroup, 7.5 of the loop launch's 11 us) - its partials are written directly.
// They are not simply +0.0: the sums are of 0 x (a product of quaternion components, a translation) over every lane, which is -0.0
// where EVERY lane's factor is negative - the signs are taken once per workgroup (13 of them) - and NaN where some lane's pose
// is not finite (then nothing is skipped).  Same bits as the sums (tests/test_gpu_knobs.py: MIDAS_MOMENTS_SKIP=0).
// FORM (cluster_logmap.hpp): CL_FORM_QUAT the ten products of the sign-fixed quaternion's components, CL_FORM_LOGMAP the six
// components of the se(3) logarithm in the first six of those slots (the other four +0.0) - the skip's signs are then the six
// components' own.  Everything else - order, extrema, translation moments - is one text.
template <int FORM = CL_FORM_QUAT, typename LV>
MD void moments_accumulate(bool live, const MomIn& in, int C, LV label_value, double* __restrict__ part, double (*s_w)[CL_MOM],
                           bool skip = true) {
    __shared__ unsigned long long s_mem[4];
    __shared__ unsigned s_sgn[4];
    const size_t nbs = gridDim.x;
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const float* P = in.P;
    const int64_t lab = in.lab;
    const double w = in.w;
    constexpr int NQ = FORM == CL_FORM_LOGMAP ? 6 : 4;
    double q[NQ];  // (log-map form: xi)
    if constexpr (FORM == CL_FORM_LOGMAP) se3_log_f64(P, q);
    else quat_of(P, q);
    // A lane beyond the live count holds whatever pose lies there (the merged launch reads before it knows the count): rows never
    // written are zero matrices, whose logarithm is NaN, and 0 x NaN would spoil every cluster's sums - such a lane counts as xi = 0,
    // t = 0 in the log-map form (a zero matrix has a finite quaternion: the quaternion form takes the lane as it is)
    constexpr bool dead_is_zero = FORM == CL_FORM_LOGMAP;
    if (dead_is_zero && !live) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) q[i] = 0.0;
    }
    const bool zt = dead_is_zero && !live;
    const double tx = zt ? 0.0 : P[3], ty = zt ? 0.0 : P[7], tz = zt ? 0.0 : P[11];
    unsigned long long wgmask = ~0ull;
    unsigned sgn = 0;
    if (skip && C <= 64) {
        unsigned long long mm = 0;
        for (int c = 0; c < C; ++c) mm |= __any(live && lab == label_value(c)) ? (1ull << c) : 0ull;
        unsigned sg = 0;
        int k = 0;
        if constexpr (FORM == CL_FORM_LOGMAP) {
#pragma unroll
            for (int i = 0; i < 6; ++i) sg |= __all(__builtin_signbit(q[i]) ? 1 : 0) ? (1u << i) : 0u;
        } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j) {
                const double qq = q[i] * q[j];
                sg |= __all(__builtin_signbit(qq) ? 1 : 0) ? (1u << k) : 0u;
                ++k;
            }
        }
        sg |= __all(__builtin_signbit(tx) ? 1 : 0) ? (1u << 10) : 0u;
        sg |= __all(__builtin_signbit(ty) ? 1 : 0) ? (1u << 11) : 0u;
        sg |= __all(__builtin_signbit(tz) ? 1 : 0) ? (1u << 12) : 0u;
        const bool fin = __builtin_isfinite(q[0]) && __builtin_isfinite(q[1]) && __builtin_isfinite(q[2]) && __builtin_isfinite(q[3]) &&
                         __builtin_isfinite(q[NQ - 2]) && __builtin_isfinite(q[NQ - 1]) &&  // (log-map form: xi's last two)
                         __builtin_isfinite(tx) && __builtin_isfinite(ty) && __builtin_isfinite(tz);
        sg |= __all(fin ? 1 : 0) ? (1u << 31) : 0u;
        if (lane == 0) { s_mem[wv] = mm; s_sgn[wv] = sg; }
        __syncthreads();
        sgn = s_sgn[0] & s_sgn[1] & s_sgn[2] & s_sgn[3];
        if ((sgn >> 31) & 1u) wgmask = s_mem[0] | s_mem[1] | s_mem[2] | s_mem[3];  // (something not finite here: 0 x inf is part of the sums)
    }
    double v[CL_MOM];
    for (int c = 0; c < C; ++c) {
        if (!((wgmask >> (c & 63)) & 1ull)) {  // (workgroup-uniform)
            if (t < CL_MOM) {
                double r = 0.0;
                if (t == M_WMAX) r = -INFINITY;
                else if (t == M_WMIN) r = INFINITY;
                else {
                    int bit = -1;
                    constexpr int NS = FORM == CL_FORM_LOGMAP ? 6 : 10;  // (log-map form: the four slots behind the six are +0.0)
                    if (t >= M_QQW && t < M_QQW + NS) bit = t - M_QQW;
                    else if (t >= M_QQ1 && t < M_QQ1 + NS) bit = t - M_QQ1;
                    else if (t >= M_TW && t < M_TW + 3) bit = 10 + t - M_TW;
                    else if (t >= M_T1 && t < M_T1 + 3) bit = 10 + t - M_T1;
                    if (bit >= 0 && ((sgn >> bit) & 1u)) r = -0.0;
                }
                part[((size_t)c * nbs + blockIdx.x) * CL_MOM + t] = r;
            }
            continue;
        }
        const bool mine = live && lab == label_value(c);
        const double a = mine ? w : 0.0, b = mine ? 1.0 : 0.0;
        v[M_SW] = a; v[M_CNT] = b; v[M_WMAX] = 0.0; v[M_WMIN] = 0.0;
        int k = 0;
        if constexpr (FORM == CL_FORM_LOGMAP) {
#pragma unroll
            for (int i = 0; i < 10; ++i) { v[M_XW + i] = i < 6 ? a * q[i % 6] : 0.0; v[M_X1 + i] = i < 6 ? b * q[i % 6] : 0.0; }
        } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j) {
                const double qq = q[i] * q[j];
                v[M_QQW + k] = a * qq; v[M_QQ1 + k] = b * qq;
                ++k;
            }
        }
        v[M_TW] = a * tx; v[M_TW + 1] = a * ty; v[M_TW + 2] = a * tz;
        v[M_T1] = b * tx; v[M_T1 + 1] = b * ty; v[M_T1 + 2] = b * tz;
        v[M_TTW] = a * tx * tx; v[M_TTW + 1] = a * ty * ty; v[M_TTW + 2] = a * tz * tz;
        v[M_TT1] = b * tx * tx; v[M_TT1 + 1] = b * ty * ty; v[M_TT1 + 2] = b * tz * tz;
        const double mx = cl_wmax(mine ? w : -INFINITY), mn = cl_wmin(mine ? w : INFINITY);
#pragma unroll
        for (int m = 0; m < CL_MOM; ++m)
            if (m != M_WMAX && m != M_WMIN && !(FORM == CL_FORM_LOGMAP && ((m >= M_XW + 6 && m < M_XW + 10) || (m >= M_X1 + 6 && m < M_X1 + 10))))
                v[m] = cl_wsum(v[m]);  // (the log-map form's eight idle slots stay +0.0: 26 wave sums a cluster)
        __syncthreads();  // the previous cluster's LDS values have been read
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < CL_MOM; ++m) s_w[wv][m] = v[m];
            s_w[wv][M_WMAX] = mx; s_w[wv][M_WMIN] = mn;
        }
        __syncthreads();
        if (t < CL_MOM) {
            double r;
            if (t == M_WMAX) { r = s_w[0][t]; for (int i = 1; i < 4; ++i) r = s_w[i][t] > r ? s_w[i][t] : r; }
            else if (t == M_WMIN) { r = s_w[0][t]; for (int i = 1; i < 4; ++i) r = s_w[i][t] < r ? s_w[i][t] : r; }
            else r = ((s_w[0][t] + s_w[1][t]) + s_w[2][t]) + s_w[3][t];
            part[((size_t)c * nbs + blockIdx.x) * CL_MOM + t] = r;
        }
    }
}

template <int FORM = CL_FORM_QUAT, typename LabelT, typename LV>
MD void cluster_moments_body(int64_t N, const float* __restrict__ poses, const double* __restrict__ w64,
                             const float* __restrict__ w32, const LabelT* __restrict__ labels, int C, LV label_value,
                             double* __restrict__ part, double (*s_w)[CL_MOM], bool skip) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = n < N;
    const MomIn in = moments_load(live ? n : N - 1, poses, w64, w32, labels);
    moments_accumulate<FORM>(live, in, C, label_value, part, s_w, skip);
}

__global__ __launch_bounds__(256) void k_cluster_moments(int64_t N, const float* __restrict__ poses, const double* __restrict__ w64,
                                                         const float* __restrict__ w32, const int64_t* __restrict__ labels, int C,
                                                         const int64_t* __restrict__ label_values, double* __restrict__ part, bool skip) {
    __shared__ double s_w[4][CL_MOM];
    cluster_moments_body(N, poses, w64, w32, labels, C, [&](int c) { return label_values[c]; }, part, s_w, skip);
}
// the log-map form (midas_cluster_centers_logmap)
__global__ __launch_bounds__(256) void k_cluster_moments_logmap(int64_t N, const float* __restrict__ poses, const double* __restrict__ w64,
                                                                const float* __restrict__ w32, const int64_t* __restrict__ labels, int C,
                                                                const int64_t* __restrict__ label_values, double* __restrict__ part,
                                                                bool skip) {
    __shared__ double s_w[4][CL_MOM];
    cluster_moments_body<CL_FORM_LOGMAP>(N, poses, w64, w32, labels, C, [&](int c) { return label_values[c]; }, part, s_w, skip);
}

// N poses -> their se(3) logarithms [u, omega], (N, 6) float64 (midas_se3_log): what the log-map moments are sums of
__global__ __launch_bounds__(256) void k_se3_log(int64_t N, const float* __restrict__ poses, double* __restrict__ xi_out) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    MomIn in;
    moments_load_pose(n, poses, in);
    double xi[6];
    se3_log_f64(in.P, xi);
#pragma unroll
    for (int i = 0; i < 6; ++i) xi_out[n * 6 + i] = xi[i];
}

// loop engine: labels are DBSCAN's int32 values in [-1, ncl), cluster slot c stands for label c - 1; the particle count
// and ncl come from the control block (midas_loop_step)
template <int FORM>
MD void loop_cluster_moments_body(const int32_t* __restrict__ ctl_i, const float* __restrict__ poses, const double* __restrict__ w64,
                                  const int32_t* __restrict__ labels, double* __restrict__ part, bool skip, int32_t cap,
                                  double (*s_w)[CL_MOM]) {
    if (blockIdx.y) {  // a batch of trajectories (midas_loop_step_batch): `cap` particles and a launch's partials per trajectory
        const int64_t b = blockIdx.y, o = b * cap;
        ctl_i += b * LOOP_CTL_I; poses += o * 16; w64 += o; labels += o;
        part += (size_t)b * gridDim.x * LOOP_MAX_CLUSTERS * CL_MOM;
    }
    const int64_t n = ctl_i[LOOP_I_N];
    int C = ctl_i[LOOP_I_NCL] + 1;
    C = C > LOOP_MAX_CLUSTERS ? LOOP_MAX_CLUSTERS : C;
    if ((int64_t)blockIdx.x * 256 >= n) return;
    cluster_moments_body<FORM>(n, poses, w64, (const float*)nullptr, labels, C, [](int c) { return (int64_t)(c - 1); }, part, s_w, skip);
}
__global__ __launch_bounds__(256) void k_loop_cluster_moments(const int32_t* __restrict__ ctl_i, const float* __restrict__ poses,
                                                              const double* __restrict__ w64, const int32_t* __restrict__ labels,
                                                              double* __restrict__ part, bool skip, int32_t cap) {
    __shared__ double s_w[4][CL_MOM];
    loop_cluster_moments_body<CL_FORM_QUAT>(ctl_i, poses, w64, labels, part, skip, cap, s_w);
}
__global__ __launch_bounds__(256) void k_loop_cluster_moments_logmap(const int32_t* __restrict__ ctl_i, const float* __restrict__ poses,
                                                                     const double* __restrict__ w64, const int32_t* __restrict__ labels,
                                                                     double* __restrict__ part, bool skip, int32_t cap) {
    __shared__ double s_w[4][CL_MOM];
    loop_cluster_moments_body<CL_FORM_LOGMAP>(ctl_i, poses, w64, labels, part, skip, cap, s_w);
}

// The same with the frame's weights computed at its head (loop_weights.hpp: k_loop_weights' arithmetic, one particle a thread):
// S and the guard from k_loop_xe's block results by every workgroup for itself, the particle's weight stored and used at once,
// the first workgroup finalises the control block.  One launch less per frame (~5 us of a 90 us frame at N ~ 10^4), and the
// moments need not read the weights back.  Everything a thread reads is requested before the live count is looked at.
#ifdef MIDAS_ANNEAL_CLOCKS  // phase clocks of workgroup 0, thread 0 (tools/anneal_clocks.py; slots 24 .. 29 of the profiling block)
#define WCK(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl_d[56 + (i)] += (double)(wall_clock64() - wck0); } while (0)
#else
#define WCK(i) do { } while (0)
#endif
template <class Args>  // LoopWeightsArgs, LoopWeightsRowsArgs - rows on different objects - or LoopWeightsParamRowsArgs (loop_weights.hpp)
__global__ __launch_bounds__(256) void k_loop_weights_moments(Args a, const int32_t* __restrict__ labels,
                                                              double* __restrict__ part, bool skip) {
    constexpr int FORM = CL_FORM_QUAT;
#include "loop_weights_moments_body.hpp"
}
// the log-map form of the same launch (MIDAS_LOOP_CENTERS_LOGMAP): one text, the moments' form apart
template <class Args>
__global__ __launch_bounds__(256) void k_loop_weights_moments_logmap(Args a, const int32_t* __restrict__ labels,
                                                                     double* __restrict__ part, bool skip) {
    constexpr int FORM = CL_FORM_LOGMAP;
#include "loop_weights_moments_body.hpp"
}

// one 64-thread workgroup per cluster: blocks summed in order, then the closed forms
// rot_out (loop step): the normalised moment matrix goes there (10 doubles per cluster) and the rotation entries of the
// centre are left to whoever solves it (cluster_rotation_write, beside the annealing); nullptr: solved here
// FORM: the closed forms of the moments' form - cluster_close, or cluster_close_logmap (the whole centre is written: no rot_out)
template <int FORM = CL_FORM_QUAT>
MD void cluster_finish_body(int nblocks, size_t nbs, int c, const double* __restrict__ part, float* __restrict__ centers,
                            float* __restrict__ stds, int64_t* __restrict__ counts, double* s_m, double* __restrict__ rot_out = nullptr) {
    const int t = threadIdx.x;
    // blocks in order (the sums' order is part of the arithmetic).  The partials of CB blocks are staged in LDS by all 64 threads
    // (independent loads in flight together), then moment t walks them - at N = 100 k (391 blocks) the direct form was
    // thirteen dependent trips by 36 threads: 66 us, the longest kernel of the loop frame
    constexpr int CB = 128;
    __shared__ double s_part[CB * CL_MOM];
    double r = 0.0;
    // (eighteen loads in flight per thread before the first LDS store: left as one load and one store per iteration the
    // compiler waits for each load in turn - 72 dependent trips, slower than the form this replaces)
    constexpr int LB = 18;
    const int NT = (int)blockDim.x;  // 64 (midas_cluster_centers) or 256 (loop step: a chunk is one batch of loads)
    const double* __restrict__ pc = part + (size_t)c * nbs * CL_MOM;  // the cluster's partials lie together, block after block
    // 256 threads: a chunk of CB blocks is ONE batch of loads, and the next chunk's batch is in flight while this one's chain is
    // walked (at N = 100k - 391 blocks, four chunks - the chunks' trips came one after the other: 22 us)
    const bool one_batch = NT * LB >= CB * CL_MOM;
    double e_mx = -INFINITY, e_mn = INFINITY, e_first_mx = 0.0, e_first_mn = 0.0;  // (second wave: the extrema, see below)
    double xn[LB];
    auto issue = [&](int b0n) {
        const int nbn = nblocks - b0n < CB ? nblocks - b0n : CB;
#pragma unroll
        for (int j = 0; j < LB; ++j) {
            const int i = t + NT * j, ic = i < nbn * CL_MOM ? i : nbn * CL_MOM - 1;
            xn[j] = pc[(size_t)b0n * CL_MOM + ic];
        }
    };
    if (one_batch && nblocks > 0) issue(0);
    for (int b0 = 0; b0 < nblocks; b0 += CB) {
        const int nb = nblocks - b0 < CB ? nblocks - b0 : CB;
        if (one_batch) {
#pragma unroll
            for (int j = 0; j < LB; ++j)
                if (t + NT * j < nb * CL_MOM) s_part[t + NT * j] = xn[j];
        } else {
            for (int i0 = t; i0 < nb * CL_MOM; i0 += NT * LB) {
                double x[LB];
#pragma unroll
                for (int j = 0; j < LB; ++j) {
                    const int i = i0 + NT * j, ic = i < nb * CL_MOM ? i : nb * CL_MOM - 1;
                    x[j] = pc[(size_t)b0 * CL_MOM + ic];
                }
#pragma unroll
                for (int j = 0; j < LB; ++j)
                    if (i0 + NT * j < nb * CL_MOM) s_part[i0 + NT * j] = x[j];
            }
        }
        __syncthreads();
        if (one_batch && b0 + CB < nblocks) issue(b0 + CB);
        // sixteen LDS reads in flight, then the chain in block order.  The sums' chain is ONE dependent addition per block: the
        // two extrema (selects in the chain) are walked by lanes of their own where the workgroup has a second wave; whole batches
        // first, the remainder one by one (no guards in the chain).  With a read, a wait and three branches per block the walk was
        // 60 of the kernel's 65 us at 391 blocks.
        const bool two_waves = blockDim.x >= 128;
        const bool sums = t < CL_MOM && !(two_waves && (t == M_WMAX || t == M_WMIN));
        const bool ext = two_waves ? (t == 64 || t == 65) : (t == M_WMAX || t == M_WMIN);
        const int m = ext && two_waves ? (t == 64 ? M_WMAX : M_WMIN) : t;
        if (sums && !(ext && !two_waves)) {
            int b1 = 0;
            if (b0 == 0) { r = s_part[m]; b1 = 1; }
            for (; b1 + 16 <= nb; b1 += 16) {
                double x[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) x[j] = s_part[(b1 + j) * CL_MOM + m];
#pragma unroll
                for (int j = 0; j < 16; ++j) r = r + x[j];
            }
            for (; b1 < nb; ++b1) r = r + s_part[b1 * CL_MOM + m];
        }
        if (two_waves) {
            // The extrema need no order: `x > r ? x : r` walked from the first block's value takes the largest value that is not NaN
            // (NaN never wins) unless the FIRST is NaN (then nothing replaces it) - the second wave's lanes take every 64th block
            // each and meet at the end; walked block after block by one lane the two selects a block were the longest chain of
            // the kernel at 391 blocks.
            if (t >= 64 && t < 128) {
                const int l = t - 64;
                if (b0 == 0) { e_first_mx = s_part[M_WMAX]; e_first_mn = s_part[M_WMIN]; }
                for (int b1 = l; b1 < nb; b1 += 64) {
                    const double x = s_part[b1 * CL_MOM + M_WMAX], y = s_part[b1 * CL_MOM + M_WMIN];
                    e_mx = x > e_mx ? x : e_mx;
                    e_mn = y < e_mn ? y : e_mn;
                }
            }
        } else if (ext) {
            const bool is_max = m == M_WMAX;
            int b1 = 0;
            if (b0 == 0) { r = s_part[m]; b1 = 1; }
            for (; b1 + 16 <= nb; b1 += 16) {
                double x[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) x[j] = s_part[(b1 + j) * CL_MOM + m];
#pragma unroll
                for (int j = 0; j < 16; ++j) r = is_max ? (x[j] > r ? x[j] : r) : (x[j] < r ? x[j] : r);
            }
            for (; b1 < nb; ++b1) {
                const double x = s_part[b1 * CL_MOM + m];
                r = is_max ? (x > r ? x : r) : (x < r ? x : r);
            }
        }
        __syncthreads();
    }
    {
        const bool two_waves = blockDim.x >= 128;
        if (two_waves && t >= 64 && t < 128) {
            const double mx = wave_max_dpp(e_mx), mn = wave_min_dpp(e_mn);
            if (t == 64) {
                s_m[M_WMAX] = nblocks > 0 ? (e_first_mx != e_first_mx ? e_first_mx : mx) : 0.0;
                s_m[M_WMIN] = nblocks > 0 ? (e_first_mn != e_first_mn ? e_first_mn : mn) : 0.0;
            }
        } else if (t < CL_MOM && !(two_waves && (t == M_WMAX || t == M_WMIN))) s_m[t] = r;
    }
    __syncthreads();
    if (t != 0) return;
    if constexpr (FORM == CL_FORM_LOGMAP)
        cluster_close_logmap(s_m, centers + (size_t)c * 16, stds + (size_t)c * 3, counts ? counts + c : nullptr);
    else
    cluster_close(s_m, centers + (size_t)c * 16, stds + (size_t)c * 3, counts ? counts + c : nullptr,
                  rot_out ? rot_out + (size_t)c * 10 : nullptr);
}

__global__ __launch_bounds__(64) void k_cluster_finish(int nblocks, int C, const double* __restrict__ part,
                                                       float* __restrict__ centers, float* __restrict__ stds,
                                                       int64_t* __restrict__ counts) {
    __shared__ double s_m[CL_MOM];
    cluster_finish_body(nblocks, (size_t)nblocks, blockIdx.x, part, centers, stds, counts, s_m);
}
__global__ __launch_bounds__(64) void k_cluster_finish_logmap(int nblocks, int C, const double* __restrict__ part,
                                                              float* __restrict__ centers, float* __restrict__ stds,
                                                              int64_t* __restrict__ counts) {
    __shared__ double s_m[CL_MOM];
    cluster_finish_body<CL_FORM_LOGMAP>(nblocks, (size_t)nblocks, blockIdx.x, part, centers, stds, counts, s_m);
}

// loop engine: cluster slot c = blockIdx.x of the LOOP_MAX_CLUSTERS launched; rows of label c - 1
template <int FORM>
MD void loop_cluster_finish_body(const int32_t* __restrict__ ctl_i, const double* __restrict__ part, float* __restrict__ centers,
                                 float* __restrict__ stds, int64_t* __restrict__ counts, double* __restrict__ rot, int32_t nbs,
                                 double* s_m) {
    if (blockIdx.y) {  // a batch of trajectories (midas_loop_step_batch): LOOP_MAX_CLUSTERS rows of everything per trajectory
        const size_t b = blockIdx.y;
        ctl_i += b * LOOP_CTL_I; part += b * (size_t)nbs * LOOP_MAX_CLUSTERS * CL_MOM;
        centers += b * LOOP_MAX_CLUSTERS * 16; stds += b * LOOP_MAX_CLUSTERS * 3; counts += b * LOOP_MAX_CLUSTERS;
        rot += b * LOOP_MAX_CLUSTERS * 10;
    }
    const int64_t n = ctl_i[LOOP_I_N];
    int C = ctl_i[LOOP_I_NCL] + 1;
    C = C > LOOP_MAX_CLUSTERS ? LOOP_MAX_CLUSTERS : C;
    if ((int)blockIdx.x >= C) return;
    cluster_finish_body<FORM>((int)((n + 255) / 256), (size_t)nbs, blockIdx.x, part, centers, stds, counts, s_m, rot);
}
__global__ __launch_bounds__(256) void k_loop_cluster_finish(const int32_t* __restrict__ ctl_i, const double* __restrict__ part,
                                                            float* __restrict__ centers, float* __restrict__ stds,
                                                            int64_t* __restrict__ counts, double* __restrict__ rot, int32_t nbs) {
    __shared__ double s_m[CL_MOM];
    loop_cluster_finish_body<CL_FORM_QUAT>(ctl_i, part, centers, stds, counts, rot, nbs, s_m);
}
// The log-map form writes the whole centre (`rot` is not touched, and the annealing kernels are launched without the workgroup
// that solves the quaternion rotation: launch_loop_decide, launch_anneal_small).  What that workgroup also did - place the
// rotation in the COMPACT row of the cluster, the row loop_decide gives it among the labels present - is the second kernel's:
// thread c of trajectory blockIdx.y copies slot c's nine entries; the decision writes the other seven of the row.
__global__ __launch_bounds__(256) void k_loop_cluster_finish_logmap(const int32_t* __restrict__ ctl_i, const double* __restrict__ part,
                                                                   float* __restrict__ centers, float* __restrict__ stds,
                                                                   int64_t* __restrict__ counts, double* __restrict__ rot, int32_t nbs) {
    __shared__ double s_m[CL_MOM];
    loop_cluster_finish_body<CL_FORM_LOGMAP>(ctl_i, part, centers, stds, counts, rot, nbs, s_m);
}
__global__ __launch_bounds__(LOOP_MAX_CLUSTERS) void k_loop_logmap_rotations(const int32_t* __restrict__ ctl_i,
                                                                             const float* __restrict__ centers_all,
                                                                             const int64_t* __restrict__ counts_all,
                                                                             float* __restrict__ centers_out) {
    const size_t b = blockIdx.x;
    ctl_i += b * LOOP_CTL_I; centers_all += b * LOOP_MAX_CLUSTERS * 16; counts_all += b * LOOP_MAX_CLUSTERS;
    centers_out += b * LOOP_MAX_CLUSTERS * 16;
    int C = ctl_i[LOOP_I_NCL] + 1;
    C = C > LOOP_MAX_CLUSTERS ? LOOP_MAX_CLUSTERS : C;
    const int c = threadIdx.x;
    if (c >= C || counts_all[c] == 0) return;
    int np = 0;
    for (int j = 0; j < c; ++j) np += counts_all[j] != 0 ? 1 : 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) centers_out[np * 16 + i * 4 + j] = centers_all[c * 16 + i * 4 + j];
}

// ---- fixed-N engines: the pose estimate of a frame, B trajectories at once (midas_pose_estimate) ----------------------------
// filter.py:184-186 takes get_cluster_centers of a particle set nobody has clustered (labels all 0, particle_filter.py:47):
// every particle of trajectory b = blockIdx.y is a member of its one cluster.  part[(b * nbs + block) * CL_MOM + m] - the layout
// cluster_finish_body walks with "cluster" = trajectory; contribution, wave tree, waves in order and blocks in order are
// moments_accumulate's (a workgroup always holds a member, so nothing is ever skipped): the bits of midas_cluster_centers on
// trajectory b alone.  Two weight sources:
//   w64     B x N masked pre-resample weights (what the eager engines hold);
//   tables  the pipelined frame's table blocks (tables_of, api_entry.hpp), tstride doubles apart: the weight k_tail_b2 would write
//           (tail.hip, a.weights[i]) is formed here - guard and S by every workgroup for itself from the at most
//           LAZY_MAX_BLOCKS block records, no flush, no N-sized temporary.
struct EstimateArgs {
    int64_t N;
    const float* poses;                               // B x N x 16
    const double* w64;                                // B x N, or nullptr: from the tables
    const double *e, *x_raw, *bsum_e, *bmax, *bmin;   // trajectory 0's arrays
    int64_t tstride;
    const uint8_t* valid;                             // B x N
    int32_t softmax;
    int32_t nbl;                                      // 4096-slot summation blocks of a trajectory (<= LAZY_MAX_BLOCKS)
    double* part;
};

__global__ __launch_bounds__(256) void k_estimate_moments(EstimateArgs a) {
    __shared__ double s_w[4][CL_MOM];
    __shared__ double s_sum[LAZY_MAX_BLOCKS];
    __shared__ double s_ex[12];
    const int t = threadIdx.x;
    const int64_t N = a.N, b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * 256 + t;
    const bool live = n < N;
    const int64_t nc = live ? n : N - 1;
    MomIn in;
    in.lab = 0;
    moments_load_pose(b * N + nc, a.poses, in);
    if (a.w64) {  // (launch-uniform)
        in.w = (double)(float)a.w64[b * N + nc];  // particles.weights.float() (:161)
    } else {
        // everything that does not depend on the guard is requested first (the softmax variant is the common one)
        const int64_t ts = b * a.tstride;
        const bool has = t < a.nbl;
        const int tb = has ? t : a.nbl - 1;
        const double bs = a.bsum_e[ts + tb], bx = a.bmax[ts + tb], bn = a.bmin[ts + tb];
        double e_i = a.e[ts + nc];
        const bool ok_i = a.valid[b * N + nc] != 0;
        // the guard of k_tail_b2: global extrema of x from the per-block ones, NaN propagates
        const bool nan = has && ((bx != bx) || (bn != bn));
        double mx = has && bx > -INFINITY ? bx : -INFINITY, mn = has && bn < INFINITY ? bn : INFINITY;
        if (has) s_sum[t] = bs;
        mx = cl_wmax(mx);
        mn = cl_wmin(mn);
        const bool wn = __any(nan);
        if ((t & 63) == 0) { s_ex[t >> 6] = mx; s_ex[4 + (t >> 6)] = mn; s_ex[8 + (t >> 6)] = wn ? 1.0 : 0.0; }
        __syncthreads();
        mx = s_ex[0]; mn = s_ex[4];
        double f = s_ex[8];
        for (int w = 1; w < 4; ++w) { mx = s_ex[w] > mx ? s_ex[w] : mx; mn = s_ex[4 + w] < mn ? s_ex[4 + w] : mn; f += s_ex[8 + w]; }
        if (f != 0.0) { mx = NAN; mn = NAN; }
        const bool apply = a.softmax && !(__builtin_fabs(mx - mn) <= ISCLOSE_ATOL);  // (workgroup-uniform)
        double S = 1.0;
        if (apply) {  // the block sums of e one after the other, in block order (the spec)
            S = 0.0;
            for (int i = 0; i < a.nbl; ++i) S = S + s_sum[i];
        } else {      // rare: every particle has the same score, or the softmax is off - the raw variant
            e_i = a.x_raw[ts + nc];
        }
        const double w = (e_i / S) * (ok_i ? 1.0 : 0.0);
        in.w = (double)(float)w;  // particles.weights.float() (:161)
    }
    moments_accumulate(live, in, 1, [](int) { return (int64_t)0; }, a.part + (size_t)b * gridDim.x * CL_MOM, s_w, false);
}

// one 256-thread workgroup per trajectory (k_loop_cluster_finish's shape: a chunk of partials is one batch of loads, the extrema
// walk on the second wave)
__global__ __launch_bounds__(256) void k_estimate_finish(int nblocks, const double* __restrict__ part, float* __restrict__ centers,
                                                        float* __restrict__ stds) {
    __shared__ double s_m[CL_MOM];
    cluster_finish_body(nblocks, (size_t)nblocks, blockIdx.x, part, centers, stds, nullptr, s_m);
}

// ---- sharded engine: the finish over the gathered partials of ALL ranks (midas_shard_estimate_finish) ------------------------
// k_estimate_finish's interface and result on G * ceil(N / 256) blocks - thousands at the sizes the sharded engine is for (3907
// at a million particles).  The additions and their order are cluster_finish_body's (r = block 0's value, then r = r + block b
// for b = 1, 2, ...; the extrema by lanes that take every 64th block and meet in wave_max_dpp / wave_min_dpp; cluster_close), so
// the bits are k_estimate_finish's on the same partials; what differs is who does what.  There every thread loads, stores to LDS
// and meets two barriers a chunk, the walking lanes included; here the chain of dependent float64 additions is the only serial part:
//   wave 0        the 36 lanes that carry the sums: they read the LDS window a batch ahead of the batch they add, nothing else;
//   wave 1        the two extrema (no order), one block a lane and window;
//   waves 2 .. 7  stream the partials (288 bytes a block): wave 2 + k % 6 holds window k in registers from SF_LOADERS windows
//                 ahead and stores it into the half of the double-buffered LDS window the walkers are NOT reading.
// One barrier a window of SF_CB blocks.  A loader's requests have six windows of walking (~384 blocks) to arrive.
constexpr int SF_CB = 64;                         // blocks of one LDS window
constexpr int SF_LOADERS = 6;                     // loader waves
constexpr int SF_LD = SF_CB * CL_MOM / 2 / 64;    // 16-byte loads of a loader lane per window
static_assert(SF_CB == 64, "the extrema wave takes one block a lane and window");
static_assert(ESTIMATE_PART_DOUBLES == CL_MOM, "what the ranks exchange is a block's CL_MOM moments");

typedef double sf_d2 __attribute__((ext_vector_type(2)));  // one 16-byte request
// window k's partials -> registers (every request out before anything waits), and from there into a half of the LDS window
MD void sf_issue(const double* __restrict__ pc, int nblocks, int k, int lane, sf_d2 (&x)[SF_LD]) {
    const int nd2 = (nblocks - k * SF_CB < SF_CB ? nblocks - k * SF_CB : SF_CB) * (CL_MOM / 2);
    const sf_d2* __restrict__ src = reinterpret_cast<const sf_d2*>(pc + (size_t)k * SF_CB * CL_MOM);
#pragma unroll
    for (int j = 0; j < SF_LD; ++j) {
        const int i = lane + 64 * j;
        x[j] = src[i < nd2 ? i : nd2 - 1];
    }
}
MD void sf_store(double* win, int nblocks, int k, int lane, const sf_d2 (&x)[SF_LD]) {
    const int nd2 = (nblocks - k * SF_CB < SF_CB ? nblocks - k * SF_CB : SF_CB) * (CL_MOM / 2);
    sf_d2* dst = reinterpret_cast<sf_d2*>(win);
#pragma unroll
    for (int j = 0; j < SF_LD; ++j) {
        const int i = lane + 64 * j;
        if (i < nd2) dst[i] = x[j];
    }
}

__global__ __launch_bounds__(64 * (2 + SF_LOADERS)) void k_shard_estimate_finish(int nblocks, const double* __restrict__ part,
                                                                                float* __restrict__ centers, float* __restrict__ stds) {
    __shared__ double s_m[CL_MOM];
    __shared__ __attribute__((aligned(16))) double s_win[2][SF_CB * CL_MOM];
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63, lw = wv - 2;
    const int nwin = (nblocks + SF_CB - 1) / SF_CB;
    const double* __restrict__ pc = part + (size_t)blockIdx.x * nblocks * CL_MOM;
    sf_d2 x[SF_LD];
    auto issue = [&](int k) { sf_issue(pc, nblocks, k, lane, x); };
    auto store = [&](int k) { sf_store(s_win[k & 1], nblocks, k, lane, x); };
    if (lw >= 0 && lw < nwin) issue(lw);
    if (lw == 0) {
        store(0);
        if (SF_LOADERS < nwin) issue(SF_LOADERS);
    }
    __syncthreads();
    double r = 0.0, e_mx = -INFINITY, e_mn = INFINITY, e_first_mx = 0.0, e_first_mn = 0.0;
    for (int c = 0; c < nwin; ++c) {
        const int nb = nblocks - c * SF_CB < SF_CB ? nblocks - c * SF_CB : SF_CB;
        const double* b = s_win[c & 1];
        if (wv == 0) {
            // the chain: one dependent addition a block.  Sixteen LDS reads are in flight while the sixteen before them are added;
            // the last, partial batch reads clamped and adds under a wave-uniform count (no read waits inside the chain)
            const double* bm = b + (lane < CL_MOM ? lane : 0);  // (lanes without a moment walk moment 0; nothing of theirs is kept)
            int j = 0;
            if (c == 0) { r = bm[0]; j = 1; }
            double xa[16], xb[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { const int jj = j + i; xa[i] = bm[(jj < nb ? jj : nb - 1) * CL_MOM]; }
            for (; j + 32 <= nb; j += 32) {  // (two batches a trip: the registers swap roles, nothing is copied)
#pragma unroll
                for (int i = 0; i < 16; ++i) { const int jj = j + 16 + i; xb[i] = bm[(jj < nb ? jj : nb - 1) * CL_MOM]; }
#pragma unroll
                for (int i = 0; i < 16; ++i) r = r + xa[i];
#pragma unroll
                for (int i = 0; i < 16; ++i) { const int jj = j + 32 + i; xa[i] = bm[(jj < nb ? jj : nb - 1) * CL_MOM]; }
#pragma unroll
                for (int i = 0; i < 16; ++i) r = r + xb[i];
            }
            if (j + 16 <= nb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) { const int jj = j + 16 + i; xb[i] = bm[(jj < nb ? jj : nb - 1) * CL_MOM]; }
#pragma unroll
                for (int i = 0; i < 16; ++i) r = r + xa[i];
#pragma unroll
                for (int i = 0; i < 16; ++i) xa[i] = xb[i];
                j += 16;
            }
            const int rem = nb - j;
#pragma unroll
            for (int i = 0; i < 15; ++i)
                if (i < rem) r = r + xa[i];
        } else if (wv == 1) {
            // (cluster_finish_body's rule: NaN never wins a select, unless the FIRST block's value is NaN)
            if (c == 0) { e_first_mx = b[M_WMAX]; e_first_mn = b[M_WMIN]; }
            if (lane < nb) {
                const double vx = b[lane * CL_MOM + M_WMAX], vy = b[lane * CL_MOM + M_WMIN];
                e_mx = vx > e_mx ? vx : e_mx;
                e_mn = vy < e_mn ? vy : e_mn;
            }
        } else {
            const int k = c + 1;  // into the half nobody reads during this window
            if (k < nwin && k % SF_LOADERS == lw) {
                store(k);
                if (k + SF_LOADERS < nwin) issue(k + SF_LOADERS);
            }
        }
        __syncthreads();
    }
    if (wv == 1) {
        const double mx = wave_max_dpp(e_mx), mn = wave_min_dpp(e_mn);
        if (lane == 0) {
            s_m[M_WMAX] = e_first_mx != e_first_mx ? e_first_mx : mx;
            s_m[M_WMIN] = e_first_mn != e_first_mn ? e_first_mn : mn;
        }
    } else if (wv == 0 && lane < CL_MOM && lane != M_WMAX && lane != M_WMIN) {
        s_m[lane] = r;
    }
    __syncthreads();
    if (t != 0) return;
    cluster_close(s_m, centers + (size_t)blockIdx.x * 16, stds + (size_t)blockIdx.x * 3, nullptr, nullptr);
}

static bool moments_skip() {  // MIDAS_MOMENTS_SKIP=0: every cluster summed by every workgroup (the parity test's other side)
    static const bool on = !(getenv("MIDAS_MOMENTS_SKIP") && atoi(getenv("MIDAS_MOMENTS_SKIP")) == 0);
    return on;
}

// rot: LOOP_MAX_CLUSTERS x 10 doubles - the moment matrices whose eigenproblem the annealing kernel's second workgroup solves
// (the decision only needs the translation spreads: the eigenvector runs beside the selection)
// logmap (MIDAS_LOOP_CENTERS_LOGMAP): the log-map twins of the same launches - the finisher writes whole centres and `rot` stays
// untouched; their rotations go to the compact rows of centers_out (the frame's cluster_poses) by one small launch
int launch_loop_cluster(midas_ctx* ctx, int64_t cap, const int32_t* ctl_i, const float* poses, const double* w64,
                        const int32_t* labels, double* part, float* centers, float* stds, int64_t* counts, double* rot,
                        const LoopWeightsParamRowsArgs* weights, int32_t B, bool logmap, float* centers_out) {
    const unsigned by = (unsigned)(B > 1 ? B : 1);
    const dim3 grid((unsigned)ceil_div(cap, 256), by);
    const bool skip = moments_skip();
    if (weights && weights->rows) {  // ... with their own filter parameters (midas_loop_step_batch_rows)
        if (logmap) hipLaunchKernelGGL(k_loop_weights_moments_logmap<LoopWeightsParamRowsArgs>, grid, dim3(256), 0, ctx->stream, *weights, labels, part, skip);
        else hipLaunchKernelGGL(k_loop_weights_moments<LoopWeightsParamRowsArgs>, grid, dim3(256), 0, ctx->stream, *weights, labels, part, skip);
    } else if (weights && weights->cb_poses_rows) {  // rows on different objects (midas_loop_step_batch_objects)
        const LoopWeightsRowsArgs& wr = static_cast<const LoopWeightsRowsArgs&>(*weights);
        if (logmap) hipLaunchKernelGGL(k_loop_weights_moments_logmap<LoopWeightsRowsArgs>, grid, dim3(256), 0, ctx->stream, wr, labels, part, skip);
        else hipLaunchKernelGGL(k_loop_weights_moments<LoopWeightsRowsArgs>, grid, dim3(256), 0, ctx->stream, wr, labels, part, skip);
    } else if (weights) {
        const LoopWeightsArgs& wp = static_cast<const LoopWeightsArgs&>(*weights);
        if (logmap) hipLaunchKernelGGL(k_loop_weights_moments_logmap<LoopWeightsArgs>, grid, dim3(256), 0, ctx->stream, wp, labels, part, skip);
        else hipLaunchKernelGGL(k_loop_weights_moments<LoopWeightsArgs>, grid, dim3(256), 0, ctx->stream, wp, labels, part, skip);
    } else {
        if (logmap) hipLaunchKernelGGL(k_loop_cluster_moments_logmap, grid, dim3(256), 0, ctx->stream, ctl_i, poses, w64, labels, part, skip, (int32_t)cap);
        else hipLaunchKernelGGL(k_loop_cluster_moments, grid, dim3(256), 0, ctx->stream, ctl_i, poses, w64, labels, part, skip, (int32_t)cap);
    }
    if (logmap) {
        hipLaunchKernelGGL(k_loop_cluster_finish_logmap, dim3(LOOP_MAX_CLUSTERS, by), dim3(256), 0, ctx->stream, ctl_i, (const double*)part,
                           centers, stds, counts, rot, (int32_t)ceil_div(cap, 256));
        hipLaunchKernelGGL(k_loop_logmap_rotations, dim3(by), dim3(LOOP_MAX_CLUSTERS), 0, ctx->stream, ctl_i, (const float*)centers,
                           (const int64_t*)counts, centers_out);
    } else {
        hipLaunchKernelGGL(k_loop_cluster_finish, dim3(LOOP_MAX_CLUSTERS, by), dim3(256), 0, ctx->stream, ctl_i, (const double*)part, centers,
                           stds, counts, rot, (int32_t)ceil_div(cap, 256));
    }
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_cluster_centers(midas_ctx* ctx, int64_t N, const float* poses, const double* w64, const float* w32,
                           const int64_t* labels, int32_t C, const int64_t* label_values, float* centers, float* stds,
                           int64_t* counts, bool logmap) {
    const int nb = (int)ceil_div(N, 256);
    void* part;
    int rc = midas_scratch(ctx, (size_t)nb * C * CL_MOM * sizeof(double), &part);
    if (rc) return rc;
    if (logmap) {
        hipLaunchKernelGGL(k_cluster_moments_logmap, dim3((unsigned)nb), dim3(256), 0, ctx->stream, N, poses, w64, w32, labels, (int)C,
                           label_values, (double*)part, moments_skip());
        hipLaunchKernelGGL(k_cluster_finish_logmap, dim3((unsigned)C), dim3(64), 0, ctx->stream, nb, (int)C, (const double*)part, centers,
                           stds, counts);
    } else {
        hipLaunchKernelGGL(k_cluster_moments, dim3((unsigned)nb), dim3(256), 0, ctx->stream, N, poses, w64, w32, labels, (int)C,
                           label_values, (double*)part, moments_skip());
        hipLaunchKernelGGL(k_cluster_finish, dim3((unsigned)C), dim3(64), 0, ctx->stream, nb, (int)C, (const double*)part, centers,
                           stds, counts);
    }
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_se3_log(midas_ctx* ctx, int64_t N, const float* poses, double* xi) {
    hipLaunchKernelGGL(k_se3_log, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, poses, xi);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_pose_estimate(midas_ctx* ctx, int64_t N, int32_t B, const float* poses, const double* w64, const TailTables* tb,
                         int64_t tstride, const uint8_t* valid, int32_t softmax, float* centers, float* stds) {
    const int nb = (int)ceil_div(N, 256);
    void* part;
    int rc = midas_scratch(ctx, (size_t)B * nb * CL_MOM * sizeof(double), &part);
    if (rc) return rc;
    EstimateArgs a;
    a.N = N; a.poses = poses; a.w64 = w64;
    a.e = a.x_raw = a.bsum_e = a.bmax = a.bmin = nullptr;
    if (tb) { a.e = tb->e; a.x_raw = tb->x_raw; a.bsum_e = tb->bsum_e; a.bmax = tb->bmax; a.bmin = tb->bmin; }
    a.tstride = tstride; a.valid = valid; a.softmax = softmax; a.nbl = (int32_t)ceil_div(N, SCAN_BLOCK);
    a.part = (double*)part;
    hipLaunchKernelGGL(k_estimate_moments, dim3((unsigned)nb, (unsigned)B), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_estimate_finish, dim3((unsigned)B), dim3(256), 0, ctx->stream, nb, (const double*)part, centers, stds);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

// sharded engine: the moment partials of this rank's blocks into a caller-owned buffer (it is exchanged), from the eager weights
int launch_shard_estimate_moments(midas_ctx* ctx, int64_t N, const float* poses, const double* w64, double* part) {
    EstimateArgs a;
    a.N = N; a.poses = poses; a.w64 = w64;
    a.e = a.x_raw = a.bsum_e = a.bmax = a.bmin = nullptr;
    a.tstride = 0; a.valid = nullptr; a.softmax = 0; a.nbl = 0;
    a.part = part;
    hipLaunchKernelGGL(k_estimate_moments, dim3((unsigned)ceil_div(N, 256), 1), dim3(256), 0, ctx->stream, a);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_shard_estimate_finish(midas_ctx* ctx, int64_t nblocks, const double* part_all, float* center, float* stds) {
    hipLaunchKernelGGL(k_shard_estimate_finish, dim3(1), dim3(64 * (2 + SF_LOADERS)), 0, ctx->stream, (int)nblocks, part_all, center, stds);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

MIDAS_WARM_TU(cluster, k_cluster_moments)

}  // namespace midas
