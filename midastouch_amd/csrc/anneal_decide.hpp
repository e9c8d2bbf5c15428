// anneal_decide.hpp - what the two annealing units of a loop frame share on the device: the multi-launch form (anneal.hip) and the
// single-workgroup form for sets up to LOOP_SMALL_MAX (anneal_small.hip) take the same decision (loop_decide, with the centres'
// rotations by a second workgroup: loop_rotations) and select on the same keys in the same order (weight_key, pair_less).
#pragma once
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "cluster_rot.hpp"

namespace midas {

constexpr int SEL_PASSES = 6;
constexpr int SEL_BINS = 2048;
constexpr int SEL_HIST_WORDS = SEL_PASSES * SEL_BINS, SEL_STATE_WORDS = 4 * (SEL_PASSES + 2);  // one trajectory's select state
// the single-workgroup form: particles it takes (the caller bounds the live count), duplicates it sorts in LDS
constexpr int LOOP_SMALL_MAX = 16384, LOOP_SMALL_PAIRS = 8192;
static_assert(LOOP_SMALL_MAX == MIDAS_LOOP_BATCH_MAX_CAP, "midas_loop_step_batch runs this regime's kernels");
static_assert((MIDAS_LOOP_BATCH_WIDE_MAX_CAP + SCAN_BLOCK - 1) / SCAN_BLOCK <= LAZY_MAX_BLOCKS, "k_loop_compact stages a trajectory's block counts in LDS");

// Order-preserving 64-bit key of a weight: a < b <=> key(a) < key(b); -0.0 == +0.0; NaN above everything (torch.topk
// treats NaN as the largest value).
MD uint64_t weight_key(double w) {
    if (w == 0.0) w = 0.0;  // -0.0 -> +0.0
    if (w != w) return ~0ull;
    const uint64_t b = (uint64_t)__double_as_longlong(w);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the order of the duplicates, (key, index) pairs with key = ~weight_key: weight descending, ties by index - torch.topk's sorted output
MD bool pair_less(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) { return ka < kb || (ka == kb && ia < ib); }

// torch.sum of n < 512 contiguous float32 values in the order ATen's CPU kernel adds them (SumKernel.cpp, the AVX2 build: 8 lanes):
// whole vectors into four interleaved vector accumulators (row_sum, ilp 4; below the cascade's first carry), leftover vectors into
// the first, the four added 0 + 1 + 2 + 3; then the scalar tail in order, then the 8 lanes in order.  Fewer than 8 values: the same
// row_sum on scalars.  A running sum differs from it in the last bit from 6 values - two clusters - on (oracle.aten_sum_f32).
MD float aten_sum_f32(const float* __restrict__ x, int n) {
    constexpr int V = 8, ILP = 4;
    const int vs = n / V;
    if (vs == 0) {
        float a[ILP] = {0.f, 0.f, 0.f, 0.f};
        const int g = n / ILP;
        for (int i = 0; i < g; ++i)
#pragma unroll
            for (int k = 0; k < ILP; ++k) a[k] = a[k] + x[i * ILP + k];
        for (int i = g * ILP; i < n; ++i) a[0] = a[0] + x[i];
        return ((a[0] + a[1]) + a[2]) + a[3];
    }
    float acc[ILP][V];
#pragma unroll
    for (int k = 0; k < ILP; ++k)
#pragma unroll
        for (int l = 0; l < V; ++l) acc[k][l] = 0.f;
    const int g = vs / ILP;
    for (int i = 0; i < g; ++i)
#pragma unroll
        for (int k = 0; k < ILP; ++k)
#pragma unroll
            for (int l = 0; l < V; ++l) acc[k][l] = acc[k][l] + x[(i * ILP + k) * V + l];
    for (int i = g * ILP; i < vs; ++i)
#pragma unroll
        for (int l = 0; l < V; ++l) acc[0][l] = acc[0][l] + x[i * V + l];
    float fin = 0.f;
    for (int j = vs * V; j < n; ++j) fin = fin + x[j];
#pragma unroll
    for (int l = 0; l < V; ++l) fin = fin + (((acc[0][l] + acc[1][l]) + acc[2][l]) + acc[3][l]);
    return fin;
}

// Python's int(x) of a float32 x >= 0 in front of a min(.., cap - 1): the truncation where it fits, `cap` from there on (and for +inf).
// The reference's int is unbounded, so a product of 2^31 and more - a tiny previous spread - still ends at the cap of its min; a bare
// (int)x is undefined there.  Every x below cap converts as before; NaN does not get here (neither branch of the rule takes it).
MD int trunc_capped(float x, int cap) { return x >= (float)cap ? cap : (int)x; }

// One workgroup: the clusters present (labels ascending) -> compact rows, var = float32 sum of their stds / count
// (torch.mean(cluster_stds), filter.py:189; a running sum, or ATen's order: loop_decide), then particle_filter.annealing's rule (:413-447) in the float32 arithmetic torch
// uses for `var / self.particle_var`, `1.0 - ratio` and `* N`.  Also clears the select histograms.
// (one thread) -> {mode, k}
// aten_order: var as torch.mean adds it on the CPU (the reference's own bits: with MIDAS_TOPK_TIES_ATEN_CPU, the mode that replays
// a CPU run), else the running sum (ties by index - torch's CUDA rule, whose reduction order is not modelled).
MD void loop_decide(int32_t* __restrict__ ctl_i, double* __restrict__ ctl_d, const float* __restrict__ centers_all,
                    const float* __restrict__ stds_all, const int64_t* __restrict__ counts_all, float* __restrict__ centers_out,
                    float* __restrict__ stds_out, int32_t floor_n, int& mode_out, int& k_out, bool aten_order = false) {
    const int32_t n = ctl_i[LOOP_I_N];
    int C = ctl_i[LOOP_I_NCL] + 1;
    if (C > LOOP_MAX_CLUSTERS) { C = LOOP_MAX_CLUSTERS; ctl_i[LOOP_I_ERR] |= 1; }
    int np = 0;
    float sum = 0.f;
    for (int c = 0; c < C; ++c) {
        if (counts_all[c] == 0) continue;
        // the translation and the bottom row; the rotation entries of the row come from loop_rotations (second workgroup)
        for (int i = 3; i < 12; i += 4) centers_out[np * 16 + i] = centers_all[c * 16 + i];
        for (int i = 12; i < 16; ++i) centers_out[np * 16 + i] = centers_all[c * 16 + i];
        for (int i = 0; i < 3; ++i) {
            const float s = stds_all[c * 3 + i];
            stds_out[np * 3 + i] = s;
            sum = sum + s;
        }
        ++np;
    }
    if (aten_order) sum = aten_sum_f32(stds_out, 3 * np);  // (the compact rows this thread has just written)
    const float var = sum / (float)(3 * np);
    ctl_i[LOOP_I_NPRES] = np;
    ctl_d[LOOP_D_VAR] = (double)var;
    int mode = 0, k = 0;
    if (!ctl_i[LOOP_I_VARSET]) {  // first call: remember the variance and the particle count (:413-417)
        ctl_d[LOOP_D_VARPREV] = (double)var;
        ctl_i[LOOP_I_INIT] = n;
        ctl_i[LOOP_I_VARSET] = 1;
    } else if (var == 0.0f) {     // converged to a single pose (:418-420)
    } else {
        const float prev = (float)ctl_d[LOOP_D_VARPREV];
        const float ratio = var / prev;
        ctl_d[LOOP_D_VARPREV] = (double)var;
        if (ratio < 1.0f) {
            const int a = trunc_capped((1.0f - ratio) * (float)n, n / 3 + 1);
            const int b = n - floor_n < 0 ? floor_n - n : n - floor_n;
            k = a < b ? a : b;
            k = k < n / 3 ? k : n / 3;
            mode = k > 0 ? 1 : 0;
        } else if (ratio > 1.0f) {
            const int a = trunc_capped((ratio - 1.0f) * (float)n, n / 3 + 1);
            k = a < n / 3 ? a : n / 3;
            mode = (k + n > ctl_i[LOOP_I_INIT] || k <= 0) ? 0 : 2;
        }
        if (!mode) k = 0;
    }
    ctl_i[LOOP_I_MODE] = mode;
    ctl_i[LOOP_I_K] = k;
    ctl_i[LOOP_I_NSET] = mode == 1 ? n - k : mode == 2 ? n + k : n;
    mode_out = mode;
    k_out = k;
}

// Second workgroup of the annealing kernels: the rotation of every present cluster's centre (top eigenvector of the moment
// matrix k_loop_cluster_finish left in `rot`), written into the compact row loop_decide gives the cluster - the selection
// does not wait for it.  Lane c < 8 of one wave takes cluster slot c.
MD void loop_rotations(const int32_t* __restrict__ ctl_i, const int64_t* __restrict__ counts_all, const double* __restrict__ rot,
                       float* __restrict__ centers_out) {
    int C = ctl_i[LOOP_I_NCL] + 1;
    C = C > LOOP_MAX_CLUSTERS ? LOOP_MAX_CLUSTERS : C;
    const int c = threadIdx.x;
    if (c >= C || counts_all[c] == 0) return;
    int np = 0;
    for (int j = 0; j < c; ++j) np += counts_all[j] != 0 ? 1 : 0;
    double A10[10];
    for (int k = 0; k < 10; ++k) A10[k] = rot[(size_t)c * 10 + k];
    cluster_rotation_write(A10, centers_out + np * 16);
}

}  // namespace midas
