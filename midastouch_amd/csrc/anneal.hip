// anneal.hip - ANNEAL of a loop frame (loop.hip) behind the clusters' moments, the multi-launch form: k_loop_decide (labels present,
// var = mean(stds), particle_filter.annealing's rule in float32 as torch evaluates it: anneal_decide.hpp; the kernel itself has to
// compile beside k_loop_anneal_small and is launched through anneal_small.hip's launch_loop_decide) -> k_loop_select x 6 (radix
// select of the k-th smallest / largest weight, 11-bit digits of the order-preserving 64-bit key) -> k_loop_compact_count /
// k_loop_compact (the annealed set as an index list: survivors in their order, or everybody + the k best) -> k_loop_sort_chunks /
// k_loop_sort_rank (the duplicates in topk's output order: weight descending, index ascending).  loop_anneal_phase, at the end, is the
// one place a frame's annealing is launched from, in any of its four regimes (LoopAnneal); launch_anneal_select is the selection alone
// on a plan made by the host (midas_anneal_select).
#include <cstdlib>

#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "anneal_decide.hpp"

namespace midas {

constexpr int SORT_CHUNK = 2048;  // (key, index) pairs sorted per workgroup in LDS
__device__ const int kSelShift[SEL_PASSES] = {53, 42, 31, 20, 9, 0};
__device__ const int kSelWidth[SEL_PASSES] = {11, 11, 11, 11, 11, 9};

// MIDAS_TOPK_TIES_ATEN_CPU (a replay of the reference's bits): the clusters' spreads once more, as the two-pass form of the spec -
// sqrt(sum w (t - m)^2 / sum w) about the float32 centre m k_loop_cluster_finish wrote, differences first - in place of the closed
// form on the moments (cluster_close), which cancels: where the members of a cluster coincide (a drifted frame puts every particle
// on a codebook pose) the spread is 0 and the closed form leaves ~1e-9, enough to move var by one float32 step.  Workgroup c takes
// label c - 1: its threads walk the particles with stride 256, the partial sums meet in a fixed tree.  Weights: the float32 values,
// or 1 when isclose(max - min, 0) (particle_filter.py:161-167), as cluster_close decides it.
__global__ __launch_bounds__(256) void k_loop_std_two_pass(const int32_t* __restrict__ ctl_i, const float* __restrict__ poses,
                                                           const double* __restrict__ w64, const int32_t* __restrict__ labels,
                                                           const float* __restrict__ centers, float* __restrict__ stds,
                                                           const int64_t* __restrict__ counts, int64_t cap) {
    __shared__ double s_r[4][256];
    __shared__ float s_x[2][256];
    if (blockIdx.y) {  // a batch of trajectories: `cap` particles and LOOP_MAX_CLUSTERS cluster rows each
        const int64_t b = blockIdx.y, o = b * cap;
        ctl_i += b * LOOP_CTL_I; poses += o * 16; w64 += o; labels += o;
        centers += b * LOOP_MAX_CLUSTERS * 16; stds += b * LOOP_MAX_CLUSTERS * 3; counts += b * LOOP_MAX_CLUSTERS;
    }
    const int c = blockIdx.x, t = threadIdx.x;
    int C = ctl_i[LOOP_I_NCL] + 1;
    C = C > LOOP_MAX_CLUSTERS ? LOOP_MAX_CLUSTERS : C;
    if (c >= C || counts[c] == 0) return;  // (uniform over the workgroup)
    int64_t n = ctl_i[LOOP_I_N];
    n = n < cap ? n : cap;
    const int32_t lab = c - 1;
    float wmax = -INFINITY, wmin = INFINITY;
    for (int64_t i = t; i < n; i += 256) {
        if (labels[i] != lab) continue;
        const float w = (float)w64[i];
        wmax = w > wmax ? w : wmax;
        wmin = w < wmin ? w : wmin;
    }
    s_x[0][t] = wmax; s_x[1][t] = wmin;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
            s_x[0][t] = s_x[0][t + h] > s_x[0][t] ? s_x[0][t + h] : s_x[0][t];
            s_x[1][t] = s_x[1][t + h] < s_x[1][t] ? s_x[1][t + h] : s_x[1][t];
        }
        __syncthreads();
    }
    const bool flat = __builtin_fabsf(s_x[0][0] - s_x[1][0]) <= 1e-8f;
    const double m0 = (double)centers[c * 16 + 3], m1 = (double)centers[c * 16 + 7], m2 = (double)centers[c * 16 + 11];
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t i = t; i < n; i += 256) {
        if (labels[i] != lab) continue;
        const double w = flat ? 1.0 : (double)(float)w64[i];
        const double d0 = (double)poses[i * 16 + 3] - m0, d1 = (double)poses[i * 16 + 7] - m1, d2 = (double)poses[i * 16 + 11] - m2;
        sw = sw + w;
        s0 = s0 + (d0 * d0) * w; s1 = s1 + (d1 * d1) * w; s2 = s2 + (d2 * d2) * w;
    }
    s_r[0][t] = sw; s_r[1][t] = s0; s_r[2][t] = s1; s_r[3][t] = s2;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s_r[k][t] = s_r[k][t] + s_r[k][t + h];
        }
        __syncthreads();
    }
    if (t < 3) stds[c * 3 + t] = (float)__builtin_sqrt(s_r[1 + t][0] / s_r[0][0]);
}

// ANNEAL under the ATen tie rule: the spreads in the two-pass form, behind the moments and in front of the decision
static void loop_std_two_pass(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, const LoopMoments& m) {
    hipLaunchKernelGGL(k_loop_std_two_pass, dim3(LOOP_MAX_CLUSTERS, g.by()), dim3(256), 0, ctx->stream, (const int32_t*)s.ctl_i_dev,
                       (const float*)s.poses_prop_dev, (const double*)s.weights_dev, (const int32_t*)s.labels_dev, (const float*)m.cen, m.sd,
                       (const int64_t*)m.cnt, (int64_t)s.cap);
}

// the selection key of particle i: ascending for a removal (k smallest weights), complemented for a duplication (k largest)
MD uint64_t select_key(const double* __restrict__ w, int64_t i, int mode) {
    const uint64_t key = weight_key(w[i]);
    return mode == 2 ? ~key : key;
}

// (prefix, rank) of pass p from the histogram of pass p - 1 and its own (prefix, rank); every workgroup computes it for
// itself, workgroup 0 also publishes it for the next pass.  state[4 * p + {0, 1, 2}] = prefix hi, prefix lo, rank.
MD void select_advance(const uint32_t* __restrict__ hist, int32_t* __restrict__ state, int p, uint64_t& prefix, int& krem,
                       int* s_scan) {
    const int t = threadIdx.x;
    prefix = ((uint64_t)(uint32_t)state[4 * (p - 1)] << 32) | (uint32_t)state[4 * (p - 1) + 1];
    krem = state[4 * (p - 1) + 2];
    const uint32_t* h = hist + (size_t)(p - 1) * SEL_BINS;
    // 2048 bins, 8 per thread: the bin in which the running count reaches the rank
    uint32_t c[8];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { c[j] = h[t * 8 + j]; mine += (int)c[j]; }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if ((t & 63) >= o) incl += v;
    }
    if ((t & 63) == 63) s_scan[t >> 6] = incl;
    __syncthreads();
    int before = incl - mine;
    for (int w = 0; w < (t >> 6); ++w) before += s_scan[w];
    __syncthreads();
    if (krem > before && krem <= before + mine) {  // exactly one thread
        int run = before, d = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (krem > run && krem <= run + (int)c[j]) { d = j; break; }
            run += (int)c[j];
        }
        s_scan[4] = t * 8 + d;
        s_scan[5] = krem - run;
    }
    __syncthreads();
    const int digit = s_scan[4];
    krem = s_scan[5];
    prefix = (prefix << kSelWidth[p - 1]) | (uint64_t)digit;
    __syncthreads();
    if (blockIdx.x == 0 && t == 0) {
        state[4 * p] = (int32_t)(uint32_t)(prefix >> 32);
        state[4 * p + 1] = (int32_t)(uint32_t)prefix;
        state[4 * p + 2] = krem;
    }
}

// pass P of the radix select: histogram of digit P over the particles whose key starts with the prefix found so far
template <int P>
__global__ __launch_bounds__(256) void k_loop_select(const int32_t* __restrict__ ctl_i, const double* __restrict__ w,
                                                     uint32_t* __restrict__ hist, int32_t* __restrict__ state, int32_t cap = 0) {
    __shared__ uint32_t s_h[SEL_BINS];
    __shared__ int s_scan[8];
    if (blockIdx.y) {  // a batch of trajectories (midas_loop_step_batch_wide): `cap` weights, its own histograms and state each
        const int64_t b = blockIdx.y;
        ctl_i += b * LOOP_CTL_I; w += b * cap; hist += b * SEL_HIST_WORDS; state += b * SEL_STATE_WORDS;
    }
    const int mode = ctl_i[LOOP_I_MODE];
    if (!mode) return;
    const int64_t n = ctl_i[LOOP_I_N];
    const int64_t bbase = (int64_t)blockIdx.x * SCAN_BLOCK;
    if (bbase >= n && blockIdx.x != 0) return;
    const int t = threadIdx.x;
    uint64_t prefix = 0;
    int krem = 0;
    if (P > 0) select_advance(hist, state, P, prefix, krem, s_scan);
    if (bbase >= n) return;
    for (int i = t; i < SEL_BINS; i += 256) s_h[i] = 0u;
    __syncthreads();
    const int shift = kSelShift[P], width = kSelWidth[P];
#pragma unroll 4
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = bbase + (int64_t)j * 256 + t;
        if (i < n) {
            const uint64_t key = select_key(w, i, mode);
            const bool match = P == 0 || (key >> (shift + width)) == prefix;
            if (match) atomicAdd(&s_h[(uint32_t)(key >> shift) & ((1u << width) - 1u)], 1u);
        }
    }
    __syncthreads();
    uint32_t* h = hist + (size_t)P * SEL_BINS;
    for (int i = t; i < SEL_BINS; i += 256)
        if (s_h[i]) atomicAdd(&h[i], s_h[i]);
}

// per 4096-slot block: particles whose key is below the threshold key, and equal to it
__global__ __launch_bounds__(256) void k_loop_compact_count(const int32_t* __restrict__ ctl_i, const double* __restrict__ w,
                                                            const uint32_t* __restrict__ hist, int32_t* __restrict__ state,
                                                            int32_t* __restrict__ c_less, int32_t* __restrict__ c_eq, int32_t cap = 0) {
    __shared__ int s_scan[8];
    __shared__ int s_a[4], s_b[4];
    if (blockIdx.y) {  // a batch of trajectories: `cap` weights, a launch's block counts, its own histograms and state each
        const int64_t b = blockIdx.y, ob = b * gridDim.x;
        ctl_i += b * LOOP_CTL_I; w += b * cap; hist += b * SEL_HIST_WORDS; state += b * SEL_STATE_WORDS; c_less += ob; c_eq += ob;
    }
    const int mode = ctl_i[LOOP_I_MODE];
    if (!mode) return;
    const int64_t n = ctl_i[LOOP_I_N];
    const int64_t bbase = (int64_t)blockIdx.x * SCAN_BLOCK;
    if (bbase >= n && blockIdx.x != 0) return;
    const int t = threadIdx.x;
    uint64_t T;
    int r;
    select_advance(hist, state, SEL_PASSES, T, r, s_scan);
    if (bbase >= n) return;
    int less = 0, eq = 0;
#pragma unroll 4
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = bbase + (int64_t)j * 256 + t;
        if (i < n) {
            const uint64_t key = select_key(w, i, mode);
            less += key < T ? 1 : 0;
            eq += key == T ? 1 : 0;
        }
    }
    less = wave_isum_dpp(less);
    eq = wave_isum_dpp(eq);
    if ((t & 63) == 0) { s_a[t >> 6] = less; s_b[t >> 6] = eq; }
    __syncthreads();
    if (t == 0) {
        c_less[blockIdx.x] = (s_a[0] + s_a[1]) + (s_a[2] + s_a[3]);
        c_eq[blockIdx.x] = (s_b[0] + s_b[1]) + (s_b[2] + s_b[3]);
    }
}

// The annealed set as an index list.  Selected = key < T, or key == T among the first r such particles in index order.
// Removal: src = the unselected particles in their order.  Duplication: src[0, n) = identity, the selected particles go to
// (sel_key, sel_idx) in index order and are put into topk's output order by the two sort kernels.
__global__ __launch_bounds__(256) void k_loop_compact(const int32_t* __restrict__ ctl_i, const double* __restrict__ w,
                                                      const int32_t* __restrict__ state, const int32_t* __restrict__ c_less,
                                                      const int32_t* __restrict__ c_eq, int32_t* __restrict__ src,
                                                      uint64_t* __restrict__ sel_key, int32_t* __restrict__ sel_idx, int32_t cap = 0,
                                                      int32_t ksel = 0) {
    __shared__ int s_l[LAZY_MAX_BLOCKS], s_e[LAZY_MAX_BLOCKS];
    __shared__ int s_wl[4], s_we[4];
    if (blockIdx.y) {  // a batch of trajectories: `cap` weights and sources, `ksel` pairs, a launch's block counts, its own state each
        const int64_t b = blockIdx.y, o = b * cap, ob = b * gridDim.x, ok = b * ksel;
        ctl_i += b * LOOP_CTL_I; w += o; src += o; state += b * SEL_STATE_WORDS; c_less += ob; c_eq += ob; sel_key += ok; sel_idx += ok;
    }
    const int mode = ctl_i[LOOP_I_MODE];
    const int64_t n = ctl_i[LOOP_I_N];
    const int blk = blockIdx.x, t = threadIdx.x;
    const int64_t bbase = (int64_t)blk * SCAN_BLOCK;
    if (bbase >= n) return;
    const int64_t base = bbase + (int64_t)t * SCAN_CHUNK;
    if (!mode) {  // no annealing this frame: the identity
#pragma unroll 4
        for (int j = 0; j < SCAN_CHUNK; ++j) {
            const int64_t i = bbase + (int64_t)j * 256 + t;
            if (i < n) src[i] = (int32_t)i;
        }
        return;
    }
    const uint64_t T = ((uint64_t)(uint32_t)state[4 * SEL_PASSES] << 32) | (uint32_t)state[4 * SEL_PASSES + 1];
    const int r = state[4 * SEL_PASSES + 2];
    for (int i = t; i < blk; i += 256) { s_l[i] = c_less[i]; s_e[i] = c_eq[i]; }
    __syncthreads();
    int less_before = 0, eq_before = 0;
    for (int i = 0; i < blk; ++i) { less_before += s_l[i]; eq_before += s_e[i]; }
    // chunk-per-thread view: flags of the own 16 slots, exclusive counts inside the block
    unsigned lbits = 0, ebits = 0;
    uint64_t keys[SCAN_CHUNK];
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = base + j;
        const bool in = i < n;
        keys[j] = select_key(w, in ? i : n - 1, mode);
        lbits |= (in && keys[j] < T) ? (1u << j) : 0u;
        ebits |= (in && keys[j] == T) ? (1u << j) : 0u;
    }
    const int ml = __popc(lbits), me = __popc(ebits);
    int il = ml, ie = me;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(il, o), b = __shfl_up(ie, o);
        if ((t & 63) >= o) { il += a; ie += b; }
    }
    if ((t & 63) == 63) { s_wl[t >> 6] = il; s_we[t >> 6] = ie; }
    __syncthreads();
    int lb = less_before + il - ml, eb = eq_before + ie - me;
    for (int wv = 0; wv < (t >> 6); ++wv) { lb += s_wl[wv]; eb += s_we[wv]; }
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = base + j;
        if (i >= n) break;
        const bool isl = (lbits >> j) & 1u, ise = (ebits >> j) & 1u;
        const int taken_eq = eb < r ? eb : r;          // equal keys before i that were selected
        const bool selected = isl || (ise && eb < r);
        const int sel_before = lb + taken_eq;
        if (mode == 1) {
            if (!selected) src[i - sel_before] = (int32_t)i;
        } else {
            src[i] = (int32_t)i;
            if (selected) { sel_key[sel_before] = keys[j]; sel_idx[sel_before] = (int32_t)i; }
        }
        lb += isl ? 1 : 0;
        eb += ise ? 1 : 0;
    }
}

// Duplication only: the k selected (key, index) pairs, key = ~weight_key (ascending = weight descending), are sorted by
// (key, index) - torch.topk's sorted output with ties by index (pair_less).  Chunks of 2048 pairs by a bitonic network in LDS ...
__global__ __launch_bounds__(1024) void k_loop_sort_chunks(const int32_t* __restrict__ ctl_i, const uint64_t* __restrict__ key_in,
                                                          const int32_t* __restrict__ idx_in, uint64_t* __restrict__ key_out,
                                                          int32_t* __restrict__ idx_out, int32_t ksel = 0) {
    __shared__ uint64_t s_k[SORT_CHUNK];
    __shared__ int32_t s_i[SORT_CHUNK];
    if (blockIdx.y) {  // a batch of trajectories: `ksel` pairs in and out each
        const int64_t b = blockIdx.y, ok = b * ksel;
        ctl_i += b * LOOP_CTL_I; key_in += ok; idx_in += ok; key_out += ok; idx_out += ok;
    }
    if (ctl_i[LOOP_I_MODE] != 2) return;
    const int k = ctl_i[LOOP_I_K];
    const int c0 = blockIdx.x * SORT_CHUNK;
    if (c0 >= k) return;
    const int t = threadIdx.x;
    for (int i = t; i < SORT_CHUNK; i += 1024) {
        const bool in = c0 + i < k;
        s_k[i] = in ? key_in[c0 + i] : ~0ull;
        s_i[i] = in ? idx_in[c0 + i] : 0x7fffffff;  // padding sorts behind every real pair
    }
    __syncthreads();
    for (int size = 2; size <= SORT_CHUNK; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int p = t; p < SORT_CHUNK / 2; p += 1024) {
                const int lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t ka = s_k[lo], kb = s_k[hi];
                const int32_t ia = s_i[lo], ib = s_i[hi];
                const bool swap = up ? pair_less(kb, ib, ka, ia) : pair_less(ka, ia, kb, ib);
                if (swap) { s_k[lo] = kb; s_k[hi] = ka; s_i[lo] = ib; s_i[hi] = ia; }
            }
            __syncthreads();
        }
    }
    for (int i = t; i < SORT_CHUNK; i += 1024)
        if (c0 + i < k) { key_out[c0 + i] = s_k[i]; idx_out[c0 + i] = s_i[i]; }
}

// ... then every pair finds its rank: its place in its own chunk plus, by binary search, the pairs of every other chunk
// that precede it (all pairs are distinct).  src[n + rank] = index.
__global__ __launch_bounds__(256) void k_loop_sort_rank(const int32_t* __restrict__ ctl_i, const uint64_t* __restrict__ key_s,
                                                        const int32_t* __restrict__ idx_s, int32_t* __restrict__ src, int32_t cap = 0,
                                                        int32_t ksel = 0) {
    if (blockIdx.y) {  // a batch of trajectories: `ksel` sorted pairs and `cap` sources each
        const int64_t b = blockIdx.y, ok = b * ksel;
        ctl_i += b * LOOP_CTL_I; key_s += ok; idx_s += ok; src += b * cap;
    }
    if (ctl_i[LOOP_I_MODE] != 2) return;
    const int k = ctl_i[LOOP_I_K];
    const int64_t n = ctl_i[LOOP_I_N];
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= k) return;
    const uint64_t key = key_s[q];
    const int32_t idx = idx_s[q];
    const int own = q / SORT_CHUNK, nch = (k + SORT_CHUNK - 1) / SORT_CHUNK;
    int rank = q - own * SORT_CHUNK;
    for (int c = 0; c < nch; ++c) {
        if (c == own) continue;
        int lo = c * SORT_CHUNK, hi = lo + SORT_CHUNK < k ? lo + SORT_CHUNK : k;
        const int c0 = lo;
        while (hi > lo) {
            const int mid = lo + ((hi - lo) >> 1);
            if (pair_less(key_s[mid], idx_s[mid], key, idx)) lo = mid + 1; else hi = mid;
        }
        rank += lo - c0;
    }
    src[n + rank] = idx;
}

struct SelectScratch {
    uint32_t* hist;
    int32_t *state, *c_less, *c_eq, *sel_idx, *srt_idx;
    uint64_t *sel_key, *srt_key;
    size_t ksel;
};

// B trajectories: every array (B, ...) contiguous - SEL_HIST_WORDS, SEL_STATE_WORDS, the block counts of a launch over `cap`, ksel pairs
static int select_scratch(midas_ctx* ctx, int64_t cap, SelectScratch& ss, int32_t B = 1) {
    const unsigned nbcap = (unsigned)ceil_div(cap, SCAN_BLOCK);
    const size_t Bz = (size_t)B;
    ss.ksel = (size_t)cap / 3 + 1;
    void* p;
    int rc;
#define SEL_SCRATCH(field, type, count)                                                \
    if ((rc = midas_scratch(ctx, Bz * (size_t)(count) * sizeof(type), &p))) return rc; \
    ss.field = (type*)p
    SEL_SCRATCH(hist, uint32_t, SEL_HIST_WORDS);
    SEL_SCRATCH(state, int32_t, SEL_STATE_WORDS);
    SEL_SCRATCH(c_less, int32_t, nbcap);
    SEL_SCRATCH(c_eq, int32_t, nbcap);
    SEL_SCRATCH(sel_key, uint64_t, ss.ksel);
    SEL_SCRATCH(sel_idx, int32_t, ss.ksel);
    SEL_SCRATCH(srt_key, uint64_t, ss.ksel);
    SEL_SCRATCH(srt_idx, int32_t, ss.ksel);
#undef SEL_SCRATCH
    return MIDAS_OK;
}

// the six digit passes, one launch each (a launch boundary is the grid-wide sync a pass needs behind the one before)
template <int P = 0>
static void launch_select_passes(dim3 grid, hipStream_t st, const int32_t* ci, const double* w, uint32_t* hist, int32_t* state, int32_t slice) {
    hipLaunchKernelGGL(k_loop_select<P>, grid, dim3(256), 0, st, ci, w, hist, state, slice);
    if constexpr (P + 1 < SEL_PASSES) launch_select_passes<P + 1>(grid, st, ci, w, hist, state, slice);
}

// ctl_i[N, MODE, K] and the cleared histograms / pass-0 state are in place: select, compact, order the duplicates.
// B trajectories (midas_loop_step_batch_wide): the same ten launches with the trajectory as grid.y - ctl_i (B, 32), w and src (B, cap),
// the scratch of select_scratch(.., B); the launch boundaries stay the grid-wide syncs between the digit passes, one set for the batch.
// A trajectory whose MODE is 0 leaves every launch at its head but k_loop_compact, which writes its identity.
static int launch_select(midas_ctx* ctx, int64_t cap, const int32_t* ci, const double* w, int32_t* src, const SelectScratch& ss,
                         int32_t B = 1) {
    hipStream_t st = ctx->stream;
    const unsigned nbcap = (unsigned)ceil_div(cap, SCAN_BLOCK), by = (unsigned)B;
    const int32_t slice = B > 1 ? (int32_t)cap : 0, ksel = (int32_t)ss.ksel;  // (read by trajectories behind the first only)
    launch_select_passes(dim3(nbcap, by), st, ci, w, ss.hist, ss.state, slice);
    hipLaunchKernelGGL(k_loop_compact_count, dim3(nbcap, by), dim3(256), 0, st, ci, w, (const uint32_t*)ss.hist, ss.state, ss.c_less,
                       ss.c_eq, slice);
    hipLaunchKernelGGL(k_loop_compact, dim3(nbcap, by), dim3(256), 0, st, ci, w, (const int32_t*)ss.state, (const int32_t*)ss.c_less,
                       (const int32_t*)ss.c_eq, src, ss.sel_key, ss.sel_idx, slice, ksel);
    hipLaunchKernelGGL(k_loop_sort_chunks, dim3((unsigned)ceil_div((int64_t)ss.ksel, SORT_CHUNK), by), dim3(1024), 0, st, ci,
                       (const uint64_t*)ss.sel_key, (const int32_t*)ss.sel_idx, ss.srt_key, ss.srt_idx, ksel);
    hipLaunchKernelGGL(k_loop_sort_rank, dim3((unsigned)ceil_div((int64_t)ss.ksel, 256), by), dim3(256), 0, st, ci,
                       (const uint64_t*)ss.srt_key, (const int32_t*)ss.srt_idx, src, slice, ksel);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// a plan made by the host (the op-by-op annealing of the class surface): control block + cleared select state
__global__ __launch_bounds__(256) void k_anneal_plan(int32_t* __restrict__ ctl_i, uint32_t* __restrict__ hist,
                                                     int32_t* __restrict__ state, int32_t n, int32_t mode, int32_t k) {
    const int t = threadIdx.x;
    for (int i = t; i < SEL_PASSES * SEL_BINS; i += 256) hist[i] = 0u;
    for (int i = t; i < 4 * (SEL_PASSES + 2); i += 256) state[i] = (i == 2) ? k : 0;
    if (t < 32) ctl_i[t] = t == LOOP_I_N ? n : t == LOOP_I_MODE ? mode : t == LOOP_I_K ? k : 0;
}

__global__ __launch_bounds__(256) void k_loop_identity(int32_t n, int32_t* __restrict__ src) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) src[i] = i;
}

int launch_anneal_select(midas_ctx* ctx, int64_t N, const double* w, int32_t mode, int64_t k, int32_t ties, int32_t* src, int32_t* info) {
    void* ctl;
    int rc;
    if ((rc = midas_scratch(ctx, 32 * sizeof(int32_t), &ctl))) return rc;
    SelectScratch ss;
    if ((rc = select_scratch(ctx, N, ss))) return rc;
    hipLaunchKernelGGL(k_anneal_plan, dim3(1), dim3(256), 0, ctx->stream, (int32_t*)ctl, ss.hist, ss.state, (int32_t)N, mode, (int32_t)k);
    if (ties == MIDAS_TOPK_TIES_ATEN_CPU) return launch_topk_aten(ctx, N, (const int32_t*)ctl, w, src, info);
    const char* small = getenv("MIDAS_ANNEAL_SMALL");  // tests: the single-workgroup path on the same plan
    if (N <= LOOP_SMALL_MAX && small && atoi(small)) {
        hipLaunchKernelGGL(k_loop_identity, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, (int32_t)N, src);
        LoopGrid g;
        g.cap = N;
        return launch_anneal_small(ctx, g, (int32_t*)ctl, nullptr, nullptr, nullptr, nullptr, 0, w, src);
    }
    return launch_select(ctx, N, (const int32_t*)ctl, w, src, ss);
}


// ANNEAL of a frame behind the moments m, for the single call and the batch alike; the caller chooses the regime.  Per regime:
//   frozen     (two-pass spreads under the ATen tie rule) -> the decision with frozen = 1, var in ATen's order under that rule; no selection
//   aten_walk  the two-pass spreads -> the decision with var in ATen's order -> launch_topk_aten
//   small      launch_anneal_small: decision and selection in one launch
//   select     the decision -> launch_select
// The select state: the single call carves it in every regime (BatchLoopEngine's and LoopEngine's scratch totals count it there) and
// every decision of it clears it; the batch carves it - B of them - only where the selection reads it, and its ATen decision gets none.
int loop_anneal_phase(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, const LoopMoments& m, LoopAnneal regime) {
    const int32_t aten = s.topk_ties == MIDAS_TOPK_TIES_ATEN_CPU;
    if (aten) loop_std_two_pass(ctx, s, g, m);
    SelectScratch ss{};
    if (!g.batch() || regime == LoopAnneal::select)
        if (int rc = select_scratch(ctx, g.cap, ss, g.B)) return rc;
    if (regime == LoopAnneal::small)
        return launch_anneal_small(ctx, g, s.ctl_i_dev, s.ctl_d_dev, &m, s.cluster_poses_dev, s.cluster_stds_dev, s.floor,
                                   (const double*)s.weights_dev, s.src_dev);
    // frozen: live count == floor == the count annealing started from: the rule (particle_filter.py:421-446) cannot remove (needs
    // |n - floor| > 0) or duplicate (needs k + n <= init) - the decision's bookkeeping runs (cluster rows, variance), the ten
    // launches of the selection, which would each find mode 0 and leave, do not (45 us of a 118 us frame at N = 100k)
    const int32_t frozen = regime == LoopAnneal::frozen, aten_order = frozen ? aten : regime == LoopAnneal::aten_walk;
    if (int rc = launch_loop_decide(ctx, s, g, m, ss.hist, ss.state, frozen, aten_order)) return rc;
    if (regime == LoopAnneal::aten_walk)  // the reference's CPU tie choices (topk_aten.hip): B walks side by side
        return launch_topk_aten(ctx, g.cap, s.ctl_i_dev, s.weights_dev, s.src_dev, nullptr, g.B);
    if (regime == LoopAnneal::select) return launch_select(ctx, g.cap, s.ctl_i_dev, s.weights_dev, s.src_dev, ss, g.B);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

MIDAS_WARM_TU(anneal, k_loop_compact)

}  // namespace midas
