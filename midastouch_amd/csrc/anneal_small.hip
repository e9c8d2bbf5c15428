// anneal_small.hip - ANNEAL of a loop frame (loop.hip) for a small set: decide + radix select + compaction + sort by ONE workgroup.
// After a few frames of annealing the set holds ~10^4 particles and the eleven launches of anneal.hip do a few microseconds of work
// each behind ~4.5 us of launch floor.  When the caller knows that n <= LOOP_SMALL_MAX (LoopEngine bounds the count it saw
// last by the largest growth annealing allows per frame) one 1024-thread workgroup does the same steps - sixteen keys per
// thread in registers, LDS histograms, the k duplicates sorted in LDS - with identical results.  The unit opens with the other
// kernel that takes the decision, k_loop_decide of the multi-launch form (anneal.hip): the two have to compile together.
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "anneal_decide.hpp"
#include "anneal_clocks.hpp"

namespace midas {

// ---- the decision with a launch of its own (anneal.hip's regimes): with k_loop_anneal_small<true> in this unit because the two have to
// compile together - loop_decide with the small form as its only caller is specialised for `aten_order = false` before it is inlined,
// and k_loop_anneal_small<true> comes out with other instructions (one compare inverted) than beside this caller's run-time value.
// Workgroup 0: the select state cleared (hist null: the decision alone - the batch's ATen walk, no radix select follows), the decision
// by thread 0; workgroup 1: the centres' rotations.
// (the body is a file of its own, included here and in the twin that takes floor_n from the rows' parameter table: the twin then
// shares every statement, and this kernel's token stream - so its code, instruction for instruction - is what it was)
__global__ __launch_bounds__(256) void k_loop_decide(int32_t* __restrict__ ctl_i, double* __restrict__ ctl_d,
                                                     const float* __restrict__ centers_all, const float* __restrict__ stds_all,
                                                     const int64_t* __restrict__ counts_all, float* __restrict__ centers_out,
                                                     float* __restrict__ stds_out, uint32_t* __restrict__ hist,
                                                     int32_t* __restrict__ sel_state, int32_t floor_n, const double* __restrict__ rot,
                                                     int32_t frozen = 0, int32_t aten_order = 0) {
#include "loop_decide_body.hpp"
}

// k_loop_decide with annealing's floor of row blockIdx.y's record (midas_loop_step_batch_rows, the wide regime's decision in front of
// the radix select): one scalar load through a uniform address in place of a kernel argument.  The regime has no frozen frames and
// breaks ties by index; the two switches stay run-time values, as in the twin (see the note on loop_decide above).
__global__ __launch_bounds__(256) void k_loop_decide_rows(int32_t* __restrict__ ctl_i, double* __restrict__ ctl_d,
                                                          const float* __restrict__ centers_all, const float* __restrict__ stds_all,
                                                          const int64_t* __restrict__ counts_all, float* __restrict__ centers_out,
                                                          float* __restrict__ stds_out, uint32_t* __restrict__ hist,
                                                          int32_t* __restrict__ sel_state, const midas_loop_row_params* __restrict__ rows,
                                                          const double* __restrict__ rot, int32_t frozen, int32_t aten_order) {
    const int32_t floor_n = rows[blockIdx.y].floor;
#include "loop_decide_body.hpp"
}

int launch_loop_decide(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, const LoopMoments& m, uint32_t* hist,
                       int32_t* sel_state, int32_t frozen, int32_t aten_order) {
    const unsigned wgs = g.logmap ? 1u : 2u;  // (log-map centres are whole when they get here: no workgroup for the rotations)
    if (g.rows)
        hipLaunchKernelGGL(k_loop_decide_rows, dim3(wgs, g.by()), dim3(256), 0, ctx->stream, s.ctl_i_dev, s.ctl_d_dev, (const float*)m.cen,
                           (const float*)m.sd, (const int64_t*)m.cnt, s.cluster_poses_dev, s.cluster_stds_dev, hist, sel_state, g.rows,
                           (const double*)m.rot, frozen, aten_order);
    else
        hipLaunchKernelGGL(k_loop_decide, dim3(wgs, g.by()), dim3(256), 0, ctx->stream, s.ctl_i_dev, s.ctl_d_dev, (const float*)m.cen,
                           (const float*)m.sd, (const int64_t*)m.cnt, s.cluster_poses_dev, s.cluster_stds_dev, hist, sel_state, s.floor,
                           (const double*)m.rot, frozen, aten_order);
    return MIDAS_OK;
}

// ---- the small set -------------------------------------------------------------------------------------------------------------------
// exclusive prefix over the 1024 threads of (a, b); totals returned in ta / tb.  s_w: 32 ints of LDS.
MD void small_scan2(int a, int b, int& ea, int& eb, int& ta, int& tb, int* s_w) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int ia = wave_iscan_dpp(a), ib = wave_iscan_dpp(b);  // (inclusive, by register moves)
    __syncthreads();
    if (lane == 63) { s_w[wv] = ia; s_w[16 + wv] = ib; }
    __syncthreads();
    int pa = 0, pb = 0;
    ta = 0; tb = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int x = s_w[w], y = s_w[16 + w];
        if (w < wv) { pa += x; pb += y; }
        ta += x; tb += y;
    }
    ea = pa + ia - a;
    eb = pb + ib - b;
}

// The sixteen weights a thread of the small-set selection owns, as order-preserving keys: particles t, 1024 + t, .., 15 x 1024 + t
// (indices clamped to the live count).  A wave's load is 64 consecutive values; with sixteen CONSECUTIVE particles per thread
// every lane was a cache line of its own - 64 tag look-ups per instruction, 16 k of them in the one compute unit this
// workgroup has: ~5 us that showed as the wait at the first barrier (tools/anneal_clocks.py "minmax end").
MD void small_keys(const double* __restrict__ w, int n, uint64_t* wkey) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = 1024 * j + t;
        wkey[j] = weight_key(w[i < n ? i : n - 1]);
    }
}

// The selection of a small set by all 1024 threads of one workgroup: radix select of the k-th key, compaction in index order, the
// duplicates in topk's order.  s_w[36 .. 39] = {mode, k, n, 0} (the caller's decision, behind a barrier); wkey: small_keys().
// s_key / s_idx: LOOP_SMALL_PAIRS entries of LDS each.
MD void anneal_small_select(int* s_w, const uint64_t* wkey, int32_t* __restrict__ src, int32_t* __restrict__ ctl_i,
                            double* __restrict__ ctl_d, long long ck0, uint64_t* s_key, int32_t* s_idx) {
    __shared__ uint32_t s_h[SEL_BINS];
    __shared__ uint64_t s_small[64];
    __shared__ uint64_t s_ext[32];   // the waves' extrema (an array of its own: no barrier before s_small's other use)
    __shared__ int2 s_ce[256];       // the compaction's (row, wave) counts (likewise: not the histogram's memory)
    __shared__ uint64_t s_T[1];
    const int t = threadIdx.x;
    const int mode = s_w[36], k = s_w[37], n = s_w[38];
    if (!mode) {
        if (n > LOOP_SMALL_MAX && t == 0) { ctl_i[LOOP_I_MODE] = 0; ctl_i[LOOP_I_K] = 0; ctl_i[LOOP_I_NSET] = n; }
        return;  // identity index list: written by k_loop_weights
    }
    // thread t owns the particles 1024 j + t: index order = (row j, wave, lane)
    uint64_t key[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) key[j] = mode == 2 ? ~wkey[j] : wkey[j];  // (select_key)
    const int mine_n = n - t <= 0 ? 0 : (n - t + 1023) >> 10;  // how many of them exist (rows 0 .. mine_n - 1; n <= 16 384)
    // rows that hold a particle at all (the same for every thread): the per-row loops below skip the others on a scalar branch - at
    // n ~ 8k half of what the sixteen waves of this ONE compute unit would issue
    const int rows = (n + 1023) >> 10;
    ACK(1);
    // ---- radix select: the k-th smallest key T and how many of its equals to take (r)
    // The digits start at the highest bit in which the keys DIFFER (weights of one frame share sign and exponent, often the
    // leading mantissa bits too): with the fixed windows of the large-set kernels the first pass put all 16 k keys into one bin -
    // 16 k same-address LDS atomics one after the other, 15 - 24 us of this kernel's 30 - 50 (phase clocks, tools/anneal_clocks.py).
    uint64_t kmin = ~0ull, kmax = 0ull;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < rows && j < mine_n) { kmin = key[j] < kmin ? key[j] : kmin; kmax = key[j] > kmax ? key[j] : kmax; }
    ACK(30);
    kmin = wave_umin64_dpp(kmin);  // (register moves: midas_math.hpp)
    kmax = wave_umax64_dpp(kmax);
    ACK(31);
    if ((t & 63) == 0) { s_ext[t >> 6] = kmin; s_ext[16 + (t >> 6)] = kmax; }
    __syncthreads();
    ACK(32);
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        kmin = s_ext[w] < kmin ? s_ext[w] : kmin;
        kmax = s_ext[16 + w] > kmax ? s_ext[16 + w] : kmax;
    }
    ACK(33);
    // Enough copies of the smallest key?  (The pruned particles' zeros when particles are dropped, the ~80 particles on the
    // best-scoring entry when the best are duplicated: k is a per cent or two of the set.)  Then T is that key: no pass at all.
    {
        int eq = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < rows) eq += (j < mine_n && key[j] == kmin) ? 1 : 0;
        eq = wave_isum_dpp(eq);
        ACK(34);
        if ((t & 63) == 0 && eq) atomicAdd(&s_w[39], eq);
        __syncthreads();
    }
    const bool at_min = s_w[39] >= k;
    ACK(9);
    int top = (kmin == kmax || at_min) ? 0 : 64 - __builtin_clzll(kmin ^ kmax);  // bits [top, 64) are common to every key
#ifdef MIDAS_ANNEAL_CLOCKS
    long long ckl = wall_clock64();  // (ACKD: from stamp to stamp)
#endif
    uint64_t prefix = top >= 64 ? 0ull : (kmin >> top);  // (top == 0: T = kmin, r = k)
    int krem = k;
#pragma unroll 1
    while (top > 0) {
        const int width = top < 11 ? top : 11, shift = top - width;
        s_h[t] = 0u; s_h[t + 1024] = 0u;
        __syncthreads();
        ACKD(10);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool match = top >= 64 || (key[j] >> top) == prefix;
            if (j < rows && j < mine_n && match) atomicAdd(&s_h[(uint32_t)(key[j] >> shift) & ((1u << width) - 1u)], 1u);
        }
        __syncthreads();
        ACKD(11);
        const int c0 = (int)s_h[2 * t], c1 = (int)s_h[2 * t + 1];
        int e0, e1, t0, t1;
        small_scan2(c0 + c1, 0, e0, e1, t0, t1, s_w);
        ACKD(12);
        if (krem > e0 && krem <= e0 + c0 + c1) {  // exactly one thread
            const bool first = krem <= e0 + c0;
            s_w[32] = 2 * t + (first ? 0 : 1);
            s_w[33] = krem - e0 - (first ? 0 : c0);
            s_w[34] = first ? c0 : c1;  // keys in the chosen bin
            s_w[35] = 0;                // (counter of the short finish below)
        }
        __syncthreads();
        prefix = (prefix << width) | (uint64_t)s_w[32];
        krem = s_w[33];
        const int in_bin = s_w[34];
        __syncthreads();
        ACKD(13);
        if (threadIdx.x == 0) ctl_d_pass(ctl_d);
        top = shift;
        // One value left?  Particles that share a nearest entry share its score and so their weight: a frame's 10^4 keys are
        // ~100 distinct values (and the pruned particles' zeros), the chosen bin usually holds ONE of them, many times - the
        // remaining digits would each be a pass of same-address atomics to learn nothing.  Somebody's key of the bin is the
        // candidate; if every key of the bin equals it, it is T.
        if (top > 0 && in_bin > 1) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < mine_n && (key[j] >> top) == prefix) s_T[0] = key[j];
            __syncthreads();
            const uint64_t cand = s_T[0];
            int eq = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < rows) eq += (j < mine_n && key[j] == cand) ? 1 : 0;
            eq = wave_isum_dpp(eq);
            if ((t & 63) == 0 && eq) atomicAdd(&s_w[35], eq);
            __syncthreads();
            const bool single = s_w[35] == in_bin;
            __syncthreads();
            if (t == 0) s_w[35] = 0;
            if (single) { prefix = cand; ACKD(14); break; }  // krem of them are taken, in index order
            __syncthreads();
        }
        // Short finish: distinct weights leave a handful of keys in the bin after one or two digits - further passes would each
        // cost a histogram, a scan and five barriers to tell one key from none.  With at most 64 keys left, one wave ranks
        // them: T = the key with #{< T} < krem <= #{<= T}.
        if (in_bin <= 64 && top > 0) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < mine_n && (key[j] >> top) == prefix) s_small[atomicAdd(&s_w[35], 1)] = key[j];
            __syncthreads();
            if (t < 64) {
                const uint64_t mk = t < in_bin ? s_small[t] : ~0ull;
                int lt = 0, le = 0;
                for (int m = 0; m < in_bin; ++m) {
                    const uint64_t o = s_small[m];
                    lt += o < mk ? 1 : 0;
                    le += o <= mk ? 1 : 0;
                }
                if (t < in_bin && lt < krem && krem <= le) {  // every lane that holds T writes the same two values
                    s_T[0] = mk;
                    s_w[33] = krem - lt;
                }
            }
            __syncthreads();
            prefix = s_T[0];
            krem = s_w[33];
            ACKD(14);
            break;
        }
    }
    const uint64_t T = prefix;
    const int r = krem;
    ACK(2);
    // ---- compaction in index order: per (row, wave) the counts of keys below / equal to T from ballots, one wave scans the 256
    // (row, wave) pairs in index order, a lane's place inside its wave's row is the ballot's bits below it
    {
        const int lane = t & 63, wv = t >> 6;
        const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
        int pl[16], pe[16];
        unsigned lbits = 0, ebits = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            pl[j] = 0; pe[j] = 0;
            if (j < rows) {
                const bool isl = j < mine_n && key[j] < T, ise = j < mine_n && key[j] == T;
                const uint64_t bl = __ballot(isl), be = __ballot(ise);
                pl[j] = __popcll(bl & below);
                pe[j] = __popcll(be & below);
                lbits |= isl ? (1u << j) : 0u;
                ebits |= ise ? (1u << j) : 0u;
                if (lane == 0) s_ce[j * 16 + wv] = make_int2(__popcll(bl), __popcll(be));
            } else if (lane == 0) {
                s_ce[j * 16 + wv] = make_int2(0, 0);
            }
        }
        __syncthreads();
        if (wv == 0) {
            const int2 c0 = s_ce[4 * lane], c1 = s_ce[4 * lane + 1], c2 = s_ce[4 * lane + 2], c3 = s_ce[4 * lane + 3];
            int sl = c0.x + c1.x + c2.x + c3.x, se = c0.y + c1.y + c2.y + c3.y;
            const int il = wave_iscan_dpp(sl), ie = wave_iscan_dpp(se);
            int el = il - sl, ee = ie - se;
            s_ce[4 * lane] = make_int2(el, ee);
            el += c0.x; ee += c0.y;
            s_ce[4 * lane + 1] = make_int2(el, ee);
            el += c1.x; ee += c1.y;
            s_ce[4 * lane + 2] = make_int2(el, ee);
            el += c2.x; ee += c2.y;
            s_ce[4 * lane + 3] = make_int2(el, ee);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < rows && j < mine_n) {
                const int i = 1024 * j + t;
                const int2 b = s_ce[j * 16 + wv];
                const int lb = b.x + pl[j], eb = b.y + pe[j];
                const bool isl = (lbits >> j) & 1u, ise = (ebits >> j) & 1u;
                const bool selected = isl || (ise && eb < r);
                const int sel_before = lb + (eb < r ? eb : r);
                if (mode == 1) {
                    if (!selected) src[i - sel_before] = i;
                } else if (selected) {
                    s_key[sel_before] = key[j];
                    s_idx[sel_before] = i;
                }
            }
        }
    }
    ACK(3);
    if (mode != 2) return;
    // ---- the k duplicates in topk's order: (key, index) ascending
    if (k <= 256) {
        // few duplicates (the usual case: the variance ratio moves by a per cent or two per frame): every pair counts the pairs
        // before it - one barrier pair instead of the network's log^2 stages of a 16-wave barrier each
        __syncthreads();
        uint64_t mk = 0;
        int32_t mi = 0;
        int rank = 0;
        if (t < k) {
            mk = s_key[t]; mi = s_idx[t];
            for (int m = 0; m < k; ++m) rank += pair_less(s_key[m], s_idx[m], mk, mi) ? 1 : 0;
        }
        ACK(4);
        if (t < k) src[n + rank] = mi;
        ACK(5);
        if (threadIdx.x == 0) { ctl_d_dbg(ctl_d, k); }
        return;
    }
    // larger sets: bitonic network over the next power of two
    int P = 2;
    while (P < k) P <<= 1;
    __syncthreads();
    for (int i = k + t; i < P; i += 1024) { s_key[i] = ~0ull; s_idx[i] = 0x7fffffff; }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int q = t; q < P / 2; q += 1024) {
                const int lo = 2 * q - (q & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t ka = s_key[lo], kb = s_key[hi];
                const int32_t ia = s_idx[lo], ib = s_idx[hi];
                const bool swap = up ? pair_less(kb, ib, ka, ia) : pair_less(ka, ia, kb, ib);
                if (swap) { s_key[lo] = kb; s_key[hi] = ka; s_idx[lo] = ib; s_idx[hi] = ia; }
            }
            __syncthreads();
        }
    }
    ACK(4);
    for (int q = t; q < k; q += 1024) src[n + q] = s_idx[q];
    ACK(5);
    if (threadIdx.x == 0) { ctl_d_dbg(ctl_d, k); }
}

// DECIDE: the frame's decision by thread 0 and, second workgroup, the centres' rotations; else a plan the host left in ctl_i
// (the body is a file of its own, included here and in the twin that takes floor_n from the rows' parameter table: the twin then
// shares every statement, and this kernel's token stream - so its code, instruction for instruction - is what it was)
template <bool DECIDE>
__global__ __launch_bounds__(1024) void k_loop_anneal_small(int32_t* __restrict__ ctl_i, double* __restrict__ ctl_d,
                                                            const float* __restrict__ centers_all, const float* __restrict__ stds_all,
                                                            const int64_t* __restrict__ counts_all, float* __restrict__ centers_out,
                                                            float* __restrict__ stds_out, int32_t floor_n,
                                                            const double* __restrict__ w, int32_t* __restrict__ src,
                                                            const double* __restrict__ rot, int32_t cap = 0) {
#include "loop_anneal_small_body.hpp"
}

// k_loop_anneal_small<true> with annealing's floor of row blockIdx.y's record (midas_loop_step_batch_rows): one scalar load through a
// uniform address in place of a kernel argument; only the deciding thread uses the value.
__global__ __launch_bounds__(1024) void k_loop_anneal_small_rows(int32_t* __restrict__ ctl_i, double* __restrict__ ctl_d,
                                                                 const float* __restrict__ centers_all, const float* __restrict__ stds_all,
                                                                 const int64_t* __restrict__ counts_all, float* __restrict__ centers_out,
                                                                 float* __restrict__ stds_out,
                                                                 const midas_loop_row_params* __restrict__ rows,
                                                                 const double* __restrict__ w, int32_t* __restrict__ src,
                                                                 const double* __restrict__ rot, int32_t cap) {
    constexpr bool DECIDE = true;
    const int32_t floor_n = rows[blockIdx.y].floor;
#include "loop_anneal_small_body.hpp"
}

// B trajectories (grid.y; slices g.slice particles apart): a frame's annealing from the moments m, or - m null - the selection alone on
// a plan the host left in ctl_i (launch_anneal_select: one workgroup, no cluster arrays)
int launch_anneal_small(midas_ctx* ctx, const LoopGrid& g, int32_t* ctl_i, double* ctl_d, const LoopMoments* m, float* centers_out,
                        float* stds_out, int32_t floor_n, const double* w, int32_t* src) {
    const unsigned wgs = g.logmap ? 1u : 2u;  // (log-map centres are whole when they get here: no workgroup for the rotations)
    if (m && g.rows)
        hipLaunchKernelGGL(k_loop_anneal_small_rows, dim3(wgs, g.by()), dim3(1024), 0, ctx->stream, ctl_i, ctl_d, (const float*)m->cen,
                           (const float*)m->sd, (const int64_t*)m->cnt, centers_out, stds_out, g.rows, w, src, (const double*)m->rot, g.slice);
    else if (m)
        hipLaunchKernelGGL(k_loop_anneal_small<true>, dim3(wgs, g.by()), dim3(1024), 0, ctx->stream, ctl_i, ctl_d, (const float*)m->cen,
                           (const float*)m->sd, (const int64_t*)m->cnt, centers_out, stds_out, floor_n, w, src, (const double*)m->rot, g.slice);
    else
        hipLaunchKernelGGL(k_loop_anneal_small<false>, dim3(1, g.by()), dim3(1024), 0, ctx->stream, ctl_i, ctl_d, (const float*)nullptr,
                           (const float*)nullptr, (const int64_t*)nullptr, centers_out, stds_out, floor_n, w, src, (const double*)nullptr,
                           g.slice);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

MIDAS_WARM_TU(anneal_small, k_loop_anneal_small<true>)

}  // namespace midas
