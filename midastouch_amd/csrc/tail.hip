// tail.hip - the fused tail of the per-frame step on one GPU (and TA2 of a shard): weights, the float64 CDF tables in the
// summation order of resample.hip's header, resample and gather; the next frame's prediction list.
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "tail_sums.hpp"
#include "tail_block.hpp"
#include "tail_group.hpp"

namespace midas {

// ------------------------------------------------------------------------------------------------
// step tail (shared by the fused single-GPU step and the particle-sharded multi-GPU step)
// ------------------------------------------------------------------------------------------------
// A shard owns N local particles = the global slots [slot_base, slot_base + N) and the global blocks
// [block_base, block_base + nb_local) of the summation spec; arrays suffixed _all span every shard.
// Single GPU: slot_base = block_base = 0 and the _all arrays are the local ones.
// (TA, the eager form's first half: k_tail_a, resample.hip - it shares block_extrema with k_exp_partial.)

// TA2 (fused single-GPU step, deferred mode): the particle update ran concurrently with the codebook scoring,
// so this kernel gathers x = scores[nn_idx] itself, takes e = exp(x - 1) and produces what TA produces - with
// the isclose guard (a GLOBAL property of x) deferred to TB:  the guard can only fire when every block's own
// range is within the tolerance, so a block whose range is wider writes the softmax variant only; a block
// whose range is within it (rare: all its particles share one score) writes the raw variant as well, and TB
// picks one after reducing the per-block extrema.  Global traffic is coalesced (slot = k * 256 + thread); the
// chunk-per-thread view the summation spec needs goes through LDS (one pad double per 16-slot chunk).
MD int pad16(int i) { return i + (i >> 4); }

MD void scan_variant(const double* val, const uint8_t* okm, int64_t base, int64_t N, double* s_a, double* s_m,
                     double* s_gtot, double* __restrict__ lp_out, double* __restrict__ gend_out,
                     double* __restrict__ ggend_out, double& W_all, double& W_masked, bool& nan) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int s = k * 256 + t;
        const bool in = base + s < N;
        const double v = in ? val[k] : 0.0;
        const double m = in ? v * (okm[k] ? 1.0 : 0.0) : 0.0;
        nan |= m != m;
        s_a[pad16(s)] = v;
        s_m[pad16(s)] = m;
    }
    __syncthreads();
    double v[SCAN_CHUNK], vm[SCAN_CHUNK], l[SCAN_CHUNK];
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) { v[j] = s_a[t * 17 + j]; vm[j] = s_m[t * 17 + j]; }
    W_all = block_scan(v, l, s_gtot);
    __syncthreads();
    W_masked = block_scan(vm, l, s_gtot);
    if (base + (int64_t)t * SCAN_CHUNK < N) gend_out[(base >> 4) + t] = l[SCAN_CHUNK - 1];  // block-local prefix at the chunk end
    if ((t & 15) == 15) ggend_out[(base >> 8) + (t >> 4)] = l[SCAN_CHUNK - 1];               // ... at the end of each 256-slot group
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) s_m[t * 17 + j] = l[j];  // own chunk only
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int s = k * 256 + t;
        if (base + s < N) lp_out[base + s] = s_m[pad16(s)];
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_tail_a2(int64_t N, const double* __restrict__ scores,
                                                 const int32_t* __restrict__ nn_idx, const uint8_t* __restrict__ valid,
                                                 int32_t softmax, double* __restrict__ e_out, double* __restrict__ x_out,
                                                 double* __restrict__ lp_soft, double* __restrict__ lp_raw,
                                                 double* __restrict__ gend_soft, double* __restrict__ gend_raw,
                                                 double* __restrict__ ggend_soft, double* __restrict__ ggend_raw,
                                                 double* __restrict__ bsum_e, double* __restrict__ btot_soft,
                                                 double* __restrict__ btot_raw, double* __restrict__ bmax,
                                                 double* __restrict__ bmin, int32_t* __restrict__ status,
                                                 double* __restrict__ flags_out, int64_t score_stride) {
    if (blockIdx.y) {  // batch of trajectories: every per-trajectory array is (B, ...) contiguous, plain strides
        const int64_t b = blockIdx.y, o = b * N, ng = (N + SCAN_CHUNK - 1) / SCAN_CHUNK, nb = gridDim.x;
        scores += b * score_stride; nn_idx += o; valid += o; e_out += o; x_out += o; lp_soft += o; lp_raw += o;
        gend_soft += b * ng; gend_raw += b * ng; ggend_soft += b * 16 * nb; ggend_raw += b * 16 * nb;
        bsum_e += b * nb; btot_soft += b * nb; btot_raw += b * nb; bmax += b * nb; bmin += b * nb;
        status += 2 * b;
    }
    __shared__ double s_a[SCAN_BLOCK + SCAN_BLOCK / 16];
    __shared__ double s_m[SCAN_BLOCK + SCAN_BLOCK / 16];
    __shared__ double s_gtot[16];
    __shared__ double s_red[24];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK;
    // loads are unconditional on clamped slots (a conditional load per slot makes the compiler wait for each
    // one before issuing the next); out-of-range slots are neutralised afterwards
    int32_t nn[SCAN_CHUNK];
    uint8_t okm[SCAN_CHUNK];
    double x[SCAN_CHUNK];
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int64_t i = base + k * 256 + t, ic = i < N ? i : N - 1;
        nn[k] = nn_idx[ic];
        okm[k] = valid[ic];
    }
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) x[k] = scores[nn[k]];
    double mx = -INFINITY, mn = INFINITY;
    bool xnan = false;
    int kept = 0;
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const bool in = base + k * 256 + t < N;
        xnan |= in && x[k] != x[k];
        mx = in && x[k] > mx ? x[k] : mx;
        mn = in && x[k] < mn ? x[k] : mn;
        kept += in && okm[k] ? 1 : 0;
        if (!in) { x[k] = 0.0; okm[k] = 0; }
    }
    // block extrema (NaN propagates, as torch.max / torch.min do)
    guard_publish<8>(mx, mn, xnan, s_red);
    __syncthreads();
    const GuardExtrema g = guard_collect<8>(s_red);
    if (t == 0) { bmax[blockIdx.x] = g.mx; bmin[blockIdx.x] = g.mn; }
    const bool close = __builtin_fabs(g.mx - g.mn) <= ISCLOSE_ATOL;  // false on NaN
    const bool need_soft = softmax != 0, need_raw = !softmax || close;
    bool nan = false;
    double Wa = 0.0, Wm = 0.0;
    if (need_soft) {
        double e[SCAN_CHUNK];
#pragma unroll
        for (int k = 0; k < SCAN_CHUNK; ++k) {
            e[k] = exp_spec(x[k] - 1.0);
            const int64_t i = base + k * 256 + t;
            if (i < N) e_out[i] = e[k];
        }
        scan_variant(e, okm, base, N, s_a, s_m, s_gtot, lp_soft, gend_soft, ggend_soft, Wa, Wm, nan);
        if (t == 0) { bsum_e[blockIdx.x] = Wa; btot_soft[blockIdx.x] = Wm; }
    }
    if (need_raw) {
#pragma unroll
        for (int k = 0; k < SCAN_CHUNK; ++k) {
            const int64_t i = base + k * 256 + t;
            if (i < N) x_out[i] = x[k];
        }
        bool nan_raw = false;
        scan_variant(x, okm, base, N, s_a, s_m, s_gtot, lp_raw, gend_raw, ggend_raw, Wa, Wm, nan_raw);
        if (t == 0) btot_raw[blockIdx.x] = Wm;
        if (!need_soft) nan = nan_raw;  // with the softmax on, x NaN <=> e NaN: counted once
    } else if (t == 0) {
        btot_raw[blockIdx.x] = 0.0;
    }
    const bool wnan = __any(nan);
    if (wnan && (t & 63) == 0) {
        atomicOr(&status[0], 2);
        if (flags_out) atomicAdd(&flags_out[0], 1.0);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    if ((t & 63) == 0 && kept) {
        atomicAdd(&status[1], kept);
        if (flags_out) atomicAdd(&flags_out[1], (double)kept);  // exact: integers far below 2^53
    }
}

// Extra workgroups of the tail (blockIdx.x >= nb): the prediction list of the NEXT frame's sparse scoring.  Every row whose
// stamp is this frame's epoch was somebody's nearest entry in this frame (claimed by its first particle, or confirmed from
// the previous list): it goes on the list - order is immaterial, one counter bump per wave - and is re-stamped epoch + 1,
// the tag the next front (epoch + 2) honours as "being scored by my streaming waves".  A cloud moves a fraction of the
// codebook's spacing per frame, so most of the rows it needs were needed the frame before: they are then scored by
// balanced, coalesced streaming waves instead of by whichever particle wave touches them first (in the frames after a
// wide start a wave claimed up to 64 rows = 16 rounds of cold 8 KB fetches, and the kernel ends with its slowest wave).
constexpr int PREDICT_PER_THREAD = 16;
// One workgroup lists the rows of its 256 x PREDICT_PER_THREAD stamps that carry this frame's epoch: counts per thread, a prefix
// over the wave (DPP), the waves' totals through LDS, ONE bump of the list's counter per workgroup.  (One bump per wave with four
// stamps a thread was 196 serialised read-modify-writes of one address whenever most waves had rows to list - the frames after
// a wide start, 10^4 rows in use: 3 - 5 us of the tail kernel there.)  s_wt: 8 ints of LDS.
MD void predict_scan(const ScorePredict& pr, int blk, int* s_wt) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t k0 = ((int64_t)blk * 256 + threadIdx.x) * PREDICT_PER_THREAD;
    uint32_t st[PREDICT_PER_THREAD];
    if (k0 + PREDICT_PER_THREAD <= pr.K) {
#pragma unroll
        for (int q = 0; q < PREDICT_PER_THREAD / 4; ++q) {
            const uint4 v = reinterpret_cast<const uint4*>(pr.stamps + k0)[q];
            st[4 * q] = v.x; st[4 * q + 1] = v.y; st[4 * q + 2] = v.z; st[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < PREDICT_PER_THREAD; ++j) st[j] = k0 + j < pr.K ? pr.stamps[k0 + j] : 0u;
    }
    // listed: the rows this frame used (stamp = epoch) and the rows that were on this frame's list unused (stamp = epoch - 1, the
    // frame's pred_tag: their second chance, ScorePredict); a second chance that was not taken (bit 31 set) is dropped
    const uint32_t unused = pr.epoch - 1u;
    // keep(st): the row goes on the next list
    auto keep = [&](uint32_t v) { return v == pr.epoch || ((v & ~PRED_SECOND) == unused && (v >> 30) < (uint32_t)MIDAS_PRED_CHANCES); };
    int n = 0;
#pragma unroll
    for (int j = 0; j < PREDICT_PER_THREAD; ++j) n += (k0 + j < pr.K && keep(st[j])) ? 1 : 0;
    const int incl = wave_iscan_dpp(n);
    if (lane == 63) s_wt[w] = incl;
    __syncthreads();
    const int t0 = s_wt[0], t1 = s_wt[1], t2 = s_wt[2], t3 = s_wt[3];
    const int total = t0 + t1 + t2 + t3;
    if (total == 0) return;  // (uniform over the workgroup)
    if (threadIdx.x == 0) s_wt[4] = atomicAdd(pr.count, total);
    __syncthreads();
    int pos = s_wt[4] + (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0) + incl - n;
#pragma unroll
    for (int j = 0; j < PREDICT_PER_THREAD; ++j)
        if (k0 + j < pr.K && keep(st[j])) {
            // (distinct rows, counter zeroed by the front: pos < K; a row that would not fit simply stays unlisted and untagged -
            // its first particle of the next frame claims it)
            if (pos < pr.K) {
                pr.list[pos] = (int32_t)(k0 + j);
                pr.stamps[k0 + j] = st[j] == pr.epoch ? pr.epoch + 1u : ((pr.epoch + 1u) | ((st[j] & PRED_SECOND) + PRED_AGE1));
            }
            ++pos;
        }
}

// prediction list from scratch (the particle set was replaced: projection onto the codebook, filter/filter.py:159-160): the rows
// idx[n] are stamped `epoch`, predict_scan then lists them and tags them epoch + 1 for the frame with epoch + 2
__global__ __launch_bounds__(256) void k_predict_mark(int64_t N, const int32_t* __restrict__ idx, uint32_t* __restrict__ stamps, int64_t K, uint32_t epoch) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int32_t r = idx[n];
    if (r >= 0 && r < K) stamps[r] = epoch;  // every marker of a row stores the same value
}
__global__ __launch_bounds__(256) void k_predict_scan(ScorePredict pr) {
    __shared__ int s_wt[8];
    predict_scan(pr, (int)blockIdx.x, s_wt);
}

// workgroups that list a frame's rows (predict_scan: 256 x PREDICT_PER_THREAD stamps each); none without a list
static int predict_blocks(const ScorePredict* predict) { return predict ? (int)ceil_div(predict->K, 256 * PREDICT_PER_THREAD) : 0; }

int launch_predict_seed(midas_ctx* ctx, int64_t N, const int32_t* idx, const ScorePredict& pr) {
    MIDAS_HIP_CHECK(ctx, hipMemsetAsync(pr.count, 0, sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(k_predict_mark, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, idx, pr.stamps, pr.K, pr.epoch);
    hipLaunchKernelGGL(k_predict_scan, dim3((unsigned)predict_blocks(&pr)), dim3(256), 0, ctx->stream, pr);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

// The frame's rmse from the front kernel's per-wave sums (nrm pairs), by one 256-thread workgroup: a strided sum per thread, the
// ordered wave sum, the four waves' totals through LDS (s_red: 8 doubles), added as a tree by thread 0.  rmse_raw: a shard's
// sums as they are (added up across the ranks by whoever reads the exchange records: k_reduce_partials' order).  stamp:
// rmse_out[2] = the device wall clock (100 MHz) in us: where this frame ended.  reused: the workgroup has read s_red for something
// else - a barrier in front of the writes (there and not in front of the call: k_tail_a2d's loads stay ahead of it).
MD void frame_rmse(const double* __restrict__ part_rmse, int nrm, int64_t N, double* s_red, double* __restrict__ rmse_out, bool rmse_raw,
                   bool stamp, bool reused = false) {
    const int t = threadIdx.x;
    double p = 0.0, q = 0.0;
    for (int k = t; k < nrm; k += 256) { p += part_rmse[2 * k]; q += part_rmse[2 * k + 1]; }
    p = wave_sum_ordered(p);
    q = wave_sum_ordered(q);
    if (reused) __syncthreads();
    if ((t & 63) == 0) { s_red[t >> 6] = p; s_red[4 + (t >> 6)] = q; }
    __syncthreads();
    if (t == 0) {
        p = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        q = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
        if (rmse_raw) {
            rmse_out[0] = p;
            rmse_out[1] = q;
            return;
        }
        rmse_out[0] = __builtin_sqrt(p / (double)N);
        rmse_out[1] = __builtin_sqrt(q / (double)N);
        if (stamp) rmse_out[2] = (double)wall_clock64() * 0.01;
    }
}

// k_tail_a2 in the chunk-per-thread view (tail_block.hpp): every thread reads and writes its own 16-slot chunk from one
// address, nothing goes through LDS.  Same outputs, 5.5 us instead of 8.0 at N = 100k (two barriers and two LDS round
// trips fewer on a latency-bound kernel).  Single trajectory, N >= 16 (smaller sets: k_tail_a2).
__global__ __launch_bounds__(256) void k_tail_a2d(int64_t N, const double* __restrict__ scores, const int32_t* __restrict__ nn_idx,
                                                  const uint8_t* __restrict__ valid, int32_t softmax, TailTables tb, bool padded,
                                                  int32_t* __restrict__ status, double* __restrict__ flags_out,
                                                  const double* __restrict__ part_rmse, int nrm, double* __restrict__ rmse_out,
                                                  int64_t score_stride = 0, int64_t tstride = 0, int nb_tail = 0x7fffffff,
                                                  ScorePredict pr = ScorePredict(), bool rmse_raw = false) {
    __shared__ double s_gtot[32];
    __shared__ double s_red[24];
    __shared__ uint32_t s_gh[TAIL_GUIDE_LDS];
    if ((int)blockIdx.x >= nb_tail) {  // (single trajectory only: the launcher adds these workgroups when pr.stamps is set)
        predict_scan(pr, (int)blockIdx.x - nb_tail, reinterpret_cast<int*>(s_red));
        return;
    }
    if (blockIdx.y) {  // pipelined batch: trajectory blockIdx.y - its own table block (tables_of layout), scores, arrays, rmse triple
        const int64_t b = blockIdx.y, o = b * N, ts = b * tstride;
        scores += b * score_stride; nn_idx += o; valid += o; status += 2 * b;
        tb.e += ts; tb.x_raw += ts; tb.lp += ts; tb.lp_raw += ts; tb.gend += ts; tb.gend_raw += ts; tb.ggend += ts; tb.ggend_raw += ts;
        tb.bsum_e += ts; tb.btot += ts; tb.btot_raw += ts; tb.bmax += ts; tb.bmin += ts;
        if (part_rmse) { part_rmse += 2 * b * nrm; rmse_out += 3 * b; }
        tb.guide = nullptr; tb.guide_raw = nullptr;  // (single trajectory only)
    }
    int kept = 0;
    bool nan = false;
    tail_a_direct(N, (int)blockIdx.x, scores, nn_idx, valid, softmax, tb, padded, s_gtot, s_red, kept, nan, tb.guide ? s_gh : nullptr);
    const int t = threadIdx.x;
    if (t == 0) {
        if (nan) atomicOr(&status[0], 2);
        if (kept) atomicAdd(&status[1], kept);
        if (flags_out) {  // sharded exchange record: NaN marker (any non-zero) and kept count (exact: integers far below 2^53)
            if (nan) atomicAdd(&flags_out[0], 1.0);
            if (kept) atomicAdd(&flags_out[1], (double)kept);
        }
    }
    if (rmse_out && blockIdx.x == 0) frame_rmse(part_rmse, nrm, N, s_red, rmse_out, rmse_raw, true, true);
}

// The tail with one WAVE per 256-slot group (tail_group.hpp): workgroups [0, nwg) hold four groups each, workgroup nwg (when
// rmse_out is set) adds up the front's rmse sums as k_tail_a2d's block 0 does, the workgroups behind it list the next frame's rows.
__global__ __launch_bounds__(256) void k_tail_a3(TailGroupArgs a, int ngroups, int nwg, const double* __restrict__ part_rmse, int nrm,
                                                 double* __restrict__ rmse_out, bool rmse_raw, ScorePredict pr) {
    __shared__ double s_E[4][2 * TG_GROUP / GUIDE_UNIT];
    __shared__ double s_red[24];
    int b = (int)blockIdx.x;
    const int t = threadIdx.x;
    if (b < nwg) {
        const int wv = __builtin_amdgcn_readfirstlane(t >> 6), G = 4 * b + wv;  // (wave-uniform: the group's own conditions are scalar branches)
        if (G < ngroups) tail_group_wave(a, G, s_E[wv]);
        return;
    }
    b -= nwg;
    if (rmse_out) {
        if (b == 0) {
            TG_SPAN(2048, wall_clock64());
            frame_rmse(part_rmse, nrm, a.N, s_red, rmse_out, rmse_raw, true);
            TG_SPAN(2049, wall_clock64());
            return;
        }
        b -= 1;
    }
    predict_scan(pr, b, reinterpret_cast<int*>(s_red));
}

// The grouped form needs the hand-over records, the whole grid resident and whole 16-byte pieces of the per-slot arrays.
// Resident = the launch's workgroups (four-wave group workgroups + the rmse workgroup + `extra` list workgroups) fit the DEVICE's
// compute units at the kernel's occupancy - queried, not assumed (a partitioned or smaller part takes the one-workgroup-per-block
// form earlier); the waves wait for each other, so a grid that cannot all start must not take this form.
static int tail_resident_workgroups(midas_ctx* ctx) {
    static int cap_dev[64] = {};
    const int di = ctx->device >= 0 && ctx->device < 64 ? ctx->device : 0;
    if (!cap_dev[di] || ctx->device != di) {
        hipDeviceProp_t prop;
        const int ncu = (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 0;
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)k_tail_a3, 256, 0) != hipSuccess) { occ = 0; (void)hipGetLastError(); }
        cap_dev[di] = ncu * occ > 0 ? ncu * occ : -1;
    }
    return cap_dev[di];
}
static bool tail_grouped_ok(midas_ctx* ctx, int64_t N, const int32_t* nn_idx, const uint8_t* valid, const TailTables& tb, int extra) {
    const char* env = getenv("MIDAS_TAIL_GROUPED");  // (read per launch: the tests compare both forms in one process)
    const bool on = !(env && env[0] == '0');
    if (!on || !ctx->tail_rec || N < SCAN_CHUNK || ceil_div(N, SCAN_BLOCK) > ctx->tail_rec_blocks) return false;
    if ((ceil_div(N, TG_GROUP) + 3) / 4 + 1 + extra > tail_resident_workgroups(ctx)) return false;
    const uintptr_t al = (uintptr_t)nn_idx | (uintptr_t)tb.e | (uintptr_t)tb.x_raw | (uintptr_t)tb.lp | (uintptr_t)tb.lp_raw;
    return (al & 15) == 0 && ((uintptr_t)valid & 3) == 0;
}
static int launch_tail_a3(midas_ctx* ctx, int64_t N, const double* scores, const int32_t* nn_idx, const uint8_t* valid, int32_t softmax,
                          const TailTables& tb, bool padded, int32_t* status, double* flags_out, const double* part_rmse, double* rmse_out,
                          bool rmse_raw, const ScorePredict* predict) {
    TailGroupArgs a;
    a.N = N; a.scores = scores; a.nn_idx = nn_idx; a.valid = valid; a.softmax = softmax; a.tb = tb; a.padded = padded;
    a.status = status; a.flags_out = flags_out; a.rec = ctx->tail_rec;
    if (++ctx->tail_tag == 0) ctx->tail_tag = 1;
    a.tag = ctx->tail_tag;
    const int ngroups = (int)ceil_div(N, TG_GROUP), nwg = (ngroups + 3) / 4;
    hipLaunchKernelGGL(k_tail_a3, dim3((unsigned)(nwg + (rmse_out ? 1 : 0) + predict_blocks(predict))), dim3(256), 0, ctx->stream, a, ngroups, nwg, part_rmse,
                       particle_update_blocks(N), rmse_out, rmse_raw, predict ? *predict : ScorePredict());
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

int launch_tail_a2(midas_ctx* ctx, int64_t N, const double* scores, const int32_t* nn_idx, const uint8_t* valid,
                   int32_t softmax, const TailTables& tb, int32_t* status, int batch, int64_t score_stride, bool padded_tables,
                   const double* part_rmse, double* rmse_out, int64_t tstride, const ScorePredict* predict) {
    const int nb = (int)ceil_div(N, SCAN_BLOCK);
    // (k_tail_a2, the LDS-staged form, serves N < 16 and the batch without table strides only)
    const ScorePredict* list = predict && predict->stamps && predict->list && batch <= 1 ? predict : nullptr;
    if (list && N < SCAN_CHUNK) return midas_set_error(ctx, MIDAS_ERR_INVALID, "score_list", "the prediction list needs the direct tail kernel (N >= 16)");
    if (batch <= 1 && tail_grouped_ok(ctx, N, nn_idx, valid, tb, predict_blocks(list)))
        return launch_tail_a3(ctx, N, scores, nn_idx, valid, softmax, tb, padded_tables, status, nullptr, part_rmse,
                              part_rmse ? rmse_out : (double*)nullptr, false, list);
    if ((batch <= 1 || tstride > 0) && N >= SCAN_CHUNK) {
        hipLaunchKernelGGL(k_tail_a2d, dim3((unsigned)(nb + predict_blocks(list)), (unsigned)(batch > 1 ? batch : 1)), dim3(256), 0, ctx->stream, N, scores, nn_idx,
                           valid, softmax, tb, padded_tables, status, (double*)nullptr, part_rmse, particle_update_blocks(N),
                           part_rmse ? rmse_out : (double*)nullptr, score_stride, tstride, nb, list ? *list : ScorePredict());
        LAUNCH_CHECK(ctx);
        return MIDAS_OK;
    }
    if (tb.guide && batch <= 1) {  // (this form of the tail writes no guide tables: "no guide" in every entry, see tail_block.hpp)
        MIDAS_HIP_CHECK(ctx, hipMemsetAsync(tb.guide, 0xFF, (size_t)nb * GUIDE_STRIDE * sizeof(guide_t), ctx->stream));
        if (tb.guide_raw) MIDAS_HIP_CHECK(ctx, hipMemsetAsync(tb.guide_raw, 0xFF, (size_t)nb * GUIDE_STRIDE * sizeof(guide_t), ctx->stream));
    }
    hipLaunchKernelGGL(k_tail_a2, dim3((unsigned)nb, (unsigned)(batch > 1 ? batch : 1)), dim3(256), 0, ctx->stream, N, scores, nn_idx, valid, softmax, tb.e, tb.x_raw,
                       tb.lp, tb.lp_raw, tb.gend, tb.gend_raw, tb.ggend, tb.ggend_raw, tb.bsum_e, tb.btot, tb.btot_raw, tb.bmax, tb.bmin,
                       status, nullptr, score_stride);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// TA2 of one shard: the exchange record r1 = [bsum_e | btot | btot_raw | bmax | bmin | NaN count, kept count | ...]
int launch_shard_tail_a(midas_ctx* ctx, int64_t N, const double* scores, const int32_t* nn_idx, const uint8_t* valid,
                        int32_t softmax, const TailTables& tb, double* r1, int32_t* status, const double* part_rmse,
                        const ScorePredict* predict) {
    const int nb = (int)ceil_div(N, SCAN_BLOCK);
    // (k_tail_a2, the LDS-staged form, serves N < 16 and the batch without table strides only)
    const ScorePredict* list = predict && predict->stamps && predict->list ? predict : nullptr;
    if ((part_rmse || list) && N < SCAN_CHUNK)
        return midas_set_error(ctx, MIDAS_ERR_INVALID, "shard tail", "rmse sums / prediction list in the tail need the direct tail kernel (N >= 16)");
    if (N >= SCAN_CHUNK) {  // the shard's per-slot tables are padded (shard_tables_of, api_shard.hip)
        TailTables t = tb;
        t.bsum_e = r1; t.btot = r1 + nb; t.btot_raw = r1 + 2 * nb; t.bmax = r1 + 3 * nb; t.bmin = r1 + 4 * nb;
        if (tail_grouped_ok(ctx, N, nn_idx, valid, t, predict_blocks(list)))
            return launch_tail_a3(ctx, N, scores, nn_idx, valid, softmax, t, true, status, r1 + 5 * nb, part_rmse,
                                  part_rmse ? r1 + 5 * nb + 2 : (double*)nullptr, true, list);
        // part_rmse: the front's per-wave sums are added up here (block 0) into r1[5 nb + 2 ..] instead of by a kernel of their own
        hipLaunchKernelGGL(k_tail_a2d, dim3((unsigned)(nb + predict_blocks(list))), dim3(256), 0, ctx->stream, N, scores, nn_idx, valid, softmax, t, true,
                           status, r1 + 5 * nb, part_rmse, particle_update_blocks(N), part_rmse ? r1 + 5 * nb + 2 : (double*)nullptr,
                           (int64_t)0, (int64_t)0, nb, list ? *list : ScorePredict(), true);
        LAUNCH_CHECK(ctx);
        return MIDAS_OK;
    }
    if (tb.guide)  // (this form of the tail writes no guide tables: "no guide" in every entry, see tail_block.hpp)
        MIDAS_HIP_CHECK(ctx, hipMemsetAsync(tb.guide, 0xFF, (size_t)2 * nb * GUIDE_STRIDE * sizeof(guide_t), ctx->stream));
    hipLaunchKernelGGL(k_tail_a2, dim3((unsigned)nb), dim3(256), 0, ctx->stream, N, scores, nn_idx, valid, softmax, tb.e, tb.x_raw,
                       tb.lp, tb.lp_raw, tb.gend, tb.gend_raw, tb.ggend, tb.ggend_raw, r1, r1 + nb, r1 + 2 * nb, r1 + 3 * nb, r1 + 4 * nb,
                       status, r1 + 5 * nb, 0);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// TB (single-GPU path): everything after TA in one kernel.  Each workgroup rebuilds the small tables (S,
// total, BP[b], cdf at the block ends) in LDS, writes the weights of its own 256 slots, then resamples
// them: the block holding the draw is found in the LDS table, the slot by a 12-step search over the
// block-local prefix with cdf(i) = (BP_b + lp_i) / total evaluated on the fly - the same values the
// sharded path materialises, so both give identical indices.
MD double cdf_at(const double* __restrict__ lp, const double* s_bp, double total, int64_t i, int64_t N) {
    return (i == N - 1) ? 1.0 : (s_bp[i >> 12] + lp[i]) / total;
}

struct TailBArgs {
    int64_t N;
    int nb;
    const double* e;
    const uint8_t* valid;
    const double* lp;
    const double* block_sums_e;
    const double* block_totals_em;
    const int32_t* flag;
    int32_t* status;
    double* weights;       // out: e/S*valid of the own slots
    int32_t mode;
    const double* u;
    float u32;
    uint64_t seed, step;
    int32_t* ridx;
    const float* poses_prop;
    float* poses_out;
    double* weights_out;
    const int32_t* nn_idx;
    int32_t* hint_out;
    const double* part_rmse;
    int nrm;
    double* rmse_out;
    int64_t slot_base;     // Philox key offset of slot 0 (b * N for trajectory b of a batch)
};

// FROM_U (k_tail_b, k_tail_b2): the twin a systematic frame with u32 == MIDAS_U32_FROM_U launches - trajectory b's offset is the first
// double of its row of `u` (midas_math.hpp systematic_draw); every other frame launches the kernel it always did.
template <bool FROM_U>
__global__ __launch_bounds__(256) void k_tail_b(TailBArgs a) {
    __shared__ double s_bp[TB_MAX_BLOCKS];
    __shared__ double s_end[TB_MAX_BLOCKS];
    __shared__ double s_tot[2];
    if (blockIdx.y) {  // batch of trajectories
        const int64_t b = blockIdx.y, o = b * a.N;
        a.e += o; a.valid += o; a.lp += o; a.block_sums_e += b * a.nb; a.block_totals_em += b * a.nb;
        a.flag += b; a.status += 2 * b; a.weights += o;
        if (a.u) a.u += o;
        a.ridx += o; a.poses_prop += o * 16; a.poses_out += o * 16; a.weights_out += o; a.nn_idx += o; a.hint_out += o;
        if (a.part_rmse) { a.part_rmse += 2 * b * a.nrm; a.rmse_out += 2 * b; }
        a.slot_base += o;
    }
    const bool apply = a.flag[0] != 0;
    // fetch the block partials in parallel (s_bp <- totals of e*valid, s_end <- sums of e), then one thread
    // turns them into the sequential prefixes the spec asks for - no dependent global loads
    for (int b = threadIdx.x; b < a.nb; b += 256) { s_bp[b] = a.block_totals_em[b]; s_end[b] = apply ? a.block_sums_e[b] : 0.0; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int b = 0; b < a.nb; ++b) { const double w = s_bp[b]; s_bp[b] = acc; acc = acc + w; }
        s_tot[0] = acc;
        double S = 1.0;
        if (apply) {
            S = 0.0;
            for (int b = 0; b < a.nb; ++b) S = S + s_end[b];
        }
        s_tot[1] = S;
    }
    __syncthreads();
    const double total = s_tot[0], S = s_tot[1];
    const int64_t N = a.N;
    // cdf at the last slot of every block (the last block ends at N-1, forced to 1)
    for (int b = threadIdx.x; b < a.nb; b += 256) {
        const int64_t last = ((int64_t)(b + 1) << 12) - 1 < N - 1 ? ((int64_t)(b + 1) << 12) - 1 : N - 1;
        s_end[b] = cdf_at(a.lp, s_bp, total, last, N);
    }
    __syncthreads();
    const bool bad_total = !(total == total) || total == 0.0;
    const int st0 = a.status[0];
    const bool usable = st0 == 0 && !bad_total;
    if (blockIdx.x == 0 && threadIdx.x == 0 && bad_total) a.status[0] = st0 | ((total != total) ? 2 : 1);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        a.weights[i] = (a.e[i] / S) * (a.valid[i] ? 1.0 : 0.0);
        int32_t src = (int32_t)i;
        if (usable) {
            double t;
            bool upper;
            if (a.mode == MIDAS_RESAMPLE_MULTINOMIAL) {
                t = a.u ? a.u[i] : philox_uniform53((uint64_t)(a.slot_base + i), a.seed, a.step);
                upper = false;
            } else {
                const float r = systematic_draw<FROM_U>(a.u32, a.u, a.seed + (uint64_t)blockIdx.y, a.step);
                const float off = r / (float)N;
                t = (double)i / (double)N + (double)off;
                t = t >= 1.0 ? t - 1.0 : t;
                upper = true;
            }
            // block: first b whose end value is >= t (lower) / > t (upper)
            int lo = 0, hi = a.nb;
            while (hi > lo) {
                const int mid = lo + ((hi - lo) >> 1);
                const double c = s_end[mid];
                if (upper ? (c <= t) : (c < t)) lo = mid + 1; else hi = mid;
            }
            if (lo >= a.nb) {
                src = (int32_t)(N - 1);
            } else {
                // Inside the 4096-slot block: a binary search on the division-free comparison (BP + lp_i) vs t * total
                // locates the slot to within rounding (probes are what this kernel pays for: 12 is the minimum);
                // the exact predicate cdf_i = (BP + lp_i) / total < t (<= for the systematic mode) then walks to the
                // true boundary - it is monotone in i, so the result is exactly the lower/upper bound over the cdf
                // values the sharded path materialises.
                const int64_t b_lo = (int64_t)lo << 12, b_hi = b_lo + SCAN_BLOCK < N ? b_lo + SCAN_BLOCK : N;
                const double bp = s_bp[lo], tt = t * total;
                int64_t l2 = b_lo, h2 = b_hi;
                while (h2 > l2) {
                    const int64_t mid = l2 + ((h2 - l2) >> 1);
                    const double c = bp + a.lp[mid];
                    // (a negative total - raw weights of a negative cosine - turns the division-free comparison round)
                    const bool lft = total < 0.0 ? (upper ? (c >= tt) : (c > tt)) : (upper ? (c <= tt) : (c < tt));
                    if (lft) l2 = mid + 1; else h2 = mid;
                }
                if (l2 >= b_hi) l2 = b_hi - 1;
                // exact fix-up
                while (l2 > b_lo) {
                    const double c = cdf_at(a.lp, s_bp, total, l2 - 1, N);
                    if (upper ? (c <= t) : (c < t)) break;
                    --l2;
                }
                while (l2 < b_hi - 1) {
                    const double c = cdf_at(a.lp, s_bp, total, l2, N);
                    if (!(upper ? (c <= t) : (c < t))) break;
                    ++l2;
                }
                src = (int32_t)(l2 < N ? l2 : N - 1);
            }
        }
        a.ridx[i] = src;
        const float4* ps = reinterpret_cast<const float4*>(a.poses_prop + (int64_t)src * 16);
        float4* pd = reinterpret_cast<float4*>(a.poses_out + i * 16);
        float4 r0 = ps[0], r1 = ps[1], r2 = ps[2], r3 = ps[3];
        pd[0] = r0; pd[1] = r1; pd[2] = r2; pd[3] = r3;
        a.weights_out[i] = (a.e[src] / S) * (a.valid[src] ? 1.0 : 0.0);
        a.hint_out[i] = a.nn_idx[src];
    }
    if (a.part_rmse && blockIdx.x == 0) {
        __shared__ double s_rm[8];
        frame_rmse(a.part_rmse, a.nrm, N, s_rm, a.rmse_out, false, false);
    }
}

// TB2 (fused single-trajectory step, after TA2): decides the isclose guard from TA2's per-block extrema, then
// weights + resample + gather like TB, with the search restructured around round trips: the cumulative value
// at the end of every 16-slot chunk (TA2's chunk-end table + block prefix) sits in LDS, so a draw is located
// to its chunk without touching memory; four probes inside the chunk and the exact fix-up follow, and the
// gathers of the winner's pose / weight / hint travel together.  Above TB2_TAB chunks per LDS table the table
// holds every 2^cshift-th chunk end and the chunk is found with cshift probes of the global table.
constexpr int TB2_TAB = 8192;
#ifdef MIDAS_DEBUG_CLOCKS  // phase clocks of one workgroup (tools/variants.sh dbg "-DMIDAS_DEBUG_CLOCKS"; tools/tb2_clocks.py)
__device__ long long g_tb2_clk[16];
__device__ long long g_ta_clk[16];
#define TB2_CLK(k) if (blockIdx.x == 97 && threadIdx.x == 64) g_tb2_clk[k] = clock64();
#define TB2_WALL(k) if (threadIdx.x == 64) { if (blockIdx.x == 0) g_tb2_clk[8 + k] = wall_clock64(); if (blockIdx.x == 195) g_tb2_clk[10 + k] = wall_clock64(); if (blockIdx.x == 390) g_tb2_clk[12 + k] = wall_clock64(); }
#else
#define TB2_CLK(k)
#define TB2_WALL(k)
#endif

struct TailB2Args {
    int64_t N;
    int nb, ng, nt, cshift;   // blocks, chunks, table entries, chunks per table entry (log2)
    const double *e, *x_raw, *lp, *lp_raw, *gend, *gend_raw, *bsum_e, *btot, *btot_raw, *bmax, *bmin;
    const uint8_t* valid;
    int32_t softmax;
    int32_t* status;
    double* weights;
    int32_t mode;
    const double* u;
    float u32;
    uint64_t seed, step;
    int32_t* ridx;
    const float* poses_prop;
    float* poses_out;
    double* weights_out;
    const int32_t* nn_idx;
    int32_t* hint_out;
    const double* part_rmse;
    int nrm;
    double* rmse_out;
    int64_t tstride;  // > 0: batch with one table block per trajectory (pipelined batch), 0: array-major batch tables
};

template <bool FROM_U>
__global__ __launch_bounds__(256) void k_tail_b2(TailB2Args a) {
    // dynamic LDS sized to this launch (nt + 3 nb doubles) so that small N keeps several workgroups per CU
    extern __shared__ double s_dyn[];
    double* s_tab = s_dyn;            // [nt] block-local prefix at the chunk ends (TA2's table, every 2^cshift-th)
    double* s_bp = s_tab + a.nt;      // [nb] exclusive prefix of the block totals of e*valid
    double* s_w = s_bp + a.nb;        // [nb] block totals of e*valid
    double* s_se = s_w + a.nb;        // [nb] block sums of e
    __shared__ double s_ex[12];
    __shared__ double s_tot[2];
    __shared__ int s_apply;
    if (blockIdx.y) {  // batch of trajectories (plain strides)
        const int64_t b = blockIdx.y, o = b * a.N;
        if (a.tstride) {
            const int64_t ts = b * a.tstride;
            a.e += ts; a.x_raw += ts; a.lp += ts; a.lp_raw += ts; a.gend += ts; a.gend_raw += ts;
            a.bsum_e += ts; a.btot += ts; a.btot_raw += ts; a.bmax += ts; a.bmin += ts;
        } else {
            a.e += o; a.x_raw += o; a.lp += o; a.lp_raw += o; a.gend += b * a.ng; a.gend_raw += b * a.ng;
            a.bsum_e += b * a.nb; a.btot += b * a.nb; a.btot_raw += b * a.nb; a.bmax += b * a.nb; a.bmin += b * a.nb;
        }
        a.valid += o; a.status += 2 * b; a.weights += o;
        if (a.u) a.u += o;
        a.ridx += o; a.poses_prop += o * 16; a.poses_out += o * 16; a.weights_out += o; a.nn_idx += o; a.hint_out += o;
        if (a.part_rmse) { a.part_rmse += 2 * b * a.nrm; a.rmse_out += 2 * b; }
    }
    const int64_t slot_base = (int64_t)blockIdx.y * a.N;  // Philox key offset of slot 0
    const int t = threadIdx.x;
    const int64_t N = a.N;
    const int64_t i = (int64_t)blockIdx.x * 256 + t, ic = i < N ? i : N - 1;
    TB2_CLK(0)
    TB2_WALL(0)
    // ---- round trip 1: everything that does not depend on the guard (the softmax variant is the common one).
    // Loads sit in uniform branches only (a per-lane conditional load would be waited for one at a time).
    constexpr int TPT = TB2_TAB / 256, BPT = TB_MAX_BLOCKS / 256;
    const int nk = (a.nt + 255) >> 8, nbk = (a.nb + 255) >> 8;
    const int ng1 = a.ng - 1, nb1 = a.nb - 1, cs = a.cshift;
    double gv[TPT], bt[BPT], bs[BPT], bx[BPT], bn[BPT];
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        gv[k] = 0.0;
        if (k < nk) {
            int c = ((k * 256 + t + 1) << cs) - 1;
            c = c < ng1 ? c : ng1;
            gv[k] = a.gend[c];
        }
    }
#pragma unroll
    for (int k = 0; k < BPT; ++k) {
        bt[k] = 0.0; bs[k] = 0.0; bx[k] = 0.0; bn[k] = 0.0;
        if (k < nbk) {
            const int b = k * 256 + t, bc = b < nb1 ? b : nb1;
            bt[k] = a.btot[bc];
            bs[k] = a.bsum_e[bc];
            bx[k] = a.bmax[bc];
            bn[k] = a.bmin[bc];
        }
    }
    double e_i = a.e[ic];
    const bool ok_i = a.valid[ic] != 0;
    const double u_i = (!FROM_U && a.u) ? a.u[ic] : 0.0;  // (FROM_U: a systematic frame, `u` holds the row's offset only)
    TB2_CLK(1)
    // ---- guard: global extrema of x from TA2's per-block ones (NaN propagates)
    double mx = -INFINITY, mn = INFINITY;
    bool nan = false;
#pragma unroll
    for (int k = 0; k < BPT; ++k) {
        const int b = k * 256 + t;
        const bool in = b < a.nb;
        nan |= in && ((bx[k] != bx[k]) || (bn[k] != bn[k]));
        mx = in && bx[k] > mx ? bx[k] : mx;
        mn = in && bn[k] < mn ? bn[k] : mn;
        if (in) { s_w[b] = bt[k]; s_se[b] = bs[k]; }
    }
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const int j = k * 256 + t;
        if (j < a.nt) s_tab[j] = gv[k];
    }
    // (guard_publish<4>, spelled out: through the helper this kernel gets one more instruction)
    mx = wmax(mx);
    mn = wmin(mn);
    const bool wn = __any(nan);
    if ((t & 63) == 0) { s_ex[t >> 6] = mx; s_ex[4 + (t >> 6)] = mn; s_ex[8 + (t >> 6)] = wn ? 1.0 : 0.0; }
    __syncthreads();
    if (t == 0) {
        const GuardExtrema g = guard_collect<4>(s_ex);
        const bool apply = a.softmax && !(__builtin_fabs(g.mx - g.mn) <= ISCLOSE_ATOL);
        s_apply = apply ? 1 : 0;
        if (apply) {  // sequential sums in block order (the spec); reads and writes on different arrays so they pipeline
            double acc = 0.0, S = 0.0;
            for (int b = 0; b < a.nb; ++b) { s_bp[b] = acc; acc = acc + s_w[b]; S = S + s_se[b]; }
            s_tot[0] = acc;
            s_tot[1] = S;
        }
    }
    __syncthreads();
    const bool apply = s_apply != 0;
    const double* __restrict__ lp = a.lp;
    const double* __restrict__ esrc = a.e;
    const double* __restrict__ gend = a.gend;
    if (!apply) {
        // rare: every particle has the same score (or the softmax is off) - switch to the raw variant TA2 wrote
        lp = a.lp_raw; esrc = a.x_raw; gend = a.gend_raw;
        for (int b = t; b < a.nb; b += 256) s_w[b] = a.btot_raw[b];
        for (int j = t; j < a.nt; j += 256) {
            int c = ((j + 1) << cs) - 1;
            c = c < ng1 ? c : ng1;
            s_tab[j] = gend[c];
        }
        e_i = esrc[ic];
        __syncthreads();
        if (t == 0) {
            double acc = 0.0;
            for (int b = 0; b < a.nb; ++b) { s_bp[b] = acc; acc = acc + s_w[b]; }
            s_tot[0] = acc;
            s_tot[1] = 1.0;
        }
        __syncthreads();
    }
    TB2_CLK(2)
    const double total = s_tot[0], S = s_tot[1];
    const bool bad_total = !(total == total) || total == 0.0;
    const int st0 = a.status[0];
    const bool usable = st0 == 0 && !bad_total;
    if (blockIdx.x == 0 && t == 0 && bad_total) a.status[0] = st0 | ((total != total) ? 2 : 1);
    TB2_CLK(3)
    if (i < N) {
        a.weights[i] = (e_i / S) * (ok_i ? 1.0 : 0.0);
        int64_t src = i;
        if (usable) {
            double tq;
            bool upper;
            if (a.mode == MIDAS_RESAMPLE_MULTINOMIAL) {
                tq = a.u ? u_i : philox_uniform53((uint64_t)(slot_base + i), a.seed, a.step);
                upper = false;
            } else {
                const float r = systematic_draw<FROM_U>(a.u32, a.u, a.seed + (uint64_t)blockIdx.y, a.step);
                const float off = r / (float)N;
                tq = (double)i / (double)N + (double)off;
                tq = tq >= 1.0 ? tq - 1.0 : tq;
                upper = true;
            }
            const double tt = tq * total;
            // "still left of the answer": cumulative value < tt (multinomial, lower bound) / <= tt (systematic, upper bound)
            // (a negative total - raw weights of a negative cosine - turns the division-free comparison round: resample_search.hpp)
            const bool neg = total < 0.0;
            auto left = [&](double c) { return neg ? (upper ? (c >= tt) : (c > tt)) : (upper ? (c <= tt) : (c < tt)); };
            auto left_exact = [&](double c) { return upper ? (c <= tq) : (c < tq); };
            // cumulative e*valid at the end of table entry j
            auto tab = [&](int j) {
                int c = ((j + 1) << cs) - 1;
                c = c < ng1 ? c : ng1;
                return s_bp[c >> 8] + s_tab[j];
            };
            // table entry: first j with !left(tab(j)); 4-ary rounds (three independent LDS probes each), then binary
            int lo = 0, hi = a.nt;
            while (hi - lo >= 4) {
                const int q = (hi - lo) >> 2;
                const int m1 = lo + q, m2 = m1 + q, m3 = m2 + q;
                const bool p1 = left(tab(m1)), p2 = left(tab(m2)), p3 = left(tab(m3));
                if (p3) lo = m3 + 1;
                else if (p2) { lo = m2 + 1; hi = m3; }
                else if (p1) { lo = m1 + 1; hi = m2; }
                else hi = m1;
            }
            while (hi > lo) {
                const int mid = lo + ((hi - lo) >> 1);
                if (left(tab(mid))) lo = mid + 1; else hi = mid;
            }
            TB2_CLK(4)
            if (lo >= a.nt) lo = a.nt - 1;
            // chunk inside the entry (only when one entry spans several chunks)
            int64_t c_lo = (int64_t)lo << cs, c_hi = c_lo + ((int64_t)1 << cs);
            c_hi = c_hi < a.ng ? c_hi : a.ng;
            while (c_hi - c_lo > 1) {
                const int64_t mid = c_lo + ((c_hi - c_lo) >> 1);
                const double c = s_bp[(mid - 1) >> 8] + gend[mid - 1];
                if (left(c)) c_lo = mid; else c_hi = mid;
            }
            // the chunk's sixteen prefix values in one round trip; slot = number of them still left of the answer
            const int64_t s0 = c_lo << 4;
            const double bp = s_bp[c_lo >> 8];
            double v[SCAN_CHUNK];
#pragma unroll
            for (int j = 0; j < SCAN_CHUNK; ++j) {
                const int64_t sj = s0 + j;
                v[j] = lp[sj < N ? sj : N - 1];
            }
            const double v_prev = lp[s0 > 0 ? s0 - 1 : 0];  // last slot of the previous chunk (its own block prefix)
            const double bp_prev = s_bp[(s0 > 0 ? s0 - 1 : 0) >> 12];
            int pos = 0;
#pragma unroll
            for (int j = 0; j < SCAN_CHUNK; ++j) pos += (s0 + j < N && left(bp + v[j])) ? 1 : 0;
            int64_t l2 = s0 + pos;
            // exact fix-up: the predicate on cdf_i = (BP + lp_i) / total is monotone in i over the whole array; the two
            // neighbours of the boundary are normally inside the chunk just fetched
            double vm = 0.0, vp = 0.0;
#pragma unroll
            for (int j = 0; j < SCAN_CHUNK; ++j) { vm = (j == pos - 1) ? v[j] : vm; vp = (j == pos) ? v[j] : vp; }
            bool walk = false;
            if (pos > 0) walk |= !left_exact((l2 - 1 == N - 1) ? 1.0 : (bp + vm) / total);
            else if (l2 > 0) walk |= !left_exact((bp_prev + v_prev) / total);
            if (pos < SCAN_CHUNK && l2 < N) walk |= left_exact((l2 == N - 1) ? 1.0 : (bp + vp) / total);
            else walk = true;
            TB2_CLK(5)
            if (walk) {
                if (l2 >= N) l2 = N - 1;
                while (l2 > 0) {
                    if (left_exact(cdf_at(lp, s_bp, total, l2 - 1, N))) break;
                    --l2;
                }
                while (l2 < N - 1) {
                    if (!left_exact(cdf_at(lp, s_bp, total, l2, N))) break;
                    ++l2;
                }
            }
            src = l2;
        }
        TB2_CLK(6)
        a.ridx[i] = (int32_t)src;
        const float4* ps = reinterpret_cast<const float4*>(a.poses_prop + src * 16);
        const float4 r0 = ps[0], r1 = ps[1], r2 = ps[2], r3 = ps[3];
        const double e_s = esrc[src];
        const uint8_t ok_s = a.valid[src];
        const int32_t nn_s = a.nn_idx[src];
        float4* pd = reinterpret_cast<float4*>(a.poses_out + i * 16);
        pd[0] = r0; pd[1] = r1; pd[2] = r2; pd[3] = r3;
        a.weights_out[i] = (e_s / S) * (ok_s ? 1.0 : 0.0);
        a.hint_out[i] = nn_s;
        TB2_CLK(7)
        TB2_WALL(1)
    }
    if (a.part_rmse && blockIdx.x == 0) {
        __shared__ double s_rm[8];
        frame_rmse(a.part_rmse, a.nrm, N, s_rm, a.rmse_out, false, false);
    }
}
static bool tail_offset_from_u(const StepTailArgs& a) { return a.mode == MIDAS_RESAMPLE_SYSTEMATIC && a.u32 == MIDAS_U32_FROM_U; }
int launch_tail_b2(midas_ctx* ctx, const StepTailArgs& a, const TailTables& tb) {
    const int nb = (int)ceil_div(a.N, SCAN_BLOCK), ng = (int)ceil_div(a.N, SCAN_CHUNK);
    if (nb > TB_MAX_BLOCKS) return midas_set_error(ctx, MIDAS_ERR_INVALID, "N", "more than 4 M particles per GPU: shard them");
    // every workgroup of TB2 loads the table: keep it whole (one entry per chunk) while that is cheap, coarser
    // for large N where (N / 256 workgroups) x table bytes would dominate
    static const int tab_env = getenv("MIDAS_TB2_TAB") ? atoi(getenv("MIDAS_TB2_TAB")) : 0;
    const int tab_cap = tab_env > 0 ? (tab_env < TB2_TAB ? tab_env : TB2_TAB) : (ng <= TB2_TAB ? TB2_TAB : (ng <= 4 * TB2_TAB ? 2048 : 1024));  // measured at N = 300k / 1M
    int cshift = 0;
    while (ceil_div((int64_t)ng, (int64_t)1 << cshift) > tab_cap) ++cshift;
    const int nt = (int)ceil_div((int64_t)ng, (int64_t)1 << cshift);
    TailB2Args b;
    b.N = a.N; b.nb = nb; b.ng = ng; b.nt = nt; b.cshift = cshift;
    b.e = tb.e; b.x_raw = tb.x_raw; b.lp = tb.lp; b.lp_raw = tb.lp_raw; b.gend = tb.gend; b.gend_raw = tb.gend_raw;
    b.bsum_e = tb.bsum_e; b.btot = tb.btot; b.btot_raw = tb.btot_raw; b.bmax = tb.bmax; b.bmin = tb.bmin;
    b.valid = a.valid; b.softmax = a.softmax; b.status = a.status; b.weights = a.weights; b.mode = a.mode;
    b.u = a.u; b.u32 = a.u32; b.seed = a.seed; b.step = a.step; b.ridx = a.ridx; b.poses_prop = a.poses_prop;
    b.poses_out = a.poses_out; b.weights_out = a.weights_out; b.nn_idx = a.nn_idx; b.hint_out = a.hint_out;
    b.part_rmse = a.part_rmse; b.nrm = a.part_rmse ? particle_update_blocks(a.N) : 0; b.rmse_out = a.rmse_out;
    b.tstride = a.tstride;
    const dim3 grid((unsigned)ceil_div(a.N, 256), (unsigned)(a.batch > 1 ? a.batch : 1));
    const size_t lds = (size_t)(nt + 3 * nb) * sizeof(double);
    if (tail_offset_from_u(a)) hipLaunchKernelGGL(k_tail_b2<true>, grid, dim3(256), lds, ctx->stream, b);
    else hipLaunchKernelGGL(k_tail_b2<false>, grid, dim3(256), lds, ctx->stream, b);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

int launch_step_tail(midas_ctx* ctx, const StepTailArgs& a, int prof_slot_base) {
    const int nb = (int)ceil_div(a.N, SCAN_BLOCK);
    if (nb > TB_MAX_BLOCKS) return midas_set_error(ctx, MIDAS_ERR_INVALID, "N", "more than 4 M particles per GPU: shard them");
    if (tail_offset_from_u(a) && !a.u) return midas_set_error(ctx, MIDAS_ERR_INVALID, "u32", "MIDAS_U32_FROM_U without the uniforms' pointer");
    void* sc;
    const int B = a.batch > 1 ? a.batch : 1;
    int rc = midas_scratch(ctx, (size_t)B * nb * 2 * sizeof(double) + (size_t)B * sizeof(int32_t) + 64, &sc);
    if (rc) return rc;
    double* psum = (double*)sc;
    double* pw = psum + (size_t)B * nb;
    double* e = a.e;
    int32_t* flag = (int32_t*)(pw + (size_t)B * nb);
    if (!a.x) {  // deferred mode: the tail gathers the scores (B trajectories as grid.y, plain strides)
        const int ng = (int)ceil_div(a.N, SCAN_CHUNK);
        void* sc2;
        if ((rc = midas_scratch(ctx, (size_t)B * ((size_t)nb * 35 + (size_t)ng * 2) * sizeof(double), &sc2))) return rc;
        TailTables tb;
        tb.e = e; tb.x_raw = a.x_raw; tb.lp = a.cdf; tb.lp_raw = a.lp_raw;
        tb.bsum_e = psum; tb.btot = pw;
        tb.btot_raw = (double*)sc2; tb.bmax = tb.btot_raw + (size_t)B * nb; tb.bmin = tb.bmax + (size_t)B * nb;
        tb.gend = tb.bmin + (size_t)B * nb; tb.gend_raw = tb.gend + (size_t)B * ng;
        tb.ggend = tb.gend_raw + (size_t)B * ng; tb.ggend_raw = tb.ggend + (size_t)B * 16 * nb;
        if ((rc = launch_tail_a2(ctx, a.N, a.scores, a.nn_idx, a.valid, a.softmax, tb, a.status, B, a.score_stride))) return rc;
        prof_mark(ctx, prof_slot_base + 1);
        if ((rc = launch_tail_b2(ctx, a, tb))) return rc;
        prof_mark(ctx, prof_slot_base + 2);
        return MIDAS_OK;
    }
    if ((rc = launch_tail_a(ctx, a.N, a.x, a.valid, a.npart, 1, a.part_max, a.part_min, a.softmax, e, a.cdf, psum, pw, nullptr,
                            flag, a.status, B)))
        return rc;
    prof_mark(ctx, prof_slot_base + 1);
    TailBArgs b;
    b.N = a.N; b.nb = nb; b.e = e; b.valid = a.valid; b.lp = a.cdf; b.block_sums_e = psum; b.block_totals_em = pw;
    b.flag = flag; b.status = a.status; b.weights = a.weights; b.mode = a.mode; b.u = a.u; b.u32 = a.u32;
    b.seed = a.seed; b.step = a.step; b.ridx = a.ridx; b.poses_prop = a.poses_prop; b.poses_out = a.poses_out;
    b.weights_out = a.weights_out; b.nn_idx = a.nn_idx; b.hint_out = a.hint_out;
    b.part_rmse = a.part_rmse; b.nrm = a.part_rmse ? particle_update_blocks(a.N) : 0; b.rmse_out = a.rmse_out;
    b.slot_base = 0;
    if (tail_offset_from_u(a)) hipLaunchKernelGGL(k_tail_b<true>, dim3((unsigned)ceil_div(a.N, 256), (unsigned)B), dim3(256), 0, ctx->stream, b);
    else hipLaunchKernelGGL(k_tail_b<false>, dim3((unsigned)ceil_div(a.N, 256), (unsigned)B), dim3(256), 0, ctx->stream, b);
    LAUNCH_CHECK(ctx);
    prof_mark(ctx, prof_slot_base + 2);
    return MIDAS_OK;
}

#ifdef MIDAS_DEBUG_CLOCKS
__device__ long long g_tg_clk[64];  // (tail_group.hpp)
__device__ long long g_tg_w[8192];
int debug_tb2_clocks(long long* out16) { return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_tb2_clk), 16 * sizeof(long long)) == hipSuccess ? 0 : 1; }
int debug_ta_clocks(long long* out16) { return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_ta_clk), 16 * sizeof(long long)) == hipSuccess ? 0 : 1; }
// stamps of the grouped tail: out64 = two waves' phases, out_w (4096) = start / end per group wave [2 G, 2 G + 1], rmse workgroup
// [2048, 2049], list workgroups [2050 + 2 b, ..]; reset: all zero
int debug_tg_clocks(long long* io64, int reset) {
    if (reset) {
        static long long zero[8192];
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tg_w), zero, sizeof(zero));
        return hipMemcpyToSymbol(HIP_SYMBOL(g_tg_clk), zero, 64 * sizeof(long long)) == hipSuccess ? 0 : 1;
    }
    return hipMemcpyFromSymbol(io64, HIP_SYMBOL(g_tg_clk), 64 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
int debug_tg_waves(long long* out8192) { return hipMemcpyFromSymbol(out8192, HIP_SYMBOL(g_tg_w), 8192 * sizeof(long long)) == hipSuccess ? 0 : 1; }
#endif

MIDAS_WARM_TU(tail, k_tail_a2d)

}  // namespace midas
