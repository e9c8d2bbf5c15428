// shard_route.hip - the sharded engine's exchange behind TA2 (tail.hip, launch_shard_tail_a): the global tables from the
// gathered block records, the resample on the gathered cdf (T4) or on the owner's side with rows that travel, the unpack.
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "tail_sums.hpp"
#include "peer_row.hpp"
#include "resample_search.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "the peer-mapped route kernel's completion protocol relies on gfx942 / gfx950 write-through store acknowledgement (see k_shard_route)"
#endif

namespace midas {

// TF (sharded path): every rank holds the gathered exchange records r1_all (one per rank, rec = 5 nb + 4 doubles:
//     nb block sums of e | nb block totals of e*valid | nb block totals of x*valid | nb block max x | nb block min x |
//     NaN count | kept count | sum |dt|^2 | sum angle^2 ) written by TA2 on each shard.  The isclose guard is decided
//     from the gathered extrema (as TB2 does on one GPU) and picks the softmax or the raw variant; then
//     weights = e / S * valid and cdf = (BP + lp) / total with S, BP, total summed sequentially over ALL shards'
//     blocks in global block order; the globally last slot is forced to 1; block 0 finalises status and rmse.
__global__ __launch_bounds__(256) void k_tail_fin(int64_t N, const double* __restrict__ e, const double* __restrict__ x_raw,
                                                  const double* __restrict__ lp, const double* __restrict__ lp_raw,
                                                  const uint8_t* __restrict__ valid,
                                                  double* __restrict__ weights, double* __restrict__ cdf_io, int G, int nb,
                                                  const double* __restrict__ r1_all, int rank, double n_total,
                                                  int32_t softmax, double* __restrict__ rmse_out,
                                                  int32_t* __restrict__ status) {
    __shared__ double s_w[TB_MAX_BLOCKS];
    __shared__ double s_se[TB_MAX_BLOCKS];
    __shared__ double s_ex[12];
    __shared__ double s_tot[3];
    __shared__ int s_apply;
    const int t = threadIdx.x;
    const int nb_all = G * nb, rec = 5 * nb + 4;
    const int my = rank * nb + (int)blockIdx.x;
    auto field = [&](int f, int i) { return r1_all[(int64_t)(i / nb) * rec + (int64_t)f * nb + (i % nb)]; };
    double mx = -INFINITY, mn = INFINITY;
    bool nan = false;
    for (int i = t; i < nb_all; i += 256) {
        const double u = field(3, i), v = field(4, i);
        nan |= (u != u) || (v != v);
        mx = u > mx ? u : mx;
        mn = v < mn ? v : mn;
        s_w[i] = field(1, i);
        s_se[i] = field(0, i);
    }
    guard_publish<4>(mx, mn, nan, s_ex);
    __syncthreads();
    if (t == 0) {
        const GuardExtrema g = guard_collect<4>(s_ex);
        s_apply = (softmax && !(__builtin_fabs(g.mx - g.mn) <= ISCLOSE_ATOL)) ? 1 : 0;
    }
    __syncthreads();
    const bool apply = s_apply != 0;
    if (!apply) {
        for (int i = t; i < nb_all; i += 256) s_w[i] = field(2, i);
        __syncthreads();
    }
    if (t == 0) {
        double bp = 0.0, total = 0.0, S = 0.0;
        for (int i = 0; i < nb_all; ++i) { if (i == my) bp = total; total = total + s_w[i]; S = S + s_se[i]; }
        s_tot[0] = bp; s_tot[1] = total; s_tot[2] = apply ? S : 1.0;
    }
    __syncthreads();
    const double bp = s_tot[0], total = s_tot[1], S = s_tot[2];
    if (blockIdx.x == 0 && t == 0) {
        double nans = 0.0, kept = 0.0, st2 = 0.0, sr2 = 0.0;
        for (int r = 0; r < G; ++r) {
            const double* fl = r1_all + (int64_t)r * rec + 5 * nb;
            nans += fl[0]; kept += fl[1]; st2 += fl[2]; sr2 += fl[3];
        }
        int st = nans != 0.0 ? 2 : 0;
        if (total != total) st |= 2;
        else if (total == 0.0) st |= 1;
        status[0] = st;
        status[1] = (int32_t)kept;
        if (rmse_out) { rmse_out[0] = __builtin_sqrt(st2 / n_total); rmse_out[1] = __builtin_sqrt(sr2 / n_total); }
    }
    const double* __restrict__ ev = apply ? e : x_raw;
    const double* __restrict__ lpv = apply ? lp : lp_raw;
    const bool is_last = rank == G - 1;
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK;
    double ee[SCAN_CHUNK], ll[SCAN_CHUNK];
    uint8_t ok[SCAN_CHUNK];
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {  // unconditional loads on clamped slots
        const int64_t i = base + (int64_t)j * 256 + t, ic = i < N ? i : N - 1;
        ee[j] = ev[ic]; ll[j] = lpv[ic]; ok[j] = valid[ic];
    }
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) {
        const int64_t i = base + (int64_t)j * 256 + t;
        if (i < N) {
            weights[i] = (ee[j] / S) * (ok[j] ? 1.0 : 0.0);
            cdf_io[i] = (is_last && i == N - 1) ? 1.0 : (bp + ll[j]) / total;
        }
    }
}
int launch_tail_fin(midas_ctx* ctx, int64_t N, const double* e, const double* x_raw, const double* lp, const double* lp_raw,
                    const uint8_t* valid, double* weights, double* cdf_io, int G, int nb, const double* r1_all, int rank,
                    double n_total, int32_t softmax, double* rmse_out, int32_t* status) {
    if ((int64_t)G * nb > TB_MAX_BLOCKS)
        return midas_set_error(ctx, MIDAS_ERR_INVALID, "G*nb", "more than 4 M particles in total in the sharded step");
    hipLaunchKernelGGL(k_tail_fin, dim3((unsigned)ceil_div(N, SCAN_BLOCK)), dim3(256), 0, ctx->stream, N, e, x_raw, lp, lp_raw, valid,
                       weights, cdf_io, G, nb, r1_all, rank, n_total, softmax, rmse_out, status);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// T4 (sharded path): resample local slot i (global slot slot_base + i) from the GLOBAL cdf and gather pose /
//     weight / hint rows of any shard; identity when the weights are unusable.  The shards' data arrive as ONE
//     all_gather of a packed per-rank record block:
//        [ cdf: n x f64 | weights: n x f64 | poses: n x 16 f32 | nn_idx: n x i32 ]   (n = particles per rank)
//     so global particle p lives in block p / n at row p % n.
struct PackView {
    const char* base;
    int64_t stride;  // bytes between rank blocks
    int64_t n;       // particles per rank
    MD const char* blk(int64_t p, int64_t& row) const {
        const int64_t r = p / n;
        row = p - r * n;
        return base + r * stride;
    }
    MD double cdf(int64_t p) const { int64_t row; const char* b = blk(p, row); return reinterpret_cast<const double*>(b)[row]; }
    MD double weight(int64_t p) const { int64_t row; const char* b = blk(p, row); return reinterpret_cast<const double*>(b + 8 * n)[row]; }
    MD const float4* pose(int64_t p) const { int64_t row; const char* b = blk(p, row); return reinterpret_cast<const float4*>(b + 16 * n) + 4 * row; }
    MD int32_t nn(int64_t p) const { int64_t row; const char* b = blk(p, row); return reinterpret_cast<const int32_t*>(b + 80 * n)[row]; }
};

struct TailResampleArgs {
    int64_t N;            // local slots
    int64_t N_all;        // global particles
    int64_t slot_base;
    PackView pk;
    const int32_t* status;
    int32_t mode;
    const double* u;      // local uniforms or null
    float u32;
    uint64_t seed, step;
    int32_t* ridx;        // local out: global source index
    float* poses_out;
    double* weights_out;
    int32_t* hint_out;
};

__global__ __launch_bounds__(256) void k_tail_resample(TailResampleArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const int64_t slot = a.slot_base + i, N = a.N_all;
    int64_t src = slot;
    if (a.status[0] == 0) {
        double t;
        bool upper;
        if (a.mode == MIDAS_RESAMPLE_MULTINOMIAL) {
            t = a.u ? a.u[i] : philox_uniform53((uint64_t)slot, a.seed, a.step);
            upper = false;
        } else {
            const float r = a.u32 >= 0.0f ? a.u32 : philox_uniform24(a.seed, a.step);
            const float off = r / (float)N;
            t = (double)slot / (double)N + (double)off;
            t = t >= 1.0 ? t - 1.0 : t;
            upper = true;
        }
        int64_t lo = 0, hi = N;
        while (hi > lo) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            const double c = a.pk.cdf(mid);
            if (upper ? (c <= t) : (c < t)) lo = mid + 1; else hi = mid;
        }
        src = lo < N ? lo : N - 1;
    }
    a.ridx[i] = (int32_t)src;
    const float4* ps = a.pk.pose(src);
    float4* pd = reinterpret_cast<float4*>(a.poses_out + i * 16);
    float4 r0 = ps[0], r1 = ps[1], r2 = ps[2], r3 = ps[3];
    pd[0] = r0; pd[1] = r1; pd[2] = r2; pd[3] = r3;
    a.weights_out[i] = a.pk.weight(src);
    a.hint_out[i] = a.pk.nn(src);
}
int launch_tail_resample(midas_ctx* ctx, const midas_tail_resample_args& r) {
    TailResampleArgs a;
    a.N = r.N; a.N_all = r.N_all; a.slot_base = r.slot_base;
    a.pk.base = (const char*)r.pack_all_dev; a.pk.stride = r.rank_stride; a.pk.n = r.n_per_rank;
    a.status = r.status_dev; a.mode = r.mode; a.u = r.u_dev; a.u32 = r.u32;
    a.seed = r.seed; a.step = r.step; a.ridx = r.ridx_dev;
    a.poses_out = r.poses_out_dev; a.weights_out = r.weights_out_dev; a.hint_out = r.hint_out_dev;
    hipLaunchKernelGGL(k_tail_resample, dim3((unsigned)ceil_div(r.N, 256)), dim3(256), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// ------------------------------------------------------------------------------------------------
// sharded step, owner-side resample: rows travel instead of whole shards
// ------------------------------------------------------------------------------------------------
// After the exchange of the per-block records (r1_all) every rank knows the GLOBAL block prefix, and the draw of
// a slot is a pure function of the slot (Philox keyed by the global slot, the replicated host uniforms, or the
// systematic comb) - so every rank can tell, for every slot of the whole filter, which rank OWNS the source particle
// (the block the draw falls in, on the exact predicate).  The owner then resolves the exact source inside its own
// tables and sends that one row (pose, weight, NN index) to the rank holding the slot: an all_to_all of N rows per
// rank in total, where gathering every shard's packed block moved G-1 times as much.
//   pass COUNT: for every global slot: owner o, destination d  ->  counts[d] += (o == me), counts[G + o] += (d == me)
//               (the split sizes of the all_to_all; the caller reads them back) ; status / rmse finalised
//   pass PACK : the slots this rank owns: source slot (search_in_block), record -> send buffer, segment d at the
//               exclusive prefix of the send counts ; the rank's own masked weights
// Record (88 bytes): int32 slot (local at the destination) | int32 global source | int32 NN index | pad | f64 weight |
// 16 x f32 pose.
constexpr int ROUTE_REC = 88;
struct ShardRouteArgs {
    int64_t N;        // particles per rank
    int G, rank, nb;  // ranks, this rank, blocks per rank
    const double* r1_all;
    const double *e, *x_raw, *lp, *lp_raw, *gend, *gend_raw, *ggend, *ggend_raw;
    const uint8_t* valid;
    const int32_t* nn_idx;
    const float* poses_prop;
    int32_t* status;
    double* rmse_out;
    double n_total;
    int32_t softmax, mode;
    const double* u_all;
    float u32;
    uint64_t seed, step;
    int32_t* counts;  // [2 G]
    int32_t* cursor;  // [G]
    char* send;
    double* weights;
    // fixed-capacity form (no count pass, no read-back): segment of destination d = rows [d * fixed_cap, + fixed_cap) of
    // `send`, unused rows keep slot -1 (the buffers were set to 0xFF); rows that do not fit go to `ovf` (gathered by all)
    int64_t fixed_cap = 0, ovf_cap = 0;
    char* ovf = nullptr;
    int32_t* ovf_count = nullptr;
    char* self_rows = nullptr;  // [N] the rows this rank owns AND needs (they never travel)
    // peer-mapped form: row `slot` of the destination's inbox, written in place (fine-grained memory, system-scope stores)
    char* const* peers = nullptr;
    // ... with the completion protocol inside this kernel (the C-side frame across processes): the LAST workgroup to finish
    // publishes frame `tag` in slot `rank` of every inbox's flag block and then waits (bounded) until the own inbox carries
    // every rank's tag - when the kernel ends this rank's inbox holds all N rows, and ONE wave polled for it.  (Polling from
    // every workgroup of the consumer was measured: 1563 waves reading one address until it changes cost 26 us per frame.)
    const char* own_inbox = nullptr;
    long long flag_off = 0;
    unsigned long long tag = 0;
    unsigned* done = nullptr;  // workgroups finished, zero between launches (reset by the last one)
    const guide_t *guide = nullptr, *guide_raw = nullptr;  // the shard's guide tables (GUIDE_BINS, midas_internal.hpp) or null
};

// (sys_store8 / sys_load8 / pack2: peer_row.hpp - the rows of the peer-mapped form are 128-byte lines written by sixteen lanes)
template <bool PACK>
__global__ __launch_bounds__(256) void k_shard_route(ShardRouteArgs a) {
    __shared__ double s_bp[TB_MAX_BLOCKS];
    __shared__ double s_end[TB_MAX_BLOCKS];
    __shared__ double s_se[TB_MAX_BLOCKS];
    __shared__ double s_ex[12];
    __shared__ double s_tot[3];
    __shared__ int s_apply, s_cnt[2], s_base[2];
    __shared__ int s_hist[128], s_soff[64];
    const int t = threadIdx.x;
    const int nb_all = a.G * a.nb, rec = 5 * a.nb + 4;
    auto field = [&](int f, int i) { return a.r1_all[(int64_t)(i / a.nb) * rec + (int64_t)f * a.nb + (i % a.nb)]; };
    // ---- tables (as k_tail_fin): guard, sequential prefix over all blocks, exact cdf at the block ends
    double mx = -INFINITY, mn = INFINITY;
    bool nan = false;
    for (int i = t; i < nb_all; i += 256) {
        const double u = field(3, i), v = field(4, i);
        nan |= (u != u) || (v != v);
        mx = u > mx ? u : mx;
        mn = v < mn ? v : mn;
        s_end[i] = field(1, i);
        s_se[i] = field(0, i);
    }
    guard_publish<4>(mx, mn, nan, s_ex);
    if (t < 128) s_hist[t] = 0;
    if (t < 2) s_cnt[t] = 0;
    __syncthreads();
    if (t == 0) {
        const GuardExtrema g = guard_collect<4>(s_ex);
        s_apply = (a.softmax && !(__builtin_fabs(g.mx - g.mn) <= ISCLOSE_ATOL)) ? 1 : 0;
    }
    __syncthreads();
    const bool apply = s_apply != 0;
    if (!apply) {
        for (int i = t; i < nb_all; i += 256) s_end[i] = field(2, i);
        __syncthreads();
    }
    if (t == 0) {
        double acc = 0.0, S = 0.0;
        for (int i = 0; i < nb_all; ++i) { s_bp[i] = acc; acc = acc + s_end[i]; S = S + s_se[i]; }
        s_tot[0] = acc; s_tot[1] = apply ? S : 1.0;
        double nans = 0.0;
        for (int r = 0; r < a.G; ++r) nans += a.r1_all[(int64_t)r * rec + 5 * a.nb];
        s_tot[2] = nans;
        if (PACK) {  // segment offsets of the send buffer = exclusive prefix of the send counts (or fixed segments)
            int o = 0;
            for (int g = 0; g < a.G; ++g) { s_soff[g] = a.fixed_cap ? (int)(g * a.fixed_cap) : o; o += a.fixed_cap ? 0 : a.counts[g]; }
        }
    }
    __syncthreads();
    const double total = s_tot[0], S = s_tot[1];
    {   // exact cdf at the last slot of every block: (BP_b + W_b) / total (the block total is the block-local prefix at
        // the block's last slot); the globally last block ends at the last particle, forced to 1
        double wv[TB_MAX_BLOCKS / 256];
#pragma unroll
        for (int k = 0; k < TB_MAX_BLOCKS / 256; ++k) wv[k] = (k * 256 + t < nb_all) ? s_end[k * 256 + t] : 0.0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TB_MAX_BLOCKS / 256; ++k) {
            const int b = k * 256 + t;
            if (b < nb_all) {
                s_end[b] = (b == nb_all - 1) ? 1.0 : (s_bp[b] + wv[k]) / total;
                s_se[b] = wv[k];  // (the sums of e are summed up: the array now holds the block totals, the guide tables' bin width)
            }
        }
        __syncthreads();
    }
    const bool bad_total = !(total == total) || total == 0.0;
    const bool usable = s_tot[2] == 0.0 && !bad_total;
    if ((!PACK || a.fixed_cap || a.peers) && blockIdx.x == 0 && t == 0) {
        double kept = 0.0, st2 = 0.0, sr2 = 0.0;
        for (int r = 0; r < a.G; ++r) {
            const double* fl = a.r1_all + (int64_t)r * rec + 5 * a.nb;
            kept += fl[1]; st2 += fl[2]; sr2 += fl[3];
        }
        int st = s_tot[2] != 0.0 ? 2 : 0;
        if (total != total) st |= 2;
        else if (total == 0.0) st |= 1;
        if (a.own_inbox) atomicOr(&a.status[0], st);  // (zeroed by the front; the last workgroup may add the "flag late" bit)
        else a.status[0] = st;
        a.status[1] = (int32_t)kept;
        if (a.rmse_out) { a.rmse_out[0] = __builtin_sqrt(st2 / a.n_total); a.rmse_out[1] = __builtin_sqrt(sr2 / a.n_total); }
    }
    // ---- per global slot
    const int64_t N = a.N, N_all = (int64_t)a.G * N;
    const int64_t i = (int64_t)blockIdx.x * 256 + t;
    const bool live = i < N_all;
    const int d = live ? (int)(i / N) : 0;
    int o = d, b = 0;
    double tq = 0.0;
    bool upper = false, past = false;
    if (live && usable) {
        if (a.mode == MIDAS_RESAMPLE_MULTINOMIAL) {
            tq = a.u_all ? a.u_all[i] : philox_uniform53((uint64_t)i, a.seed, a.step);
        } else {
            const float r = a.u32 >= 0.0f ? a.u32 : philox_uniform24(a.seed, a.step);
            const float off = r / (float)N_all;
            tq = (double)i / (double)N_all + (double)off;
            tq = tq >= 1.0 ? tq - 1.0 : tq;
            upper = true;
        }
        int lo = 0, hi = nb_all;
        while (hi > lo) {
            const int mid = lo + ((hi - lo) >> 1);
            const double c = s_end[mid];
            if (upper ? (c <= tq) : (c < tq)) lo = mid + 1; else hi = mid;
        }
        past = lo >= nb_all;  // beyond every block end: the last particle
        b = past ? nb_all - 1 : lo;
        o = b / a.nb;
    }
    if (!PACK) {
        if (live) {
            if (o == a.rank) atomicAdd(&s_hist[d], 1);
            if (d == a.rank) atomicAdd(&s_hist[64 + o], 1);
        }
        __syncthreads();
        if (t < a.G) {
            if (s_hist[t]) atomicAdd(&a.counts[t], s_hist[t]);
            if (s_hist[64 + t]) atomicAdd(&a.counts[a.G + t], s_hist[64 + t]);
        }
        return;
    }
    // ---- PACK: this rank's own masked weights, then the rows it owns
    const double* __restrict__ ev = apply ? a.e : a.x_raw;
    if (live && d == a.rank) {
        const int64_t il = i - (int64_t)a.rank * N;
        a.weights[il] = (ev[il] / S) * (a.valid[il] ? 1.0 : 0.0);
    }
    const bool mine = live && o == a.rank;
    if (a.peers) {
        // straight into the slot's row of the destination's inbox: the rows of a wave are staged in LDS and go out sixteen
        // lanes per row - whole 128-byte lines (peer_row.hpp)
        __shared__ unsigned long long s_stage[4][64][PEER_PIECES];
        __shared__ char* s_dst[4][64];
        const int w = t >> 6, lane = t & 63;
        const unsigned long long mm = __ballot(mine);
        if (mine) {
            int64_t src;
            if (!usable) src = i - (int64_t)a.rank * N;  // the resampler keeps the particles
            else if (past) src = N - 1;
            else
                src = search_in_block_t<const double*, const double*>(apply ? a.lp : a.lp_raw, apply ? a.gend : a.gend_raw, apply ? a.ggend : a.ggend_raw,
                                                                      b - a.rank * a.nb, N, a.rank == a.G - 1 ? N - 1 : -1, s_bp[b], total, tq, upper,
                                                                      (const double*)nullptr, apply ? a.guide : a.guide_raw, s_se[b]);
            const float4* ps = reinterpret_cast<const float4*>(a.poses_prop + src * 16);
            const float4 r0 = ps[0], r1 = ps[1], r2 = ps[2], r3 = ps[3];
            const double wgt = (ev[src] / S) * (a.valid[src] ? 1.0 : 0.0);
            const int k = __popcll(mm & ((1ull << lane) - 1ull));
            unsigned long long* st = s_stage[w][k];
            st[0] = pack2((int)(i - (int64_t)d * N), (int)((int64_t)a.rank * N + src));
            st[1] = pack2(a.nn_idx[src], d);
            st[2] = (unsigned long long)__double_as_longlong(wgt);
            st[3] = 0ull;
            st[4] = pack2f(r0.x, r0.y); st[5] = pack2f(r0.z, r0.w);
            st[6] = pack2f(r1.x, r1.y); st[7] = pack2f(r1.z, r1.w);
            st[8] = pack2f(r2.x, r2.y); st[9] = pack2f(r2.z, r2.w);
            st[10] = pack2f(r3.x, r3.y); st[11] = pack2f(r3.z, r3.w);
            s_dst[w][k] = a.peers[d] + (size_t)(i - (int64_t)d * N) * PEER_ROW;
        }
        __syncthreads();  // (uniform branch: every thread of the workgroup is here)
        peer_rows_store(s_stage[w], s_dst[w], __popcll(mm));
        if (a.own_inbox) {
            // The barrier waits for every wave's outstanding stores (s_waitcnt vmcnt(0) in front of s_barrier), and the row
            // stores are system-scope write-through stores: acknowledged = performed at the destination.  (That is a property of
            // gfx942 / gfx950's memory system, not of the programming model - which would want a release on every workgroup's
            // add: the build refuses any other target, below.)  So the count needs
            // no release of its own (a release fence here is a write-back of the XCD's whole L2 per workgroup: measured,
            // +7 us per launch); the workgroup that sees the full count publishes with a system-scope release store.
            __syncthreads();
            __shared__ int s_last;
            if (t == 0) s_last = __hip_atomic_fetch_add(a.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
            __syncthreads();
            if (s_last && w == 0) {
                if (lane == 0) __hip_atomic_store(a.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                PeerInboxSrc f;
                f.rows = a.own_inbox; f.flag_off = a.flag_off; f.tag = a.tag; f.G = a.G; f.rank = a.rank; f.peers = a.peers; f.status = a.status;
                peer_flags_publish_wait(f, true);
            }
        }
        return;
    }
    const int d0 = (int)(((int64_t)blockIdx.x * 256) / N);  // a workgroup spans at most two destinations (N >= 256)
    int pos = 0;
    {
        if (mine) pos = atomicAdd(&s_cnt[d - d0], 1);
        __syncthreads();
        if (t < 2 && s_cnt[t]) s_base[t] = atomicAdd(&a.cursor[d0 + t], s_cnt[t]);
        __syncthreads();
    }
    if (mine) {
        int64_t src;
        if (!usable) src = i - (int64_t)a.rank * N;  // the resampler keeps the particles
        else if (past) src = N - 1;
        else
            src = search_in_block(apply ? a.lp : a.lp_raw, apply ? a.gend : a.gend_raw, apply ? a.ggend : a.ggend_raw,
                                  b - a.rank * a.nb, N, a.rank == a.G - 1 ? N - 1 : -1, s_bp[b], total, tq, upper);
        char* rp = a.send + (size_t)(s_soff[d] + s_base[d - d0] + pos) * ROUTE_REC;
        if (a.fixed_cap && d == a.rank) {  // own slot, own source: stays here (systematic draws are mostly of this kind)
            rp = a.self_rows + (size_t)(s_base[d - d0] + pos) * ROUTE_REC;
        } else if (a.fixed_cap && s_base[d - d0] + pos >= a.fixed_cap) {  // segment full: the row travels in the overflow block
            const int q = atomicAdd(a.ovf_count, 1);
            if (q >= a.ovf_cap) rp = nullptr;  // lost: the caller sees ovf_count > ovf_cap (counts_dev[3 G])
            else rp = a.ovf + (size_t)q * ROUTE_REC;
        }
        if (rp) {
        const float4* ps = reinterpret_cast<const float4*>(a.poses_prop + src * 16);
        const float4 r0 = ps[0], r1 = ps[1], r2 = ps[2], r3 = ps[3];
        const double w = (ev[src] / S) * (a.valid[src] ? 1.0 : 0.0);
        const int32_t nn = a.nn_idx[src];
        // records are 8-byte aligned (88 = 8 x 11): everything goes out as 8-byte pieces
        reinterpret_cast<int2*>(rp)[0] = make_int2((int)(i - (int64_t)d * N), (int)((int64_t)a.rank * N + src));
        reinterpret_cast<int2*>(rp)[1] = make_int2(nn, d);  // d: the destination rank (read from overflow rows)
        *reinterpret_cast<double*>(rp + 16) = w;
        float2* p2 = reinterpret_cast<float2*>(rp + 24);
        p2[0] = make_float2(r0.x, r0.y); p2[1] = make_float2(r0.z, r0.w);
        p2[2] = make_float2(r1.x, r1.y); p2[3] = make_float2(r1.z, r1.w);
        p2[4] = make_float2(r2.x, r2.y); p2[5] = make_float2(r2.z, r2.w);
        p2[6] = make_float2(r3.x, r3.y); p2[7] = make_float2(r3.z, r3.w);
        }
    }
}
int launch_shard_route(midas_ctx* ctx, const midas_shard_route_args& r, const TailTables& tb, bool pack, const PeerRouteSync* sync) {
    const int nb = (int)ceil_div(r.N, SCAN_BLOCK);
    if ((int64_t)r.G * nb > TB_MAX_BLOCKS)
        return midas_set_error(ctx, MIDAS_ERR_INVALID, "G*nb", "more than 4 M particles in total in the sharded step");
    ShardRouteArgs a;
    a.N = r.N; a.G = r.G; a.rank = r.rank; a.nb = nb; a.r1_all = r.r1_all_dev;
    a.e = tb.e; a.x_raw = tb.x_raw; a.lp = tb.lp; a.lp_raw = tb.lp_raw; a.gend = tb.gend; a.gend_raw = tb.gend_raw;
    a.guide = tb.guide; a.guide_raw = tb.guide_raw;
    a.ggend = tb.ggend; a.ggend_raw = tb.ggend_raw;
    a.valid = r.valid_dev; a.nn_idx = r.nn_idx_dev; a.poses_prop = r.poses_prop_dev;
    a.status = r.status_dev; a.rmse_out = r.rmse_dev; a.n_total = (double)r.G * (double)r.N;
    a.softmax = r.softmax; a.mode = r.resample_mode; a.u_all = r.u_all_dev; a.u32 = r.u32; a.seed = r.seed; a.step = r.step;
    a.counts = r.counts_dev; a.cursor = r.counts_dev + 2 * r.G; a.send = (char*)r.send_dev; a.weights = r.weights_dev;
    const unsigned grid = (unsigned)ceil_div((int64_t)r.G * r.N, 256);
    if (pack && r.peers_dev) {  // rows stored straight into the destinations' inboxes
        a.peers = (char* const*)r.peers_dev;
        if (sync) { a.own_inbox = sync->inbox; a.flag_off = sync->flag_off; a.tag = sync->tag; a.done = reinterpret_cast<unsigned*>(const_cast<char*>(sync->inbox) + sync->flag_off + 64 * 8); }
        hipLaunchKernelGGL(k_shard_route<true>, dim3(grid), dim3(256), 0, ctx->stream, a);
    } else if (pack && r.fixed_cap > 0) {  // one pass, no counts: padded segments + overflow block
        a.fixed_cap = r.fixed_cap; a.ovf_cap = r.ovf_cap; a.ovf = (char*)r.ovf_dev; a.ovf_count = r.counts_dev + 2 * r.G + r.G;
        a.self_rows = (char*)r.self_dev;
        MIDAS_HIP_CHECK(ctx, hipMemsetAsync(r.self_dev, 0xFF, (size_t)r.N * ROUTE_REC, ctx->stream));
        MIDAS_HIP_CHECK(ctx, hipMemsetAsync(r.counts_dev, 0, (size_t)(3 * r.G + 1) * sizeof(int32_t), ctx->stream));
        MIDAS_HIP_CHECK(ctx, hipMemsetAsync(r.send_dev, 0xFF, (size_t)r.G * r.fixed_cap * ROUTE_REC, ctx->stream));
        MIDAS_HIP_CHECK(ctx, hipMemsetAsync(r.ovf_dev, 0xFF, (size_t)r.ovf_cap * ROUTE_REC, ctx->stream));
        hipLaunchKernelGGL(k_shard_route<true>, dim3(grid), dim3(256), 0, ctx->stream, a);
    } else if (pack) {
        hipLaunchKernelGGL(k_shard_route<true>, dim3(grid), dim3(256), 0, ctx->stream, a);
    } else {
        MIDAS_HIP_CHECK(ctx, hipMemsetAsync(r.counts_dev, 0, (size_t)3 * r.G * sizeof(int32_t), ctx->stream));
        hipLaunchKernelGGL(k_shard_route<false>, dim3(grid), dim3(256), 0, ctx->stream, a);
    }
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// rows: records to look at; dest >= 0: only rows addressed to that rank (overflow block), rows with slot -1 are padding
__global__ __launch_bounds__(256) void k_shard_unpack(int64_t N, const char* __restrict__ recv, int32_t* __restrict__ ridx,
                                                      float* __restrict__ poses_out, double* __restrict__ weights_out,
                                                      int32_t* __restrict__ hint_out, int32_t dest) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const char* rp = recv + (size_t)r * ROUTE_REC;
    const int2 h0 = *reinterpret_cast<const int2*>(rp), h1 = *reinterpret_cast<const int2*>(rp + 8);
    if (h0.x < 0 || (dest >= 0 && h1.y != dest)) return;
    const double w = *reinterpret_cast<const double*>(rp + 16);
    const float2* p2 = reinterpret_cast<const float2*>(rp + 24);
    float2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p2[k];
    const int64_t slot = h0.x;
    ridx[slot] = h0.y;
    hint_out[slot] = h1.x;
    weights_out[slot] = w;
    float2* pd = reinterpret_cast<float2*>(poses_out + slot * 16);
#pragma unroll
    for (int k = 0; k < 8; ++k) pd[k] = v[k];
}
int launch_shard_unpack(midas_ctx* ctx, int64_t N, const void* recv, int32_t* ridx, float* poses_out, double* weights_out,
                        int32_t* hint_out, int32_t dest) {
    hipLaunchKernelGGL(k_shard_unpack, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, (const char*)recv, ridx,
                       poses_out, weights_out, hint_out, dest);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// the N rows other ranks stored into this rank's inbox (row r = slot r)
__device__ __forceinline__ void unpack_peer_row(const char* __restrict__ inbox, int64_t r, int32_t* __restrict__ ridx, float* __restrict__ poses_out,
                                                double* __restrict__ weights_out, int32_t* __restrict__ hint_out) {
    const PeerRow v = peer_row_load(inbox, r);
    ridx[r] = (int32_t)(v.head[0] >> 32);
    hint_out[r] = (int32_t)(v.head[1] & 0xFFFFFFFFull);
    weights_out[r] = __longlong_as_double((long long)v.head[2]);
    unsigned long long* pd = reinterpret_cast<unsigned long long*>(poses_out + r * 16);
#pragma unroll
    for (int k = 0; k < 8; ++k) pd[k] = v.pose[k];
}

__global__ __launch_bounds__(256) void k_shard_unpack_peer(int64_t N, const char* __restrict__ inbox, int32_t* __restrict__ ridx,
                                                           float* __restrict__ poses_out, double* __restrict__ weights_out,
                                                           int32_t* __restrict__ hint_out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    unpack_peer_row(inbox, r, ridx, poses_out, weights_out, hint_out);
}
int launch_shard_unpack_peer(midas_ctx* ctx, int64_t N, const void* inbox, int32_t* ridx, float* poses_out, double* weights_out,
                             int32_t* hint_out) {
    hipLaunchKernelGGL(k_shard_unpack_peer, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, (const char*)inbox, ridx,
                       poses_out, weights_out, hint_out);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// Device-side completion flags of the peer-mapped exchange (the C-side sharded frame, midas_shard_step): behind its route
// kernel - a kernel boundary, so every row it stored is out - a rank stores the frame's tag into slot `rank` of the flag
// block that follows the N rows of every inbox; the unpack kernel of a rank waits until all G slots of its OWN inbox carry the
// tag.  That replaces the 4-byte collective the host-driven frame used as a barrier.  No cycle: a rank's flag kernel sits
// behind its record all_gather, which completes only when every rank has joined it - and every rank enqueues its join before
// its own waiting kernel.  The wait is bounded (2 s of the 100 MHz wall clock): on expiry status[0] gets bit 16 and the
// kernel goes on - a stuck peer must not hang the device.
__global__ void k_peer_flag_write(char* const* peers, int G, int rank, long long flag_off, unsigned long long tag) {
    const int d = threadIdx.x;
    if (d < G) __hip_atomic_store(reinterpret_cast<unsigned long long*>(peers[d] + flag_off) + rank, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
int launch_peer_flag_write(midas_ctx* ctx, void* const* peers, int G, int rank, int64_t flag_off, uint64_t tag) {
    hipLaunchKernelGGL(k_peer_flag_write, dim3(1), dim3(64), 0, ctx->stream, (char* const*)peers, G, rank, (long long)flag_off, (unsigned long long)tag);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

__global__ __launch_bounds__(256) void k_shard_unpack_peer_wait(int64_t N, const char* __restrict__ inbox, int32_t* __restrict__ ridx,
                                                                float* __restrict__ poses_out, double* __restrict__ weights_out,
                                                                int32_t* __restrict__ hint_out, int G, long long flag_off,
                                                                unsigned long long tag, int32_t* __restrict__ status,
                                                                char* const* __restrict__ peers, int rank) {
    // peers != NULL: this kernel also PUBLISHES the rank's completion flag (its first workgroup, before anybody waits): it was
    // launched behind the route kernel, so every row this rank stored is out - one launch fewer than a flag kernel of its own
    if (peers && blockIdx.x == 0 && (int)threadIdx.x < G)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(peers[threadIdx.x] + flag_off) + rank, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if ((int)threadIdx.x < G) {
        const unsigned long long* f = reinterpret_cast<const unsigned long long*>(inbox + flag_off) + threadIdx.x;
        const long long t0 = wall_clock64();
        bool late = false;
        while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < tag) {
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t0 > 200000000ll) { late = true; break; }
        }
        if (late && status) atomicOr(&status[0], 16);
    }
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    unpack_peer_row(inbox, r, ridx, poses_out, weights_out, hint_out);
}
int launch_shard_unpack_peer_wait(midas_ctx* ctx, int64_t N, const void* inbox, int32_t* ridx, float* poses_out, double* weights_out,
                                  int32_t* hint_out, int G, int64_t flag_off, uint64_t tag, int32_t* status, void* const* peers, int rank) {
    hipLaunchKernelGGL(k_shard_unpack_peer_wait, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, (const char*)inbox, ridx,
                       poses_out, weights_out, hint_out, G, (long long)flag_off, (unsigned long long)tag, status, (char* const*)peers, rank);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

// start-up self test of the peer data path (include/midas_hip.h)
__global__ void k_peer_probe_write(char* const* peers, int G, int rank, int nonce) {
    const int d = threadIdx.x;
    if (d < G) sys_store8(peers[d] + (size_t)rank * ROUTE_REC, pack2(nonce, rank));
}
__global__ void k_peer_probe_check(const char* inbox, int G, int nonce, int32_t* ok) {
    const int r = threadIdx.x;
    const bool good = r >= G || sys_load8(inbox + (size_t)r * ROUTE_REC) == pack2(nonce, r);
    const bool all = __all(good);
    if (r == 0) ok[0] = all ? 1 : 0;
}
int launch_peer_probe(midas_ctx* ctx, void* const* peers, const void* inbox, int G, int rank, int nonce, int32_t* ok) {
    if (peers) hipLaunchKernelGGL(k_peer_probe_write, dim3(1), dim3(64), 0, ctx->stream, (char* const*)peers, G, rank, nonce);
    else hipLaunchKernelGGL(k_peer_probe_check, dim3(1), dim3(64), 0, ctx->stream, (const char*)inbox, G, nonce, ok);
    LAUNCH_CHECK(ctx);
    return MIDAS_OK;
}

MIDAS_WARM_TU(shard_route, k_shard_unpack)

}  // namespace midas
