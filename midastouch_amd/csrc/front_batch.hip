// front_batch.hip - the batch form of k_frame_front (a grid row per trajectory, whole-record list scans) and the presort in
// front of it.
#include "front_wave.hpp"

namespace midas {

// =================================================================================================
// presort: the folded resample's sources, and an execution order that groups the slots by their hint
// =================================================================================================
// A particle wave's list scans start from the hinted entry's neighbour and vertex lists.  In slot order a wave's 64 particles start
// from ~50 different entries (c5, frames 20 - 70: the set sits on 200 - 600 entries per trajectory, the multinomial draws scatter
// them over the slots), so every list record a wave touches is a look-up and a line of its own; in an order that keeps equal hints
// together it is 3 - 5 entries per wave: the lanes ask for the SAME addresses.  The hint of slot n is nn_prev[src(n)] - known once
// the resample search is done - so the search moves out of the front into k_presort_search (one lane per slot, the front's own
// functions: same sources), and k_presort_group builds the order per chunk of 16384 slots in one workgroup: an LDS hash table of
// the chunk's hints (count per hint, first come first served), an exclusive scan of the counts, a scatter.  The order inside a
// group is whatever the LDS atomics made it; nothing depends on it (a particle's arithmetic does not know its lane).
constexpr int PS_CHUNK = 4096, PS_THREADS = 1024, PS_PER = PS_CHUNK / PS_THREADS, PS_TAB = 4096;  // (chunks of 16384 slots in one workgroup
// a trajectory: 18 us of serialised LDS atomics on 64 of the 256 CUs)
constexpr int PS_GEND_MAX = 2048;  // chunk ends the search kernel stages in LDS (N <= 32768); beyond, the two line fetches

MD void presort_offset_traj(ParticleUpdateArgs& a, int traj) {
    if (!traj) return;
    const int64_t b = traj, o = b * a.N, ts = b * a.rs.tstride;
    a.rs.e += ts; a.rs.x_raw += ts; a.rs.lp += ts; a.rs.lp_raw += ts; a.rs.gend += ts; a.rs.gend_raw += ts;
    a.rs.ggend += ts; a.rs.ggend_raw += ts; a.rs.bsum_e += ts; a.rs.btot += ts; a.rs.btot_raw += ts; a.rs.bmax += ts; a.rs.bmin += ts;
    a.rs.poses_prev += o * 16; a.rs.nn_prev += o; a.rs.status_prev += 2 * b;
    if (a.rs.ridx_out) a.rs.ridx_out += o;
    if (a.rs.u) a.rs.u += o;
    a.rs.key_base = o;
    a.rs.traj = traj;
}

// slot n -> src[n] (= lazy_source, what the front computes for itself otherwise), hint[n] = nn_prev[src].  Four waves a workgroup:
// every wave builds the block tables for itself (lazy_tables_wave), then the four copy the trajectory's chunk-end table (the
// softmax or the raw variant, as the guard decided) into LDS - N = 10 000: 5 KB - and a lane finds its chunk there; the scattered
// fetches of a search drop from 25 sixteen-byte pieces to 9 (this kernel is bound by the vector cache's look-up rate: 35 -> 15 us).
template <bool FU>
__global__ __launch_bounds__(256) void k_presort_search(ParticleUpdateArgs a, int32_t* __restrict__ src_out, int32_t* __restrict__ hint_out) {
    __shared__ alignas(16) double s_rs[4][LAZY_WAVE_LDS];
    __shared__ double s_gend[PS_GEND_MAX];
    const int traj = (int)blockIdx.y, t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int64_t o = (int64_t)traj * a.N;
    presort_offset_traj(a, traj);
    const LazyRecords rec = lazy_records_load(a.rs);
    lazy_tables_wave(a.rs, rec, s_rs[w]);
    const bool staged = a.rs.ng <= PS_GEND_MAX;
    if (staged) {
        const bool apply = s_rs[w][2 * LAZY_WAVE_LD + 2] != 0.0;  // (every wave computes the same guard)
        const double* __restrict__ g = apply ? a.rs.gend : a.rs.gend_raw;
        for (int i = t; i < a.rs.ng; i += 256) s_gend[i] = g[i];
        __syncthreads();
    }
    const int64_t n = (int64_t)blockIdx.x * 256 + t;
    if (n >= a.N) return;
    const int64_t src = staged ? lazy_source<lds_cdp, const double*, NoMid, FU>(a.rs, s_rs[w], n, a.N, LAZY_WAVE_LD, (lds_cdp)s_gend)
                               : lazy_source<const double*, const double*, NoMid, FU>(a.rs, s_rs[w], n, a.N, LAZY_WAVE_LD);
    if (a.rs.ridx_out) a.rs.ridx_out[n] = (int32_t)src;
    src_out[o + n] = (int32_t)src;
    hint_out[o + n] = a.rs.nn_prev[src];
    (void)lane;
}

// chunk c of trajectory b: order[o + base + pos] = slot, srcr[o + base + pos] = its source, equal hints adjacent
// deal > 0: the grouped sequence is dealt to the chunk's waves in runs of `deal` slots (wave w takes runs w, w + W, ...): a wave
// then holds 64 / deal entries' particles instead of one entry's - the particles of a hard entry (whose cooperative
// continuations serve one owner per pass) spread over many waves again, while `deal` lanes still ask for the same records.
__global__ __launch_bounds__(PS_THREADS) void k_presort_group(int64_t N, const int32_t* __restrict__ src, const int32_t* __restrict__ hint,
                                                              int32_t* __restrict__ order, int32_t* __restrict__ srcr, int deal) {
    __shared__ int s_key[PS_TAB];
    __shared__ int s_cnt[PS_TAB];
    __shared__ int s_w[PS_THREADS / 64];
    __shared__ int s_fail;
    const int t = threadIdx.x;
    const int64_t o = (int64_t)blockIdx.y * N, base = (int64_t)blockIdx.x * PS_CHUNK;
    const int64_t end = base + PS_CHUNK < N ? base + PS_CHUNK : N;
    for (int i = t; i < PS_TAB; i += PS_THREADS) { s_key[i] = -2; s_cnt[i] = 0; }
    if (t == 0) s_fail = 0;
    __syncthreads();
    int slot[PS_PER], rk[PS_PER], sv[PS_PER];
    int32_t hv[PS_PER];
#pragma unroll
    for (int j = 0; j < PS_PER; ++j) {  // the chunk's hints and sources: coalesced, all in flight together
        const int64_t n = base + (int64_t)j * PS_THREADS + t;
        const int64_t nc = n < end ? n : end - 1;
        hv[j] = hint[o + nc];
        sv[j] = src[o + nc];
    }
#pragma unroll
    for (int j = 0; j < PS_PER; ++j) {
        const int64_t n = base + (int64_t)j * PS_THREADS + t;
        slot[j] = -1; rk[j] = 0;
        if (n < end) {
            const int key = hv[j] < 0 ? -1 : hv[j];
            unsigned h = ((unsigned)key * 2654435761u) >> 20;  // 12 bits
            for (int probe = 0; probe < 64; ++probe) {
                const int old = atomicCAS(&s_key[h], -2, key);
                if (old == -2 || old == key) { slot[j] = (int)h; rk[j] = atomicAdd(&s_cnt[h], 1); break; }
                h = (h + 1) & (PS_TAB - 1);
            }
            if (slot[j] < 0) s_fail = 1;  // more distinct hints than the table takes: slot order for this chunk
        }
    }
    __syncthreads();
    // exclusive scan of the PS_TAB counts: eight per thread
    constexpr int E = PS_TAB / PS_THREADS;
    int v[E], mine = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) { v[k] = s_cnt[t * E + k]; mine += v[k]; }
    const int incl = wave_iscan_dpp(mine);  // (DPP row shifts and broadcasts: midas_math.hpp)
    if ((t & 63) == 63) s_w[t >> 6] = incl;
    __syncthreads();
    int run = incl - mine;
    for (int w = 0; w < (t >> 6); ++w) run += s_w[w];
    const bool fail = s_fail != 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < E; ++k) { s_cnt[t * E + k] = run; run += v[k]; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PS_PER; ++j) {
        const int64_t n = base + (int64_t)j * PS_THREADS + t;
        if (n < end) {
            int64_t pos = fail ? n - base : (int64_t)(s_cnt[slot[j]] + rk[j]);
            const int64_t W = (end - base) >> 6;  // whole waves of the chunk; the ragged rest keeps its place
            if (deal > 0 && !fail && pos < (W << 6)) {
                const int64_t q = pos / deal, within = pos - q * deal;
                pos = ((q % W) << 6) + (q / W) * deal + within;
            }
            order[o + base + pos] = (int32_t)n;
            srcr[o + base + pos] = sv[j];
        }
    }
}

// Both steps in ONE kernel for trajectories of up to PS_LP_MAX particles (c5: 10 000): a workgroup stages the trajectory's whole
// per-slot prefix table (80 KB) and its chunk-end table in LDS - coalesced - and every level of its slots' searches reads LDS;
// the only scattered fetch left is the hint nn_prev[src].  (The two-kernel form is bound by the vector cache's look-up rate on
// the searches' line fetches: 26 + 11 us at c5; this one is a launch less and ~12 us.)  Same sources, same grouping.
constexpr int PS_LP_MAX = 10240;
struct PresortLds {  // dynamic LDS of k_presort_fused
    double lp[PS_LP_MAX];
    double gend[PS_LP_MAX / SCAN_CHUNK];
    double rs[PS_THREADS / 64][LAZY_WAVE_LDS];
    int key[PS_TAB];
    int cnt[PS_TAB];
    int w[PS_THREADS / 64];
    int fail;
};
template <bool FU>
__global__ __launch_bounds__(PS_THREADS) void k_presort_fused(ParticleUpdateArgs a, int32_t* __restrict__ order, int32_t* __restrict__ srcr, int deal, int chunk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ps_raw[];
    PresortLds& L = *reinterpret_cast<PresortLds*>(ps_raw);
    const int traj = (int)blockIdx.y, t = threadIdx.x, wv = t >> 6;
    // chunk (<= PS_CHUNK, whole waves): slots per workgroup - the launcher cuts a trajectory into as many chunks as fill the CUs
    const int64_t N = a.N, o = (int64_t)traj * N, base = (int64_t)blockIdx.x * chunk;
    const int64_t end = base + chunk < N ? base + chunk : N;
    presort_offset_traj(a, traj);
    const LazyRecords rec = lazy_records_load(a.rs);
    lazy_tables_wave(a.rs, rec, L.rs[wv]);
    {
        const bool apply = L.rs[wv][2 * LAZY_WAVE_LD + 2] != 0.0;  // (every wave computes the same guard)
        const double2* __restrict__ lsrc = reinterpret_cast<const double2*>(apply ? a.rs.lp : a.rs.lp_raw);  // padded to 16 values (tables_of)
        const int n2 = (int)((N + 1) >> 1);
        for (int i = t; i < n2; i += PS_THREADS) reinterpret_cast<double2*>(L.lp)[i] = lsrc[i];
        const double* __restrict__ g = apply ? a.rs.gend : a.rs.gend_raw;
        for (int i = t; i < a.rs.ng; i += PS_THREADS) L.gend[i] = g[i];
        for (int i = t; i < PS_TAB; i += PS_THREADS) { L.key[i] = -2; L.cnt[i] = 0; }
        if (t == 0) L.fail = 0;
    }
    __syncthreads();
    int slot[PS_PER], rk[PS_PER], sv[PS_PER];
    int32_t hv[PS_PER];
#pragma unroll
    for (int j = 0; j < PS_PER; ++j) {
        const int64_t n = base + (int64_t)j * PS_THREADS + t;
        sv[j] = 0; hv[j] = -1;
        if (n < end) {
            const int64_t src = lazy_source<lds_cdp, lds_cdp, NoMid, FU>(a.rs, L.rs[wv], n, N, LAZY_WAVE_LD, (lds_cdp)L.gend, (lds_cdp)L.lp);
            if (a.rs.ridx_out) a.rs.ridx_out[n] = (int32_t)src;
            sv[j] = (int)src;
            hv[j] = a.rs.nn_prev[src];
        }
    }
#pragma unroll
    for (int j = 0; j < PS_PER; ++j) {
        const int64_t n = base + (int64_t)j * PS_THREADS + t;
        slot[j] = -1; rk[j] = 0;
        if (n < end) {
            const int key = hv[j] < 0 ? -1 : hv[j];
            unsigned h = ((unsigned)key * 2654435761u) >> 20;  // 12 bits
            for (int probe = 0; probe < 64; ++probe) {
                const int old = atomicCAS(&L.key[h], -2, key);
                if (old == -2 || old == key) { slot[j] = (int)h; rk[j] = atomicAdd(&L.cnt[h], 1); break; }
                h = (h + 1) & (PS_TAB - 1);
            }
            if (slot[j] < 0) L.fail = 1;
        }
    }
    __syncthreads();
    constexpr int E = PS_TAB / PS_THREADS;
    int v[E], mine = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) { v[k] = L.cnt[t * E + k]; mine += v[k]; }
    const int incl = wave_iscan_dpp(mine);  // (DPP row shifts and broadcasts: midas_math.hpp)
    if ((t & 63) == 63) L.w[t >> 6] = incl;
    __syncthreads();
    int run = incl - mine;
    for (int w = 0; w < (t >> 6); ++w) run += L.w[w];
    const bool fail = L.fail != 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < E; ++k) { L.cnt[t * E + k] = run; run += v[k]; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PS_PER; ++j) {
        const int64_t n = base + (int64_t)j * PS_THREADS + t;
        if (n < end) {
            int64_t pos = fail ? n - base : (int64_t)(L.cnt[slot[j]] + rk[j]);
            const int64_t W = (end - base) >> 6;
            if (deal > 0 && !fail && pos < (W << 6)) {
                const int64_t q = pos / deal, within = pos - q * deal;
                pos = ((q % W) << 6) + (q / W) * deal + within;
            }
            order[o + base + pos] = (int32_t)n;
            srcr[o + base + pos] = sv[j];
        }
    }
}

// per-wave rmse sums in SLOT order from the presorted front's per-slot terms: exactly what an unsorted wave leaves in part_rmse
__global__ __launch_bounds__(64) void k_rmse_parts(int64_t N, int nwaves, const double* __restrict__ terms, double* __restrict__ part_rmse) {
    const int64_t b = blockIdx.y, n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const double2 v = n < N ? reinterpret_cast<const double2*>(terms + 2 * b * N)[n] : make_double2(0.0, 0.0);
    const double p = wave_sum(v.x), q = wave_sum(v.y);
    if (threadIdx.x == 0) { part_rmse[2 * (b * nwaves + blockIdx.x)] = p; part_rmse[2 * (b * nwaves + blockIdx.x) + 1] = q; }
}

// the two launches in front of a frame front with folded resample and per-wave tables; fills a.pre_order / a.pre_src
int launch_presort(midas_ctx* ctx, ParticleUpdateArgs& a) {
    void *p_src = nullptr, *p_hint = nullptr, *p_order, *p_srcr;
    const size_t bytes = (size_t)a.batch * (size_t)a.N * sizeof(int32_t);
    int rc;
    if ((rc = midas_scratch(ctx, bytes, &p_order))) return rc;
    if ((rc = midas_scratch(ctx, bytes, &p_srcr))) return rc;
    static const int run_env = getenv("MIDAS_PRESORT_RUN") ? atoi(getenv("MIDAS_PRESORT_RUN")) : 8;
    const int run = (run_env == 1 || run_env == 2 || run_env == 4 || run_env == 8 || run_env == 16 || run_env == 32) ? run_env : 0;  // divisors of 64; else none
    static const bool fused_env = !(getenv("MIDAS_PRESORT_FUSED") && getenv("MIDAS_PRESORT_FUSED")[0] == '0');
    if (fused_env && a.N <= PS_LP_MAX) {
        // per device: the dynamic-LDS limit of the kernel and the CU count (a second GPU's context must not inherit the first's)
        constexpr int MAXDEV = 64;
        static bool attr_set[MAXDEV] = {};
        static int ncu_dev[MAXDEV] = {};
        const int di = ctx->device >= 0 && ctx->device < MAXDEV ? ctx->device : 0;
        if (!attr_set[di] || ctx->device != di) {
            MIDAS_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_presort_fused<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PresortLds)));
            MIDAS_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_presort_fused<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PresortLds)));
            attr_set[di] = true;
        }
        // One workgroup per CU is all the kernel's LDS allows, and a workgroup's life is a chain of round trips whatever its share: as many
        // chunks per trajectory as fill the chip (c5: 64 trajectories x 4 chunks of 2560 slots on 256 CUs instead of 3 of 4096 -
        // 285 / 270 -> 277 / 266 us per batch frame; 5 or 8 chunks - a second round of workgroups - lose: 290 / 285), whole waves each
        if (!ncu_dev[di] || ctx->device != di) {
            hipDeviceProp_t prop;
            ncu_dev[di] = (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
        }
        const int ncu = ncu_dev[di];
        static const int chunk_env = getenv("MIDAS_PRESORT_CHUNK") ? atoi(getenv("MIDAS_PRESORT_CHUNK")) : 0;
        int64_t nch = ceil_div(a.N, PS_CHUNK);
        if (ncu / a.batch > nch) nch = ncu / a.batch;
        int64_t chunk = ceil_div(ceil_div(a.N, nch), 64) * 64;
        if (chunk < 1024) chunk = 1024;  // (a chunk groups its own slots only: small ones share few list records)
        if (chunk_env >= 64 && chunk_env <= PS_CHUNK && chunk_env % 64 == 0) chunk = chunk_env;
        const dim3 grid((unsigned)ceil_div(a.N, chunk), (unsigned)a.batch);
        if (front_from_u(a))
            hipLaunchKernelGGL(k_presort_fused<true>, grid, dim3(PS_THREADS), sizeof(PresortLds), ctx->stream, a, (int32_t*)p_order, (int32_t*)p_srcr, run, (int)chunk);
        else
            hipLaunchKernelGGL(k_presort_fused<false>, grid, dim3(PS_THREADS), sizeof(PresortLds), ctx->stream, a, (int32_t*)p_order, (int32_t*)p_srcr, run, (int)chunk);
    } else {
        if ((rc = midas_scratch(ctx, bytes, &p_src))) return rc;  // (the two-kernel form hands sources and hints over through memory)
        if ((rc = midas_scratch(ctx, bytes, &p_hint))) return rc;
        if (front_from_u(a))
            hipLaunchKernelGGL(k_presort_search<true>, dim3((unsigned)ceil_div(a.N, 256), (unsigned)a.batch), dim3(256), 0, ctx->stream, a, (int32_t*)p_src, (int32_t*)p_hint);
        else
            hipLaunchKernelGGL(k_presort_search<false>, dim3((unsigned)ceil_div(a.N, 256), (unsigned)a.batch), dim3(256), 0, ctx->stream, a, (int32_t*)p_src, (int32_t*)p_hint);
        hipLaunchKernelGGL(k_presort_group, dim3((unsigned)ceil_div(a.N, PS_CHUNK), (unsigned)a.batch), dim3(PS_THREADS), 0, ctx->stream, a.N,
                           (const int32_t*)p_src, (const int32_t*)p_hint, (int32_t*)p_order, (int32_t*)p_srcr, run);
    }
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    a.pre_order = (const int32_t*)p_order;
    a.pre_src = (const int32_t*)p_srcr;
    if (a.gt16) {
        void* p_terms;
        if ((rc = midas_scratch(ctx, (size_t)a.batch * (size_t)a.N * 2 * sizeof(double), &p_terms))) return rc;
        a.pre_rmse_terms = (double*)p_terms;
    }
    return MIDAS_OK;
}

// the batch form (and its profiling twin); the other families: front.hip, front_folded.hip
bool launch_front_batch(const FrontLaunch& L, const FrontForm& f) {
    if (!(launch_if_form<2, 1, false, false>(L, f) || launch_if_form<2, 1, false, false, true>(L, f))) return false;
    if (L.a.pre_rmse_terms)  // presorted launch with rmse: the per-wave sums the tail reads, formed in slot order
        hipLaunchKernelGGL(k_rmse_parts, dim3((unsigned)L.nwaves, (unsigned)L.a.batch), dim3(64), 0, L.ctx->stream, L.a.N, L.nwaves,
                           (const double*)L.a.pre_rmse_terms, L.a.part_rmse);
    return true;
}
MIDAS_WARM_TU(front_batch, k_presort_search<false>)

}  // namespace midas
