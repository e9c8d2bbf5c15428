// loop_xe_body.hpp - the body of k_loop_xe and k_loop_xe_rows (loop_weights.hip), included between their braces: in scope are the
// kernels' parameters, `softmax`, `unit` and `clk`.
#ifdef MIDAS_ANNEAL_CLOCKS  // phase clocks of workgroup 0, thread 0 (anneal_clocks.hpp: XCK)
    const long long xck0 = wall_clock64();
#endif
    __shared__ double s_gtot[16];
    __shared__ double s_mx[4], s_mn[4];
    __shared__ int s_k[4], s_f[4];
    __shared__ double s_t[LDS_CHUNK_DOUBLES];
    if (blockIdx.y) {  // a batch of trajectories (midas_loop_step_batch): cap_n slots, K scores and a launch's block results per trajectory
        const int64_t b = blockIdx.y, o = b * cap_n, ob = b * gridDim.x;
        ctl_i += b * LOOP_CTL_I; scores += b * K; nn_idx += o; valid += o; x_out += o; e_out += o;
        bsum += ob; bmax += ob; bmin += ob; bkept += ob; bnan += ob;
    }
    const int blk = blockIdx.x, t = threadIdx.x;
    const int64_t bbase = (int64_t)blk * SCAN_BLOCK;
    // batched, unconditional loads on clamped indices (a branch around a load makes hipcc wait for each one in turn); clamped to
    // what the launch was sized for, not to the live count - the control block is a trip of its own, the indices and the scores
    // travel beside it (a slot behind the live count holds anything: its row number is clamped too, its values are masked)
    double v[SCAN_CHUNK];
    int32_t nn[SCAN_CHUNK];
    unsigned okbits = 0;
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int64_t i = bbase + (int64_t)k * 256 + t, ic = i < cap_n ? i : cap_n - 1;
        const int32_t r = nn_idx[ic];
        nn[k] = r < 0 ? 0 : ((int64_t)r >= K ? (int32_t)(K - 1) : r);
        okbits |= valid[ic] != 0 ? (1u << k) : 0u;
    }
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) v[k] = unit ? 1.0 : scores[nn[k]];
    const int64_t n = ctl_i[LOOP_I_N];
    if (bbase >= n) return;
    double mx = -INFINITY, mn = INFINITY;
    XCK(36);
    int kept = 0;
    bool nan = false;
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int64_t i = bbase + (int64_t)k * 256 + t;
        const bool in = i < n;
        const double xv = v[k];
        mx = in && xv > mx ? xv : mx;
        mn = in && xv < mn ? xv : mn;
        kept += in && ((okbits >> k) & 1u) ? 1 : 0;
        nan |= in && xv != xv;
        if (in) x_out[i] = xv;
    }
    XCK(37);  // scores there
    if (softmax) {
#pragma unroll
        for (int k = 0; k < SCAN_CHUNK; ++k) {
            v[k] = exp_spec(v[k] - 1.0);
            // four exponentials interleaved: each is a dependent chain of ~25 fma at ~20 cycles a step, and the workgroup's four
            // waves are alone on their SIMDs
            if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int k = 0; k < SCAN_CHUNK; ++k) {
        const int il = k * 256 + t;
        const bool in = bbase + il < n;
        if (in) e_out[bbase + il] = v[k];
        s_t[lds_chunk_pos(il)] = in ? v[k] : 0.0;
    }
    XCK(38);  // exponentials done, values stored
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK; ++j) v[j] = s_t[17 * t + j];  // the own chunk: slots 16 t .. 16 t + 15 of the block
    const double W = block_total(v, s_gtot);
    XCK(39);  // block total
    mx = wave_max_dpp(mx);  // (register moves; NaN never wins, as in the shuffle form - flagged beside)
    mn = wave_min_dpp(mn);
    kept = wave_isum_dpp(kept);
    const bool wnan = __any(nan);
    if ((t & 63) == 0) { s_mx[t >> 6] = mx; s_mn[t >> 6] = mn; s_k[t >> 6] = kept; s_f[t >> 6] = wnan ? 1 : 0; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w) {
            mx = s_mx[w] > mx ? s_mx[w] : mx;
            mn = s_mn[w] < mn ? s_mn[w] : mn;
            kept += s_k[w];
        }
        const int f = s_f[0] | s_f[1] | s_f[2] | s_f[3];
        bsum[blk] = W;
        bmax[blk] = f ? NAN : mx;  // NaN propagates, as torch.max / torch.min do
        bmin[blk] = f ? NAN : mn;
        bkept[blk] = kept;
        bnan[blk] = f;
    }
    XCK(40);
    XCK_COUNT(41);
