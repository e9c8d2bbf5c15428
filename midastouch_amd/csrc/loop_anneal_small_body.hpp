// loop_anneal_small_body.hpp - the body of k_loop_anneal_small<DECIDE> and k_loop_anneal_small_rows (anneal_small.hip), included
// between their braces: in scope are the kernels' parameters, `DECIDE` and `floor_n`.
#ifdef MIDAS_ANNEAL_CLOCKS
    const long long ck0 = wall_clock64();
#else
    const long long ck0 = 0;
#endif
    if (blockIdx.y) {  // a batch of trajectories (midas_loop_step_batch): `cap` particles and LOOP_MAX_CLUSTERS cluster rows per trajectory
        const int64_t b = blockIdx.y;
        ctl_i += b * LOOP_CTL_I; ctl_d += b * LOOP_CTL_D;
        centers_all += b * LOOP_MAX_CLUSTERS * 16; stds_all += b * LOOP_MAX_CLUSTERS * 3; counts_all += b * LOOP_MAX_CLUSTERS;
        centers_out += b * LOOP_MAX_CLUSTERS * 16; stds_out += b * LOOP_MAX_CLUSTERS * 3; rot += b * LOOP_MAX_CLUSTERS * 10;
        w += b * cap; src += b * cap;
    }
    if (DECIDE && blockIdx.x == 1) { loop_rotations(ctl_i, counts_all, rot, centers_out); ACK(7); return; }
    __shared__ int s_w[40];
    const int t = threadIdx.x;
    if (t == 0) {
        int mode = ctl_i[LOOP_I_MODE], k = ctl_i[LOOP_I_K];  // !DECIDE: a plan made by the host (midas_anneal_select)
        if (DECIDE) loop_decide(ctl_i, ctl_d, centers_all, stds_all, counts_all, centers_out, stds_out, floor_n, mode, k);
        const int n0 = ctl_i[LOOP_I_N];
        if (n0 > LOOP_SMALL_MAX) { ctl_i[LOOP_I_ERR] |= 4; mode = 0; }  // the caller's bound was wrong: no annealing, flagged
        s_w[36] = mode; s_w[37] = k; s_w[38] = n0; s_w[39] = 0;
    }
    __syncthreads();
    ACK(0);
    __shared__ uint64_t s_key[LOOP_SMALL_PAIRS];
    __shared__ int32_t s_idx[LOOP_SMALL_PAIRS];
    uint64_t wkey[16];
    small_keys(w, s_w[38], wkey);
    anneal_small_select(s_w, wkey, src, ctl_i, ctl_d, ck0, s_key, s_idx);
    if (threadIdx.x == 0) ctl_d_count(ctl_d, 35);  // launches that got here
