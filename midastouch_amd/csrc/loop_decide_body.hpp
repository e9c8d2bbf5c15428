// loop_decide_body.hpp - the body of k_loop_decide and k_loop_decide_rows (anneal_small.hip), included between their braces: in
// scope are the kernels' parameters and `floor_n`.
    if (blockIdx.y) {  // a batch of trajectories: LOOP_MAX_CLUSTERS cluster rows each; no select state (midas_loop_step_batch_draws'
        const int64_t b = blockIdx.y;  // ATen walk), or every trajectory's own histograms and state (midas_loop_step_batch_wide)
        ctl_i += b * LOOP_CTL_I; ctl_d += b * LOOP_CTL_D;
        centers_all += b * LOOP_MAX_CLUSTERS * 16; stds_all += b * LOOP_MAX_CLUSTERS * 3; counts_all += b * LOOP_MAX_CLUSTERS;
        centers_out += b * LOOP_MAX_CLUSTERS * 16; stds_out += b * LOOP_MAX_CLUSTERS * 3; rot += b * LOOP_MAX_CLUSTERS * 10;
        if (hist) { hist += b * SEL_HIST_WORDS; sel_state += b * SEL_STATE_WORDS; }
    }
    if (blockIdx.x == 1) { loop_rotations(ctl_i, counts_all, rot, centers_out); return; }
    const int t = threadIdx.x;
    if (!hist) {  // the decision alone (the batch's ATen walk: no radix select follows)
        if (t != 0) return;
        int mode, k;
        loop_decide(ctl_i, ctl_d, centers_all, stds_all, counts_all, centers_out, stds_out, floor_n, mode, k, aten_order != 0);
        return;
    }
    for (int i = t; i < SEL_HIST_WORDS; i += 256) hist[i] = 0u;
    for (int i = t; i < SEL_STATE_WORDS; i += 256) sel_state[i] = 0;
    __syncthreads();
    if (t != 0) return;
    int mode, k;
    loop_decide(ctl_i, ctl_d, centers_all, stds_all, counts_all, centers_out, stds_out, floor_n, mode, k, aten_order != 0);
    if (frozen && mode) {  // the caller said annealing cannot act and no selection was launched: the set stays, the frame says so
        ctl_i[LOOP_I_ERR] |= 128;
        ctl_i[LOOP_I_MODE] = 0; ctl_i[LOOP_I_K] = 0; ctl_i[LOOP_I_NSET] = ctl_i[LOOP_I_N];
        k = 0;
    }
    sel_state[0] = 0; sel_state[1] = 0; sel_state[2] = k;  // pass 0: empty prefix, rank k
