// loop_weights_moments_body.hpp - the body of k_loop_weights_moments<Args> and k_loop_weights_moments_logmap<Args> (cluster.hip),
// included between their braces: in scope are the kernels' parameters and `FORM` (cluster_logmap.hpp), the form of the moments.
#ifdef MIDAS_ANNEAL_CLOCKS
    const long long wck0 = wall_clock64();
#endif
    __shared__ double s_w[4][CL_MOM];
    __shared__ double s_sum[LAZY_MAX_BLOCKS];
    __shared__ double s_red[8], s_ab[8];
    __shared__ int s_ired[8];
    if (blockIdx.y || loop_weights_every_row(a)) {  // a batch of trajectories (midas_loop_step_batch)
        labels += (int64_t)blockIdx.y * a.grid_n;
        part += (size_t)blockIdx.y * gridDim.x * LOOP_MAX_CLUSTERS * CL_MOM;
        loop_weights_batch(a, blockIdx.y);
    }
    const int t = threadIdx.x;
    const int64_t idx = (int64_t)blockIdx.x * 256 + t, ic = idx < a.grid_n ? idx : a.grid_n - 1;
    const LoopWeightsPre pre = loop_weights_prefetch(a, blockIdx.x == 0);
    const double e_i = a.e[ic], x_i = a.x[ic];
    const uint8_t v_i = a.valid[ic];
    const int32_t nn_i = a.nn_idx[ic];
    MomIn in = moments_load(ic, a.poses_prop, (const double*)nullptr, (const float*)nullptr, labels);  // (w: below)
    const int64_t n = a.ctl_i[LOOP_I_N];
    int C = a.ctl_i[LOOP_I_NCL] + 1;
    C = C > LOOP_MAX_CLUSTERS ? LOOP_MAX_CLUSTERS : C;
    if ((int64_t)blockIdx.x * 256 >= n && blockIdx.x != 0) return;
    WCK(24);
    const LoopWeightsHead h = loop_weights_head(a, pre, n, s_sum, s_red, s_ired);
    WCK(25);
    const bool live = idx < n;
    double w = 0.0;
    if (live) {
        w = loop_weight_store(a, h, idx, e_i, x_i, v_i);
        if (h.drifted) {  // every particle back onto its codebook pose; the moments are taken of the re-projected set
            const float4* s4 = reinterpret_cast<const float4*>(a.cb_poses + (size_t)nn_i * 16);
            float4* d4 = reinterpret_cast<float4*>(a.poses_prop + (size_t)idx * 16);
            const float4 r0 = s4[0], r1 = s4[1], r2 = s4[2], r3 = s4[3];
            d4[0] = r0; d4[1] = r1; d4[2] = r2; d4[3] = r3;
            in.P[0] = r0.x; in.P[1] = r0.y; in.P[2] = r0.z; in.P[3] = r0.w;
            in.P[4] = r1.x; in.P[5] = r1.y; in.P[6] = r1.z; in.P[7] = r1.w;
            in.P[8] = r2.x; in.P[9] = r2.y; in.P[10] = r2.z; in.P[11] = r2.w;
        }
    }
    in.w = (double)(float)w;  // particles.weights.float() (:161)
    WCK(26);
    if ((int64_t)blockIdx.x * 256 < n) moments_accumulate<FORM>(live, in, C, [](int c) { return (int64_t)(c - 1); }, part, s_w, skip);
    WCK(27);
    if (blockIdx.x == 0) loop_weights_finalise(a, h, pre, s_ab);
    WCK(28);
#ifdef MIDAS_ANNEAL_CLOCKS
    if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl_d[56 + 29] += 1.0;
#endif
