// front_objects_body.hpp - the body of k_front_small_objects and k_front_small_rows (front.hip), included between their braces: in
// scope are the kernels' parameters recs, row_object, a, nwaves and feat.
    const int64_t b = blockIdx.y, o = b * a.N;
    const ObjectRecord& r = recs[row_object[b]];
    const TreeView<Kd6> t6 = r.t6;
    const TreeView<Kd3> t3 = r.t3;
    a.vlist = r.vlist; a.vscr = r.vscr; a.field = r.field;
    a.sp.emb = r.emb; a.sp.norms = r.norms; a.sp.K = r.K;
    a.n_live += b * LOOP_CTL_I;
    a.poses_in += o * 16; a.poses_prop += o * 16; a.odom16 += b * 16;
    if (a.hint_in) a.hint_in += o;
    a.nn_idx += o; a.valid += o;
    if (a.gt16) { a.gt16 += b * 16; a.part_rmse += 2 * b * nwaves; }
    a.sp.stamps += b * a.score_stride; a.sp.scores += b * a.score_stride; a.sp.code += b * (int64_t)(a.sp.nj * 64);
    a.seed += (uint64_t)b;  // (the row, not its object: the draws of a single engine built with seed + row)
    if (a.tn) { a.tn += o * 3; a.rot += o * 3; }
    feat += o;
    if (threadIdx.x < 64 && (int)blockIdx.x < nwaves) particle_front_wave(a, (int64_t)blockIdx.x, nullptr, feat);
    __syncthreads();  // (as in k_front_small)
    particle_nn_prune_wg<4>(t6, t3, a, feat);
