#!/usr/bin/env python3
"""G14: two T = 16 frame traces of the reference's loop body (filter/filter.py:150-190) on ONE torch stream that runs across
guard frames, driven through the REAL reference functions (build container only; imports the reference as
tools/gen_loop_trace.py does).

The reference's `resampler` returns its input before it draws anything when the normalised weights are all zero or hold a NaN
(modules/particle_filter.py:237-241): after such a frame torch's generator has not moved.  G10b / G13 re-seed torch every frame,
so a replay that draws on those frames anyway is never caught by them.  Here torch is seeded ONCE (`torch.manual_seed(777)`
before frame 1) and every frame draws `torch.normal` tn, then rot, then whatever `resampler` itself draws:

  loop   clustering and annealing (floor 500, DBSCAN on frames with (t - 1) % 5 == 0), N0 = 2048.  odoms[6] is pushed 0.5 m off
         the mesh: frame 6 prunes every particle (drifted, CDF status 1), annealing still acts on its all-zero weights (a top-k
         over a fully tied array) and the resampler consumes nothing.
  fixed  no clustering or annealing, N = 2048: the same drift frame, and codes[12][3] = NaN - a frame whose weights are NaN
         (CDF status 2), which consumes nothing either.

A NaN frame in the clustering loop is out of scope: the reference's get_cluster_centers cannot run here (removed Tensor.eig,
theseus) - the cluster centres come from the oracle, as in G13 - and the oracle's np.linalg.eigh raises on NaN moments.

Per frame: N, N2, drifted, consumed (did `resampler` move the generator) and G13's digests (SHA-256 + head / tail of 32) of nn,
wprune, ridx, rmse - the loop trace also dbscan, cl_labels, var, keep.  Both traces end with tail_u = torch.rand(8, float64): the
position the stream is left at.  The motion model is the oracle's fixed-order float32 compose, as in G10b / G13.
The archive is written with fixed member dates: a re-run reproduces it byte for byte.
"""
import copy
import io
import os
import sys
import zipfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from gen_goldens import import_reference, new_pf  # noqa: E402
from gen_loop_trace import digest, sha  # noqa: E402

from midastouch_amd.synthetic import make_codebook, make_trajectory, mesh_scale  # noqa: E402
from oracle import oracle as orc  # noqa: E402

K, D, T, N0 = 3000, 256, 16, 2048
CB_SEED, TRAJ_SEED, STREAM_SEED = 1013, 2013, 777
FLOOR, CLUSTER_EVERY = 500, 5
T_DRIFT, SHIFT = 6, np.float32(0.5)
T_NAN, NAN_AT = 12, 3


def run(pfm, cb, traj, poses0, cluster: bool, tr: str, out: dict):
    from sklearn.neighbors import KDTree
    odoms, codes = traj.odoms.copy(), traj.codes.copy()
    odoms[T_DRIFT][:3, 3] += SHIFT
    guards = {T_DRIFT}
    if not cluster:
        codes[T_NAN][NAN_AT] = np.nan
        guards.add(T_NAN)
    assert all(T - g >= 3 for g in guards), "at least three frames follow each guard frame"
    pf = new_pf(pfm)
    pf.mesh_kdtree = KDTree(cb.mesh_vertices)
    shadow = new_pf(pfm)  # the same annealing on index markers: which particles the reference kept
    cb_feat = orc.R3_SE3(cb.poses)
    emb64 = torch.tensor(cb.embeddings).double()
    aten_ann = orc.Annealer(ties="aten_cpu")
    poses, labels = poses0.copy(), np.zeros(N0, dtype=np.int64)
    torch.manual_seed(STREAM_SEED)  # once: the stream runs across every frame
    for t in range(1, T + 1):
        N = poses.shape[0]
        tn = torch.normal(mean=0.0, std=2e-4, size=(N, 3)).numpy()      # add_noise_to_odom's draws, its order (:326-335)
        rot = torch.normal(mean=0.0, std=0.5, size=(N, 3)).numpy()
        st0 = torch.get_rng_state()
        prop = orc.propagate(poses, odoms[t], tn, rot)
        rt, rr = pfm.particle_rmse(pfm.Particles(torch.tensor(prop)), torch.tensor(traj.gt_poses[t]))
        nn_idx = orc.nn6(orc.R3_SE3(prop), cb_feat)[0]
        w_sim = pf.get_similarity(torch.tensor(codes[t])[None], emb64[torch.as_tensor(nn_idx.astype(np.int64))], softmax=True)
        parts = pfm.Particles(torch.tensor(prop), w_sim.clone(), torch.tensor(labels))
        parts, drifted = pf.remove_invalid_particles(parts)
        if bool(drifted):  # filter.py:176-179
            prop = cb.poses[nn_idx].copy()
            parts.poses = torch.tensor(prop)
        w_pruned = parts.weights.clone().numpy()
        k = f"{tr}_"
        out[k + f"N_{t}"] = np.int64(N)
        out[k + f"rmse_{t}"] = np.array([rt.item(), rr.item()], dtype=np.float32)
        digest(out, k + f"nn_{t}", nn_idx.astype(np.int32))
        digest(out, k + f"wprune_{t}", w_pruned)
        out[k + f"drifted_{t}"] = np.bool_(bool(drifted))
        keep = np.arange(N)
        if cluster:
            if (t - 1) % CLUSTER_EVERY == 0:
                parts = pf.cluster_particles(parts)
                labels = parts.labels.numpy().astype(np.int64)
                digest(out, k + f"dbscan_{t}", labels.astype(np.int32))
            uniq, _, stds = orc.cluster_centers(prop, w_pruned, labels)
            var = torch.mean(torch.tensor(stds))                       # filter.py:189
            assert np.float32(var.item()) == orc.cluster_var(stds, "aten_cpu"), "torch.mean differs from the restatement of ATen's sum"
            out[k + f"cl_labels_{t}"] = uniq.astype(np.int32)
            out[k + f"var_{t}"] = np.float32(var.item())
            shadow.particle_var = copy.copy(pf.particle_var)
            if hasattr(pf, "init_particles"):
                shadow.init_particles = pf.init_particles
            marker = pfm.Particles(torch.tensor(prop), parts.weights.clone(), torch.arange(N, dtype=torch.float64))
            parts = pf.annealing(parts, var, floor=FLOOR)
            keep = shadow.annealing(marker, var, floor=FLOOR).labels.numpy().astype(np.int64)
            assert len(keep) == len(parts) and torch.equal(parts.poses, torch.tensor(prop)[keep])
            assert np.array_equal(aten_ann.step(w_pruned, np.float32(var.item()), FLOOR), keep), \
                f"frame {t}: aten_topk restatement differs from torch.topk"
            digest(out, k + f"keep_{t}", keep.astype(np.int32))
        assert torch.equal(st0, torch.get_rng_state()), "only add_noise_to_odom and the resampler draw"
        n2 = len(parts)
        if cluster and t == T_DRIFT:
            assert n2 != N, "annealing acts on the drift frame's all-zero weights"
        carried = parts.labels.clone()
        parts.labels = torch.arange(n2, dtype=torch.float64)             # marker: which slot each draw took
        res = pf.resampler(parts)                                        # torch.multinomial's n2 draws - or none at all
        consumed = not torch.equal(st0, torch.get_rng_state())
        assert consumed == (t not in guards), f"frame {t}: consumed = {consumed}"
        assert (t == T_DRIFT) == bool(drifted)
        ridx = res.labels.numpy().astype(np.int32)
        digest(out, k + f"ridx_{t}", ridx)
        out[k + f"N2_{t}"] = np.int64(n2)
        out[k + f"consumed_{t}"] = np.bool_(consumed)
        src = keep[ridx]
        poses = prop[src]
        assert np.array_equal(res.poses.numpy(), poses)
        labels = carried.numpy().astype(np.int64)[ridx]
        print(f"  {tr} t={t:2d} N={N:5d} -> {n2:5d} kept={(w_pruned > 0).sum():5d} drifted={bool(drifted)} consumed={consumed}"
              + (f" clusters={list(uniq)} var={var.item():.3e}" if cluster else ""))
    out[f"{tr}_tail_u"] = torch.rand(8, dtype=torch.float64).numpy()  # where the stream ends


def save_fixed_dates(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01: the archive depends on its contents only."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(1)
    pfm, _ = import_reference()
    cb = make_codebook(K=K, D=D, seed=CB_SEED, mesh_points=20000)
    traj = make_trajectory(cb, T=T + 1, seed=TRAJ_SEED)
    pf = new_pf(pfm)
    pf.init_noise = [mesh_scale(cb.extents) / 3.0 * 0.15, 60.0 * 0.15]
    torch.manual_seed(100)
    parts = pf.init_filter(torch.tensor(traj.gt_poses[0]), N0)
    poses0 = cb.poses[orc.nn6(orc.R3_SE3(parts.poses.numpy()), orc.R3_SE3(cb.poses))[0]].copy()
    out = {"N0": N0, "K": K, "D": D, "T": T, "cb_seed": CB_SEED, "traj_seed": TRAJ_SEED, "stream_seed": STREAM_SEED,
           "floor": FLOOR, "cluster_every": CLUSTER_EVERY, "poses0": poses0, "cb_sha": np.str_(sha(cb.embeddings.astype(np.float32))),
           "shift": SHIFT, "shift_frame": T_DRIFT, "nan_frame": T_NAN, "nan_at": NAN_AT}
    run(pfm, cb, traj, poses0, True, "loop", out)
    run(pfm, cb, traj, poses0, False, "fixed", out)
    path = os.path.join(REPO, "tests", "golden", "g14_guard_trace.npz")
    save_fixed_dates(path, out)
    print(f"g14_guard_trace: {os.path.getsize(path) / 1024:.1f} KiB, sha256 {sha(np.fromfile(path, dtype=np.uint8))}")


if __name__ == "__main__":
    main()
