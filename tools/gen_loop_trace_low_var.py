#!/usr/bin/env python3
"""G19: G13's T = 64 frame trace of the reference's loop body (filter/filter.py:150-190) with the SYSTEMATIC resampler -
`pf.resampler(parts, resample="low_var")` (modules/particle_filter.py:251-261, 288-307) - driven through the REAL reference
functions (build container only; imports the reference, see tools/gen_goldens.py).

Everything but the resampler's mode is tools/gen_loop_trace.py's G13: the oracle's fixed-order float32 compose fed with the
reference's draw order, cluster centres from the oracle, DBSCAN, `torch.mean(cluster_stds)`, annealing and the resampler from the
reference.  Per frame: torch.manual_seed(3000 + t), the draws tn, rot (torch.normal, add_noise_to_odom's order), then the
resampler's ONE draw: `torch.rand(1)`, a float32 value - stored (`u32_t`), with the words the generator had consumed in its
current 624-word block in front of and behind it (`pos_t`: two values read off torch's generator state).

The kept sets are the reference's (torch.topk on the CPU: the replay runs the ATen tie rule), stored as digests like every
per-particle array (SHA-256 + head / tail).

low_var's loop leaves TRAILING ZERO ROWS when the last sample locations reach weightsSum[-1] (the cumsum of the normalised
weights may end below 1, or the last location wraps): such a frame is out of spec - the script refuses to write a fixture that
holds one (choose another seed).  With the seeds below every frame emitted all nSamples slots.
"""
import copy
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from gen_goldens import import_reference, new_pf  # noqa: E402
from gen_loop_trace import CB_SEED, D, K, N0, T, TRAJ_SEED, digest, sha  # noqa: E402

from midastouch_amd.synthetic import make_codebook, make_trajectory, mesh_scale  # noqa: E402
from midastouch_amd.torch_rng import _host_state_row  # noqa: E402
from oracle import oracle as orc  # noqa: E402

FRAME_SEED = 3000  # torch.manual_seed(FRAME_SEED + t) in front of frame t's draws


def stream_pos() -> int:
    """Words of the current 624-word block torch's default CPU generator has consumed (624: a new block is due)."""
    return int(_host_state_row(None).view(np.uint32)[624])


def run(pfm, name: str, init_ratio: float):
    from sklearn.neighbors import KDTree
    cb = make_codebook(K=K, D=D, seed=CB_SEED, mesh_points=20000)
    traj = make_trajectory(cb, T=T + 1, seed=TRAJ_SEED)
    pf = new_pf(pfm)
    pf.mesh_kdtree = KDTree(cb.mesh_vertices)
    shadow = new_pf(pfm)  # the same annealing on index markers: which particles the reference kept
    cb_feat = orc.R3_SE3(cb.poses)
    emb64 = torch.tensor(cb.embeddings).double()
    pf.init_noise = [mesh_scale(cb.extents) / 3.0 * init_ratio, 60.0 * init_ratio]
    torch.manual_seed(100)
    parts = pf.init_filter(torch.tensor(traj.gt_poses[0]), N0)
    idx0 = orc.nn6(orc.R3_SE3(parts.poses.numpy()), cb_feat)[0]
    poses = cb.poses[idx0].copy()
    labels = np.zeros(N0, dtype=np.int64)
    out = {"N0": N0, "K": K, "D": D, "T": T, "cb_seed": CB_SEED, "traj_seed": TRAJ_SEED, "frame_seed": FRAME_SEED, "poses0": poses.copy(),
           "cb_sha": np.str_(sha(cb.embeddings.astype(np.float32)))}
    aten_ann = orc.Annealer(ties="aten_cpu")  # the restatement of ATen's CPU top-k: must make the reference's choice in EVERY frame
    for t in range(1, T + 1):
        N = poses.shape[0]
        torch.manual_seed(FRAME_SEED + t)
        tn = torch.normal(mean=0.0, std=2e-4, size=(N, 3)).numpy()      # add_noise_to_odom's draws, its order (:326-335)
        rot = torch.normal(mean=0.0, std=0.5, size=(N, 3)).numpy()
        prop = orc.propagate(poses, traj.odoms[t], tn, rot)
        rt, rr = pfm.particle_rmse(pfm.Particles(torch.tensor(prop)), torch.tensor(traj.gt_poses[t]))
        nn_idx = orc.nn6(orc.R3_SE3(prop), cb_feat)[0]
        code = torch.tensor(traj.codes[t])[None]
        w_sim = pf.get_similarity(code, emb64[torch.as_tensor(nn_idx.astype(np.int64))], softmax=True)
        parts = pfm.Particles(torch.tensor(prop), w_sim.clone(), torch.tensor(labels))
        parts, drifted = pf.remove_invalid_particles(parts)
        if bool(drifted):  # filter.py:176-179
            prop = cb.poses[nn_idx].copy()
            parts.poses = torch.tensor(prop)
        w_pruned = parts.weights.clone().numpy()
        out[f"N_{t}"] = np.int64(N)
        out[f"rmse_{t}"] = np.array([rt.item(), rr.item()], dtype=np.float32)
        digest(out, f"nn_{t}", nn_idx.astype(np.int32))
        digest(out, f"wprune_{t}", w_pruned)
        out[f"drifted_{t}"] = np.bool_(bool(drifted))
        if (t - 1) % 50 == 0:  # count % 50 == 0, count = 0 on the first frame
            parts = pf.cluster_particles(parts)
            labels = parts.labels.numpy().astype(np.int64)
            digest(out, f"dbscan_{t}", labels.astype(np.int32))
        uniq, centers, stds = orc.cluster_centers(prop, w_pruned, labels)
        var = torch.mean(torch.tensor(stds))                       # filter.py:189
        assert np.float32(var.item()) == orc.cluster_var(stds, "aten_cpu"), "torch.mean differs from the restatement of ATen's sum"
        out[f"cl_labels_{t}"] = uniq.astype(np.int32)
        out[f"var_{t}"] = np.float32(var.item())
        shadow.particle_var = copy.copy(pf.particle_var)
        if hasattr(pf, "init_particles"):
            shadow.init_particles = pf.init_particles
        marker = pfm.Particles(torch.tensor(prop), parts.weights.clone(), torch.arange(N, dtype=torch.float64))
        parts = pf.annealing(parts, var)
        keep = shadow.annealing(marker, var).labels.numpy().astype(np.int64)
        assert len(keep) == len(parts) and torch.equal(parts.poses, torch.tensor(prop)[keep])
        assert np.array_equal(aten_ann.step(w_pruned, np.float32(var.item())), keep), f"frame {t}: aten_topk restatement differs from torch.topk"
        digest(out, f"keep_{t}", keep.astype(np.int32))
        n2 = len(parts)
        carried = parts.labels.clone()
        parts.labels = torch.arange(n2, dtype=torch.float64)             # marker: which slot each draw took
        # the resampler's one draw, read off the stream where it stands - then the stream is put back and the reference draws it
        state, pos0 = torch.get_rng_state(), stream_pos()
        u32 = torch.rand(1)
        pos1 = stream_pos()
        torch.set_rng_state(state)
        res = pf.resampler(parts, resample="low_var")
        assert stream_pos() == pos1, f"frame {t}: the resampler consumed other words than torch.rand(1)"
        if not bool((res.weights > 0).all()):
            raise SystemExit(f"frame {t}: low_var left trailing zero rows (the last sample locations reached weightsSum[-1]) - "
                             "such a frame is out of spec: choose another seed")
        ridx = res.labels.numpy().astype(np.int32)
        want, status = orc.resample_indices(parts.weights.numpy(), "low_var", u32=np.float32(u32.item()))
        assert status == 0 and np.array_equal(ridx, want), f"frame {t}: the oracle's systematic search differs from the reference's low_var loop"
        digest(out, f"ridx_{t}", ridx)
        out[f"N2_{t}"] = np.int64(n2)
        out[f"u32_{t}"] = np.float32(u32.item())
        out[f"pos_{t}"] = np.array([pos0, pos1], dtype=np.int32)
        src = keep[ridx]
        poses = prop[src]
        assert np.array_equal(res.poses.numpy(), poses)
        labels = carried.numpy().astype(np.int64)[ridx]
        print(f"  {name} t={t:2d} N={N:5d} -> {n2:5d} rmse_t={1e3 * rt.item():6.2f} mm kept={(w_pruned > 0).sum():5d} u32={u32.item():.7f}"
              f" clusters={list(uniq)} var={var.item():.3e}")
    path = os.path.join(REPO, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB; every frame emitted all nSamples slots")


def main():
    torch.set_num_threads(1)
    pfm, _ = import_reference()
    run(pfm, "g19_loop_trace_low_var", 0.15)


if __name__ == "__main__":
    main()
