#!/usr/bin/env python3
"""Generate tests/golden/g18_prune_edges.npz: the weights and the `drifted` flag of the REAL particle_filter.remove_invalid_particles
(modules/particle_filter.py:379-403, sklearn's KDTree over the mesh vertices queried with the float32 translations passed through
numpy) on the lattice world of tests/_recipes.py ("prune edges"): every case of every family - a vertex exactly on the threshold
sphere, at m^2 - 1 and at m^2 + 1 in every direction class, collinear entry / particle / vertex, the deciding vertex at the list
records 1 .. 256 and behind the list's end, ties, the tree's axis-aligned vertices, the field-decided distances - as the particles of
one call per threshold: the world of 131 u with invalid_dist = 131 u, 0, +inf, -1e-3 and NaN, and the world of 113 u (where
squared_threshold(thr) is thr^2 exactly, so that an on-sphere vertex has d2 == t2) with 113 u.

Like tools/gen_goldens.py this runs only where the reference can be imported (its import_reference() and new_pf are used); the fixture
holds data only: the particles' and the vertices' lattice coordinates as int32 (x = V 2^-16), the thresholds, w_out as bytes (the
weights going in are ones) and drifted.  A particle with a NaN translation is not in it: sklearn's query raises on NaN positions.

  G18 particle_filter.remove_invalid_particles at the predicate's edges    modules/particle_filter.py:379-403

The file is written entry by entry with fixed zip dates: a second run gives the same bytes.
Usage:  python tools/gen_prune_edges.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from _recipes import PE_DEGENERATE, PE_MS, PE_U, pe_world  # noqa: E402
from gen_anneal_rule import save_fixed  # noqa: E402
from gen_goldens import import_reference, new_pf  # noqa: E402


def main():
    from sklearn.neighbors import KDTree
    torch.set_num_threads(1)
    pfm, _ = import_reference()
    pf = new_pf(pfm)
    arrays = {"ms": np.array(PE_MS, dtype=np.int64)}
    for m in PE_MS:   # (131 u with the degenerate thresholds; 113 u, where t2 == thr^2 and an on-sphere vertex has d2 == t2)
        w = pe_world(m)
        pf.mesh_kdtree = KDTree(w.verts.astype(np.float64) * PE_U)
        P = torch.eye(4)[None].repeat(w.n, 1, 1).clone()
        P[:, :3, 3] = torch.tensor((w.parts * PE_U).astype(np.float32))
        thrs = np.array((w.thr,) + (PE_DEGENERATE if m == PE_MS[0] else ()), dtype=np.float64)
        w_out, drifted = [], []
        for thr in thrs:
            parts = pfm.Particles(P.clone(), torch.ones(w.n, dtype=torch.float64), torch.zeros(w.n))
            out, d = pf.remove_invalid_particles(parts, invalid_dist=float(thr))
            wo = out.weights.numpy()
            assert wo.shape == (w.n,) and np.isin(wo, (0.0, 1.0)).all()
            w_out.append(wo.astype(np.uint8))
            drifted.append(bool(d))
        arrays.update({f"parts_{m}": w.parts.astype(np.int32), f"verts_{m}": w.verts.astype(np.int32), f"thr_{m}": thrs,
                       f"w_out_{m}": np.stack(w_out), f"drifted_{m}": np.array(drifted)})
        print(f"m = {m}: {w.n} cases, {len(w.verts)} vertices, {len(thrs)} thresholds, kept {[int(x.sum()) for x in w_out]}")
    save_fixed("g18_prune_edges", arrays)


if __name__ == "__main__":
    main()
