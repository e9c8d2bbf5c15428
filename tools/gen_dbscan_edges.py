#!/usr/bin/env python3
"""Generate tests/golden/g17_dbscan_edges.npz: the labels of the REAL particle_filter.cluster_particles (modules/particle_filter.py:208-228,
sklearn's DBSCAN with min_samples = N / 5) on the lattice cases of tests/_recipes.py whose min_samples is n // 5: probes with points
exactly on eps and a neighbour count exactly at (and one below) min_samples, single-pair bridges on eps and at m^2 + 1, border points
whose only link lies on eps, and the sets of 5 .. 9 points.  (Below 5 points min_samples is 0 and sklearn refuses: nothing to record.)

Like tools/gen_goldens.py this runs only where the reference can be imported (its import_reference() and new_pf are used, the call is
the one g9_dbscan of tools/gen_goldens_r2.py makes); the fixture holds data only.  The points are stored as small integers - the local
lattice coordinates - with k, the lattice offset and m per case: x = (local + off) 2^-k as float32, eps = m 2^-k; the labels as int16.

  G17 particle_filter.cluster_particles at the predicate's edges    modules/particle_filter.py:208-217

The file is written entry by entry with fixed zip dates: a second run gives the same bytes.
Usage:  python tools/gen_dbscan_edges.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from _recipes import db_fixture_cases  # noqa: E402
from gen_anneal_rule import save_fixed  # noqa: E402
from gen_goldens import import_reference, new_pf  # noqa: E402


def main():
    torch.set_num_threads(1)
    pfm, _ = import_reference()
    pf = new_pf(pfm)
    cases = db_fixture_cases()
    out = {"names": np.array([c["name"] for c in cases])}
    rec = {k: [] for k in ("n", "k", "m", "ms", "at")}
    offs, locs, labs, at = [], [], [], 0
    for c in cases:
        X = c["X"]
        n = len(X)
        P = torch.eye(4)[None].repeat(n, 1, 1).clone()
        P[:, :3, 3] = torch.tensor(X)
        parts = pfm.Particles(P, torch.ones(n, dtype=torch.float64), torch.zeros(n))
        lab = pf.cluster_particles(parts, eps=c["eps"]).labels.numpy()
        assert lab.shape == (n,) and n // 5 == c["ms"]
        local = c["V"] - np.asarray(c["off"], dtype=np.int64)
        assert np.abs(local).max() < (1 << 15) and np.abs(lab).max() < (1 << 15)
        for key, val in (("n", n), ("k", c["k"]), ("m", c["m"]), ("ms", c["ms"]), ("at", at)):
            rec[key].append(val)
        offs.append(c["off"])
        locs.append(local.astype(np.int16))
        labs.append(lab.astype(np.int16))
        at += n
    for key, vals in rec.items():
        out[f"case_{key}"] = np.array(vals, dtype=np.int64)
    out["case_off"] = np.array(offs, dtype=np.int64)
    out["local"] = np.concatenate(locs)
    out["labels"] = np.concatenate(labs)
    save_fixed("g17_dbscan_edges", out)
    print(f"{len(cases)} cases, {at} points")


if __name__ == "__main__":
    main()
