#!/usr/bin/env python3
"""Generate tests/golden/g15_anneal_rule.npz: the decisions of the REAL particle_filter.annealing (modules/particle_filter.py:405-447)
on inputs at the edges of its float32 rule.

Like tools/gen_goldens.py this runs only where the reference can be imported (its import_reference(), new_pf and marker_poses are
used); the fixture holds data only.  The inputs come from tests/_recipes.py (ANNEAL_FIXTURE_SETS, recipe_anneal_rule_cases), the
recipe the GPU tests build their cases with.  Per case: particle_var = a 0-dim float32 tensor holding `prev` (the first call:
tensor([inf])), init_particles = init, annealing(Particles(marker poses, weights, ids), torch.tensor(var), floor) - and what came
back: the ids, the count, particle_var and init_particles afterwards, or the class name of the exception raised.

  G15 particle_filter.annealing, one decision per case    modules/particle_filter.py:413-447

The file is written entry by entry with fixed zip dates: a second run gives the same bytes.
Usage:  python tools/gen_anneal_rule.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from _recipes import ANNEAL_FIXTURE_SETS, f32_bits, recipe_anneal_rule_cases  # noqa: E402
from gen_goldens import OUT, import_reference, marker_poses, new_pf  # noqa: E402


def fixture_weights(n, s):
    """Distinct weights (no tie: the kept set is the same under every tie rule), a permutation per set."""
    w = np.random.default_rng([1500, s]).permutation(n).astype(np.float64) + 1.0
    return w / w.sum()


def save_fixed(name, arrays):
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    torch.set_num_threads(1)
    pfm, _ = import_reference()
    out = {"sets": np.array([[int(f32_bits(v)), n, fl, init, int(main)] for v, n, fl, init, main in ANNEAL_FIXTURE_SETS], dtype=np.int64)}
    rec = {k: [] for k in ("set", "prev_bits", "var_bits", "tag", "kind", "count", "pv_after_bits", "init_after", "raises", "ids_at")}
    ids_all, at = [], 0
    for s, (var, n, floor, init, _main) in enumerate(ANNEAL_FIXTURE_SETS):
        w = fixture_weights(n, s)
        out[f"w_{s}"] = w
        for c in recipe_anneal_rule_cases(var, n, floor, init):
            pf = new_pf(pfm)  # particle_var = tensor([inf]): the first call
            if not np.isinf(c["prev"]):
                pf.particle_var = torch.tensor(c["prev"])
                assert pf.particle_var.dim() == 0 and pf.particle_var.dtype == torch.float32
            pf.init_particles = init
            parts = pfm.Particles(marker_poses(n), torch.tensor(w), torch.arange(n, dtype=torch.float32))
            v = torch.tensor(c["var"])
            assert v.dim() == 0 and v.dtype == torch.float32
            try:
                res = pf.annealing(parts, v, floor=floor)
                ids, raised = res.poses[:, 0, 3].numpy().astype(np.int32), ""
                assert np.array_equal(res.labels.numpy().astype(np.int32), ids) and len(res.weights) == ids.shape[0]
            except Exception as e:  # noqa: BLE001  (the out-of-spec case: OverflowError)
                ids, raised = np.zeros(0, dtype=np.int32), type(e).__name__
            for key, val in (("set", s), ("prev_bits", int(f32_bits(c["prev"]))), ("var_bits", int(f32_bits(c["var"]))), ("tag", c["tag"]),
                             ("kind", c["kind"]), ("count", ids.shape[0]),
                             ("pv_after_bits", int(f32_bits(np.float32(torch.as_tensor(pf.particle_var).reshape(-1)[0].item())))),
                             ("init_after", int(pf.init_particles)), ("raises", raised), ("ids_at", at)):
                rec[key].append(val)
            ids_all.append(ids)
            at += ids.shape[0]
    for key, vals in rec.items():
        out[f"case_{key}"] = np.array(vals) if key in ("tag", "kind", "raises") else np.array(vals, dtype=np.int64)
    out["ids"] = np.concatenate(ids_all).astype(np.int32)
    save_fixed("g15_anneal_rule", out)
    print(f"{len(rec['set'])} cases, raised: {sorted(set(rec['raises']) - {''})}")


if __name__ == "__main__":
    main()
