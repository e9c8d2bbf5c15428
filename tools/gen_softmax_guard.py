#!/usr/bin/env python3
"""Generate tests/golden/g16_softmax_guard.npz: the weights of the REAL particle_filter.get_similarity (modules/particle_filter.py:449-469)
on clouds collapsed onto one score with ONE dissenting particle, at the edges of its isclose guard.

Like tools/gen_goldens.py this runs only where the reference can be imported (its import_reference() and new_pf are used); the fixture
holds data only.  The inputs come from tests/_recipes.py (guard_rows, GUARD_ROWS: the kinds a float32 codebook row can produce): the
query is the code e_0 as float64, the targets are N copies of the row (0, 1, 0, ...) with the kind's dissenting row at `slot`,
widened to float64 as filter/filter.py hands them over.  Per case: N, kind, slot and what get_similarity(query, targets) returned.

  G16 particle_filter.get_similarity, one dissenting slot    modules/particle_filter.py:459-468

The file is written entry by entry with fixed zip dates: a second run gives the same bytes.
Usage:  python tools/gen_softmax_guard.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from _recipes import GUARD_D, GUARD_ROWS, guard_rows  # noqa: E402
from gen_anneal_rule import save_fixed  # noqa: E402
from gen_goldens import import_reference, new_pf  # noqa: E402

SIZES = (2, 17, 4097)


def main():
    torch.set_num_threads(1)
    pfm, _ = import_reference()
    pf = new_pf(pfm)
    kinds = list(GUARD_ROWS)
    out = {"D": np.int64(GUARD_D), "kinds": np.array(kinds)}
    code = torch.zeros(1, GUARD_D, dtype=torch.float64)
    code[0, 0] = 1.0
    out["code"] = code.numpy()[0]
    rec = {k: [] for k in ("N", "kind", "slot", "w_at")}
    ws, at = [], 0
    for ki, kind in enumerate(kinds):
        base, row = guard_rows(kind)
        out[f"rows_{kind}"] = np.stack([base, row])
        for N in SIZES:
            for slot in (0, N - 1):
                targets = torch.tensor(base).double()[None].repeat(N, 1)
                targets[slot] = torch.tensor(row).double()
                w = pf.get_similarity(code, targets, softmax=True).numpy()
                assert w.shape == (N,) and w.dtype == np.float64
                for key, val in (("N", N), ("kind", ki), ("slot", slot), ("w_at", at)):
                    rec[key].append(val)
                ws.append(w)
                at += N
    for key, vals in rec.items():
        out[f"case_{key}"] = np.array(vals, dtype=np.int64)
    out["w"] = np.concatenate(ws)
    save_fixed("g16_softmax_guard", out)
    print(f"{len(rec['N'])} cases")


if __name__ == "__main__":
    main()
