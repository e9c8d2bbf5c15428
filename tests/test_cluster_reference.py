"""The cluster centres' yardsticks against each other, on the CPU: `oracle.cluster_centers` (numpy sums, scipy quaternions, eigh)
against `_recipes.cluster_reference` (exactly rounded sums, a Shepperd extraction for one- and two-member clusters) on every
input set of tests/test_gpu_cluster_pin.py - the far-off, collapsed, half-turn, degenerate and boundary sets included - so
that a kernel pinned to the reference is pinned to the oracle the loop tests compare with."""
import numpy as np
import pytest

from _recipes import (ROT_GAP_ASSERTED, ROT_TOL, assert_cluster, cluster_nan_set, cluster_reference, cluster_set_names, cluster_set_reference,
                      quat_shepperd64, shepperd_branch)
from oracle import oracle as orc


def _oracle_rows(s):
    """oracle.cluster_centers's rows in the order of the set's label_values (a value nobody carries: NaN rows)."""
    uniq, oc, os_ = orc.cluster_centers(s["poses"], s["w"], s["labels"])
    vals = s["label_values"]
    C = np.full((len(vals), 4, 4), np.nan, dtype=np.float32)
    S = np.full((len(vals), 3), np.nan, dtype=np.float32)
    at = {int(u): i for i, u in enumerate(uniq)}
    for j, v in enumerate(vals):
        if int(v) in at:
            C[j], S[j] = oc[at[int(v)]], os_[at[int(v)]]
    return C, S


@pytest.mark.parametrize("group", list(cluster_set_names()))
def test_oracle_against_the_exactly_summed_reference(group):
    """assert_cluster's bounds (the kernels' own), and more, since both sides are two-pass: the spreads agree to one float32
    ulp and a collapsed set's spread is exactly 0 on both sides."""
    log = {}
    for name in cluster_set_names()[group]:
        s, ref = cluster_set_reference(name)
        assert s["oracle"] and s["nonneg"]
        C, S = _oracle_rows(s)
        assert_cluster(C, S, ref, -(-len(s["labels"]) // 256), f"oracle on {name}", log=log)
        for i, r in enumerate(ref):
            if r["count"]:
                assert (np.abs(S[i].astype(np.float64) - r["std"]) <= np.spacing(r["std"])).all(), (name, i, S[i], r["std"])
                if (r["var"] == 0.0).all():
                    assert (S[i] == 0.0).all(), (name, i, S[i])
    print(f"oracle vs reference, {group}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in log.items()))
    assert log["t_total"] > 0


def test_reference_rules():
    """What the reference does where no sum is involved: empty label, NaN weight, the flatten rule's boundary, the eigen gap of the
    exactly degenerate pair, and the two extractions agreeing where both apply."""
    s, ref = cluster_set_reference("labels/missing")
    empty = [r for r in ref if r["count"] == 0]
    assert len(empty) == 1 and empty[0]["label"] == 77 and np.isnan(empty[0]["center"]).all() and np.isnan(empty[0]["std"]).all()
    _, twin = cluster_set_reference("nan/twin")
    for where in ("first", "last", "block2"):
        n = cluster_nan_set(where)
        assert int(np.isnan(n["w"]).sum()) == 1
        r = cluster_reference(n["poses"], n["w"], n["labels"], n["label_values"])
        assert r[0]["nan"] and np.isnan(r[0]["center"][:3]).all() and np.isnan(r[0]["std"]).all() and r[0]["count"] == twin[0]["count"]
        assert np.array_equal(r[1]["center"], twin[1]["center"]) and np.array_equal(r[1]["std"], twin[1]["std"])
    flat = {a: cluster_set_reference(f"flatten/{a}")[1][0]["flat"] for a in ("1e-8", "above", "below", "zero", "signed_zero", "all_zero", "below_f32")}
    assert flat == {"1e-8": True, "above": False, "below": True, "zero": True, "signed_zero": True, "all_zero": True, "below_f32": True}
    w = cluster_set_reference("flatten/1e-8")[0]["w"]
    assert w.dtype == np.float32 and np.float32(w.max() - w.min()) == np.float32(1e-8)
    assert cluster_set_reference("gap/degenerate")[1][0]["gap"] < 1e-15
    assert cluster_set_reference("gap/uniform")[1][0]["gap"] >= ROT_GAP_ASSERTED
    # scipy's extraction and Shepperd's, on float32 matrices of every branch: the same quaternion to the matrices' own 6e-8
    P = cluster_set_reference("straddle/0")[0]["poses"]
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(P[:, :3, :3].astype(np.float64)).as_quat()
    q[q[:, 3] < 0] *= -1.0
    assert np.bincount(shepperd_branch(P), minlength=4).min() >= 100
    assert np.abs(q - quat_shepperd64(P)).max() < 3e-7
    # ... and on a LONE float32 matrix, where nothing averages the difference out: the rotation each extraction gives back, as
    # float32.  The figure of DESIGN.md: it is half of assert_cluster's 2^-23, not more than it - the one- and two-member
    # clusters go to quat_shepperd64 because a kernel that is itself 2^-24 off would sit ON the bound, not because scipy breaks it.
    worst, lone = 0.0, 0
    for name in ("count/1000", "count/130", "size/1", "size/2", "gap/single"):
        s = cluster_set_reference(name)[0]
        for v in s["label_values"]:
            m = s["labels"] == v
            if 1 <= m.sum() <= 2:
                lone += 1
                Pm = s["poses"][m][:1]
                qs = Rotation.from_matrix(Pm[:, :3, :3].astype(np.float64)).as_quat()
                Ra = Rotation.from_quat(quat_shepperd64(Pm)[0]).as_matrix().astype(np.float32)
                Rb = Rotation.from_quat(qs[0]).as_matrix().astype(np.float32)
                worst = max(worst, float(np.abs(Ra.astype(np.float64) - Rb).max()))
    print(f"\nscipy's extraction against Shepperd's on the first matrix of {lone} one- and two-member clusters: "
          f"largest float32 rotation entry deviation {worst:.3g}")
    assert lone > 100 and 0.0 < worst <= ROT_TOL
