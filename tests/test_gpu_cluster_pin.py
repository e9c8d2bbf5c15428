"""`ops.cluster_centers` (k_cluster_moments + the 64-thread k_cluster_finish, cluster_rot.hpp's closed forms) pinned to
`_recipes.cluster_reference` - exactly rounded sums, eigh, a two-pass spread - with `_recipes.assert_cluster`'s derived bounds:
every size class of the finisher's staging, many and absent clusters, Shepperd's four branches, eigen gaps down to exactly 0,
clusters far from the origin and collapsed onto one pose, the flatten rule's boundary, a NaN weight.  tests/test_cluster_reference.py
pins the oracle to the same reference on the same sets; tests/test_gpu_cluster_finishers.py ties the other finishers in.
Needs an MI355X."""
import numpy as np
import pytest

from _recipes import (CL_DISTS, CL_ENV_SEEDS, CL_FLATTEN, CL_NAN_AT, CL_SIGMAS, CL_SIZES, CL_WKINDS, assert_cluster, cluster_nan_set,
                      cluster_reference, cluster_set_names, cluster_set_reference, shepperd_branch)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def run_set(dev, s, wdtype=None):
    """ops.cluster_centers on a set of _recipes.cluster_set -> (centres, spreads, counts) as numpy arrays."""
    from midastouch_amd import ops
    w = np.asarray(s["w"])
    if wdtype is not None:
        w = w.astype(wdtype)
    c, sd, cnt = ops.cluster_centers(torch.as_tensor(s["poses"]).to(dev), torch.as_tensor(w).to(dev), torch.as_tensor(s["labels"]).to(dev),
                                     torch.as_tensor(s["label_values"]).to(dev))
    return c.cpu().numpy(), sd.cpu().numpy(), cnt.cpu().numpy()


def check_set(dev, name, log, wdtype=None):
    s, ref = cluster_set_reference(name)
    c, sd, cnt = run_set(dev, s, wdtype)
    assert cnt.tolist() == [r["count"] for r in ref], name
    return assert_cluster(c, sd, ref, -(-len(s["labels"]) // 256), name, log=log)


def show(what, log):
    print(f"\n{what}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in log.items()))


@pytest.mark.parametrize("wdtype", [np.float64, np.float32])
@pytest.mark.parametrize("N", CL_SIZES)
def test_sizes_and_finisher_chunks(dev, N, wdtype):
    """One cluster; 32 768 particles are the 128 blocks one staging chunk of the 64-thread finisher holds, 32 769 reach its
    second chunk, 65 537 its third."""
    log = {}
    check_set(dev, f"size/{N}", log, wdtype)
    show(f"N = {N}, {np.dtype(wdtype).name} weights", log)


@pytest.mark.parametrize("name", cluster_set_names()["count"] + cluster_set_names()["labels"])
def test_cluster_counts_and_label_values(dev, name):
    """1 .. 1000 clusters over 4096 particles (beyond 64 nothing is skipped; at 1000 most clusters have no member in most
    workgroups, a few have none at all: NaN rows, count 0); label_values unsorted, with a value nobody carries in the middle,
    holding -1, 0 and 2^40; every translation negative with most clusters skipped by most workgroups."""
    log = {}
    s, ref = cluster_set_reference(name)
    if name == "labels/missing":
        assert [r["count"] == 0 for r in ref] == [False] * 4 + [True] + [False] * 5
    if name == "labels/wide":
        assert sorted(s["label_values"].tolist()) == [-1, 0, 1 << 40] and all(r["count"] > 1000 for r in ref)
    if name == "count/1000":
        cnt = np.array([r["count"] for r in ref])
        assert (cnt == 0).any() and (cnt == 1).any() and (cnt == 2).any()
    check_set(dev, name, log)
    show(name, log)


def test_shepperds_four_branches(dev):
    """Centres at pi - 1e-3, pi - 0.05 and exactly pi about x, y, z and (1,1,0)/sqrt 2 with 0.05 rad around them, and a set
    straddling tr = 0: from the inputs, every branch of the extraction receives at least 100 particles - and the half turns about an
    axis send a whole set through ONE of the three branches the comfortable sets never take."""
    log, total = {}, np.zeros(4, dtype=np.int64)
    for name in cluster_set_names()["shepperd"]:
        s, _ = cluster_set_reference(name)
        br = np.bincount(shepperd_branch(s["poses"]), minlength=4)
        total += br
        if name.startswith("pi/"):
            ax = name.split("/")[1]
            assert br[0] == 0, (name, br)
            if ax in ("x", "y", "z"):
                assert br[1 + "xyz".index(ax)] == 1000, (name, br)
            else:
                assert br[1] >= 100 and br[2] >= 100, (name, br)
        else:
            assert br.min() >= 100, (name, br)
        check_set(dev, name, log)
    assert total.min() >= 100, total
    show(f"Shepperd branches {total.tolist()}", log)


def test_eigen_gaps(dev):
    """Rotation spreads of 0.01 .. 2.0 rad, uniformly random rotations (gap 0.011), two groups 170 degrees apart, the exactly
    degenerate pair (finite and orthonormal, nothing more), a single member, a cluster whose weight sits on one particle."""
    log = {}
    for name in cluster_set_names()["gap"]:
        _, ref = cluster_set_reference(name)
        seen = check_set(dev, name, log)
        print(f"{name}: gap {ref[0]['gap']:.4g}, rotation deviation {seen['rot_dev']:.3g}")
        assert seen["rot_checked"] + seen["rot_arbitrary"] == 1, name
    assert log["rot_arbitrary"] == 1
    show("eigen gaps", log)


@pytest.fixture(scope="module")
def envelope(dev):
    """Every set of the spread envelope once: {(dist, sigma): [what assert_cluster saw, per set]} (an assertion error of any set
    is kept and raised by the test that asserts the bound)."""
    cells, errors = {}, []
    for name in cluster_set_names()["env"]:
        _, d, sg, kind, _seed = name.split("/")
        try:
            cells.setdefault((float(d), float(sg)), []).append((kind, check_set(dev, name, {})))
        except AssertionError as e:
            errors.append(str(e))
    return cells, errors


def test_spread_envelope_within_the_derived_bound(envelope):
    """Centres 0.05, 0.5, 1 and 10 m from the origin x sigma 2e-3 .. 2e-7 and 0 (the set collapsed onto one pose: the reference is
    exactly 0, the kernel stays under sqrt(E)) x random, flat and peaky weights: all inside assert_cluster's bound."""
    cells, errors = envelope
    assert not errors, f"{len(errors)} sets outside the bound:\n" + "\n".join(errors[:10])
    assert len(cells) == len(CL_DISTS) * len(CL_SIGMAS) and all(len(v) == len(CL_WKINDS) * CL_ENV_SEEDS for v in cells.values())


def test_spread_envelope_float32_agreement_table(envelope):
    """The table of DESIGN.md ("The cluster centre's arithmetic"): per (distance, sigma) cell, how many of the float32 spreads
    (12 sets x 3 axes) equal the two-pass reference's, the largest deviation as a fraction of the bound and the measured kappa ratio.
    Equality is asserted only where a float64 emulation of the two formulas showed none of 40 sets differing: abs(t) <= 0.05 with
    sigma >= 2e-5 and abs(t) <= 0.5 with sigma >= 2e-3."""
    cells, _ = envelope
    print("\nfloat32 spreads equal to the two-pass reference's, of 36 per cell (largest deviation / bound; measured kappa ratio)")
    print("  dist [m] | " + " | ".join(f"sigma {s:g}".center(20) for s in CL_SIGMAS))
    for d in CL_DISTS:
        row = []
        for sg in CL_SIGMAS:
            seen = [x for _, x in cells.get((d, sg), [])]
            eq, tot = sum(x["sd_equal"] for x in seen), sum(x["sd_total"] for x in seen)
            frac = max([x["sd_frac"] for x in seen], default=float("nan"))
            ratio = max([x["kappa_ratio"] for x in seen], default=float("nan"))
            row.append(f"{eq:2d}/{tot:2d} ({frac:.2f}; {ratio:5.1f})".center(20))
        print(f"  {d:8g} | " + " | ".join(row))
    for (d, sg), v in cells.items():
        if (d <= 0.05 and sg >= 2e-5) or (d <= 0.5 and sg >= 2e-3):
            eq, tot = sum(x["sd_equal"] for _, x in v), sum(x["sd_total"] for _, x in v)
            assert eq == tot, f"dist {d} m, sigma {sg}: {tot - eq} of {tot} float32 spreads differ from the two-pass reference's"


@pytest.mark.parametrize("case", CL_FLATTEN)
def test_flatten_boundary(dev, case):
    """float32 weights whose max - min is, in float32, exactly 1e-8, the next value above (weighted) and below it, 0, -0.0 beside
    +0.0; all zero; float64 weights that differ only below float32 resolution: the kernel flattens exactly where the reference does
    (a flattened set and a weighted one have different centres: the weights are 0 or d)."""
    log = {}
    s, ref = cluster_set_reference(f"flatten/{case}")
    assert ref[0]["flat"] == (case != "above")
    check_set(dev, f"flatten/{case}", log)
    if case in ("1e-8", "above", "below"):  # the other branch's centre is elsewhere: the check above can tell them apart
        other = cluster_reference(s["poses"], np.where(np.asarray(s["w"]) > 0, 1.0, 0.0) if ref[0]["flat"] else np.ones(len(s["w"])), s["labels"])
        assert np.abs(other[0]["center"][:3, 3] - ref[0]["center"][:3, 3]).max() > 1e-5
    show(f"flatten/{case}", log)


@pytest.mark.parametrize("where", CL_NAN_AT)
def test_nan_weight(dev, where):
    """One NaN weight in a cluster whose other weights are all equal - at particle 0, at the last particle, in the third workgroup.
    The reference's max - min is NaN, isclose is false, the weighted branch runs: rotation, translation and spread of that
    cluster are NaN (the bottom row stays 0 0 0 1), its count is its member count, and the other cluster is bit for bit what it
    is without the NaN."""
    s = cluster_nan_set(where)
    ref = cluster_reference(s["poses"], s["w"], s["labels"], s["label_values"])
    assert ref[0]["nan"] and not ref[1]["nan"]
    c, sd, cnt = run_set(dev, s)
    twin, twin_ref = cluster_set_reference("nan/twin")
    c0, sd0, cnt0 = run_set(dev, twin)
    assert cnt.tolist() == cnt0.tolist() == [r["count"] for r in ref]
    assert_cluster(c, sd, ref, 4, f"nan/{where}")
    assert_cluster(c0, sd0, twin_ref, 4, "nan/twin")
    assert np.array_equal(c[1], c0[1]) and np.array_equal(sd[1], sd0[1])
