"""The prune at its edges on the CPU: invalid = dist_to_nearest_vertex > pen_max (modules/particle_filter.py:379-403) on the lattice
world of tests/_recipes.py ("prune edges") against four statements of the same mask: the integer predicate |dV|^2 <= m^2 the recipes
carry, oracle.nn3_dist(...) > thr, sklearn's KDTree.query(k=1) called as the reference calls it (the float32 translations passed
through numpy), and fixture G18, written by the reference's own remove_invalid_particles (tools/gen_prune_edges.py).  The ulp family
- off the lattice, d2 exactly t2 = squared_threshold(thr) and the next double above it - is held to the oracle only: sklearn's
reduced distance is a plain sum of rounded squares, not the fma chain of the spec, and lands on either side of such a point.  Every
recipe asserts its own conditions while it builds its cases: the isolation of the regions, the ranks, the counts of the direction
classes ("The prune's rule").  No GPU."""
import numpy as np
import pytest

from _recipes import (PE_DEGENERATE, PE_DEPTHS, PE_FACE_MS, PE_LIST, PE_M, PE_M_STRICT, PE_MS, PE_TINY_SIZES, PE_U, PE_ULP_THRS, pe_classes, pe_degenerate_expected,
                      pe_face_world, pe_frames, pe_nan_pose, pe_orbit, pe_squared_threshold, pe_tiny_world, pe_ulp_d2, pe_ulp_world, pe_world)


@pytest.fixture(scope="module")
def w():
    return pe_world()   # (every recipe condition is asserted in here)


def _worlds():
    return [pe_world(m) for m in PE_MS] + [pe_face_world(m) for m in PE_FACE_MS] + [pe_tiny_world(nv) for nv in PE_TINY_SIZES]


def test_direction_classes_and_families(w):
    """18 classes on the sphere of 131, 40 at 131^2 +- 1 of both signs, the axis-aligned one among them; every family with both
    sides of its edge; the frames on both sides of the two-kernel form's limits."""
    on, below, above = pe_classes(PE_M), pe_classes(PE_M, -1), pe_classes(PE_M, 1)
    assert len(on) == 18 and len(below) + len(above) == 40 and below and above
    assert (0, 0, 131) in on and (6, 15, 130) in on and (6, 90, 95) in on and (0, 1, 131) in above and (2, 16, 130) in below
    assert len(pe_orbit((0, 0, 131))) == 6 and len(pe_orbit((6, 15, 130))) == 48
    fam = lambda f, k=None: int(((w.family == f) & ((w.kind == k) if k else True)).sum())  # noqa: E731
    assert fam("sphere", "on") == 2 * sum(len(pe_orbit(c)) for c in on)
    assert fam("sphere", "in") == sum(len(pe_orbit(c)) for c in below) and fam("sphere", "out") == sum(len(pe_orbit(c)) for c in above)
    assert fam("collinear") == 18 + 18 and fam("depth") == 4 * len(PE_DEPTHS) and fam("tie") == 6 and fam("tree") == 12 and fam("field") == 14
    for j in PE_DEPTHS:
        got = {c["kind"]: c for c in w.cases if c["family"] == "depth" and c["rank"] == j}
        assert sorted(got) == ["in", "none", "on", "out"] and got["on"]["d2"] == PE_M ** 2 and got["in"]["d2"] == PE_M ** 2 - 1 and got["out"]["d2"] == PE_M ** 2 + 1
        assert len(got["none"]["V"]) == j - 1 and not got["none"]["keep"]
    assert int(w.tree.sum()) == 4 + 12 + 1 and (w.rank[w.tree] > PE_LIST).all() and int(w.tree_open.sum()) == 2
    f = pe_frames(w)
    assert len(f["small"]) <= 512 and len(f["all"]) > 2048 and w.keep[f["shallow"]].all() and len(f["shallow"]) > 1000
    assert set(w.family[f["small"]]) == set(w.family)
    print(f"{w.n} cases, {len(w.verts)} vertices, kept {int(w.keep.sum())}")


def test_lt_for_le_and_thr_thr_change_the_mask(w):
    """A strict integer predicate prunes every on-sphere case and nothing else.  On the device the comparison is d2 <= t2 in double
    with t2 = squared_threshold(thr): for 131 u t2 lies one ulp above thr^2 - an on-sphere vertex has d2 < t2, and `<` for `<=` (or
    t2 = thr thr) changes NOTHING on that world; for 113 u t2 is thr^2 exactly and `<` prunes every on-sphere case of every family."""
    strict = (w.d2 >= 0) & (w.d2 < PE_M ** 2)
    assert np.array_equal(strict != w.keep, w.d2 == PE_M ** 2) and int((w.d2 == PE_M ** 2).sum()) > 1600
    for m, on_t2 in ((PE_M, False), (PE_M_STRICT, True)):
        wd = pe_world(m)
        t2, has = pe_squared_threshold(wd.thr), wd.d2 >= 0
        d2 = wd.d2.astype(np.float64) * PE_U * PE_U      # (exact: integers below 2^53 times a power of two)
        assert (t2 == wd.thr * wd.thr) == on_t2 and np.array_equal(has & (d2 <= t2), wd.keep)
        changed = (has & (d2 < t2)) != wd.keep
        assert np.array_equal(changed, (wd.d2 == m * m) if on_t2 else np.zeros(wd.n, dtype=bool))
        if on_t2:
            for fam in ("sphere", "collinear", "depth", "tie", "tree"):
                assert changed[wd.family == fam].any(), fam
            assert set(wd.rank[changed & (wd.family == "depth")]) == set(PE_DEPTHS)


def test_oracle_matches_the_integer_predicate(oracle):
    for wd in _worlds():
        d = oracle.nn3_dist(wd.poses, wd.verts64)
        assert np.array_equal(~(d > wd.thr), wd.keep), wd.m
        has = wd.d2 >= 0
        assert np.array_equal(d[has], np.sqrt(wd.d2[has].astype(np.float64)) * PE_U)   # (a power-of-two scale: sqrt commutes with it)
        t2 = pe_squared_threshold(wd.thr)
        assert np.array_equal(wd.d2[has].astype(np.float64) * PE_U * PE_U <= t2, wd.keep[has])
        idx = oracle.nn6(oracle.R3_SE3(wd.poses), oracle.R3_SE3(wd.cb_poses))[0]
        assert np.array_equal(idx, np.arange(wd.n))


def test_sklearn_kdtree_as_the_reference_calls_it():
    from sklearn.neighbors import KDTree
    for wd in _worlds():
        di = KDTree(wd.verts64).query(np.atleast_2d(wd.poses[:, :3, 3]), k=1, return_distance=True)[0].squeeze()
        assert np.array_equal(~(di > wd.thr), wd.keep), wd.m


def test_fixture_g18(golden):
    g = golden("g18_prune_edges")
    assert g["ms"].tolist() == list(PE_MS)
    for m in PE_MS:
        w = pe_world(m)
        assert np.array_equal(g[f"parts_{m}"], w.parts) and np.array_equal(g[f"verts_{m}"], w.verts)
        thrs, w_out, drifted = g[f"thr_{m}"], g[f"w_out_{m}"], g[f"drifted_{m}"]
        assert np.array_equal(thrs, np.array((w.thr,) + (PE_DEGENERATE if m == PE_M else ())), equal_nan=True)
        assert np.array_equal(w_out[0] != 0, w.keep) and not drifted[0]
        for t, thr in enumerate(thrs[1:], 1):
            ref = pe_degenerate_expected(w, float(thr))
            assert np.array_equal(w_out[t] != 0, ref) and bool(drifted[t]) == (not ref.any()), thr
    w_out = g[f"w_out_{PE_M}"]
    assert w_out[1].sum() == 2 and w_out[2].all() and not w_out[3].any() and w_out[4].all()


def test_degenerate_thresholds_by_the_oracle(w):
    """The oracle's ~(dist > thr): NaN and +inf keep everybody - a NaN translation (dist = +inf) too -, a negative threshold nobody,
    0 exactly the particles on a vertex."""
    poses = np.concatenate([w.poses, pe_nan_pose()[None]])
    for thr, kept in zip(PE_DEGENERATE, (2, w.n + 1, 0, w.n + 1)):
        assert int(pe_degenerate_expected(w, thr, poses).sum()) == kept, thr
    assert not pe_degenerate_expected(w, w.thr, poses)[-1]


def test_squared_threshold_restated():
    """t2 is one ulp above fl(thr thr) for 0.002, 1e-4, 0.004, 0.0025 and 131 2^-16, equal to it for 0.05 and 0.003; the edges."""
    for thr in (0.002, 1e-4, 0.004, 0.0025, 131 * 2.0 ** -16):
        assert pe_squared_threshold(thr) == np.nextafter(thr * thr, np.inf), thr
    for thr in (0.05, 0.003):
        assert pe_squared_threshold(thr) == thr * thr, thr
    assert pe_squared_threshold(0.0) == 0.0 and pe_squared_threshold(np.inf) == np.inf and pe_squared_threshold(-1e-3) == -1.0 and pe_squared_threshold(np.nan) == -1.0
    for thr in (0.002, 1e-4, 0.004, 0.05, 0.003, 163 * PE_U):
        t2 = pe_squared_threshold(thr)
        assert np.sqrt(t2) <= thr < np.sqrt(np.nextafter(t2, np.inf))


@pytest.mark.parametrize("thr", PE_ULP_THRS)
def test_ulp_family_against_the_oracle(oracle, thr):
    """d2 == t2 is kept and lies above fl(thr thr); the next double is pruned; the oracle's sqrt(d2) > thr says the same; and some
    of the points change sides under a reversed chain and under an uncontracted sum."""
    wd = pe_ulp_world(thr)
    assert wd.t2 != thr * thr and wd.keep.sum() == wd.n // 2
    d = oracle.nn3_dist(wd.poses, wd.verts64)
    assert np.array_equal(~(d > thr), wd.keep)
    d2 = np.array([pe_ulp_d2(wd.poses[i, :3, 3], wd.verts64[i]) for i in range(wd.n)])
    assert np.array_equal(d2[wd.keep], np.full(wd.n // 2, wd.t2)) and np.array_equal(d2[~wd.keep], np.full(wd.n // 2, np.nextafter(wd.t2, np.inf)))
    assert (d2 > thr * thr).all()      # (t2 = thr thr would prune the kept half)
    print(f"thr {thr}: points that change sides: {wd.flips}")
    assert wd.flips["reversed"] >= 1 and wd.flips["uncontracted"] >= 1


def test_face_and_tiny_worlds():
    for m in PE_FACE_MS:
        wd = pe_face_world(m)
        out_kept = int((wd.keep & wd.outside).sum())
        assert out_kept == (12 if m == 180 else 0), (m, out_kept)   # (170 and 180 units out on six axes)
    for nv in PE_TINY_SIZES:
        assert len(pe_tiny_world(nv).verts) == nv
