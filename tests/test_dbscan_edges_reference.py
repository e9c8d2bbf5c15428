"""DBSCAN at its edges on the CPU: the lattice cases of tests/_recipes.py - points exactly on eps, neighbour counts exactly at
min_samples, clusters that hang together by one pair, border points whose only link lies on the sphere - against four statements of
the same labels: the brute-force DBSCAN over int64 the recipes carry, oracle.dbscan, sklearn's DBSCAN (fed float32 and float64 copies)
and fixture G17, written by the reference's own cluster_particles (tools/gen_dbscan_edges.py).  The rounding cases - near-origin pairs
whose float64 sum depends on its order, on contraction and on the format - are held to the oracle and to a numpy float64 restatement
only (sklearn's KD-tree accepts a node wholly inside the ball on sqrt(sum) <= eps, which can differ from sum <= eps eps by an ulp).
Every recipe asserts its own conditions while it builds its cases: the cell classes, the counts, the single links ("DBSCAN's
rule").  No GPU."""
import numpy as np
import pytest

from _recipes import (DB_POINTS_SIZES, DB_ROUNDING_MIN, DB_ROUNDING_MUTANTS, db_cells, db_edge_cases, db_f64_dbscan, db_fixture_cases, db_int_dbscan,
                      db_points_case, db_rounding_separations)


@pytest.fixture(scope="module")
def cases():
    return db_edge_cases()  # (every recipe condition is asserted in here)


def _lattice(cases):
    return [c for c in cases.values() if "V" in c]


def test_recipe_families_and_their_conditions(cases):
    """What the case list holds: every family, dense and hashed, both sides of every edge."""
    names = list(cases)
    count = lambda *parts: sum(all(p in n.split("/") for p in parts) for n in names)  # noqa: E731
    assert count("probe", "dense", "c") >= 12 and count("probe", "hashed", "c+1") >= 12
    assert count("probe", "pops8") == 8 and count("own") == 16 and count("corner") == 12 and count("tiny") == 9
    assert count("bridge", "one", "on", "dense", "ms") == 16          # a scan of part of the other cell misses all 16 with p < 1e-5
    assert count("bridge", "one", "on", "hashed", "ms") == 16 and count("probe", "pops4cut0") == 8
    for kind in ("box", "cut", "one"):
        for side in ("on", "plus"):
            assert count("bridge", kind, side, "dense") >= 3 and count("bridge", kind, side, "hashed") >= 3
    for mode in ("on", "plus", "none"):
        for apop in ("apop1", "apop65", "apop130"):
            assert count("border", mode, apop, "dense") == 3 and count("border", mode, apop, "hashed") == 3
    for c in _lattice(cases):
        if not c["name"].startswith("tiny"):
            assert c["hashed"] == ("hashed" in c["name"].split("/")) or c["fifth"], c["name"]
            assert db_cells(c["X"], c["eps"])[1].max() > 128 or not c["hashed"]
    big = [c for c in cases.values() if "pops8" in c["name"]]
    assert all(sorted(c["classes"]) == ["corner", "cut", "decoy", "on", "within"] for c in big)
    assert max(len(c["X"]) for c in cases.values()) < 3000   # the O(N^2) references stay well under a second


def test_lt_for_le_changes_the_labels(cases):
    """A strict predicate (|dV|^2 <= m^2 - 1) changes the labels of every probe at c, every on-eps bridge and every on-eps border."""
    for c in _lattice(cases):
        parts = c["name"].split("/")
        lab = db_int_dbscan(c["V"], c["m"] * c["m"] - 1, c["ms"])[0]
        if (parts[0] == "probe" and parts[-1] == "c") or (parts[0] in ("bridge", "border") and "on" in parts):
            assert not np.array_equal(lab, c["labels"]), c["name"]
            if parts[0] == "probe":
                assert (lab == -1).all()


def test_oracle_matches_the_integer_reference(cases, oracle):
    for c in _lattice(cases):
        lab, ncl = oracle.dbscan(c["X"], c["eps"], c["ms"])
        assert np.array_equal(lab, c["labels"]) and ncl == c["ncl"], c["name"]


def test_sklearn_matches_the_integer_reference(cases):
    cluster = pytest.importorskip("sklearn.cluster")
    for c in _lattice(cases):
        if c["ms"] < 1:
            with pytest.raises(Exception):   # out of spec: sklearn refuses min_samples = 0
                cluster.DBSCAN(eps=c["eps"], min_samples=c["ms"]).fit(c["X"])
            continue
        for X in (c["X"], c["X"].astype(np.float64)):
            lab = cluster.DBSCAN(eps=c["eps"], min_samples=c["ms"]).fit(X).labels_
            assert np.array_equal(lab, c["labels"]), (c["name"], X.dtype)


def test_g17_reference_labels(cases, golden, oracle):
    """Fixture G17: the reference's cluster_particles on the cases whose min_samples is n // 5 - the points rebuilt from the stored
    integers are the recipe's, the labels the integer reference's and the oracle's."""
    g = golden("g17_dbscan_edges")
    g = {k: g[k] for k in g.files}
    fx = db_fixture_cases()
    assert [str(n) for n in g["names"]] == [c["name"] for c in fx] and len(fx) >= 40
    assert g["local"].dtype == np.int16 and g["labels"].dtype == np.int16
    for i, c in enumerate(fx):
        at, n = int(g["case_at"][i]), int(g["case_n"][i])
        V = g["local"][at:at + n].astype(np.int64) + g["case_off"][i]
        X = (V * 2.0 ** -int(g["case_k"][i])).astype(np.float32)
        assert np.array_equal(X.view(np.uint32), c["X"].view(np.uint32)) and int(g["case_m"][i]) == c["m"] and int(g["case_ms"][i]) == c["ms"] == n // 5
        ref = g["labels"][at:at + n].astype(np.int64)
        assert np.array_equal(ref, c["labels"]), c["name"]
        lab, _ = oracle.dbscan(X, int(g["case_m"][i]) * 2.0 ** -int(g["case_k"][i]), n // 5)
        assert np.array_equal(lab, ref), c["name"]
    kinds = {c["name"].split("/")[0] for c in fx}
    assert kinds == {"probe", "bridge", "border", "tiny"} and any(c["hashed"] for c in fx)


def test_tiny_sets_out_of_spec(cases, oracle):
    """n < 5: min_samples = n // 5 = 0, which sklearn refuses.  The oracle counts every point as a core point, as with min_samples 1."""
    for n in range(1, 10):
        c = cases[f"tiny/n{n}"]
        assert c["ms"] == n // 5
        assert np.array_equal(oracle.dbscan(c["X"], c["eps"], c["ms"])[0], oracle.dbscan(c["X"], c["eps"], 1)[0])


def test_rounding_cases(cases, oracle):
    """The oracle takes the spec's side on every rounding case; each mutant has at least 8 cases either way."""
    for mutant in DB_ROUNDING_MUTANTS:
        mine = [c for c in cases.values() if c.get("mutant") == mutant]
        assert sum(c["within"] for c in mine) >= DB_ROUNDING_MIN and sum(not c["within"] for c in mine) >= DB_ROUNDING_MIN
        for c in mine:
            lab, ncl = oracle.dbscan(c["X"], c["eps"], c["ms"])
            assert np.array_equal(lab, c["labels"]) and ncl == c["ncl"], c["name"]
            assert np.array_equal(db_f64_dbscan(c["X"], c["eps"], c["ms"])[0], lab)
            assert not np.array_equal(c["mutant_labels"], lab), c["name"]


def test_rounding_separation_counts():
    """Near the origin an eps separates the spec's sum from the reversed order and from the contracted chain on about a quarter of the
    pairs, from a float32 evaluation on all of them."""
    n = 1000
    count = db_rounding_separations(n)
    print(count)
    assert count["f32"] == n and count["reversed"] >= n // 8 and count["contracted"] >= n // 8


@pytest.mark.parametrize("dim", [2, 3, 4, 5, 6])
def test_points_cases(dim):
    """The all-pairs kernel's cases build (their conditions are asserted inside) and, in three dimensions, are float32 lattices the
    grid kernel can be given as well."""
    for N in DB_POINTS_SIZES:
        c = db_points_case(dim, N)
        assert len(c["X"]) == N and c["X"].shape[1] == dim and c["ncl"] == 2
