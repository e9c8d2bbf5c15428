"""The annealing decision on the CPU: fixture G15 - the reference's own particle_filter.annealing on inputs at the edges of its float32
rule (tools/gen_anneal_rule.py) - against oracle.Annealer under both tie rules and against particle_filter._anneal_plan, the class
surface's statement of the rule, fed 0-dim float32 tensors as the loop feeds it; and the conditions that keep the recipe honest: every
set holds inputs on which a rule evaluated in float64, with a float64 product or with a reciprocal division decides otherwise
("The annealing rule's arithmetic").  No GPU."""
import numpy as np
import pytest

from _recipes import (ANNEAL_FIXTURE_SETS, ANNEAL_MUTANTS, anneal_rule, assert_anneal_recipe_conditions, f32_bits, f32_from_bits,
                      recipe_anneal_rule_cases)

torch = pytest.importorskip("torch")


def _cases(g):
    """-> per fixture case: dict(set, n, floor, init, prev, var, tag, kind, ids, count, pv_after, init_after, raises)."""
    g = {k: g[k] for k in g.files}  # (every read of an npz member unpacks it again)
    sets = g["sets"]
    out = []
    for i in range(g["case_set"].shape[0]):
        s = int(g["case_set"][i])
        at, cnt = int(g["case_ids_at"][i]), int(g["case_count"][i])
        out.append(dict(set=s, n=int(sets[s, 1]), floor=int(sets[s, 2]), init=int(sets[s, 3]),
                        prev=f32_from_bits(g["case_prev_bits"][i])[()], var=f32_from_bits(g["case_var_bits"][i])[()],
                        tag=str(g["case_tag"][i]), kind=str(g["case_kind"][i]), ids=g["ids"][at:at + cnt], count=cnt,
                        pv_after_bits=int(g["case_pv_after_bits"][i]), init_after=int(g["case_init_after"][i]), raises=str(g["case_raises"][i])))
    return out


def _plan_ids(w, plan):
    """The ids a plan (mode, k) of _anneal_plan selects on distinct weights: the original order without the k lightest, or with the k
    heaviest appended heaviest first (Particles.remove / add)."""
    n = w.shape[0]
    if plan is None:
        return np.arange(n)
    mode, k = plan
    if mode == 1:
        keep = np.ones(n, dtype=bool)
        keep[np.argsort(w, kind="stable")[:k]] = False
        return np.flatnonzero(keep)
    return np.concatenate([np.arange(n), np.argsort(-w, kind="stable")[:k]])


def test_fixture_is_the_recipe(golden):
    """The fixture's inputs are what the recipe gives today, set by set and bit for bit; the out-of-spec input raised OverflowError in
    the reference and nothing else raised; the edges the issue names are all there with the outcome the reference's source implies."""
    g = golden("g15_anneal_rule")
    cases = _cases(g)
    assert len(ANNEAL_FIXTURE_SETS) == g["sets"].shape[0]
    at = 0
    for s, (var, n, floor, init, main) in enumerate(ANNEAL_FIXTURE_SETS):
        assert [int(f32_bits(var)), n, floor, init, int(main)] == g["sets"][s].tolist()
        for c in recipe_anneal_rule_cases(var, n, floor, init):
            f = cases[at]
            assert (f["set"], f["tag"], f["kind"]) == (s, c["tag"], c["kind"])
            assert f32_bits(f["prev"]) == f32_bits(c["prev"]) and f32_bits(f["var"]) == f32_bits(c["var"]), (s, c["tag"])
            at += 1
    assert at == len(cases)
    for f in cases:
        assert f["raises"] == ("OverflowError" if f["kind"] == "out_of_spec" else ""), f["tag"]
        var_bits = int(f32_bits(f["var"]))
        if f["tag"] == "nan":
            assert f["count"] == f["n"] and f["pv_after_bits"] == var_bits
        elif f["tag"] == "first":
            assert f["count"] == f["n"] and f["pv_after_bits"] == var_bits and f["init_after"] == f["n"]
        elif f["kind"] == "var0":
            assert f["count"] == f["n"] and f["pv_after_bits"] == int(f32_bits(f["prev"]))
        elif f["tag"] == "tiny":  # the product is finite and beyond 2^31: Python's int holds it, the cap by n // 3 decides
            k = f["n"] // 3
            assert f["count"] == (f["n"] + k if k + f["n"] <= f["init"] else f["n"]), (f["set"], f["count"])
        elif f["tag"] in ("m-0+0", "m+0+0"):
            assert f["prev"] == f["var"] and f["count"] == f["n"]
        if f["kind"] != "first" and f["tag"] != "first":
            assert f["init_after"] == f["init"]
    # one ulp either side of ratio == 1 nothing happens either; the set with n + n // 3 == init grows to its last slot; n < floor removes
    by = {(f["set"], f["tag"]): f for f in cases}
    for s, (_, n, floor, init, _m) in enumerate(ANNEAL_FIXTURE_SETS):
        for tag in ("m-0+1", "m-0-1"):
            assert by[(s, tag)]["count"] == n
    counts = lambda s: {f["count"] for f in cases if f["set"] == s}  # noqa: E731
    s_fill = [s for s, (_, n, _f, init, _m) in enumerate(ANNEAL_FIXTURE_SETS) if n + n // 3 == init][0]
    assert ANNEAL_FIXTURE_SETS[s_fill][3] in counts(s_fill)
    s_low = [s for s, (_, n, floor, _i, _m) in enumerate(ANNEAL_FIXTURE_SETS) if n < floor and n > 4][0]
    assert min(counts(s_low)) < ANNEAL_FIXTURE_SETS[s_low][1]
    for s, (_, n, _f, _i, _m) in enumerate(ANNEAL_FIXTURE_SETS):
        if n < 3:
            assert counts(s) == {n, 0} or counts(s) == {n}, (n, counts(s))  # n // 3 == 0: never acts (0: the case that raised)


def test_restated_rule_is_the_reference(golden):
    """anneal_rule - the numpy statement the recipe searches with and the conditions count by - decides every fixture case as the
    reference did: the search separates mutants from the reference's rule, not from a misreading of it."""
    for f in _cases(golden("g15_anneal_rule")):
        if f["kind"] == "var0" or np.isinf(f["prev"]):
            continue
        mode, k = (int(v[0]) for v in anneal_rule(f["var"], f["prev"], f["n"], f["floor"], f["init"]))
        if f["raises"]:
            assert mode == -1, f["tag"]
        else:
            assert f["n"] + {0: 0, 1: -k, 2: k}[mode] == f["count"], (f["set"], f["tag"], mode, k, f["count"])


@pytest.mark.parametrize("ties", ["index", "aten_cpu"])
def test_oracle_annealer_matches_reference_fixture(golden, oracle, ties):
    g = golden("g15_anneal_rule")
    ws = [g[f"w_{s}"] for s in range(len(ANNEAL_FIXTURE_SETS))]
    for f in _cases(g):
        w = ws[f["set"]]
        an = oracle.Annealer(ties)
        an.particle_var, an.init_particles = (float("inf") if np.isinf(f["prev"]) else np.float32(f["prev"])), f["init"]
        if f["raises"]:
            with pytest.raises(OverflowError), np.errstate(divide="ignore"):
                an.step(w, f["var"], f["floor"])
        else:
            keep = an.step(w, f["var"], f["floor"])
            assert keep.shape[0] == f["count"] and np.array_equal(keep, f["ids"]), (f["set"], f["tag"])
        assert int(f32_bits(np.float32(an.particle_var))) == f["pv_after_bits"], (f["set"], f["tag"])
        assert an.init_particles == f["init_after"]


def test_anneal_plan_matches_reference_fixture(golden):
    """particle_filter._anneal_plan on an instance made with __new__, var and particle_var 0-dim float32 tensors."""
    from midastouch_amd.particle_filter import particle_filter
    g = golden("g15_anneal_rule")
    ws = [g[f"w_{s}"] for s in range(len(ANNEAL_FIXTURE_SETS))]
    for f in _cases(g):
        w = ws[f["set"]]
        pf = particle_filter.__new__(particle_filter)
        pf.particle_var = torch.tensor([float("inf")]) if np.isinf(f["prev"]) else torch.tensor(f["prev"])
        pf.init_particles = f["init"]
        var = torch.tensor(f["var"])
        assert var.dim() == 0 and var.dtype == torch.float32
        if f["raises"]:
            with pytest.raises(OverflowError):
                pf._anneal_plan(f["n"], var, f["floor"])
        else:
            ids = _plan_ids(w, pf._anneal_plan(f["n"], var, f["floor"]))
            assert ids.shape[0] == f["count"] and np.array_equal(ids, f["ids"]), (f["set"], f["tag"])
        after = torch.as_tensor(pf.particle_var).reshape(-1)[0]
        assert after.dtype == torch.float32 and int(f32_bits(np.float32(after.item()))) == f["pv_after_bits"], (f["set"], f["tag"])
        assert int(pf.init_particles) == f["init_after"]


def test_recipe_conditions():
    """Every main set of the fixture - and the sets of the sizes the GPU tests use, at two spreads each; the GPU tests assert the same on
    the spreads their frames have - holds at least 8 inputs that separate the float32 rule from each mutant (the float64 product: up to
    300 particles), and the mutants are mutants: each agrees with the rule on most of the recipe."""
    sets = [(v, n, fl, i) for v, n, fl, i, main in ANNEAL_FIXTURE_SETS if main]
    sets += [(v, n, fl, i) for v in (0.0123456, 3.3e-4) for n, fl, i in ((300, 100, 400), (299, 100, 398), (298, 100, 400), (17000, 8000, 22666))]
    for var, n, floor, init in sets:
        cases = recipe_anneal_rule_cases(var, n, floor, init)
        sep = assert_anneal_recipe_conditions(cases, n, floor, init, what=(var, n, floor, init))
        assert set(sep) == set(ANNEAL_MUTANTS) and max(sep.values()) < len(cases) // 2, sep
        kinds = {c["kind"] for c in cases}
        assert kinds == {"special", "var0", "out_of_spec", "target", "search"}, kinds
