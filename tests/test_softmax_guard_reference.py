"""The softmax guard on the CPU: get_similarity (modules/particle_filter.py:449-469) skips the softmax when
isclose(max(x) - min(x), 0) holds over ALL particles of the frame - |max - min| <= 1e-8 in float64, NaN never close - and every
reference the GPU tests lean on restates that rule: oracle.softmax_weights (mo_softmax, C), oracle.softmax_numerators (numpy), the
oracle shard backend's rule on gathered block extrema (tests/_oracle_shard_backend.py).  Here each is held to a torch restatement
of the reference's own lines (tests/_recipes.py guard_rule_torch) and to fixture G16, the real get_similarity's weights, on the one
kind of input that sees a dropped value: a cloud collapsed onto one score with ONE dissenting slot (recipe_guard_scores), wide, at
the 1e-8 edge and a step either side of it, a signed zero, a NaN.

Bounds.  `applied` is equal.  Where the softmax is skipped the weights ARE the scores: bit for bit.  Where it applies, two
float64 sums of N positive terms added in different orders differ by at most N * 2^-52 relative (worst case; the exponentials
themselves differ by an ulp or two, far inside it); the measured maximum is printed per N.  A NaN frame is all NaN in both."""
import os
import types

import numpy as np
import pytest

from _recipes import (GUARD_KINDS, GUARD_N, GUARD_N66, GUARD_ROWS, guard_applied, guard_cases, guard_rows, guard_rule_torch,
                      recipe_guard_scores)

torch = pytest.importorskip("torch")

CASES = guard_cases(big=(GUARD_N66,))
SIZES = sorted({c[0] for c in CASES})


def _compare(got, applied, ref, ref_applied, N, what, seen):
    assert applied == ref_applied, f"{what}: applied {applied}, the reference's rule says {ref_applied}"
    if np.isnan(ref).any():
        assert np.isnan(ref).all() and np.isnan(got).all(), f"{what}: a NaN frame must be all NaN"
        return
    if not ref_applied:
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), f"{what}: the raw weights are not the scores bit for bit"
        return
    rel = float(np.max(np.abs(got - ref) / ref))
    seen[N] = max(seen.get(N, 0.0), rel)
    assert rel <= N * 2.0 ** -52, f"{what}: relative difference {rel:.3g} beyond N * 2^-52 = {N * 2.0 ** -52:.3g}"


def test_recipe_kinds_against_the_rule():
    """The kinds' expectations are the torch rule's, not a table's say-so: spread exactly 1e-8 and one step below raw, one step
    above applied, the float32-reachable pair either side, -0.0 beside +0.0 raw, NaN applied; one particle always raw."""
    assert float(np.float32(1e-8)) < 1e-8 < float(np.nextafter(np.float32(1e-8), np.float32(1)))
    for kind, (val, applied) in GUARD_KINDS.items():
        for N, slot in ((2, 0), (2, 1), (17, 5), (GUARD_N, GUARD_N - 1)):
            x = recipe_guard_scores(N, kind, slot)
            assert x.dtype == np.float64 and np.count_nonzero(x != 0.0) == (0 if kind == "signed_zero" else 1)
            w, ap = guard_rule_torch(x)
            assert ap == applied == guard_applied(N, kind), (kind, N, slot)
            if kind == "nan":
                assert np.isnan(w).all()
        x = recipe_guard_scores(1, kind, 0)
        w, ap = guard_rule_torch(x)
        assert not ap and np.array_equal(w, x, equal_nan=True)


@pytest.mark.parametrize("N", SIZES)
def test_oracle_rules_against_torch(oracle, N):
    """oracle.softmax_weights and oracle.softmax_numerators (torch's shift, and the fused step's constant shift 1 with the blocked
    sum) on every kind and slot of size N."""
    seen = {}
    n = 0
    for _, kind, slot in (c for c in CASES if c[0] == N):
        x = recipe_guard_scores(N, kind, slot)
        ref, ref_applied = guard_rule_torch(x)
        if N > 1:   # (one target: get_similarity returns the 0-dim score; the array forms below take N >= 1 alike)
            assert ref_applied == GUARD_KINDS[kind][1]
        what = f"N={N} {kind} slot {slot}"
        w, applied = oracle.softmax_weights(x)
        if N == 1 and kind == "nan":   # a single NaN: raw and softmax are both NaN
            assert np.isnan(w).all()
        else:
            _compare(w, applied, ref, ref_applied, N, "softmax_weights " + what, seen)
        for shift in (None, 1.0):
            e, applied = oracle.softmax_numerators(x, True, shift=shift)
            S = oracle.blocked_scan(e)[1] if applied else 1.0
            if N == 1 and kind == "nan":
                assert np.isnan(e / S).all()
            else:
                _compare(e / S, applied, ref, ref_applied, N, f"softmax_numerators(shift={shift}) " + what, seen)
        n += 1
    print(f"softmax guard [oracle vs torch] N={N}: {n} cases, largest relative difference where applied {seen.get(N, 0.0):.3g} "
          f"(bound {N * 2.0 ** -52:.3g})")


def _shard_weights(N, x, world):
    """The weights the oracle shard backend's ranks report for scores x (every particle valid), world ranks of N // world slots."""
    from _oracle_shard_backend import OracleShardBackend
    be = OracleShardBackend.__new__(OracleShardBackend)
    n_loc = N // world
    assert n_loc * world == N
    nb = -(-n_loc // 4096)
    Np = -(-n_loc // 16) * 16
    sts = []
    for r in range(world):
        st = types.SimpleNamespace(N=n_loc, nb=nb, scores=torch.as_tensor(x[r * n_loc:(r + 1) * n_loc].copy()),
                                   nn_idx=torch.arange(n_loc), valid=torch.ones(n_loc, dtype=torch.uint8),
                                   tables=torch.zeros(4 * Np, dtype=torch.float64), r1=torch.zeros(5 * nb + 4, dtype=torch.float64),
                                   weights=torch.zeros(n_loc, dtype=torch.float64), cdf=torch.zeros(n_loc, dtype=torch.float64),
                                   status=torch.zeros(2, dtype=torch.int32), rmse=torch.zeros(2, dtype=torch.float64))
        be.tail_a(st, True)
        sts.append(st)
    r1_all = torch.cat([st.r1 for st in sts])
    applied = None
    for r, st in enumerate(sts):
        ap = be._globals(st, r1_all, world, True)[1]
        assert applied in (None, ap)
        applied = ap
        be.tail_fin(st, r1_all, r, world, N, True, False)
    return torch.cat([st.weights for st in sts]).numpy(), applied, int(sts[0].status[0])


@pytest.mark.parametrize("N,world", [(n, 1) for n in SIZES] + [(GUARD_N, 3), (2, 2), (16, 2)])
def test_oracle_shard_rule_against_torch(oracle, N, world):
    """The rule on the gathered per-block extrema (one rank, and the dissenter in the first, a middle and the last rank of three)."""
    seen = {}
    n = 0
    for _, kind, slot in (c for c in CASES if c[0] == N):
        x = recipe_guard_scores(N, kind, slot)
        ref, ref_applied = guard_rule_torch(x)
        w, applied, status = _shard_weights(N, x, world)
        if N == 1 and kind == "nan":
            assert np.isnan(w).all()
        else:
            _compare(w, applied, ref, ref_applied, N, f"shard rule x{world} N={N} {kind} slot {slot}", seen)
        assert (status & 2 != 0) == (kind == "nan")
        n += 1
    print(f"softmax guard [shard rule x{world} vs torch] N={N}: {n} cases, largest relative difference {seen.get(N, 0.0):.3g}")


def test_golden_g16(oracle, golden):
    """The real get_similarity's weights (fixture G16) against oracle.get_similarity on the fixture's own rows and code, and against
    the torch restatement: what the recipes call raw and applied is what the reference did."""
    g = golden("g16_softmax_guard")
    kinds = [str(k) for k in g["kinds"]]
    assert kinds == list(GUARD_ROWS)
    code = g["code"]
    seen = {}
    for N, ki, slot, at in zip(g["case_N"], g["case_kind"], g["case_slot"], g["case_w_at"]):
        N, slot, at, kind = int(N), int(slot), int(at), kinds[int(ki)]
        rows = g[f"rows_{kind}"]
        base, row = guard_rows(kind, int(g["D"].reshape(-1)[0]))
        assert np.array_equal(rows, np.stack([base, row]), equal_nan=True), "the recipe's rows drifted from the fixture"
        ref = g["w"][at:at + N]
        targets = np.tile(rows[0], (N, 1))
        targets[slot] = rows[1]
        x = recipe_guard_scores(N, kind, slot)
        ref_applied = GUARD_KINDS[kind][1]
        if not ref_applied:   # the reference returned the scores themselves: the recipe's values exactly
            assert np.array_equal(ref.view(np.uint64), x.view(np.uint64)), (N, kind, slot)
        assert np.array_equal(oracle.score_codebook(targets, code), x, equal_nan=True)
        w = oracle.get_similarity(code, targets)
        _compare(w, oracle.softmax_weights(x)[1], ref, ref_applied, N, f"G16 N={N} {kind} slot {slot}", seen)
        wt, ap = guard_rule_torch(x)
        _compare(wt, ap, ref, ref_applied, N, f"G16 vs the torch restatement N={N} {kind} slot {slot}", seen)
    print(f"softmax guard [G16]: {len(g['case_N'])} cases, largest relative difference where applied {max(seen.values()):.3g}")


def test_golden_g16_is_small():
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "g16_softmax_guard.npz")) < 64 * 1024
