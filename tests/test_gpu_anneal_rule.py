"""The annealing decision on the device (loop_decide, csrc/anneal_decide.hpp) at the edges of its float32 rule, at every site that
compiles or launches it: one frame per case - the particle set, `particle_var` and `init_particles` set, one step - against the
oracle's frame with oracle.Annealer in the same state, by exact equality throughout.  The frame's spread `var` is whatever the
propagated set has; the cases (tests/_recipes.py: recipe_anneal_rule_cases, the recipe fixture G15 was written from) place the previous
spread so that |1 - var / prev| * n stands on and beside the integers at which the rule changes its answer, and on inputs a float64
rule, a float64 product or a reciprocal division decide otherwise.  DESIGN.md, "The annealing rule's arithmetic", has the sites:

  S1 k_loop_anneal_small<DECIDE>          LoopEngine, up to 16 384 particles, ties by index
  S2 k_loop_decide + launch_select        LoopEngine, 17 000 particles
  S3 two-pass spreads, ATen's sum, walk   LoopEngine(topk_ties="aten_cpu")
  S4 the frozen decision                  floor == n == init_particles, both tie rules
  S5 the batch's small form               BatchLoopEngine, a case per row
  S6 the batch's decision alone           BatchLoopEngine, topk_ties = "aten_cpu"
  S7 k_loop_decide with blockIdx.y > 0    BatchLoopEngine(wide=True), 17 000 particles
and the class surface, particle_filter.annealing, on fixture G15."""
import numpy as np
import pytest

from _recipes import ANNEAL_FIXTURE_SETS, ANNEAL_MUTANTS, anneal_rule, assert_anneal_recipe_conditions, f32_bits, f32_from_bits, recipe_anneal_rule_cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K, D, SEED = 3000, 256, 4301       # the scenario of test_loop_engine_frozen_annealing_under_the_aten_tie_rule
N_SMALL, N_LARGE = 300, 17000      # S1 / S3 / S4 / S5 / S6, and the smallest set beyond the single-workgroup form (16 384)
# (floor, init_particles) per single-engine site of 300 particles; the first carries the recipe's conditions
CONFIGS_SMALL = ((100, 400),       # n + n // 3 == init == the engine's capacity: the largest duplication fills the last slot
                 (250, 340),       # |n - floor| = 50 caps the removal below n // 3, init caps the growth at 40
                 (350, 400))       # n < floor: the reference's abs lets the rule remove
CONFIG_LARGE = (8000, N_LARGE + N_LARGE // 3)
FLOOR_ABOVE = 20000                # a floor above 17 000 particles: |n - floor| = 3000 caps the removal


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cb():
    from midastouch_amd.synthetic import make_codebook
    return make_codebook(K=K, D=D, seed=1014, mesh_points=20000)


@pytest.fixture(scope="module")
def traj(cb):
    from midastouch_amd.synthetic import make_trajectory
    return make_trajectory(cb, T=2, seed=2014)


def _particle_set(cb, n, layout, salt=0):
    """n codebook poses and their labels: "one" cluster (3 spreads) or "three" (9 spreads: ATen's sum order and the running sum part)."""
    rng = np.random.default_rng([5, n, salt])
    poses = cb.poses[rng.integers(0, K, n)]
    labels = np.zeros(n, dtype=np.int64) if layout == "one" or n < 6 else rng.integers(0, 3, n).astype(np.int64)
    if layout == "three" and n >= 6:
        labels[:3] = (0, 1, 2)
    return poses, labels


def _host_draws(n, salt=0):
    rng = np.random.default_rng([6, n, salt])
    return (rng.normal(0.0, 2e-4, (n, 3)).astype(np.float32), rng.normal(0.0, 0.5, (n, 3)).astype(np.float32), rng.random(n + n // 3))


def _front(orc, loop, poses, labels, odom, code, tn, rot, ties):
    """The oracle's frame up to the annealing decision (OracleLoop.step's first half, no DBSCAN): what every case of a set shares."""
    f = loop.f
    p1 = orc.propagate(poses, odom, tn, rot)
    idx = orc.nn6(orc.R3_SE3(p1), f.cb_feat)[0]
    x = orc.score_codebook(f.emb, code)[idx]
    mask = ~(orc.nn3_dist(p1, f.verts) > f.pen_max)
    e, applied = orc.softmax_numerators(x, loop.softmax, shift=1.0)
    S = orc.blocked_scan(e)[1] if applied else 1.0
    w = e / S * mask
    assert mask.sum() > 0  # (no re-projection: the sets stay on the mesh)
    uniq, centers, stds = orc.cluster_centers(p1, w, labels)
    var = orc.cluster_var(stds, ties)
    return dict(poses_prop=p1, nn_idx=idx, mask=mask, weights=w, drifted=False, e=e, labels_in=np.asarray(labels), cluster_labels=uniq,
                cluster_poses=centers, cluster_stds=stds, var=var)


def _tail(orc, fr, keep, u):
    """... and behind it (OracleLoop.step's second half): the resample over the annealed set `keep`."""
    n2 = keep.shape[0]
    em = (fr["e"] * fr["mask"])[keep]
    status = orc.cdf(em)[1]
    ridx = np.arange(n2, dtype=np.int32) if status else orc.resample_indices(em, "weighted_random", u=np.asarray(u)[:n2])[0]
    src = keep[ridx]
    ref = {k: fr[k] for k in ("poses_prop", "nn_idx", "mask", "weights", "drifted", "cluster_labels", "cluster_poses", "cluster_stds", "var")}
    ref.update(keep=keep.astype(np.int32), status=status, ridx=ridx.astype(np.int32), src=src.astype(np.int32), poses=fr["poses_prop"][src],
               weights_res=fr["weights"][src], nn_idx_res=fr["nn_idx"][src], labels=fr["labels_in"][src], N=n2)
    return ref


def _annealer(orc, ties, prev, init):
    an = orc.Annealer(ties)
    an.particle_var, an.init_particles = (float("inf") if np.isinf(prev) else np.float32(prev)), int(init)
    return an


def _gpu_cases(var, n, floor, init):
    """The recipe's cases a frame of spread `var` can be given: those that keep the frame's var (not "var0") and lie within the
    spec (not the infinite ratio, on which the reference raises: DESIGN.md)."""
    return [c for c in recipe_anneal_rule_cases(var, n, floor, init) if c["kind"] in ("special", "target", "search")]


def _by_priority(cases, n, floor, init):
    """The specials (the finite overflow first), then the search's cases with the mutants taking turns, then the targets."""
    special = sorted((c for c in cases if c["kind"] == "special"), key=lambda c: ("tiny", "nan", "first").index(c["tag"]))
    per = {m: [] for m in ANNEAL_MUTANTS}
    for c in cases:
        if c["kind"] == "search":
            rule = anneal_rule(c["var"], c["prev"], n, floor, init)
            for m in ANNEAL_MUTANTS:
                other = anneal_rule(c["var"], c["prev"], n, floor, init, m)
                if rule[0][0] != other[0][0] or rule[1][0] != other[1][0]:
                    per[m].append(c)
                    break
    search = [per[m][i] for i in range(max(map(len, per.values()), default=0)) for m in ANNEAL_MUTANTS if i < len(per[m])]
    return special + search + [c for c in cases if c["kind"] == "target"]


def _check_decision(fv, an_after, var, prev, n, floor, init, keep, what, frozen=False):
    """The log row and the state afterwards against the annealer and the restated rule: mode, k, n_after, err == 0, var's bits,
    particle_var (by bits, a float32 value held in the double; it becomes var on the NaN case and on the first call, which also sets
    init_particles to n) and init_particles."""
    if np.isinf(prev):
        mode, k = 0, 0
    else:
        mode, k = (int(v[0]) for v in anneal_rule(var, prev, n, floor, init))
    assert keep.shape[0] == n + {0: 0, 1: -k, 2: k}[mode], what  # (the annealer and the restated rule: one decision)
    if frozen:
        assert mode == 0, what
    assert (fv["mode"], fv["k"], fv["n"], fv["n_after"], fv["err"]) == (mode, k, n, keep.shape[0], 0), (what, fv["mode"], fv["k"], fv["n_after"], fv["err"], mode, k)
    from midastouch_amd import _lib
    assert f32_bits(np.float32(fv["var"])) == f32_bits(var) and np.float32(fv["var"]) == fv["var"], what
    got_prev = fv["ctl_d"][_lib.LOOP_D_VARPREV]
    assert np.float32(got_prev) == got_prev or np.isnan(got_prev), what
    assert f32_bits(np.float32(got_prev)) == f32_bits(np.float32(an_after.particle_var)), (what, got_prev, an_after.particle_var)
    assert int(fv["ctl_i"][_lib.LOOP_I_INIT]) == an_after.init_particles and int(fv["ctl_i"][_lib.LOOP_I_VARSET]) == 1, what
    assert int(fv["ctl_i"][_lib.LOOP_I_N]) == keep.shape[0], what
    return mode, k


def _single_site(dev, orc, cb, traj, n, cap, ties, layout, configs, pick=None, frozen=False):
    """Every case of every (floor, init) configuration on one LoopEngine; -> (cases run, {mode: count}, largest n_after)."""
    from test_gpu_loop import _compare_frame
    from midastouch_amd.loop_engine import LoopEngine
    poses, labels = _particle_set(cb, n, layout)
    tn, rot, u = _host_draws(n)
    loop = orc.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, ties=ties)
    odom, code = traj.odoms[1], traj.codes[1]
    fr = _front(orc, loop, poses, labels, odom, code, tn, rot, ties)
    var = fr["var"]
    assert var > 0 and np.isfinite(var)
    eng = LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, cap, seed=SEED, floor=configs[0][0], device=dev, topk_ties=ties)
    t_poses, t_labels = torch.as_tensor(poses), torch.as_tensor(labels)
    d_odom, d_code = torch.as_tensor(odom).to(dev), torch.as_tensor(code).to(dev)
    d_tn, d_rot, d_u = torch.as_tensor(tn).to(dev), torch.as_tensor(rot).to(dev), torch.as_tensor(u).to(dev)
    ran, modes, top = 0, {0: 0, 1: 0, 2: 0}, 0
    for ci, (floor, init) in enumerate(configs):
        # the frozen site takes the INPUTS of the first configuration's recipe under floor == n == init
        cases = _gpu_cases(var, n, *(CONFIGS_SMALL[0] if frozen else (floor, init)))
        sep = assert_anneal_recipe_conditions(cases, n, *(CONFIGS_SMALL[0] if frozen else (floor, init)), what=(float(var), n, floor, init),
                                              one_sided=ci > 0)
        if ci == 0:
            print(f"anneal rule {ties} {layout} n={n}: var={float(var)!r}, {len(cases)} cases, separating {sep}")
        if pick is not None:
            cases = pick(cases, n, floor, init)
        eng.floor = floor
        for c in cases:
            what = f"{ties}/{layout}/n={n}/floor={floor}/init={init}/{c['tag']} prev={float(c['prev'])!r}"
            an = _annealer(orc, ties, c["prev"], init)
            keep = an.step(fr["weights"], var, floor)
            ref = _tail(orc, fr, keep, u)
            if ran == 0:  # the two halves above are OracleLoop.step cut in two
                whole = orc.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, ties=ties, floor=floor)
                whole.count, whole.annealer = 1, _annealer(orc, ties, c["prev"], init)
                full = whole.step(poses, labels, odom, code, tn, rot, u=u)
                for key, val in ref.items():
                    assert np.array_equal(np.asarray(full[key]), np.asarray(val)), key
            eng.set_particles(t_poses, t_labels)
            eng.set_annealing_state(float(c["prev"]), init)
            assert eng._frozen() is frozen
            eng.step(d_odom, d_code, tn=d_tn, rot=d_rot, u=d_u, dbscan=False)
            fv = eng.frame_view()
            mode, _ = _check_decision(fv, an, var, c["prev"], n, floor, init, keep, what, frozen)
            _compare_frame(fv, ref, what, False)
            ran, top = ran + 1, max(top, fv["n_after"])
            modes[mode] += 1
    assert int(eng.ctl_i[14].item()) == 0
    return ran, modes, top


@pytest.mark.parametrize("layout", ["one", "three"])
@pytest.mark.parametrize("ties", ["index", "aten_cpu"])
def test_decision_small_set_every_recipe_case(dev, oracle, cb, traj, ties, layout):
    """S1 (ties by index: k_loop_anneal_small<true>) and S3 (ATen's rule: the two-pass spreads, var in ATen's order, k_loop_decide, the
    walk): every recipe case of three (floor, init) configurations on 300 particles in a 400-slot engine."""
    cap = N_SMALL + N_SMALL // 3
    assert CONFIGS_SMALL[0][1] == cap
    ran, modes, top = _single_site(dev, oracle, cb, traj, N_SMALL, cap, ties, layout, CONFIGS_SMALL)
    print(f"S{1 if ties == 'index' else 3} {layout}: {ran} cases, modes {modes}")
    assert min(modes.values()) >= 30 and top == cap, (modes, top)  # each answer often; a duplication filled the buffers to the last slot


@pytest.mark.parametrize("layout", ["one", "three"])
@pytest.mark.parametrize("ties", ["index", "aten_cpu"])
def test_decision_frozen_does_nothing_on_every_recipe_input(dev, oracle, cb, traj, ties, layout):
    """S4: floor == n == init_particles, the engine states that annealing cannot act and launches the decision alone - on every input
    of the recipe it must agree (mode 0, no err bit 7) and keep the state as the rule does."""
    ran, modes, top = _single_site(dev, oracle, cb, traj, N_SMALL, N_SMALL, ties, layout, ((N_SMALL, N_SMALL),), frozen=True)
    print(f"S4 {ties} {layout}: {ran} cases")
    assert modes == {0: ran, 1: 0, 2: 0} and top == N_SMALL and ran > 100


def _pick_large(cases, n, floor, init, most=12):
    """At most 12: the specials and the first discriminating cases, the mutants taking turns."""
    return [c for c in _by_priority(cases, n, floor, init) if c["kind"] != "target"][:most]


def _pick_large_single(cases, n, floor, init):
    """S2's 12: eight of the main configuration, and under the floor above the set the first four discriminating removals."""
    if floor < n:
        return _pick_large(cases, n, floor, init, 8)
    return [c for c in _pick_large(cases, n, floor, init, len(cases)) if c["kind"] == "search" and anneal_rule(c["var"], c["prev"], n, floor, init)[0][0] == 1][:4]


def test_decision_multi_launch_form(dev, oracle, cb, traj):
    """S2: 17 000 particles, beyond the single-workgroup form: k_loop_decide, then the radix selection's launches.  Capacity == init ==
    n + n // 3: the finite overflow duplicates n // 3 particles into the last slot.  Four of the twelve cases under a floor of 20 000:
    n < floor, removals by the reference's abs."""
    ran, modes, top = _single_site(dev, oracle, cb, traj, N_LARGE, CONFIG_LARGE[1], "index", "three", (CONFIG_LARGE, (FLOOR_ABOVE, CONFIG_LARGE[1])),
                                   pick=_pick_large_single)
    print(f"S2: {ran} cases, modes {modes}")
    assert ran == 12 and modes[1] > 0 and modes[2] > 0 and top == CONFIG_LARGE[1], (ran, modes, top)


# ---- the batch ----------------------------------------------------------------------------------------------------------------------
def _batch_site(dev, orc, cb, traj, rows, cap, floor, ties, wide, steps, layout="three"):
    """rows: (n, init) per trajectory.  Trajectory b draws from Philox (seed + b, frame 0) in every step (the frame counter is put
    back), so its front is computed once; step s gives row b case b + B s of its own recipe in priority order.
    -> (decisions checked, {mode: count}, largest n_after, rows whose spread is 0)."""
    from test_gpu_loop import _compare_frame
    from midastouch_amd import BatchLoopEngine, _lib
    B = len(rows)
    eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, cap, seed=SEED, floor=floor, device=dev, wide=wide)
    if ties == "aten_cpu":
        eng.topk_ties = "aten_cpu"
    loop = orc.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, ties=ties)
    odom, code = traj.odoms[1], traj.codes[1]
    sets, fronts, lists, us = [], [], [], []
    for b, (n, init) in enumerate(rows):
        poses, labels = _particle_set(cb, n, layout, salt=b)
        tn, rot = orc.philox_noise(n, SEED + b, 0, np.float32(2e-4), np.float32(0.5))
        fr = _front(orc, loop, poses, labels, odom, code, tn, rot, ties)
        sets.append((torch.as_tensor(poses), torch.as_tensor(labels)))
        fronts.append(fr)
        us.append(orc.philox_uniform64(n + n // 3, SEED + b, 0))
        if n == 1:   # one particle has no spread: var == 0, the rule leaves its state alone whatever it holds
            assert fr["var"] == 0
            lists.append([dict(tag="var0", kind="var0", prev=np.float32(0.0123), var=np.float32(0.0))])
            continue
        assert fr["var"] > 0 and np.isfinite(fr["var"]), (b, n)
        cases = _gpu_cases(fr["var"], n, floor, init)
        if n >= 288:  # the rows that carry the conditions; the short rows are the rule's small regimes
            assert_anneal_recipe_conditions(cases, n, floor, init, what=(b, float(fr["var"]), n, floor, init))
        lists.append(_by_priority(cases, n, floor, init))
    rep = lambda a: torch.as_tensor(a)[None].repeat(B, *([1] * a.ndim)).contiguous()  # noqa: E731
    d_odoms, d_codes = rep(odom), rep(code)
    checked, modes, top, zero = 0, {0: 0, 1: 0, 2: 0}, 0, 0
    for s in range(steps):
        chosen = [lst[(b + B * s) % len(lst)] for b, lst in enumerate(lists)]
        eng.set_particles([p for p, _ in sets], [lb for _, lb in sets])
        eng.set_annealing_state([float(c["prev"]) for c in chosen], [init for _, init in rows])
        eng.step_count = 0
        eng.step(d_odoms, d_codes, dbscan=False)
        for b, ((n, init), c, fr) in enumerate(zip(rows, chosen, fronts)):
            what = f"{ties}/row {b}/step {s}/n={n}/init={init}/{c['tag']} prev={float(c['prev'])!r}"
            an = _annealer(orc, ties, c["prev"], init)
            keep = an.step(fr["weights"], fr["var"], floor)
            fv = eng.frame_view(b)
            if fr["var"] == 0:
                assert keep.shape[0] == n and (fv["mode"], fv["k"], fv["n_after"], fv["err"], fv["var"]) == (0, 0, n, 0, 0.0), what
                assert f32_bits(np.float32(fv["ctl_d"][_lib.LOOP_D_VARPREV])) == f32_bits(c["prev"]), what  # left as it was
                zero += 1
                mode = 0
            else:
                mode, _ = _check_decision(fv, an, fr["var"], c["prev"], n, floor, init, keep, what)
            _compare_frame(fv, _tail(orc, fr, keep, us[b]), what, False)
            checked, top = checked + 1, max(top, fv["n_after"])
            modes[mode] += 1
    assert not eng.ctl_i[:, 14].any()
    return checked, modes, top, zero


# 56 rows of 297 .. 300 particles - init = n + n // 3 (row 0: 300 + 100 == the capacity) or one less (the largest duplication is then one
# too many) - and 8 short ones (floor 100 above them: removals by the reference's abs; n // 3 of 0, 1, 2; a single particle, whose
# spread is 0)
ROWS_SMALL = tuple((n, n + n // 3 - (b // 4) % 2) for b in range(56) for n in (300 - b % 4,)) + \
    ((1, 8), (2, 8), (3, 8), (4, 8), (7, 9), (64, 80), (65, 86), (5, 5))


@pytest.mark.parametrize("ties", ["index", "aten_cpu"])
def test_decision_batch_a_case_per_row(dev, oracle, cb, traj, ties):
    """S5 (midas_loop_step_batch: the small form with the trajectory as grid.y) and S6 (midas_loop_step_batch_draws under ATen's tie
    rule: k_loop_decide without select state, the walk): 64 rows that differ in n, prev and init, three steps - 192 decisions."""
    assert ROWS_SMALL[0] == (300, 400) and len(ROWS_SMALL) == 64
    checked, modes, top, zero = _batch_site(dev, oracle, cb, traj, ROWS_SMALL, 400, 100, ties, False, 3)
    print(f"S{5 if ties == 'index' else 6}: {checked} decisions, modes {modes}, {zero} with var == 0")
    assert checked == 192 and min(modes.values()) >= 15 and top == 400 and zero == 3, (checked, modes, top, zero)


def test_decision_wide_batch_second_trajectory(dev, oracle, cb, traj):
    """S7: two trajectories of 17 000 particles in a wide batch: k_loop_decide with blockIdx.y > 0 on its own control block, cluster
    rows and select state.  12 decisions in six steps, each row's cases from its own 12 (the specials, the first discriminating ones);
    capacity == init == n + n // 3, and the floor above the set (a batch has one floor): every removal goes through the reference's abs."""
    floor, init = FLOOR_ABOVE, CONFIG_LARGE[1]
    rows = ((N_LARGE, init), (N_LARGE, init))
    from test_gpu_loop import _compare_frame
    from midastouch_amd import BatchLoopEngine
    eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, 2, init, seed=SEED, floor=floor, device=dev, wide=True)
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices)
    odom, code = traj.odoms[1], traj.codes[1]
    sets, fronts, lists, us = [], [], [], []
    for b, (n, _) in enumerate(rows):
        poses, labels = _particle_set(cb, n, "three", salt=b)
        tn, rot = oracle.philox_noise(n, SEED + b, 0, np.float32(2e-4), np.float32(0.5))
        fr = _front(oracle, loop, poses, labels, odom, code, tn, rot, "index")
        assert fr["var"] > 0
        cases = _gpu_cases(fr["var"], n, floor, init)
        assert_anneal_recipe_conditions(cases, n, floor, init, what=(b, float(fr["var"])))
        sets.append((torch.as_tensor(poses), torch.as_tensor(labels)))
        fronts.append(fr)
        lists.append(_pick_large(cases, n, floor, init))
        us.append(oracle.philox_uniform64(n + n // 3, SEED + b, 0))
    assert all(len(lst) == 12 for lst in lists)
    rep = lambda a: torch.as_tensor(a)[None].repeat(2, *([1] * a.ndim)).contiguous()  # noqa: E731
    modes, top = {0: 0, 1: 0, 2: 0}, 0
    for s in range(6):   # row 0 takes cases 0 .. 5, row 1 cases 6 .. 11 and, first, the finite overflow
        chosen = [lists[0][s], lists[1][(6 + s) if s else 0]]
        eng.set_particles([p for p, _ in sets], [lb for _, lb in sets])
        eng.set_annealing_state([float(c["prev"]) for c in chosen], [init, init])
        eng.step_count = 0
        eng.step(rep(odom), rep(code), dbscan=False)
        for b, (c, fr) in enumerate(zip(chosen, fronts)):
            what = f"wide/row {b}/step {s}/{c['tag']} prev={float(c['prev'])!r}"
            an = _annealer(oracle, "index", c["prev"], init)
            keep = an.step(fr["weights"], fr["var"], floor)
            fv = eng.frame_view(b)
            mode, _ = _check_decision(fv, an, fr["var"], c["prev"], N_LARGE, floor, init, keep, what)
            _compare_frame(fv, _tail(oracle, fr, keep, us[b]), what, False)
            modes[mode] += 1
            top = max(top, fv["n_after"]) if b == 1 else top
    print(f"S7: 12 decisions, modes {modes}")
    assert modes[1] > 0 and modes[2] > 0 and top == init, (modes, top)  # row 1 filled its buffers to the last slot
    assert not eng.ctl_i[:, 14].any()


# ---- the class surface --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", ["index", "aten_cpu"])
def test_annealing_api_on_the_rule_fixture(dev, golden, ties):
    """particle_filter.annealing end to end on fixture G15 - the reference's own decisions: ids, count and state afterwards; the
    infinite ratio raises as the reference does."""
    from midastouch_amd.config import load_config
    from midastouch_amd.particle_filter import Particles, particle_filter
    g = golden("g15_anneal_rule")
    g = {k: g[k] for k in g.files}
    pf = particle_filter(load_config(), np.zeros((8, 3)), 1.0, downsample=1, device=dev)
    pf.topk_ties = ties
    sets = g["sets"]
    parts = []
    for s in range(len(ANNEAL_FIXTURE_SETS)):
        n = int(sets[s, 1])
        ids = torch.arange(n, dtype=torch.float32, device=dev)
        P = torch.eye(4, device=dev)[None].repeat(n, 1, 1).contiguous()
        P[:, 0, 3] = ids
        parts.append((P, torch.as_tensor(g[f"w_{s}"]).to(dev), ids))
    acted = 0
    for i in range(g["case_set"].shape[0]):
        s = int(g["case_set"][i])
        n, floor, init = (int(v) for v in sets[s, 1:4])
        prev, var = f32_from_bits(g["case_prev_bits"][i])[()], f32_from_bits(g["case_var_bits"][i])[()]
        what = (s, str(g["case_tag"][i]))
        pf.particle_var = torch.tensor([float("inf")]) if np.isinf(prev) else torch.tensor(prev)
        pf.init_particles = init
        P, w, ids = parts[s]
        p = Particles(P, w, ids.clone())
        if str(g["case_raises"][i]):
            with pytest.raises(OverflowError):
                pf.annealing(p, torch.tensor(var), floor=floor)
        else:
            out = pf.annealing(p, torch.tensor(var), floor=floor)
            at, cnt = int(g["case_ids_at"][i]), int(g["case_count"][i])
            want = g["ids"][at:at + cnt]
            assert len(out.weights) == cnt and np.array_equal(out.labels.cpu().numpy().astype(np.int32), want), what
            assert np.array_equal(out.poses[:, 0, 3].cpu().numpy().astype(np.int32), want), what
            acted += int(cnt != n)
        after = torch.as_tensor(pf.particle_var).reshape(-1)[0]
        assert int(f32_bits(np.float32(after.item()))) == int(g["case_pv_after_bits"][i]) and int(pf.init_particles) == int(g["case_init_after"][i]), what
    assert acted > 200
