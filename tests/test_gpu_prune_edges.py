"""The prune on the device at its edges: invalid = dist_to_nearest_vertex > pen_max (modules/particle_filter.py:379-403) on the
lattice world of tests/_recipes.py ("prune edges") - a vertex exactly on the threshold sphere, at m^2 - 1 and at m^2 + 1 in every
direction class, entry, particle and vertex on one line, the deciding vertex at the records 1, 8 | 9, 16 | 17, 32 | 33, 80 | 81,
144 | 145, 256 of its entry's list and behind its end (257, 300), ties at the list's end, axis-aligned vertices only the tree reaches,
particles the distance field decides - at every site that takes the decision, by exact equality with the integer predicate
|dV|^2 <= m^2; tests/test_prune_edges_reference.py holds the same cases against the oracle, sklearn and fixture G18 on the CPU.
DESIGN.md, "The prune's rule", has the sites:

  P1 ops.nn3_dist + ops.prune_                    P5 LoopEngine, live count below the capacity
  P2 particle_filter.remove_invalid_particles     P6 BatchLoopEngine: batched, serial, wide
  P3 FilterEngine, PipelinedFilterEngine          P7 ShardedFilterEngine, one rank
  P4 BatchFilterEngine, PipelinedBatchFilterEngine  P8 the same frames under the MIDAS_* switches that choose the prune's path

The paths are shown, not assumed: the exported vertex lists hold every deciding vertex at the record the recipe claims, and
telemetry[1] (prune decisions that went to the tree) grows by at least the cases the lists cannot settle and not at all on a frame
of on-sphere cases within the first 16 records.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _recipes import (PE_DEGENERATE, PE_FACE_MS, PE_LIST, PE_M, PE_MS, PE_TINY_SIZES, PE_U, PE_ULP_THRS, pe_degenerate_expected, pe_face_world, pe_frames,
                      pe_nan_pose, pe_tiled, pe_tiny_world, pe_ulp_world, pe_world)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", params=PE_MS, ids=[f"m{m}" for m in PE_MS])
def w(request):
    """The world of 131 u, where t2 lies an ulp above thr^2, and the world of 113 u, where an on-sphere vertex has d2 == t2 exactly:
    only there does a `<` for the `<=` of a hit test change a mask (the recipes assert their conditions while they build)."""
    return pe_world(request.param)


@pytest.fixture(scope="module")
def frames(w):
    return pe_frames(w)


@pytest.fixture(scope="module")
def lists(dev, w):
    """The vertex lists as the device builder made them, checked against the recipe's ranks once: -> per case, whether the vertex
    within reach is missing from its list (ranks 257, 300; a tie the builder resolved the other way)."""
    import prune_edges_case as pc
    c, rho = pc.vertex_lists(dev, w)
    bad, absent = pc.check_vertex_lists(w, c, rho)
    assert not bad, bad[:8]
    return absent


def _tree_min(w, absent, idx):
    """The cases of a frame that must reach the tree: the recipe's (within a unit of the sphere behind the list's end, under a header
    that cannot stop: 17 in a world), and the ties whose vertex within reach is not listed (all six with either builder): 23 in `all`
    and `small` - what the two-kernel forms report exactly.  The two list-exhausted twins with nothing within reach (`tree_open`)
    come on top where the field does not decide them."""
    return int((w.tree | ((w.family == "tie") & absent))[idx].sum())


def _assert_frame(w, fr, what, want_idx=None):
    import prune_edges_case as pc
    bad, cs = pc.differing(w, fr, want_idx)
    names = [c["name"] for c in w.cases] if hasattr(w, "cases") else [f"{w.name}[{i}]" for i in range(w.n)]
    assert not len(bad), (what, len(bad), [(names[cs[b]], bool(fr["mask"][b]), int(fr["nn"][b])) for b in bad[:8]])
    return cs


# ---- the lists ------------------------------------------------------------------------------------------------------------------
def test_vertex_lists_hold_the_ranks(w, lists):
    """Every list-depth case's deciding vertex at its record, the 257th / 300th absent with the header's rho as claimed (asserted by
    the fixture); here: the families that need the tree are there."""
    assert lists[(w.rank > PE_LIST) & (w.kind != "none")].all() and not lists[(w.rank >= 1) & (w.rank <= PE_LIST) & (w.family != "tie")].any()
    print(f"ties whose vertex within reach is not listed: {int(lists[w.family == 'tie'].sum())} of {int((w.family == 'tie').sum())}")


# ---- P1 -------------------------------------------------------------------------------------------------------------------------
def test_ops_nn3_dist_and_prune(dev, w, oracle):
    """ops.nn3_dist: on the lattice the distances are the oracle's bit for bit and sqrt(d2) u exactly; ops.prune_: the mask and the
    kept count, at the world's threshold and at the degenerate ones (a NaN translation among the particles)."""
    import prune_edges_case as pc
    o = pc.site_ops(dev, w, w.poses, w.thr)
    assert np.array_equal(o["dist"].view(np.uint64), oracle.nn3_dist(w.poses, w.verts64).view(np.uint64))
    has = w.d2 >= 0
    assert np.array_equal(o["dist"][has], np.sqrt(w.d2[has].astype(np.float64)) * PE_U)
    assert np.array_equal(o["mask"], w.keep) and o["kept"] == int(w.keep.sum())
    poses = pc.frame_poses(w, np.arange(w.n), pe_nan_pose())
    for thr in PE_DEGENERATE:
        o = pc.site_ops(dev, w, poses, thr)
        ref = pe_degenerate_expected(w, thr, poses)
        assert np.array_equal(o["mask"], ref) and o["kept"] == int(ref.sum()), thr
    print(f"P1: {w.n} cases, 1 + {len(PE_DEGENERATE)} invocations")


# ---- P2 -------------------------------------------------------------------------------------------------------------------------
def test_class_surface_on_g18(dev, w, golden):
    """particle_filter.remove_invalid_particles on fixture G18: the reference's own w_out and drifted per threshold."""
    from midastouch_amd import ops
    from midastouch_amd.particle_filter import Particles, particle_filter
    g = golden("g18_prune_edges")
    gp, gv, thrs, w_out, gd = (g[f"{k}_{w.m}"] for k in ("parts", "verts", "thr", "w_out", "drifted"))
    assert np.array_equal(gp, w.parts) and np.array_equal(gv, w.verts) and len(thrs) == (5 if w.m == PE_M else 1)
    pf = particle_filter.__new__(particle_filter)
    pf._mesh_tree = ops.Tree(torch.as_tensor(gv.astype(np.float64) * PE_U).to(dev))
    pf.pen_max = 0.002
    P = torch.eye(4)[None].repeat(w.n, 1, 1).clone()
    P[:, :3, 3] = torch.as_tensor((gp * PE_U).astype(np.float32))
    for t, thr in enumerate(thrs):
        parts = Particles(P.to(dev), torch.ones(w.n, dtype=torch.float64, device=dev))
        out, drifted = pf.remove_invalid_particles(parts, invalid_dist=float(thr))
        assert np.array_equal(out.weights.cpu().numpy(), w_out[t].astype(np.float64)) and bool(drifted) == bool(gd[t]), thr
    print(f"P2: {len(thrs)} calls")


# ---- P3, P7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["all", "small"])
@pytest.mark.parametrize("name", ["FilterEngine", "PipelinedFilterEngine", "ShardedFilterEngine"])
def test_engine_frame(dev, w, frames, lists, name, frame):
    """N on both sides of the two-kernel form's limits (512 pipelined, 2048 plain); the pipelined engine runs a second frame whose
    front folds the resample: it holds the cases the first frame kept, in the resampler's order."""
    import prune_edges_case as pc
    idx = frames[frame]
    out = pc.site_engine(name, dev, w, pc.frame_poses(w, idx), w.thr, frames=2 if name == "PipelinedFilterEngine" else 1)
    _assert_frame(w, out[0], f"{name} {frame}", idx)
    lo = _tree_min(w, lists, idx)
    assert lo <= out[0]["tree"] <= lo + int(w.tree_open[idx].sum()), (out[0]["tree"], lo)
    if len(out) > 1:
        cs = _assert_frame(w, out[1], f"{name} {frame}, folded frame")
        assert w.keep[cs].all() and out[1]["tree"] >= _tree_min(w, lists, cs)
    assert out[-1]["kept"] == int(out[-1]["mask"].sum())
    print(f"{name} {frame}: {len(idx)} cases, {len(out)} frames, tree decisions {[o['tree'] for o in out]}")


@pytest.mark.parametrize("name", ["FilterEngine", "PipelinedFilterEngine", "ShardedFilterEngine"])
def test_shallow_frame_stays_off_the_tree(dev, w, frames, name):
    """Only on-sphere cases whose vertex sits within the first 16 records: every decision is a list's, telemetry[1] does not move -
    at 400 and at the frame's own size (the two-kernel form of the eager engine) and tiled twice, past 2048 (its single kernel)."""
    import prune_edges_case as pc
    idx = frames["shallow"]
    for sub in (idx, idx[:400], np.tile(idx, 2)):
        assert len(sub) in (400, len(idx)) or len(sub) > 2048
        out = pc.site_engine(name, dev, w, pc.frame_poses(w, sub), w.thr)
        _assert_frame(w, out[0], f"{name} shallow", sub)
        assert out[0]["mask"].all() and out[0]["tree"] == 0, out[0]["tree"]


# ---- P4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["all", "small"])
@pytest.mark.parametrize("name", ["BatchFilterEngine", "PipelinedBatchFilterEngine"])
def test_batch_engine_frame(dev, w, frames, lists, name, frame):
    """B = 3, the cases dealt differently to each trajectory; the pipelined batch engine's second frame is the folded, presorted one."""
    import prune_edges_case as pc
    rows = pc.deal(w, frames[frame], 3)
    out = pc.site_batch(name, dev, w, [w.poses[r] for r in rows], w.thr, frames=2 if name.startswith("Pipelined") else 1)
    for f, o in enumerate(out):
        for b in range(3):
            fr = dict(prop=o["prop"][b], nn=o["nn"][b], mask=o["mask"][b])
            cs = _assert_frame(w, fr, f"{name} {frame} frame {f} row {b}", rows[b] if f == 0 else None)
            assert f == 0 or w.keep[cs].all()
    lo = 3 * _tree_min(w, lists, frames[frame])
    assert lo <= out[0]["tree"] <= lo + 3 * int(w.tree_open[frames[frame]].sum()), (out[0]["tree"], lo)
    assert np.array_equal(out[-1]["kept"], out[-1]["mask"].sum(1))
    print(f"{name} {frame}: 3 x {len(rows[0])} cases, {len(out)} frames, tree decisions {[o['tree'] for o in out]}")


# ---- P5, P6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["all", "small", "shallow", "shallow x 2"])
def test_loop_engine_frame(dev, w, frames, lists, frame):
    import prune_edges_case as pc
    idx = np.tile(frames["shallow"], 2) if frame == "shallow x 2" else frames[frame]
    fr = pc.site_loop(dev, w, pc.frame_poses(w, idx), w.thr)
    _assert_frame(w, fr, f"LoopEngine {frame}", idx)
    lo = _tree_min(w, lists, idx)
    assert lo <= fr["tree"] <= lo + int(w.tree_open[idx].sum()) and (not frame.startswith("shallow") or fr["tree"] == 0), (fr["tree"], lo)
    print(f"LoopEngine {frame}: {len(idx)} cases, tree decisions {fr['tree']}")


BATCH_LOOP_FORMS = {"batched": dict(batched=True), "serial": dict(batched=False), "wide": dict(wide=True)}


@pytest.mark.parametrize("form", list(BATCH_LOOP_FORMS))
def test_batch_loop_engine_frame(dev, w, frames, lists, form):
    """B = 3: the whole world, the small frame reversed and the shallow frame, a trajectory each (ragged live counts) - with
    batched_dbscan True and False and wide=True; then three trajectories of shallow cases only (tiled past 2048, whole, 400):
    nothing reaches the tree."""
    import prune_edges_case as pc
    rows = [frames["all"], frames["small"][::-1].copy(), frames["shallow"]]
    out = pc.site_batch_loop(dev, w, [w.poses[r] for r in rows], w.thr, **BATCH_LOOP_FORMS[form])
    for b, fr in enumerate(out):
        _assert_frame(w, fr, f"BatchLoopEngine {form} row {b}", rows[b])
    lo = sum(_tree_min(w, lists, r) for r in rows)
    assert lo <= out[0]["tree"] <= lo + sum(int(w.tree_open[r].sum()) for r in rows), (out[0]["tree"], lo)
    print(f"BatchLoopEngine {form}: {[len(r) for r in rows]} cases, tree decisions {out[0]['tree']}")
    rows = [np.tile(frames["shallow"], 2), frames["shallow"], frames["shallow"][:400]]
    out = pc.site_batch_loop(dev, w, [w.poses[r] for r in rows], w.thr, **BATCH_LOOP_FORMS[form])
    for b, fr in enumerate(out):
        _assert_frame(w, fr, f"BatchLoopEngine {form} shallow row {b}", rows[b])
    assert out[0]["tree"] == 0, out[0]["tree"]


# ---- degenerate thresholds ------------------------------------------------------------------------------------------------------
def _assert_degenerate(w, fr, ref_case, ref_nan, what, want=None, loop=False):
    """A frame under a degenerate threshold: every slot's mask is its case's by the oracle (a NaN translation's: ref_nan), its
    nearest entry the case's own; `want`: the cases the slots must hold (-1: the NaN translation).  -> the expected mask."""
    import prune_edges_case as pc
    if loop and want is not None and not np.where(want >= 0, ref_case[np.maximum(want, 0)], ref_nan).any():
        # (a loop engine's frame that prunes everybody: its view's poses_prop no longer holds the frame's propagated poses - the
        # slots are identified by position instead; the valid bytes are the frame's)
        assert len(fr["mask"]) == len(want) and not fr["mask"].any(), (what, int(fr["mask"].sum()))
        return np.zeros(len(want), dtype=bool)
    cs = pc.case_of(w, fr["prop"])
    assert want is None or np.array_equal(cs, want), f"{what}: the frame's particles are not the cases handed in"
    assert np.isnan(np.asarray(fr["prop"]).reshape(-1, 4, 4)[cs < 0, 0, 3]).all(), what
    exp = np.where(cs >= 0, ref_case[np.maximum(cs, 0)], ref_nan)
    bad = np.flatnonzero((fr["mask"] != exp) | ((fr["nn"] != cs) & (cs >= 0)))
    assert not len(bad), (what, len(bad), [(int(cs[b]), bool(fr["mask"][b]), bool(exp[b])) for b in bad[:8]])
    return exp


@pytest.mark.parametrize("frame", ["all", "small"])
@pytest.mark.parametrize("thr", PE_DEGENERATE, ids=[str(t) for t in PE_DEGENERATE])
def test_degenerate_thresholds(dev, w, frames, thr, frame):
    """thr in 0, +inf, -1e-3, NaN with a NaN translation in the last slot: every site follows ~(dist > thr) as the oracle states it -
    thr = 0 keeps the particle exactly on a vertex (one of them at the world's origin, where the float32 screen's bounds collapse)
    and prunes the one 1 u off it; +inf and NaN keep everybody, the NaN translation (dist = +inf) included; a negative threshold
    prunes everybody.  `small`: the two-kernel form of the eager, pipelined, sharded and loop engines; `all`: the single kernel of the
    eager and the pipelined engine (with its folded second frame), both batch engines (the pipelined one's second frame folded and
    presorted) and BatchLoopEngine.  Masks, nearest entries and the kept counts the sites report."""
    import prune_edges_case as pc
    ref_case = pe_degenerate_expected(w, thr)
    ref_nan = bool(pe_degenerate_expected(w, thr, pe_nan_pose()[None])[0])
    assert ref_nan == (not np.isfinite(thr) or np.isnan(thr)) and not w.poses[w.kind == "0"][0, :3, 3].any()
    if thr == 0.0:
        assert np.array_equal(ref_case, (w.family == "field") & (w.kind == "0")) and ref_case.sum() == 2
    idx = frames["small"][1:] if frame == "small" else frames["all"]   # (small: even with the NaN translation, as the sharded step wants)
    want = np.concatenate([idx, [-1]])
    poses = pc.frame_poses(w, idx, pe_nan_pose())
    ran = 0
    if frame == "small":
        for name in ("FilterEngine", "PipelinedFilterEngine", "ShardedFilterEngine"):
            fr = pc.site_engine(name, dev, w, poses, thr)[0]
            exp = _assert_degenerate(w, fr, ref_case, ref_nan, f"{name} {thr}", want)
            assert fr["kept"] == int(exp.sum()), (name, thr, fr["kept"])
        _assert_degenerate(w, pc.site_loop(dev, w, poses, thr), ref_case, ref_nan, f"LoopEngine {thr}", want, loop=True)
        ran = 4
    else:
        assert len(poses) > 2048
        for name in ("FilterEngine", "PipelinedFilterEngine"):
            out = pc.site_engine(name, dev, w, poses, thr, frames=2 if name.startswith("Pipelined") else 1)
            for f, fr in enumerate(out):
                exp = _assert_degenerate(w, fr, ref_case, ref_nan, f"{name} {thr} frame {f}", want if f == 0 else None)
            assert out[-1]["kept"] == int(exp.sum()), (name, thr, out[-1]["kept"])
            ran += len(out)
        rows = pc.deal(w, idx, 3)
        for name in ("BatchFilterEngine", "PipelinedBatchFilterEngine"):
            out = pc.site_batch(name, dev, w, [pc.frame_poses(w, r, pe_nan_pose()) for r in rows], thr, frames=2 if name.startswith("Pipelined") else 1)
            for f, o in enumerate(out):
                exps = [_assert_degenerate(w, dict(prop=o["prop"][b], nn=o["nn"][b], mask=o["mask"][b]), ref_case, ref_nan, f"{name} {thr} frame {f} row {b}",
                                           np.concatenate([rows[b], [-1]]) if f == 0 else None) for b in range(3)]
            assert out[-1]["kept"].tolist() == [int(e.sum()) for e in exps], (name, thr, out[-1]["kept"])
            ran += 3 * len(out)
        lrows = [idx, frames["small"][::-1].copy(), frames["shallow"]]
        for b, fr in enumerate(pc.site_batch_loop(dev, w, [pc.frame_poses(w, r, pe_nan_pose()) for r in lrows], thr)):
            _assert_degenerate(w, fr, ref_case, ref_nan, f"BatchLoopEngine {thr} row {b}", np.concatenate([lrows[b], [-1]]), loop=True)
        ran += 3
    print(f"degenerate {thr} {frame}: {ran} frames / rows")


def test_nan_translation_at_the_worlds_threshold(dev, w, frames):
    """The NaN translation under an ordinary threshold: dist = +inf, pruned; the cases beside it are untouched - in the two-kernel
    form (small) and in the single kernel (all)."""
    import prune_edges_case as pc
    for idx in (frames["small"], frames["all"]):
        poses = pc.frame_poses(w, idx, pe_nan_pose())
        ref = np.concatenate([w.keep[idx], [False]])
        for name in ("FilterEngine", "PipelinedFilterEngine"):
            fr = pc.site_engine(name, dev, w, poses, w.thr)[0]
            assert np.array_equal(fr["mask"], ref) and np.array_equal(fr["nn"][:-1], idx) and fr["kept"] == int(ref.sum()), name


# ---- the worlds of their own: mesh faces and the field's reach, tiny meshes, the ulp family -------------------------------------------
SMALL_WORLDS = [("face", m) for m in PE_FACE_MS] + [("tiny", nv) for nv in PE_TINY_SIZES] + [("ulp", thr) for thr in PE_ULP_THRS]


@pytest.mark.parametrize("kind,arg", SMALL_WORLDS, ids=[f"{k}-{a}" for k, a in SMALL_WORLDS])
def test_small_worlds(dev, oracle, kind, arg):
    """face: the mesh's extreme vertex on each axis, the particle straight outward at m, m + 1 and beyond the grown grid, with
    thr = 163 u (outside = pruned is armed), 164 u and 180 u (it is not: at 180 u a particle outside the grid is within thr and kept).
    tiny: meshes of 1, 2, 16, 17, 256 and 257 vertices (padding records and a header with rho = inf, a tree of one leaf).
    ulp: off the lattice, d2 == squared_threshold(thr) kept, the next double pruned - a t2 of thr thr, a reversed chain or an
    uncontracted sum puts some of them on the other side.  Every world at its own size and tiled past the two-kernel form's limits."""
    import prune_edges_case as pc
    wd = {"face": pe_face_world, "tiny": pe_tiny_world, "ulp": pe_ulp_world}[kind](arg)
    o = pc.site_ops(dev, wd, wd.poses, wd.thr)
    assert np.array_equal(o["dist"].view(np.uint64), oracle.nn3_dist(wd.poses, wd.verts64).view(np.uint64))
    assert np.array_equal(o["mask"], wd.keep) and o["kept"] == int(wd.keep.sum())
    ran = 1
    for name, n in (("FilterEngine", wd.n), ("FilterEngine", 2100), ("PipelinedFilterEngine", wd.n), ("PipelinedFilterEngine", 600), ("ShardedFilterEngine", 2100)):
        poses, idx = pe_tiled(wd, n)
        out = pc.site_engine(name, dev, wd, poses, wd.thr, frames=2 if (name, n) == ("PipelinedFilterEngine", 600) else 1)
        _assert_frame(wd, out[0], f"{wd.name} {name} N={n}", idx)
        if len(out) > 1:
            assert wd.keep[_assert_frame(wd, out[1], f"{wd.name} {name} N={n}, folded frame")].all()
        ran += len(out)
    _assert_frame(wd, pc.site_loop(dev, wd, wd.poses, wd.thr), f"{wd.name} LoopEngine", np.arange(wd.n))
    idx = pe_tiled(wd, 600)[1]
    rows = [np.roll(idx, 7 * b) for b in range(3)]
    for f, o in enumerate(pc.site_batch("PipelinedBatchFilterEngine", dev, wd, [wd.poses[r] for r in rows], wd.thr, frames=2)):
        for b in range(3):
            _assert_frame(wd, dict(prop=o["prop"][b], nn=o["nn"][b], mask=o["mask"][b]), f"{wd.name} batch frame {f} row {b}", rows[b] if f == 0 else None)
    print(f"{wd.name}: {wd.n} cases, kept {int(wd.keep.sum())}, {ran + 3} engine frames")


# ---- P8 -------------------------------------------------------------------------------------------------------------------------
SWITCHES = [("MIDAS_NO_VSCR", "1"), ("MIDAS_MESH_FIELD", "0"), ("MIDAS_HOST_INDEX", "1"), ("MIDAS_SPLIT_FRONT", "0"), ("MIDAS_SPLIT_FRONT", "3"),
            ("MIDAS_FRONT_SMALL", "0"), ("MIDAS_OVERLAP", "0")]


def _run_case(env_extra):
    env = dict(os.environ)
    for k, _ in SWITCHES:
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "prune_edges_case.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if "bad=" in ln]
    assert len(lines) == 30, r.stdout[-2000:]   # (per world: the lists, and seven per frame: ops, eager, pipelined x 2, batch x 2, loop)
    return {ln[0]: (ln[1], ln[2]) for ln in lines}


@pytest.fixture(scope="module")
def default_lines(dev):
    return _run_case({})


def test_case_script_by_default(default_lines):
    assert all(v[1] == "bad=0" for v in default_lines.values()), default_lines


@pytest.mark.parametrize("name,value", SWITCHES, ids=[f"{k}={v}" for k, v in SWITCHES])
def test_switch_variant(default_lines, name, value):
    """A fresh process per switch: the vertex lists hold the ranks (MIDAS_HOST_INDEX=1: the host builder's), every site's masks
    and nearest entries are the integer predicate's and the digests are the default's - the first frames' all of them; a folded
    frame's too, since the set it resamples is the same."""
    got = _run_case({name: value})
    assert all(v[1] == "bad=0" for v in got.values()), got
    differ = [k for k in got if got[k][0] != default_lines[k][0] and not (name == "MIDAS_HOST_INDEX" and k.endswith("vlist"))]
    assert not differ, differ
