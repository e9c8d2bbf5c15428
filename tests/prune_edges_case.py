"""The prune's lattice cases (tests/_recipes.py, "prune edges") through the sites that take the decision, one function per site;
tests/test_gpu_prune_edges.py calls them in its own process.  Run as a script it sends the frames "all" and "small" through the
stand-alone ops, the vertex lists' export, FilterEngine, PipelinedFilterEngine (two frames), PipelinedBatchFilterEngine and LoopEngine
and prints one line per site: a sha256 of the masks and nearest entries and the number of slots that differ from the integer
predicate - the test starts it in a fresh process per MIDAS_* switch (the library reads them once).  Needs an MI355X."""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from _recipes import PE_LIST, PE_MS, PE_U, pe_frames, pe_world  # noqa: E402

SEED = 4700


def _t(a, dev, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).to(dev)


def case_of(w, prop):
    """The case each propagated pose stands on, by its translation's bits (-1: none, e.g. a NaN translation); asserts that the
    rotations are the identity and the translations the lattice's bit for bit."""
    prop = np.asarray(prop).reshape(-1, 4, 4)
    key = {w.poses[i, :3, 3].tobytes(): i for i in range(w.n)}
    out = np.array([key.get(p[:3, 3].tobytes(), -1) for p in prop])
    rot = prop[out >= 0].copy()   # (a NaN translation spreads over its pose's rows in the product with the odometry: no case's)
    rot[:, :3, 3] = 0
    assert np.array_equal(rot, np.tile(np.eye(4, dtype=np.float32), (len(rot), 1, 1))), "a propagated pose that is not a pure translation"
    return out


def frame_poses(w, idx, extra=None):
    P = w.poses[idx]
    return P if extra is None else np.concatenate([P, np.asarray(extra, dtype=np.float32).reshape(-1, 4, 4)])


def _kw(dev, thr):
    return dict(sig_t=0.0, sig_r=0.0, pen_max=thr, seed=SEED, device=dev)


def _draws(n, dev):
    return _t((np.arange(n, dtype=np.float64) + 0.5) / n, dev)


# ---- the vertex lists ---------------------------------------------------------------------------------------------------------
def vertex_lists(dev, w):
    """Tree.export("vlist") of the world: -> (records' vertices (K, 257, 3) float64, rho (K, 257) float32)."""
    from midastouch_amd import ops
    cbp = _t(w.cb_poses, dev)
    t6, t3 = ops.Tree(ops.se3_feature(cbp)), ops.Tree(_t(w.verts64, dev))
    t6.attach_mesh(t3, cbp)
    raw = t6.export("vlist")
    c = np.ascontiguousarray(raw[:, :, :24]).view(np.float64).reshape(w.n, PE_LIST + 1, 3)
    rho = np.ascontiguousarray(raw[:, :, 24:28]).view(np.float32).reshape(w.n, PE_LIST + 1)
    return c, rho


def check_vertex_lists(w, c, rho):
    """Each case's deciding vertex sits at the record the recipe claims (a tie: it or its twin at the last record); a vertex of rank
    257 or 300 is absent and the header's rho is its distance (rank 257) or the 257th filler's, rounded down; records past a case's own
    vertices are foreign ones, beyond the stop's reach.  -> (problems, per case: the vertex within reach is missing from the list)."""
    bad, absent = [], np.zeros(w.n, dtype=bool)
    for i, cs in enumerate(w.cases):
        hd = c[i, 0]
        if not np.array_equal(hd, w.entries[i] * PE_U):
            bad.append((cs["name"], "header is not the entry"))
        if cs["decider"] is None:
            continue
        V = (cs["V"][cs["decider"]] + w.org[i]) * PE_U
        at = np.flatnonzero((c[i, 1:] == V).all(1)) + 1
        r = cs["rank"]
        if cs["tie"]:
            absent[i] = not len(at)
            if len(at) and at.tolist() != [PE_LIST]:
                bad.append((cs["name"], f"the tie's vertex at {at.tolist()}"))
            twin = (-cs["V"][cs["decider"]] + w.org[i]) * PE_U
            if not ((c[i, PE_LIST] == V).all() or (c[i, PE_LIST] == twin).all()):
                bad.append((cs["name"], "the last record is neither of the tied vertices"))
        elif r <= PE_LIST:
            if at.tolist() != [r]:
                bad.append((cs["name"], f"deciding vertex at {at.tolist()}, want [{r}]"))
        else:
            absent[i] = True
            if len(at):
                bad.append((cs["name"], f"a vertex of rank {r} in the list at {at.tolist()}"))
            rho2 = np.sort(((cs["V"] - cs["E"]) ** 2).sum(1))[PE_LIST]
            want = np.float32(np.sqrt(float(rho2)) * PE_U)
            want = want if float(want) <= np.sqrt(float(rho2)) * PE_U else np.nextafter(want, np.float32(0))
            if rho[i, 0] != want:
                bad.append((cs["name"], f"header rho {rho[i, 0]!r}, want {want!r}"))
    return bad, absent


# ---- the sites ----------------------------------------------------------------------------------------------------------------
def site_ops(dev, w, poses, thr):
    from midastouch_amd import ops
    t3 = ops.Tree(_t(w.verts64, dev))
    dist = ops.nn3_dist(t3, _t(poses, dev))
    wt = torch.ones(len(poses), dtype=torch.float64, device=dev)
    kept = ops.prune_(wt, dist, thr)
    return dict(mask=(wt != 0).cpu().numpy(), kept=int(kept.cpu()[0]), dist=dist.cpu().numpy())


def _engine_frame(eng, valid=None):
    d = dict(prop=eng.poses_prop.cpu().numpy(), nn=eng.nn_idx.cpu().numpy())
    d["mask"] = (eng.weights != 0).cpu().numpy() if valid is None else valid.cpu().numpy() != 0
    return d


def site_engine(name, dev, w, poses, thr, frames=1):
    """FilterEngine / PipelinedFilterEngine / ShardedFilterEngine (one rank): `frames` frames with identity odometry and no noise.
    The pipelined engine's frames are read from the valid bytes, so that the second one runs the folded resample; its weights
    (which materialise the set) are read last and must agree.  -> one dict per frame: prop, nn, mask, kept, tree (telemetry[1]'s growth)."""
    import midastouch_amd.engine as E
    from midastouch_amd.dist import ShardedFilterEngine, SingleComm
    N = len(poses)
    kw = _kw(dev, thr)
    if name == "ShardedFilterEngine":
        eng = ShardedFilterEngine(w.cb_poses, w.emb, w.verts64, N, comm=SingleComm(), **kw)
        tel = eng.st.telemetry
    else:
        eng = getattr(E, name)(w.cb_poses, w.emb, w.verts64, N, **kw)
        tel = eng.telemetry
    eng.set_particles(torch.as_tensor(poses))
    z = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    odom, code, u = torch.eye(4, device=dev), _t(w.code, dev), _draws(N, dev)
    lazy = name == "PipelinedFilterEngine"
    out = []
    for f in range(frames):
        t0 = int(tel[1].cpu())
        eng.step(odom, code, tn=z, rot=z, u=u)
        fr = _engine_frame(eng, eng._valid if lazy else None)
        fr["tree"] = int(tel[1].cpu()) - t0
        out.append(fr)
    last = (eng.weights != 0).cpu().numpy()
    assert np.array_equal(last, out[-1]["mask"]), f"{name}: weights != 0 is not the valid bytes"
    out[-1]["kept"] = int(eng.status.cpu().reshape(-1)[1])
    return out


def site_batch(name, dev, w, rows, thr, frames=1):
    """BatchFilterEngine / PipelinedBatchFilterEngine: `rows` = B pose sets of one size, a trajectory each."""
    import midastouch_amd.engine as E
    B, N = len(rows), len(rows[0])
    eng = getattr(E, name)(w.cb_poses, w.emb, w.verts64, B, N, **_kw(dev, thr))
    eng.set_particles(torch.as_tensor(np.stack(rows)))
    z = torch.zeros((B, N, 3), dtype=torch.float32, device=dev)
    odom, code = torch.eye(4, device=dev)[None].repeat(B, 1, 1), _t(w.code, dev)[None].repeat(B, 1)
    u = _draws(N, dev)[None].repeat(B, 1).contiguous()
    lazy = name == "PipelinedBatchFilterEngine"
    out = []
    for f in range(frames):
        t0 = int(eng.telemetry[1].cpu())
        eng.step(odom, code, tn=z, rot=z, u=u)
        fr = _engine_frame(eng, eng._valid if lazy else None)
        fr["tree"] = int(eng.telemetry[1].cpu()) - t0
        out.append(fr)
    assert np.array_equal((eng.weights != 0).cpu().numpy(), out[-1]["mask"]), f"{name}: weights != 0 is not the valid bytes"
    out[-1]["kept"] = eng.status.cpu().numpy().reshape(B, -1)[:, 1]
    return out


def site_loop(dev, w, poses, thr, cap=None):
    """LoopEngine's first frame on a live count below the capacity (the slots behind it hold a pose 5 m away)."""
    from midastouch_amd.loop_engine import LoopEngine
    n = len(poses)
    cap = cap or n + 77
    kw = _kw(dev, thr)
    eng = LoopEngine(w.cb_poses, w.emb, w.verts64, cap, floor=100000, cluster=False, **kw)
    eng.set_particles(torch.as_tensor(poses))
    z = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    t0 = int(eng.telemetry[1].cpu())
    eng.step(torch.eye(4, device=dev), _t(w.code, dev), tn=z, rot=z, u=_draws(cap, dev), dbscan=False)
    fv = eng.frame_view()
    assert fv["n"] == n
    valid = fv["valid"].cpu().numpy() != 0
    assert np.array_equal(valid, (fv["weights"] != 0).cpu().numpy()), "LoopEngine: weights != 0 is not the valid bytes"
    return dict(prop=fv["poses_prop"].cpu().numpy(), nn=fv["nn_idx"].cpu().numpy(), mask=valid, tree=int(eng.telemetry[1].cpu()) - t0)


def site_batch_loop(dev, w, rows, thr, wide=False, batched=None):
    """BatchLoopEngine's first frame: `rows` = B pose sets of different sizes, a trajectory each."""
    from midastouch_amd import BatchLoopEngine
    B, cap = len(rows), max(len(r) for r in rows) + 77
    eng = BatchLoopEngine(w.cb_poses, w.emb, w.verts64, B, cap, floor=100000, cluster=False, wide=wide, batched_dbscan=batched, **_kw(dev, thr))
    eng.set_particles([torch.as_tensor(r) for r in rows])
    t0 = int(eng.telemetry[1].cpu())
    eng.step(torch.eye(4)[None].repeat(B, 1, 1), torch.as_tensor(w.code)[None].repeat(B, 1), dbscan=False)
    out = []
    for b in range(B):
        fv = eng.frame_view(b)
        assert fv["n"] == len(rows[b])
        valid = fv["valid"].cpu().numpy() != 0
        assert np.array_equal(valid, (fv["weights"] != 0).cpu().numpy()), "BatchLoopEngine: weights != 0 is not the valid bytes"
        out.append(dict(prop=fv["poses_prop"].cpu().numpy(), nn=fv["nn_idx"].cpu().numpy(), mask=valid))
    out[0]["tree"] = int(eng.telemetry[1].cpu()) - t0
    return out


def deal(w, idx, B):
    """B different deals of a frame's cases: rolled by a third each and every other row reversed."""
    rows = []
    for b in range(B):
        r = np.roll(idx, b * (len(idx) // B) + b)
        rows.append(r[::-1].copy() if b % 2 else r)
    return rows


def differing(w, fr, want_idx=None):
    """Slots of an engine frame whose mask or nearest entry is not its case's (the case read from the propagated pose; want_idx:
    the cases the slots must hold, in order)."""
    cs = case_of(w, fr["prop"])
    assert (cs >= 0).all(), "a propagated pose that is no case's"
    if want_idx is not None:
        assert np.array_equal(cs, want_idx), "the frame's particles are not the cases handed in"
    return np.flatnonzero((fr["mask"] != w.keep[cs]) | (fr["nn"] != cs)), cs


def _line(site, fr, bad):
    h = hashlib.sha256()
    for a in (fr["mask"], fr["nn"]):
        h.update(np.ascontiguousarray(a).tobytes())
    print(site, h.hexdigest(), f"bad={len(bad)}", flush=True)


def main():
    dev = torch.device("cuda", 0)
    for m in PE_MS:
        world_lines(dev, pe_world(m))


def world_lines(dev, w):
    frames = pe_frames(w)
    c, rho = vertex_lists(dev, w)
    bad, _ = check_vertex_lists(w, c, rho)
    print(f"m{w.m}-vlist", hashlib.sha256(rho.tobytes()).hexdigest(), f"bad={len(bad)}", flush=True)
    for fname in ("all", "small"):
        fname, idx = f"m{w.m}-{fname}", frames[fname]
        poses = frame_poses(w, idx)
        o = site_ops(dev, w, poses, w.thr)
        _line(f"ops-{fname}", dict(mask=o["mask"], nn=idx), np.flatnonzero(o["mask"] != w.keep[idx]))
        for name in ("FilterEngine", "PipelinedFilterEngine"):
            for f, fr in enumerate(site_engine(name, dev, w, poses, w.thr, frames=2 if name.startswith("Pipelined") else 1)):
                _line(f"{name}-{fname}-{f}", fr, differing(w, fr, idx if f == 0 else None)[0])
        rows = deal(w, idx, 3)
        for f, fr in enumerate(site_batch("PipelinedBatchFilterEngine", dev, w, [w.poses[r] for r in rows], w.thr, frames=2)):
            fr = {k: (v.reshape((-1,) + v.shape[2:]) if isinstance(v, np.ndarray) and v.ndim >= 2 else v) for k, v in fr.items()}
            _line(f"batch-{fname}-{f}", fr, differing(w, fr, np.concatenate(rows) if f == 0 else None)[0])
        fr = site_loop(dev, w, poses, w.thr)
        _line(f"loop-{fname}", fr, differing(w, fr, idx)[0])


if __name__ == "__main__":
    main()
