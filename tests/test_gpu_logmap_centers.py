"""`ops.cluster_centers(method="logmap")` (k_cluster_moments_logmap + k_cluster_finish_logmap, cluster_logmap.hpp) against the
yardstick and the derived bounds of tests/_logmap_reference.py, the bit-level properties of the forms (two calls, the workgroup skip
off in a fresh process, weights of mixed sign), the untouched quaternion form, and the torch route of
`particle_filter.get_cluster_centers(method="logmap")`, which stays what it was."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from _logmap_reference import assert_logmap_cluster, logmap_cluster_reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# (N, label values): every staging chunk of the finisher (128 blocks each: 65 537 particles are 257 blocks), one and several
# blocks, C on either side of the workgroup skip (64 | 65) and far beyond it
SIZES = [(1, 1), (2, 2), (255, 1), (256, 2), (257, 3), (4097, 64), (4097, 65), (65537, 2), (65537, 1000)]
SPECIAL = ["flat", "flat_tiny", "flat_edge", "nan_weight", "far", "collapsed", "correlated", "sorted_negative"]
LOG = {}


def _members(rng, n, Rc, tc, rot_deg=3.0, sigma=2e-3):
    P = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    P[:, :3, :3] = (Rc * Rotation.from_rotvec(np.deg2rad(rot_deg) * rng.standard_normal((n, 3)))).as_matrix().astype(np.float32)
    P[:, :3, 3] = (tc + sigma * rng.standard_normal((n, 3))).astype(np.float32)
    return P


def build_set(name):
    """name -> dict(poses (N,4,4) f32, w (N,) float64, labels (N,) i64, label_values (C,) i64, nonneg).  "size/N/C": C label values -
    the label -1 among them and, from C = 2 on, one label nobody carries - over N particles in random order; the SPECIAL names;
    "signed": weights of mixed sign."""
    rng = np.random.default_rng(list(hashlib.sha256(name.encode()).digest()[:8]))
    kind = name.split("/")[0]
    if kind == "size":
        N, C = int(name.split("/")[1]), int(name.split("/")[2])
        carried = max(C - 1, 1)
        labels = rng.integers(0, carried, N) - 1  # -1 .. carried - 2
        if N >= carried:
            labels[rng.permutation(N)[:carried]] = np.arange(carried) - 1  # every carried label has a member
        values = np.arange(carried) - 1
        if C >= 2:
            values = np.concatenate([values, [7777]])
        rots = Rotation.random(carried, random_state=int(rng.integers(1 << 30)))
        tcs = rng.uniform(-0.1, 0.1, (carried, 3))
        P = np.empty((N, 4, 4), dtype=np.float32)
        for c in range(carried):
            m = labels == c - 1
            P[m] = _members(rng, int(m.sum()), rots[c], tcs[c])
        return dict(poses=P, w=rng.uniform(0.0, 1.0, N), labels=labels.astype(np.int64), label_values=values.astype(np.int64), nonneg=True)
    N = 700
    Rc, tc = Rotation.from_rotvec([0.4, -0.9, 0.3]), np.array([0.05, -0.08, 0.1])
    labels, values, w = np.zeros(N, dtype=np.int64), np.array([0], dtype=np.int64), rng.uniform(0.0, 1.0, N)
    P = _members(rng, N, Rc, tc)
    if kind == "flat":
        w = np.full(N, 0.37)
    elif kind == "flat_tiny":  # flat by the rule (max - min <= 1e-8) with weights that differ a hundredfold: every member counts 1
        w = rng.uniform(1e-10, 1e-8, N)
    elif kind == "flat_edge":  # two clusters: max - min the largest float32 difference that is flat, and one float32 step more
        labels = (np.arange(N) % 2).astype(np.int64)
        values = np.array([0, 1], dtype=np.int64)
        w0 = np.float32(1e-3)
        steps = [k for k in range(1, 200) if abs(np.float32(w0 + k * np.spacing(w0)) - w0) <= 1e-8]
        k = max(steps)
        assert abs(np.float32(np.float32(w0 + (k + 1) * np.spacing(w0)) - w0)) > 1e-8
        w = np.full(N, float(w0))
        w[10], w[11] = float(np.float32(w0 + k * np.spacing(w0))), float(np.float32(w0 + (k + 1) * np.spacing(w0)))
    elif kind == "nan_weight":  # not the first member's: the extrema's select lets it lose, the sum does not
        labels = (np.arange(N) % 2).astype(np.int64)
        values = np.array([0, 1], dtype=np.int64)
        w[301] = np.nan
    elif kind == "far":
        labels = (np.arange(N) % 2).astype(np.int64)
        values = np.array([0, 1], dtype=np.int64)
        P[labels == 0] = _members(rng, int((labels == 0).sum()), Rc, np.array([6.0, -8.0, 0.3]))
        P[labels == 1] = _members(rng, int((labels == 1).sum()), Rc.inv(), np.array([-10.0, 0.1, 0.2]), sigma=2e-5)
    elif kind == "collapsed":
        P[:] = P[0]
    elif kind == "correlated":
        # rotations spread 8 degrees, the translation moving with the rotation: t = tc + 0.02 e x g where omega ~ 0.14 g, so that
        # mean(omega x t) = 0.14 * 0.02 * 2 e does not vanish and the centre's translation is NOT the weighted mean translation
        g = rng.standard_normal((N, 3))
        e = np.array([0.0, 0.0, 1.0])
        P[:, :3, :3] = Rotation.from_rotvec(np.deg2rad(8.0) * g).as_matrix().astype(np.float32)
        P[:, :3, 3] = (np.array([0.1, 0.0, 0.0]) + 0.02 * np.cross(e, g)).astype(np.float32)
    elif kind == "sorted_negative":
        # five clusters one after the other (most workgroups hold members of one or two: the skip writes the others' partials) with
        # every translation and most xi components negative: the skipped sums are -0.0 there
        N = 2600
        labels = np.sort(rng.integers(-1, 4, N)).astype(np.int64)
        values = np.array([-1, 0, 1, 2, 3, 9], dtype=np.int64)
        P = _members(rng, N, Rotation.from_rotvec([-0.3, -0.2, -0.25]), np.array([-0.3, -0.2, -0.4]), rot_deg=1.0)
        w = rng.uniform(0.0, 1.0, N)
    elif kind == "signed":
        N = 2600
        labels = np.sort(rng.integers(0, 3, N)).astype(np.int64)
        values = np.array([0, 1, 2], dtype=np.int64)
        P = _members(rng, N, Rc, tc)
        w = rng.uniform(-1.0, 1.0, N)
        return dict(poses=P, w=w, labels=labels, label_values=values, nonneg=False)
    else:
        raise KeyError(name)
    return dict(poses=P, w=w, labels=labels, label_values=values, nonneg=True)


def skip_sets():
    return ["size/4097/64", "size/257/3", "sorted_negative", "signed", "far", "nan_weight"]


def _run(ops, s, method="logmap"):
    dev = torch.device("cuda", 0)
    return ops.cluster_centers(torch.as_tensor(s["poses"]).to(dev), torch.as_tensor(s["w"]).to(dev), torch.as_tensor(s["labels"]).to(dev),
                               torch.as_tensor(s["label_values"]).to(dev), method=method)


def _against_reference(name):
    from midastouch_amd import ops
    s = build_set(name)
    c, sd, cnt = _run(ops, s)
    ref = logmap_cluster_reference(s["poses"], s["w"], s["labels"], s["label_values"])
    assert cnt.cpu().tolist() == [r["count"] for r in ref]
    seen = assert_logmap_cluster(c, sd, ref, -(-len(s["labels"]) // 256), name, LOG)
    print(name, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in seen.items()})
    c2, sd2, cnt2 = _run(ops, s)  # same call twice: the same bits
    assert torch.equal(c.view(torch.int32), c2.view(torch.int32)) and torch.equal(sd.view(torch.int32), sd2.view(torch.int32))
    return s, ref, c.cpu().numpy(), sd.cpu().numpy()


@pytest.mark.parametrize("N,C", SIZES)
def test_sizes(N, C):
    s, ref, c, sd = _against_reference(f"size/{N}/{C}")
    assert len(ref) == C and ref[0]["label"] == -1 and ref[0]["count"] > 0
    if C >= 2:
        assert ref[-1]["count"] == 0 and np.isnan(c[-1]).all() and np.isnan(sd[-1]).all()


@pytest.mark.parametrize("name", SPECIAL)
def test_special(name):
    s, ref, c, sd = _against_reference(name)
    if name in ("flat", "flat_tiny"):
        assert ref[0]["flat"]
    if name == "flat_edge":
        assert ref[0]["flat"] and not ref[1]["flat"]
        assert not np.array_equal(c[0], c[1])
    if name == "nan_weight":
        assert ref[1]["nan"] and not ref[0]["nan"] and np.isnan(c[1, :3]).all() and np.isfinite(c[0]).all()
    if name == "collapsed":
        assert np.array_equal(c[0, :3, 3], s["poses"][0, :3, 3]) and np.abs(sd[0]).max() <= 1e-8
        assert np.abs(c[0, :3, :3] - s["poses"][0, :3, :3]).max() < 3e-6
    if name == "correlated":
        w32 = s["w"].astype(np.float32).astype(np.float64)
        mean_t = (s["poses"][:, :3, 3].astype(np.float64) * w32[:, None]).sum(0) / w32.sum()
        assert np.abs(ref[0]["center64"][:3, 3] - mean_t).max() > 1e-3  # the case's point: a millimetre and more apart
        assert np.abs(c[0, :3, 3] - mean_t).max() > 1e-3
    if name == "sorted_negative":
        assert ref[-1]["count"] == 0 and (c[:-1, :3, 3] < 0).all()


def test_what_was_seen():
    """The largest deviations over this file's cases, beside their bounds (DESIGN.md 2 quotes them); runs after the cases above."""
    if not LOG:
        pytest.skip("runs with the rest of the file")
    print("seen:", {k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in LOG.items()})
    assert LOG["t_f64_frac"] <= 1.0
    assert LOG["sd_frac"] <= 1.0 and LOG["rot_dev"] <= 2.0 ** -23


def test_skip_off_in_a_fresh_process_gives_the_same_bits():
    """MIDAS_MOMENTS_SKIP=0 (every workgroup sums every cluster) against the default, where a workgroup writes the partials of the
    clusters none of its particles belongs to with the log-map form's own signs of zero - and both against this process."""
    from logmap_skip_case import digests
    env = {k: v for k, v in os.environ.items() if k != "MIDAS_MOMENTS_SKIP"}
    lines = []
    for extra in ({}, {"MIDAS_MOMENTS_SKIP": "0"}):
        r = subprocess.run([sys.executable, os.path.join(HERE, "logmap_skip_case.py")], env=dict(env, **extra), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append([ln for ln in r.stdout.splitlines() if ln.strip()])
    assert len(lines[0]) == len(skip_sets()) and lines[0] == lines[1]
    if "MIDAS_MOMENTS_SKIP" not in os.environ:
        assert digests() == lines[0]


def test_mixed_sign_weights_two_calls():
    from midastouch_amd import ops
    s = build_set("signed")
    a, b = _run(ops, s), _run(ops, s)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int64), y.view(torch.int32 if y.dtype == torch.float32 else torch.int64))
    assert a[2].cpu().tolist() == [int((s["labels"] == v).sum()) for v in s["label_values"]]


def test_quat_avg_is_what_it_was():
    """The default, the explicit keyword and - one cluster of everybody - the fixed-N estimate (an untouched instantiation of the
    same accumulation) give the same bits; an unknown method raises."""
    from midastouch_amd import ops
    from midastouch_amd._lib import MidasError
    dev = torch.device("cuda", 0)
    s = build_set("size/4097/64")
    P, w, lab, vals = (torch.as_tensor(s[k]).to(dev) for k in ("poses", "w", "labels", "label_values"))
    d = ops.cluster_centers(P, w, lab, vals)
    q = ops.cluster_centers(P, w, lab, vals, method="quat_avg")
    for x, y in zip(d, q):
        assert torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int64), y.view(torch.int32 if y.dtype == torch.float32 else torch.int64))
    lm = ops.cluster_centers(P, w, lab, vals, method="logmap")
    assert not torch.equal(lm[0][:-1], d[0][:-1])  # (another centre)
    one = ops.cluster_centers(P, w, torch.zeros_like(lab), torch.tensor([0], device=dev))
    ec, es = ops.pose_estimate(P[None], w[None])
    assert torch.equal(one[0][0], ec[0]) and torch.equal(one[1][0], es[0])
    with pytest.raises(MidasError):
        ops.cluster_centers(P, w, lab, vals, method="mean")


# ---- the torch route, which this change leaves alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_per", [[500], [300, 900, 41], [2000, 17, 600, 5, 1200]])
def test_against_the_torch_route(n_per):
    """pf.get_cluster_centers(parts, method="logmap") - pose.logmap_cluster_centers, torch ops - on its own parity cases: centres
    within 5e-6, spreads at rtol 2e-4 (that route's contract, tests/test_cluster_centers.py)."""
    from midastouch_amd import ops
    from midastouch_amd.particle_filter import Particles, particle_filter
    from test_cluster_centers import _clustered
    dev = torch.device("cuda", 0)
    poses, w, labels = _clustered(n_per, seed=21, flat=1 if len(n_per) > 1 else None)
    parts = Particles(torch.as_tensor(poses).to(dev), torch.as_tensor(w).to(dev), torch.as_tensor(labels).to(dev))
    pf = particle_filter.__new__(particle_filter)
    cp, cs = pf.get_cluster_centers(parts, method="logmap")
    c, sd, cnt = ops.cluster_centers(parts.poses, parts.weights, parts.labels, torch.unique(parts.labels), method="logmap")
    assert cnt.cpu().tolist() == [int((labels == u).sum()) for u in np.unique(labels)]
    assert np.abs(c.cpu().numpy() - cp.cpu().numpy()).max() < 5e-6
    np.testing.assert_allclose(sd.cpu().numpy(), cs.cpu().numpy(), rtol=2e-4, atol=1e-8)
    assert_logmap_cluster(c, sd, logmap_cluster_reference(poses, w, labels), -(-len(labels) // 256), f"n_per {n_per}")


def test_no_membership_matrix():
    """N = 65 537, C = 1000: the torch route's (C, N) float64 membership matrix alone is 0.52 GB; the kernel's call allocates the
    three result tensors through torch and 74 MB of partials in the library's scratch."""
    from midastouch_amd import ops
    dev = torch.device("cuda", 0)
    s = build_set("size/65537/1000")
    P, w, lab, vals = (torch.as_tensor(s[k]).to(dev) for k in ("poses", "w", "labels", "label_values"))
    ops.cluster_centers(P[:256], w[:256], lab[:256], vals[:2], method="logmap")  # (the context exists)
    torch.cuda.synchronize(dev)
    free0 = torch.cuda.mem_get_info(dev)[0]
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    c, sd, cnt = ops.cluster_centers(P, w, lab, vals, method="logmap")
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    grown = free0 - torch.cuda.mem_get_info(dev)[0]  # (what the library's scratch took from the device, if it had to grow)
    print(f"peak through torch {peak} B, device memory taken {grown} B")
    assert peak < 0.5e9 and peak < 1 << 20
    assert grown < 0.5e9
    assert int(cnt.sum()) == 65537
