"""Input recipes shared by the CPU and GPU parity tests (pure integer / exact float64 arithmetic, so the fixtures can
store digests instead of megabytes; the digests in the fixtures guard against drift)."""
import hashlib

import numpy as np


def recipe_weights(n: int, kind: str, seed: int) -> np.ndarray:
    """The weight sets of fixture G2b (same construction as tools/gen_goldens_r2.py::recipe_weights)."""
    i = np.arange(n, dtype=np.uint64)
    h = (i + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    frac = ((h >> np.uint64(11)) & np.uint64((1 << 20) - 1)).astype(np.float64) / float(1 << 20)
    expo = (h & np.uint64(63)).astype(np.int64)
    if kind == "flat":
        w = 1.0 + frac
    elif kind == "peaky":
        w = np.ldexp(1.0 + frac, -(expo % 40))
    elif kind == "masked":
        w = np.ldexp(1.0 + frac, -(expo % 8)) * ((h >> np.uint64(40)) % np.uint64(10) < np.uint64(4))
    elif kind == "dupes":
        w = np.ldexp(1.0, -((expo % 12).astype(np.int64))) * (1.0 + (expo % 3) / 4.0)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(w, dtype=np.float64)


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def g2b_cases(g):
    """-> iterator of (case id, weights, mode, torch seed, sha of the reference's indices, head, tail)."""
    n = int(g["N"])
    for ci in range(int(g["ncases"])):
        w = recipe_weights(n, str(g[f"c{ci}_kind"]), int(g[f"c{ci}_wseed"]))
        assert sha(w) == str(g[f"c{ci}_w_sha"]), "weight recipe drifted from the fixture"
        for mode in ("weighted_random", "low_var"):
            yield (ci, w, mode, int(g[f"c{ci}_{mode}_seed"]), str(g[f"c{ci}_{mode}_sha"]), g[f"c{ci}_{mode}_head"],
                   g[f"c{ci}_{mode}_tail"])


def guard_trace_inputs(g, trace):
    """The operands the G14 traces were made from (tools/gen_guard_trace.py): codebook, odometry with the jump off the mesh at the
    shift frame ("loop", "fixed"; "plain": the trajectory as it is), codes with the NaN entry of the `fixed` trace, ground truth."""
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    cb = make_codebook(K=int(g["K"]), D=int(g["D"]), seed=int(g["cb_seed"]), mesh_points=20000)
    assert sha(cb.embeddings.astype(np.float32)) == str(g["cb_sha"])
    traj = make_trajectory(cb, T=int(g["T"]) + 1, seed=int(g["traj_seed"]))
    odoms, codes = traj.odoms.copy(), traj.codes.copy()
    assert trace in ("loop", "fixed", "plain")
    if trace != "plain":
        odoms[int(g["shift_frame"])][:3, 3] += np.float32(g["shift"])
    if trace == "fixed":
        codes[int(g["nan_frame"])][int(g["nan_at"])] = np.nan
    return cb, odoms, codes, traj.gt_poses


# rmse_r of a kernel against the oracle: both feed bit-identical x = (tr - 1) / 2 to acosf, so only acosf itself (device
# ocml: 4 ulp, the OpenCL bound; glibc: 1 ulp) and the product and the square after it (about 1 ulp a side) can differ -
# under 7 * 2^-23 = 8.3e-7 per term, and an RMS of terms each off by at most eps is off by at most eps ("rmse").
RMSE_R_REL = 2e-6
RMSE_T_REL = 1e-9


def rmse_rel_dev(got, ref) -> float:
    """|got - ref| / |ref| of one rmse value; 0 where both are the same zero or both NaN, inf where only the class differs."""
    got, ref = float(got), float(ref)
    if np.isnan(got) or np.isnan(ref):
        return 0.0 if np.isnan(got) and np.isnan(ref) else float("inf")
    if got == ref:
        return 0.0
    return abs(got - ref) / abs(ref) if ref != 0.0 else float("inf")


def assert_rmse(got2, ref2, what="") -> float:
    """(rmse_t, rmse_r) of a kernel against the oracle's: column 0 within 1e-9 relative, column 1 within RMSE_R_REL, no
    absolute slack (an exact 0 must be an exact 0), NaN equal to NaN.  -> the rotation column's relative deviation."""
    got2 = np.asarray(got2.detach().cpu().numpy() if hasattr(got2, "detach") else got2, dtype=np.float64).reshape(-1)
    ref2 = np.asarray(ref2, dtype=np.float64).reshape(-1)
    assert got2.shape == (2,) and ref2.shape == (2,), (got2.shape, ref2.shape)
    dt, dr = rmse_rel_dev(got2[0], ref2[0]), rmse_rel_dev(got2[1], ref2[1])
    assert dt <= RMSE_T_REL, f"{what}: rmse_t {got2[0]!r} vs oracle {ref2[0]!r} (rel {dt:.3g})"
    assert dr <= RMSE_R_REL, f"{what}: rmse_r {got2[1]!r} vs oracle {ref2[1]!r} (rel {dr:.3g})"
    return dr


# ---- rmse inputs shared by tests/test_oracle_math.py (CPU) and tests/test_gpu_rmse.py ------------------------------------------
RMSE_CLOUDS = ("band5", "band20", "noise0.5", "noise3")
# rmse_r against the float64 geodesic angle (derivations: tests/test_oracle_math.py::test_rmse_clouds_vs_float64)
RMSE_R_REL_F64 = {"band5": 1e-5, "band20": 1e-5, "noise0.5": 1e-4, "noise3": 1e-4}
RMSE_T_REL_F64 = 1e-8


def _pose(R, t):
    P = np.zeros(R.shape[:-2] + (4, 4), dtype=np.float32)
    P[..., :3, :3], P[..., :3, 3], P[..., 3, 3] = R, t, 1.0
    return P


def rmse_cloud(kind: str, n: int, seed: int = 0):
    """-> (poses (n,4,4) float32, gt (4,4) float32): a random gt and n particles turned away from it by an angle uniform in
    [5, 175] / [20, 160] degrees about a random axis ("band5", "band20"), or by zyx Euler noise of 0.5 / 3 degrees per axis
    ("noise0.5", "noise3": the motion model's regime), 2 mm of translation noise.  The gt depends on (kind, seed) only: the
    clouds of one kind at every size stand around the same pose."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng([seed, 2000, RMSE_CLOUDS.index(kind)])
    Rgt = Rotation.from_rotvec(_unit(rng, 1)[0] * rng.uniform(0.3, 3.0)).as_matrix()
    tgt = rng.uniform(-0.1, 0.1, 3)
    if n != 2000:  # (2000 particles: the stream goes on, the cloud of tests/test_oracle_math.py)
        rng = np.random.default_rng([seed, n, RMSE_CLOUDS.index(kind), 1])
    if kind.startswith("band"):
        lo = float(kind[4:])
        Rd = Rotation.from_rotvec(_unit(rng, n) * np.deg2rad(rng.uniform(lo, 180.0 - lo, (n, 1)))).as_matrix()
    else:
        Rd = Rotation.from_euler("zyx", rng.normal(0.0, float(kind[5:]), (n, 3)), degrees=True).as_matrix()
    return _pose(Rgt @ Rd, tgt + rng.normal(0.0, 2e-3, (n, 3))), _pose(Rgt, tgt)


def _unit(rng, n):
    a = rng.standard_normal((n, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def rmse_ref64(poses, gt, angles=False):
    """(rmse_t, rmse_r) - with angles=True, (rmse_t, rmse_r, the terms' angles in degrees) - from the float32 inputs widened to float64: R_d = R_gt R_n^T, the geodesic angle
    atan2(|vee(R_d - R_d^T)| / 2, (tr R_d - 1) / 2) in degrees (well conditioned at every angle, unlike acos), the float64 norm."""
    P, G = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4), np.asarray(gt, dtype=np.float64)
    Rd = G[None, :3, :3] @ P[:, :3, :3].transpose(0, 2, 1)
    A = Rd - Rd.transpose(0, 2, 1)
    s = 0.5 * np.sqrt(A[:, 2, 1] ** 2 + A[:, 0, 2] ** 2 + A[:, 1, 0] ** 2)
    c = 0.5 * (np.trace(Rd, axis1=1, axis2=2) - 1.0)
    th = np.degrees(np.arctan2(s, c))
    e2 = ((G[None, :3, 3] - P[:, :3, 3]) ** 2).sum(axis=1)
    return (float(np.sqrt(e2.mean())), float(np.sqrt((th ** 2).mean()))) + ((th,) if angles else ())


def rmse_edge_terms(seed: int = 0):
    """-> [(name, pose (4,4), gt (4,4))]: the single terms at which the rotation formula changes class (about 200): pose equal
    to gt; gt turned by exactly pi and by pi -+ 1e-3 about the frame axes and random ones; rotation rows of gt scaled by
    1 +- 2^-20 (x = (tr - 1) / 2 above 1: NaN, hence 0; just below 1); a zero rotation block (120 degrees); a NaN or an Inf in a
    rotation or a translation entry of the pose or of gt."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng([seed, 77])
    eye = _pose(np.eye(3), np.zeros(3))
    gts = [eye] + [_pose(Rotation.from_rotvec(_unit(rng, 1)[0] * rng.uniform(0.2, 3.0)).as_matrix(), rng.uniform(-0.1, 0.1, 3))
                   for _ in range(7)]
    axes = list(np.eye(3)) + list(_unit(rng, 5))
    out = []
    for g, G in enumerate(gts):
        shifted = G.copy()
        shifted[:3, 3] += np.float32(1e-3)
        out.append((f"same g{g}", G.copy(), G))
        out.append((f"same rotation g{g}", shifted, G))
        for a, ax in enumerate(axes):
            for d in (0.0, -1e-3, 1e-3):
                P = shifted.copy()
                P[:3, :3] = G[:3, :3].astype(np.float64) @ Rotation.from_rotvec(ax * (np.pi + d)).as_matrix()
                out.append((f"pi{d:+g} axis{a} g{g}", P, G))
        for s in (2.0 ** -20, -(2.0 ** -20)):
            Gs = G.copy()
            Gs[:3, :3] *= np.float32(1.0 + s)
            out.append((f"rows scaled 1{s:+.3g} g{g}", shifted, Gs))
        Z = shifted.copy()
        Z[:3, :3] = 0.0
        out.append((f"zero rotation g{g}", Z, G))
        turned = shifted.copy()  # 30 degrees away: a term that stays finite where only the translation is spoilt
        turned[:3, :3] = G[:3, :3].astype(np.float64) @ Rotation.from_rotvec(axes[3 + g % 5] * np.deg2rad(30.0)).as_matrix()
        out.append((f"30 degrees g{g}", turned, G))
        for val, vn in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
            for where, (i, j) in (("rotation", (int(rng.integers(3)), int(rng.integers(3)))), ("translation", (int(rng.integers(3)), 3))):
                if g < 4 or vn == "nan":
                    P = turned.copy()
                    P[i, j] = val
                    out.append((f"{vn} in the pose's {where} g{g}", P, G))
                if g < 2:
                    Gb = G.copy()
                    Gb[i, j] = val
                    out.append((f"{vn} in gt's {where} g{g}", turned, Gb))
    return out


def rmse_mixed_cloud(n: int, seed: int = 0, nan_translation_last: bool = False):
    """A "noise0.5" cloud of n particles with edge terms at lane 0, lane 63, the first lane of the last (partial) wave and the very
    last particle, and next to them: NaN-to-0 terms beside finite ones, a 180 degree term, an exact-zero term, a 120 degree one.
    nan_translation_last: the last particle's translation holds a NaN instead (rmse_t NaN, the rotation column as before)."""
    from scipy.spatial.transform import Rotation
    poses, gt = rmse_cloud("noise0.5", n, seed + 100)
    last_wave = (n - 1) // 64 * 64
    R = gt[:3, :3].astype(np.float64)
    poses[0, :3, :3] = gt[:3, :3] * np.float32(1.0 + 2.0 ** -20)             # x > 1: NaN, hence 0
    poses[1, 0, 1] = np.inf                                                  # Inf in the trace: NaN, hence 0
    poses[62, :3, :3] = 0.0                                                  # 120 degrees
    poses[63, :3, :3] = R @ Rotation.from_rotvec([np.pi, 0.0, 0.0]).as_matrix()   # 180 degrees (or NaN-to-0: x = -1 to an ulp)
    poses[64, :3, :3] = R @ Rotation.from_rotvec([0.0, np.pi - 1e-3, 0.0]).as_matrix()
    poses[last_wave] = gt                                                    # the identical pose: an exact zero in both columns
    if last_wave + 1 < n - 1:
        poses[last_wave + 1, 2, 2] = np.nan                                  # NaN rotation entry: 0
    if nan_translation_last:
        poses[n - 1, 1, 3] = np.nan
    else:
        poses[n - 1, 1, 1] = np.nan
    return poses, gt


# ---- cluster centres: a reference that is not the oracle's twin, the derived bounds, the input sets -----------------------------
# (tests/test_cluster_reference.py on the CPU, tests/test_gpu_cluster_pin.py and tests/test_gpu_cluster_finishers.py on the GPU)
U64 = 2.0 ** -53   # unit roundoff of float64
U32 = 2.0 ** -24   # unit roundoff of float32
ROT_GAP_ASSERTED = 1e-3    # eigen gap from which the rotation is compared entry by entry
ROT_GAP_ARBITRARY = 1e-9   # eigen gap below which any method's rotation is arbitrary: finite and orthonormal is all that is asked
ROT_TOL = 2.0 ** -23       # two float32 roundings of an entry in [-1, 1]


def shepperd_branch(poses):
    """The branch of the kernel's quaternion extraction (cluster.hip, quat_of) every pose takes, from the float32 entries widened
    to float64: 0 `tr > 0`, 1 `r00` the largest diagonal entry, 2 `r11 > r22`, 3 the rest."""
    R = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
    r00, r11, r22 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    tr = r00 + r11 + r22
    return np.where(tr > 0.0, 0, np.where((r00 > r11) & (r00 > r22), 1, np.where(r11 > r22, 2, 3)))


def quat_shepperd64(poses):
    """Shepperd's extraction in float64 with the kernel's branch rule, (n, 4) as x, y, z, w with w >= 0, normalised - the yardstick of
    the one- and two-member clusters, where the float32 matrix is the whole input and two extractions of a matrix that is
    orthonormal only to 6e-8 may differ by as much."""
    R = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
    br = shepperd_branch(poses)
    q = np.zeros((R.shape[0], 4))
    for n in range(R.shape[0]):
        r = R[n]
        if br[n] == 0:
            s = np.sqrt(r[0, 0] + r[1, 1] + r[2, 2] + 1.0) * 2.0
            q[n] = ((r[2, 1] - r[1, 2]) / s, (r[0, 2] - r[2, 0]) / s, (r[1, 0] - r[0, 1]) / s, 0.25 * s)
        elif br[n] == 1:
            s = np.sqrt(1.0 + r[0, 0] - r[1, 1] - r[2, 2]) * 2.0
            q[n] = (0.25 * s, (r[0, 1] + r[1, 0]) / s, (r[0, 2] + r[2, 0]) / s, (r[2, 1] - r[1, 2]) / s)
        elif br[n] == 2:
            s = np.sqrt(1.0 + r[1, 1] - r[0, 0] - r[2, 2]) * 2.0
            q[n] = ((r[0, 1] + r[1, 0]) / s, 0.25 * s, (r[1, 2] + r[2, 1]) / s, (r[0, 2] - r[2, 0]) / s)
        else:
            s = np.sqrt(1.0 + r[2, 2] - r[0, 0] - r[1, 1]) * 2.0
            q[n] = ((r[0, 2] + r[2, 0]) / s, (r[1, 2] + r[2, 1]) / s, 0.25 * s, (r[1, 0] - r[0, 1]) / s)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 3] < 0] *= -1.0
    return q


def cluster_reference(poses, w, labels, label_values=None):
    """The cluster centres of particle_filter.get_cluster_centers(method="quat_avg") per label value (default: the sorted unique
    labels) from the float32 poses and the float32-rounded weights exactly as given - not the oracle's arithmetic restated:
      * the flatten rule abs(float32(max - min)) <= 1e-8 (every weight then counts 1); a NaN weight is never flat and makes the
        cluster's rotation, translation and spread NaN (the reference's max, min and sums propagate it);
      * quaternions as the oracle takes them (scipy, qw >= 0) - clusters of ONE OR TWO members take quat_shepperd64 instead;
      * the moment matrix and every translation sum by math.fsum (exactly rounded sums of the float64 products);
      * the rotation from numpy.linalg.eigh; the float32 centre; the spread in two passes around that float32 centre.
    -> a list of dicts, one per label value: center (4,4) f32, std (3,) f32, var (3,) float64 (the two-pass variance), mean64 (3,),
    gap (lambda_1 - lambda_2; inf for a NaN or empty cluster), tmax (max abs(t) of the members), count, flat, nan.  An empty
    cluster: NaN everywhere, count 0, as midas_cluster_centers reports it."""
    import math

    from scipy.spatial.transform import Rotation
    P = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
    w32 = np.asarray(w).astype(np.float32).reshape(-1)
    labels = np.asarray(labels).reshape(-1)
    values = np.unique(labels) if label_values is None else np.asarray(label_values).reshape(-1)
    out = []
    for lab in values:
        sel = labels == lab
        n = int(sel.sum())
        rec = dict(label=int(lab), count=n, flat=False, nan=False, gap=float("inf"), tmax=0.0,
                   center=np.full((4, 4), np.nan, dtype=np.float32), std=np.full(3, np.nan, dtype=np.float32),
                   var=np.full(3, np.nan), mean64=np.full(3, np.nan))
        out.append(rec)
        if n == 0:
            continue
        tp, tw = P[sel].astype(np.float64), w32[sel]
        t = tp[:, :3, 3]
        rec["tmax"] = float(np.abs(t).max())
        rec["center"][3] = (0.0, 0.0, 0.0, 1.0)
        if np.isnan(tw).any():
            rec["nan"] = True
            continue
        rec["flat"] = bool(abs(np.float32(tw.max() - tw.min())) <= 1e-8)
        tw = np.ones(n) if rec["flat"] else tw.astype(np.float64)
        sw = math.fsum(tw)
        if n <= 2:
            q = quat_shepperd64(P[sel])
        else:
            q = Rotation.from_matrix(tp[:, :3, :3]).as_quat()
            q[q[:, 3] < 0] *= -1.0
        M = np.zeros((4, 4))
        for i in range(4):
            for j in range(i, 4):
                M[i, j] = M[j, i] = math.fsum(tw * (q[:, i] * q[:, j])) / sw
        if np.isfinite(M).all():
            evals, evecs = np.linalg.eigh(M)  # ascending
            rec["gap"] = float(evals[3] - evals[2])
            aq = evecs[:, 3] if evecs[3, 3] >= 0 else -evecs[:, 3]
            rec["center"][:3, :3] = Rotation.from_quat(aq).as_matrix()
        mean = np.array([math.fsum(tw * t[:, k]) for k in range(3)]) / sw
        rec["mean64"] = mean
        rec["center"][:3, 3] = mean  # (rounded to float32 here)
        d = t - rec["center"][:3, 3].astype(np.float64)
        rec["var"] = np.array([math.fsum(tw * (d[:, k] * d[:, k])) for k in range(3)]) / sw
        rec["std"] = np.sqrt(rec["var"]).astype(np.float32)
    return out


def spread_kappa(nblocks: int) -> int:
    return 4 * (int(nblocks) + 12) + 4


def assert_cluster(got_c, got_s, ref, nblocks, tag="", log=None):
    """Centres (C,4,4) and spreads (C,3) of a device form against cluster_reference's records `ref`, with bounds that follow from
    the arithmetic (nblocks = the 256-particle workgroups whose partials the finisher adds up).  The effective weights - 1 where the
    set is flattened - must be >= 0: with weights of mixed sign neither the spread bound nor the rotation applies (the moment matrix
    is then not positive semi-definite, which top_eigvec4's trace test assumes):

    Translation.  The kernel's mean is a float64 quotient of two sums whose error (see below) is far under a float32 ulp, rounded
    once to float32: within ONE float32 ulp of float32(the exactly summed mean); exact equality is counted.

    Spread (weights >= 0).  sd = sqrt(var) with var = (S2 - 2 m S1 + m^2 S0) / S0 from the one-pass moments S2 = sum w t^2,
    S1 = sum w t, S0 = sum w and the float32 centre m, in float64 (u = 2^-53).  Every moment is a sum taken through six butterfly
    levels, three additions over the waves and a chain over the blocks - at most nblocks + 8 additions deep - of terms that carry
    at most two product roundings (w t is exact: 24 + 24 bits): each moment is within (nblocks + 10) u of the sum of its terms'
    magnitudes, and with weights >= 0 the three terms of the closed form are bounded by S0 T^2, 2 S0 T^2 and S0 T^2 with
    T = max abs(t): 4 (nblocks + 10) u S0 T^2 in all.  The closed form adds three products (m S1, m m, (m m) S0), two additions
    and the division on the same magnitudes: under 4 * 2 + 4 more.  Hence |var - var_ref| <= E = kappa u T^2 with
    kappa = 4 (nblocks + 12) + 4, and |sd - sd_ref| = |var - var_ref| / (sd + sd_ref), bounded here by E / (sd_ref + sqrt(E))
    - the collapsed set, sd_ref = 0, may report up to sqrt(E) - plus one float32 rounding on either side, 2^-23 sd_ref.
    No slack beyond that: a case outside it means the kernel or this derivation is wrong.

    Rotation.  Eigen gap >= 1e-3: every entry within 2^-23 of the reference's float32 entry (two float32 roundings; the float64
    eigenvector error, about 1e-13 / gap, is far below).  Gap < 1e-9: any answer is arbitrary - finite and orthonormal
    (abs(R R^T - I) < 1e-6) is all that is asked.  In between nothing but finiteness.

    NaN and empty clusters: NaN where the reference is NaN (the bottom row of a cluster with members stays 0 0 0 1).
    -> dict of what was seen: t_ulp (largest translation deviation in ulps), t_exact / t_total, sd_frac (largest deviation as a
    fraction of its bound), sd_equal / sd_total (float32 spreads equal to the reference's), kappa_ratio (largest
    abs(sd^2 - var_ref) / (u T^2) - the measured counterpart of kappa - after taking off 2^-22 var_ref, what rounding sd to
    float32 can account for; kappa_ratio_collapsed: over the sets with var_ref = 0 alone, where nothing is taken off), rot_dev
    (largest entry deviation among the asserted clusters), rot_checked, rot_arbitrary."""
    got_c = np.asarray(got_c.detach().cpu().numpy() if hasattr(got_c, "detach") else got_c, dtype=np.float32).reshape(-1, 4, 4)
    got_s = np.asarray(got_s.detach().cpu().numpy() if hasattr(got_s, "detach") else got_s, dtype=np.float32).reshape(-1, 3)
    assert got_c.shape[0] == len(ref) and got_s.shape[0] == len(ref), (tag, got_c.shape, got_s.shape, len(ref))
    seen = dict(t_ulp=0.0, t_exact=0, t_total=0, sd_frac=0.0, sd_equal=0, sd_total=0, kappa_ratio=0.0, kappa_ratio_collapsed=0.0,
                rot_dev=0.0, rot_checked=0, rot_arbitrary=0)
    kappa = spread_kappa(nblocks)
    for i, r in enumerate(ref):
        what = f"{tag}: cluster {i} (label {r['label']}, {r['count']} members)"
        c, s = got_c[i], got_s[i]
        if r["count"] == 0 or r["nan"]:
            assert np.isnan(s).all() and np.isnan(c[:3]).all(), f"{what}: expected NaN, got {c} {s}"
            if r["count"] == 0:
                assert np.isnan(c[3]).all(), what
            else:
                assert np.array_equal(c[3], np.float32([0, 0, 0, 1])), what
            continue
        assert np.isfinite(c).all() and np.isfinite(s).all(), f"{what}: not finite: {c} {s}"
        assert np.array_equal(c[3], np.float32([0, 0, 0, 1])), what
        # translation
        rt = r["center"][:3, 3]
        ulp = np.spacing(np.abs(rt))
        dev = np.abs(c[:3, 3].astype(np.float64) - rt.astype(np.float64)) / ulp.astype(np.float64)
        seen["t_ulp"] = max(seen["t_ulp"], float(dev.max()))
        seen["t_exact"] += int((c[:3, 3] == rt).sum())
        seen["t_total"] += 3
        assert dev.max() <= 1.0, f"{what}: translation {c[:3, 3]!r} vs {rt!r} ({dev.max():.3g} ulp)"
        # spread
        T2 = r["tmax"] ** 2
        E = kappa * U64 * T2
        rs = r["std"].astype(np.float64)
        bound = 2.0 ** -23 * rs + (E / (rs + np.sqrt(E)) if E > 0.0 else 0.0)
        d = np.abs(s.astype(np.float64) - rs)
        frac = np.where(d == 0.0, 0.0, d / np.where(bound > 0.0, bound, 1e-300))
        seen["sd_frac"] = max(seen["sd_frac"], float(frac.max()))
        seen["sd_equal"] += int((s == r["std"]).sum())
        seen["sd_total"] += 3
        if T2 > 0.0:
            ratio = np.maximum(np.abs(s.astype(np.float64) ** 2 - r["var"]) - 2.0 ** -22 * r["var"], 0.0) / (U64 * T2)
            seen["kappa_ratio"] = max(seen["kappa_ratio"], float(ratio.max()))
            if (r["var"] == 0.0).all():
                seen["kappa_ratio_collapsed"] = max(seen["kappa_ratio_collapsed"], float(ratio.max()))
        assert (d <= bound).all(), (f"{what}: spread {s!r} vs {r['std']!r}: off by {d} where kappa = {kappa}, max|t| = {r['tmax']:.3g} "
                                    f"allow {bound}")
        # rotation
        R = c[:3, :3].astype(np.float64)
        if r["gap"] >= ROT_GAP_ASSERTED:
            dr = float(np.abs(R - r["center"][:3, :3].astype(np.float64)).max())
            seen["rot_dev"] = max(seen["rot_dev"], dr)
            seen["rot_checked"] += 1
            assert dr <= ROT_TOL, f"{what}: rotation off by {dr:.3g} (gap {r['gap']:.3g})\n{c[:3, :3]}\n{r['center'][:3, :3]}"
        elif r["gap"] < ROT_GAP_ARBITRARY:
            seen["rot_arbitrary"] += 1
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6, f"{what}: degenerate mean (gap {r['gap']:.3g}) is not a rotation:\n{R}"
    if log is not None:
        for k, v in seen.items():
            log[k] = (log.get(k, 0) + v) if isinstance(v, int) else max(log.get(k, 0.0), v)
    return seen


# ---- the input sets.  cluster_set(name) -> dict(poses (N,4,4) f32, w (N,) float64 or float32, labels (N,) i64, label_values (C,) i64,
# oracle: whether oracle.cluster_centers applies (no NaN weight, weights >= 0 with a positive sum, label_values its sorted unique
# labels or a permutation with extras), nonneg: weights >= 0).  Names are "group/parameters"; everything is drawn from the name.
CL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4097, 32768, 32769, 65537)
CL_COUNTS = (1, 2, 9, 130, 1000)
CL_AXES = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0), "xy": (2.0 ** -0.5, 2.0 ** -0.5, 0.0)}
CL_PI_ANGLES = {"pi-1e-3": np.pi - 1e-3, "pi-0.05": np.pi - 0.05, "pi": np.pi}
CL_ROT_SPREADS = (0.01, 0.14, 0.5, 1.0, 2.0)
CL_DISTS = (0.05, 0.5, 1.0, 10.0)
CL_SIGMAS = (2e-3, 2e-4, 2e-5, 2e-6, 2e-7, 0.0)
CL_WKINDS = ("random", "flat", "peaky")
CL_ENV_SEEDS = 4
CL_FLATTEN = ("1e-8", "above", "below", "zero", "signed_zero", "all_zero", "below_f32")
CL_NAN_AT = ("first", "last", "block2")
CL_FIN_N = 24577  # 97 blocks; cut at multiples of 4096 into two and three slices
# the other finishers' sets, as the rows of one ops.pose_estimate call each ("neg", "zerosum": bit equality of the forms only)
CL_FIN_ROWS = [[f"fin/far/{CL_FIN_N}", f"fin/collapsed/{CL_FIN_N}", f"fin/uniform/{CL_FIN_N}"],
               [f"fin/pi_x/{CL_FIN_N}", f"fin/pi_y/{CL_FIN_N}", f"fin/pi_z/{CL_FIN_N}"],
               [f"fin/pi_xy/{CL_FIN_N}", f"fin/neg/{CL_FIN_N}", f"fin/zerosum/{CL_FIN_N}"],
               ["size/32769", "fin/collapsed/32769", "fin/uniform/32769"]]  # 129 blocks: the second staging chunk


def _name_seed(name):
    return list(hashlib.sha256(name.encode()).digest()[:8])


def _weights(rng, n, kind):
    if kind == "random":
        w = rng.uniform(0.0, 1.0, n)
    elif kind == "flat":
        return np.full(n, 1.0 / n)
    elif kind == "peaky":
        w = rng.uniform(0.0, 1.0, n) ** 12
    else:
        raise ValueError(kind)
    return w / w.sum()


def _cloud(rng, n, Rc, rot_sigma, tc, sigma_t):
    """n float32 poses: rotation Rc turned by a rotation vector of rot_sigma per axis, translation tc + sigma_t noise."""
    from scipy.spatial.transform import Rotation
    R = (Rc * Rotation.from_rotvec(rot_sigma * rng.standard_normal((n, 3)))).as_matrix() if rot_sigma else np.tile(Rc.as_matrix(), (n, 1, 1))
    return _pose(R, np.asarray(tc) + sigma_t * rng.standard_normal((n, 3)))


def _one(poses, w, **kw):
    n = poses.shape[0]
    return dict(dict(poses=poses, w=w, labels=np.zeros(n, dtype=np.int64), label_values=np.zeros(1, dtype=np.int64), oracle=True, nonneg=True), **kw)


def cluster_set(name: str):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(_name_seed(name))
    rnd_rot = lambda: Rotation.from_rotvec(_unit(rng, 1)[0] * rng.uniform(0.3, 2.5))  # noqa: E731
    group, _, arg = name.partition("/")
    if group == "size":       # one cluster of N particles
        n = int(arg)
        return _one(_cloud(rng, n, rnd_rot(), 0.14, (0.05, -0.03, 0.08), 2e-3), _weights(rng, n, "random"))
    if group == "count":      # C clusters over 4096 particles, labels drawn at random: at C = 1000 most clusters have no member
        C, n = int(arg), 4096  # in most workgroups, some have one or two members and some none at all
        labels = rng.integers(0, C, n).astype(np.int64)
        poses = np.empty((n, 4, 4), dtype=np.float32)
        for c in range(C):
            m = labels == c
            poses[m] = _cloud(rng, int(m.sum()), rnd_rot(), 0.1, rng.uniform(-0.1, 0.1, 3), 2e-3)
        return dict(poses=poses, w=_weights(rng, n, "random"), labels=labels, label_values=np.arange(C, dtype=np.int64), oracle=True, nonneg=True)
    if group == "labels":
        n = 4096
        if arg == "neg_t":    # every translation negative in every coordinate, three clusters in contiguous runs: most workgroups
            labels = np.sort(rng.integers(0, 3, n)).astype(np.int64)  # skip two of them (the signed zeros of the skipped partials)
            vals = np.arange(3, dtype=np.int64)
        elif arg == "wide":   # label values -1, 0 and 2^40
            vals = np.array([1 << 40, -1, 0], dtype=np.int64)
            labels = vals[rng.integers(0, 3, n)]
        else:
            labels = rng.integers(0, 9, n).astype(np.int64)
            vals = rng.permutation(9).astype(np.int64)             # "unsorted"
            if arg == "missing":                                    # a value nobody carries in the middle
                vals = np.concatenate([vals[:4], [77], vals[4:]]).astype(np.int64)
            elif arg != "unsorted":
                raise ValueError(name)
        poses = np.empty((n, 4, 4), dtype=np.float32)
        for v in np.unique(labels):
            m = labels == v
            tc = -rng.uniform(0.2, 0.5, 3) if arg == "neg_t" else rng.uniform(-0.1, 0.1, 3)
            poses[m] = _cloud(rng, int(m.sum()), rnd_rot(), 0.1, tc, 2e-3)
        if arg == "neg_t":
            assert (poses[:, :3, 3] < 0).all()
        return dict(poses=poses, w=_weights(rng, n, "random"), labels=labels, label_values=vals, oracle=True, nonneg=True)
    if group == "pi":         # centres a half turn (nearly, exactly) about an axis, 0.05 rad around them: Shepperd's other branches
        ax, ang = arg.split("/")
        n = 1000
        return _one(_cloud(rng, n, Rotation.from_rotvec(np.array(CL_AXES[ax]) * CL_PI_ANGLES[ang]), 0.05, (0.04, 0.02, -0.07), 2e-3),
                    _weights(rng, n, "random"))
    if group == "straddle":   # 120 degrees about random axes, +- a few degrees: tr = 1 + 2 cos(angle) on both sides of 0
        n = 1000
        R = Rotation.from_rotvec(_unit(rng, n) * (2.0 * np.pi / 3.0 + 0.05 * rng.standard_normal((n, 1)))).as_matrix()
        return _one(_pose(R, np.array((0.04, 0.02, -0.07)) + 2e-3 * rng.standard_normal((n, 3))), _weights(rng, n, "random"))
    if group == "gap":
        n = 2000
        tc = (0.04, 0.02, -0.07)
        if arg.startswith("spread"):
            return _one(_cloud(rng, n, rnd_rot(), float(arg[6:]), tc, 2e-3), _weights(rng, n, "random"))
        if arg == "uniform":
            R = Rotation.random(n, random_state=int(rng.integers(1 << 31))).as_matrix()
            return _one(_pose(R, np.asarray(tc) + 2e-3 * rng.standard_normal((n, 3))), _weights(rng, n, "random"))
        if arg == "two_groups":  # two tight groups 170 degrees apart, 0.6 / 0.4 of the weight
            Ra = rnd_rot()
            Rb = Ra * Rotation.from_rotvec(_unit(rng, 1)[0] * np.deg2rad(170.0))
            P = np.concatenate([_cloud(rng, n // 2, Ra, 0.01, tc, 2e-3), _cloud(rng, n // 2, Rb, 0.01, tc, 2e-3)])
            w = np.concatenate([0.6 * _weights(rng, n // 2, "random"), 0.4 * _weights(rng, n // 2, "random")])
            return _one(P, w)
        if arg == "degenerate":  # two rotations a half turn apart, equal weights: lambda_1 = lambda_2 exactly
            R = np.stack([np.eye(3), np.diag([1.0, -1.0, -1.0])])
            return _one(_pose(R, np.array([tc, tc]) + np.array([[1e-3, 0, 0], [-1e-3, 0, 0]])), np.array([0.5, 0.5]))
        if arg == "single":
            return _one(_cloud(rng, 1, rnd_rot(), 0.0, tc, 0.0), np.array([1.0]))
        if arg == "one_weight":  # the whole weight on one particle
            w = np.zeros(500)
            w[137] = 1.0
            return _one(_cloud(rng, 500, rnd_rot(), 0.14, tc, 2e-3), w)
        raise ValueError(name)
    if group in ("env", "fin"):  # a cluster `dist` metres from the origin, translation noise sigma (0: collapsed onto ONE pose)
        if group == "env":
            dist, sigma, kind, _seed = arg.split("/")
            n, rot = 1000, None
        else:                    # the other finishers' sets: fin/<regime>/<N>
            regime, n = arg.split("/")
            n, kind = int(n), "random"
            dist, sigma, rot = {"far": ("1.0", "0.0002", None), "collapsed": ("1.0", "0.0", None), "uniform": ("0.05", "0.002", "uniform"),
                                "neg": ("0.05", "0.002", None), "zerosum": ("0.05", "0.002", None)}.get(regime, ("0.05", "0.002", regime))
        dist, sigma = float(dist), float(sigma)
        tc = dist * np.array([0.6, -0.64, 0.48])  # a unit vector, no coordinate 0
        if rot is None:
            P = _cloud(rng, n, rnd_rot(), 0.05 if sigma else 0.0, tc, sigma)
        elif rot == "uniform":
            P = _pose(Rotation.random(n, random_state=int(rng.integers(1 << 31))).as_matrix(), tc + sigma * rng.standard_normal((n, 3)))
        else:                    # "pi_x" ..: centred on the exact half turn
            P = _cloud(rng, n, Rotation.from_rotvec(np.array(CL_AXES[rot[3:]]) * np.pi), 0.05, tc, sigma)
        if group == "fin" and regime == "neg":  # weights of mixed sign: no reference applies, the forms agree bit for bit
            return _one(P, rng.uniform(-1.0, 1.0, n), oracle=False, nonneg=False, reference=False)
        if group == "fin" and regime == "zerosum":
            # pairs +a, -a with a in {0.5, 1, 2, 3} (an odd last particle weighs 0): not flat, and the float32 weights add up to
            # exactly 0 in any order - cluster_close divides every moment by sw == 0.  No reference: the forms agree bit for bit.
            a = np.repeat(rng.choice([0.5, 1.0, 2.0, 3.0], n // 2), 2) * np.tile([1.0, -1.0], n // 2)
            w = np.concatenate([a, np.zeros(n - a.shape[0])])
            assert w.astype(np.float32).sum(dtype=np.float64) == 0.0 and w.max() - w.min() > 1.0
            return _one(P, w, oracle=False, nonneg=False, reference=False)
        return _one(P, _weights(rng, n, kind))
    if group == "flatten":    # float32 weights at the flatten rule's boundary, 1000 particles (four workgroups)
        n = 1000
        P = _cloud(rng, n, rnd_rot(), 0.14, (0.05, -0.03, 0.08), 2e-3)
        d = np.float32(1e-8)
        pick = rng.integers(0, 2, n).astype(np.float32)
        pick[:2] = (0.0, 1.0)
        if arg == "1e-8":
            w = pick * d
        elif arg == "above":
            w = pick * np.nextafter(d, np.float32(1.0))
        elif arg == "below":
            w = pick * np.nextafter(d, np.float32(0.0))
        elif arg == "zero":
            w = np.full(n, 0.37, dtype=np.float32)
        elif arg == "signed_zero":
            w = np.where(pick > 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        elif arg == "all_zero":
            w = np.zeros(n, dtype=np.float32)
        elif arg == "below_f32":  # float64 weights that differ only below float32 resolution
            w = 0.37 + 1e-12 * rng.uniform(0.0, 1.0, n)
            assert w.max() > w.min() and np.float32(w.max()) == np.float32(w.min())
        else:
            raise ValueError(name)
        return _one(P, w)
    if group == "nan":        # two clusters; cluster 0's weights all equal but for one NaN; arg: where ("none": the NaN-free twin)
        n = 1000
        labels = (np.arange(n) % 2).astype(np.int64)
        labels[[0, 600, n - 1]] = 0
        P = np.empty((n, 4, 4), dtype=np.float32)
        for c in range(2):
            m = labels == c
            P[m] = _cloud(rng, int(m.sum()), rnd_rot(), 0.1, rng.uniform(-0.1, 0.1, 3), 2e-3)
        w = np.where(labels == 0, 0.37, rng.uniform(0.0, 1.0, n))
        return dict(poses=P, w=w, labels=labels, label_values=np.arange(2, dtype=np.int64), oracle=True, nonneg=True)
    raise ValueError(name)


def cluster_nan_set(where: str):
    """The "nan" set with a NaN weight in cluster 0 at particle 0 ("first"), the last particle ("last") or particle 600, in the third
    workgroup ("block2").  The poses, labels and every other weight are the NaN-free set's."""
    s = dict(cluster_set("nan/twin"))
    w = s["w"].copy()
    w[{"first": 0, "last": -1, "block2": 600}[where]] = np.nan
    return dict(s, w=w, oracle=False)


def cluster_set_names(envelope_seeds: int = CL_ENV_SEEDS):
    """Every set of tests/test_gpu_cluster_pin.py, by group, and ("fin") the sets of tests/test_gpu_cluster_finishers.py to which a
    reference with weights >= 0 applies."""
    return {
        "size": [f"size/{n}" for n in CL_SIZES],
        "count": [f"count/{c}" for c in CL_COUNTS],
        "labels": ["labels/unsorted", "labels/missing", "labels/wide", "labels/neg_t"],
        "shepperd": [f"pi/{ax}/{ang}" for ax in CL_AXES for ang in CL_PI_ANGLES] + ["straddle/0"],
        "gap": [f"gap/spread{s}" for s in CL_ROT_SPREADS] + ["gap/uniform", "gap/two_groups", "gap/degenerate", "gap/single", "gap/one_weight"],
        "env": [f"env/{d}/{s}/{k}/{i}" for d in CL_DISTS for s in CL_SIGMAS for k in CL_WKINDS for i in range(envelope_seeds)],
        "flatten": [f"flatten/{a}" for a in CL_FLATTEN],
        "nan": ["nan/twin"],
        "fin": sorted({n for row in CL_FIN_ROWS for n in row if n.startswith("fin/") and n.split("/")[1] not in ("neg", "zerosum")}),
    }


_CL_REF_CACHE = {}


def cluster_set_reference(name: str):
    """(the set, cluster_reference's records of it) - computed once per process and shared; nobody writes into either."""
    if name not in _CL_REF_CACHE:
        s = cluster_set(name)
        _CL_REF_CACHE[name] = (s, cluster_reference(s["poses"], s["w"], s["labels"], s["label_values"]))
    return _CL_REF_CACHE[name]


# ---- the resample search: the plain reference and draws that land ON the CDF --------------------------------------------------
# (tests/test_resample_reference.py on the CPU, tests/test_gpu_resample_pin.py on the GPU; DESIGN.md, "resample search")
U_MAX = 1.0 - 2.0 ** -53   # the largest draw of a 53-bit uniform
RS_KINDS = ("on", "below", "above", "ends")
RS_SIZES = (1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8193)


def expected_slots(cdf, u, upper):
    """The rule every search claims, by numpy: the lower bound (first slot whose entry is >= u: torch.multinomial), or the upper bound
    (first slot whose entry is > u: the reference's `sampleLocs[c] < weightsSum[i]` loop); a draw beyond the last entry takes N - 1."""
    cdf = np.asarray(cdf, dtype=np.float64)
    return np.minimum(np.searchsorted(cdf, np.asarray(u, dtype=np.float64), "right" if upper else "left"), cdf.shape[0] - 1).astype(np.int32)


def systematic_locs(M, u32):
    """The low-variance sampler's locations restated (modules/particle_filter.py:254-261): float32 offset, float64 grid, fmod 1."""
    off = np.float32(u32) / np.float32(M)
    return np.fmod(np.arange(M, dtype=np.float64) / float(M) + np.float64(off), 1.0)


def tie_share(cdf, u):
    """Fraction of the draws that EQUAL a CDF entry."""
    u = np.asarray(u, dtype=np.float64)
    return float(np.isin(u, np.asarray(cdf, dtype=np.float64)).mean()) if u.size else 0.0


def structural_slots(cdf, guide_unit=4):
    """The slots at which a search changes table, line or path: the ends of the 16-slot chunks, the 256-slot groups and the
    4096-slot blocks with the slot before and after each; the guide-unit ends (units of 4, which contain those of 8 and 16: any
    layout midas_lazy_guide_layout reports); the first and the last valid slot (an entry above its predecessor); both ends of every
    flat run; slot 0, N - 2 and N - 1."""
    cdf = np.asarray(cdf, dtype=np.float64)
    N = cdf.shape[0]
    pick = [np.array([0, N - 2, N - 1])]
    for step in (16, 256, 4096):
        e = np.arange(step - 1, N, step)
        pick += [e - 1, e, e + 1]
    pick.append(np.arange(guide_unit - 1, N, guide_unit))
    rises = np.flatnonzero(np.diff(np.concatenate([[0.0], cdf])) != 0.0)   # slots that carry weight
    if rises.size:
        pick.append(rises[[0, -1]])
    same = np.diff(cdf) == 0.0                                             # slot i + 1 repeats slot i
    starts = np.flatnonzero(same & ~np.concatenate([[False], same[:-1]]))
    stops = np.flatnonzero(same & ~np.concatenate([same[1:], [False]])) + 1
    pick += [starts, stops]
    s = np.unique(np.concatenate(pick))
    return s[(s >= 0) & (s < N)]


def crafted_draws(cdf, kind, rng, M=None, guide_unit=4):
    """M (default N) float64 draws in [0, 1) made from the CDF's own entries, in an `rng` order:
      "on"     every distinct entry itself; with more distinct entries than draws the entries of structural_slots first, then an
               rng sample of the rest;
      "below", "above"  nextafter of the same entries towards 0 and towards 1;
      "ends"   0, 2^-53, 1 - 2^-53, cdf[N - 2] and its two neighbours, the midpoints of the first and of the last interval.
    A value >= 1 (the last entry is 1) becomes 1 - 2^-53.  "below" leaves out the entry 0.0 (a run of pruned particles at the start:
    nothing lies below it).  Spare draws - a frame that lost nine particles in ten has a tenth as many distinct entries as draws -
    come from rng: three in four an entry drawn again (the same treatment), one in four a plain rng.random()."""
    cdf = np.asarray(cdf, dtype=np.float64)
    N = cdf.shape[0]
    M = N if M is None else int(M)
    if kind == "ends":
        distinct = np.unique(cdf)
        vals = [0.0, 2.0 ** -53, U_MAX]
        if N >= 2:
            vals += [cdf[N - 2], np.nextafter(cdf[N - 2], 0.0), np.nextafter(cdf[N - 2], 1.0)]
        pos = distinct[distinct > 0.0]
        vals += [0.5 * pos[0], 0.5 * ((distinct[-2] if distinct.size > 1 else 0.0) + distinct[-1])]
        vals = np.array(vals)
    elif kind in ("on", "below", "above"):
        first = np.unique(cdf[structural_slots(cdf, guide_unit)])
        rest = np.setdiff1d(np.unique(cdf), first)
        if first.size > M:
            first = rng.choice(first, M, replace=False)
        rest = rng.choice(rest, min(rest.size, M - first.size), replace=False)
        vals = np.concatenate([first, rest])
        if kind == "below":
            vals = vals[vals > 0.0]
        if vals.size and vals.size < M:
            vals = np.concatenate([vals, rng.choice(vals, 3 * (M - vals.size) // 4)])
        if kind == "below":
            vals = np.nextafter(vals, 0.0)
        elif kind == "above":
            vals = np.nextafter(vals, 1.0)
    else:
        raise ValueError(kind)
    vals = vals[:M]
    u = np.concatenate([vals, rng.random(M - vals.shape[0])])
    u = np.where(u >= 1.0, U_MAX, u)
    assert u.shape == (M,) and (u >= 0.0).all() and (u < 1.0).all()
    return np.ascontiguousarray(u[rng.permutation(M)])


def tie_weights(N, pruned):
    """The masks of the tie frames: raw weights of exactly 1.0 (or -1.0) * mask.  pruned: "all" valid, every other particle
    ("half"), the second half, the first half, the last particle alone, or the first k particles ("lead<k>")."""
    m = np.ones(N, dtype=bool)
    if pruned == "half":
        m[1::2] = False
    elif pruned == "second":
        m[N // 2:] = False
    elif pruned == "first":
        m[: N // 2] = False
    elif pruned == "last":
        m[N - 1] = False
    elif pruned.startswith("lead"):
        m[: int(pruned[4:])] = False
    elif pruned != "all":
        raise ValueError(pruned)
    return m


# ---- the annealing rule: the float32 decision restated, its mutants, inputs at its edges -----------------------------------------
# (tools/gen_anneal_rule.py writes G15 from these; tests/test_anneal_rule_reference.py on the CPU, tests/test_gpu_anneal_rule.py on
# the GPU; DESIGN.md, "The annealing rule's arithmetic")
ANNEAL_MUTANTS = ("f64", "f64_product", "reciprocal")
ANNEAL_SEARCH_KEEP = 16    # discriminating cases kept per mutant
ANNEAL_SEPARATE_MIN = 8    # ... of which a recipe must hold at least this many (f64_product: sets of at most 300 particles)
# the sets of fixture G15 as (var, n, floor, init, main): main sets carry the discriminating search's conditions; the others are the
# rule's small and one-sided regimes (n < floor: the reference's abs lets it remove; n in 1 .. 4: n // 3 is 0 or 1)
ANNEAL_FIXTURE_SETS = (
    (0.0123456, 300, 100, 400, True),   # the cap by n // 3 bites (|n - floor| = 200), room to grow by n // 3 exactly
    (3.3e-4, 299, 150, 398, True),      # n + n // 3 == init: the largest duplication fills the set to its last slot
    (0.0123456, 300, 250, 340, False),  # the cap by |n - floor| bites (50 < n // 3), growth stops at 40 < n // 3
    (0.0123456, 200, 300, 300, False),  # n < floor
    (3.3e-4, 1, 8, 8, False), (3.3e-4, 2, 8, 8, False), (3.3e-4, 3, 8, 8, False), (3.3e-4, 4, 8, 8, False),
)


def f32_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def f32_from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def anneal_rule(var, prev, n, floor, init, variant="f32"):
    """particle_filter.annealing's rule (modules/particle_filter.py:422-447) behind the first-call and var == 0 exits, over an array
    of previous spreads `prev` (float32): ratio = var / prev; ratio < 1: k = min(int((1 - ratio) * n), |n - floor|, n // 3), remove
    if k; ratio > 1: k = min(int((ratio - 1) * n), n // 3), duplicate if k and k + n <= init.  `int` is Python's: unbounded, and an
    OverflowError on an infinite product.  -> (mode, k) int64 arrays: mode 1 remove, 2 duplicate, 0 nothing (k = 0), -1 raises.
    variant "f32": every operation in float32, as torch evaluates it on 0-dim float32 tensors - THE rule.  The mutants: "f64" all in
    float64; "f64_product" the float32 ratio, then 1 - ratio and the product in float64; "reciprocal" var * (1 / prev) in float32."""
    var, prev, n = np.float32(var), np.atleast_1d(np.asarray(prev, dtype=np.float32)), int(n)
    one, nf = np.float32(1.0), np.float32(n)
    with np.errstate(all="ignore"):
        if variant == "f64":
            ratio = np.float64(var) / prev.astype(np.float64)
            lo, hi = (1.0 - ratio) * float(n), (ratio - 1.0) * float(n)
        elif variant == "f64_product":
            ratio = (var / prev).astype(np.float32)
            lo, hi = (1.0 - ratio.astype(np.float64)) * float(n), (ratio.astype(np.float64) - 1.0) * float(n)
        elif variant in ("f32", "reciprocal"):
            ratio = (var / prev if variant == "f32" else var * (one / prev)).astype(np.float32)
            lo, hi = (one - ratio) * nf, (ratio - one) * nf
            assert lo.dtype == np.float32 and hi.dtype == np.float32
        else:
            raise ValueError(variant)
        lo, hi = np.trunc(lo.astype(np.float64)), np.trunc(hi.astype(np.float64))
        k1 = np.minimum(np.minimum(lo, float(abs(n - int(floor)))), float(n // 3))
        k2 = np.minimum(hi, float(n // 3))
        remove, grow = (ratio < 1) & (k1 > 0), (ratio > 1) & (k2 > 0) & (k2 + n <= int(init))
        raises = (ratio > 1) & np.isinf(hi)
    mode = np.where(raises, -1, np.where(remove, 1, np.where(grow, 2, 0))).astype(np.int64)
    k = np.where(mode == 1, k1, np.where(mode == 2, k2, 0.0)).astype(np.int64)
    return mode, k


def _ulp_steps(x, steps):
    """The float32 values `steps` ulps away from each positive finite x (an array per x, flattened in order)."""
    b = f32_bits(x).astype(np.int64).reshape(-1, 1) + np.asarray(steps, dtype=np.int64).reshape(1, -1)
    return f32_from_bits(b.reshape(-1).astype(np.uint32))


def _prev_for(var, n, m, sign):
    """float32(var / float32(1 -+ m / n)): the previous spread at which |1 - ratio| * n stands at the integer m."""
    return np.float32(np.float64(np.float32(var)) / np.float64(np.float32(1.0 - sign * np.asarray(m, dtype=np.float64) / n)))


def recipe_anneal_rule_cases(var, n, floor, init):
    """The inputs of one annealing decision at the rule's edges, for a frame of mean cluster spread `var` (float32, > 0) over n
    particles: a list of dicts tag, kind, prev (np.float32: particle_var before the call; inf: the first call), var (np.float32).

    kind "target": for m in {0, 1, 2, n // 7, |n - floor| - 1 .. + 1, n // 3 - 1 .. + 1, init - n - 1 .. + 1} within [0, n) and both
    signs, prev0 = float32(var / float32(1 -+ m / n)) and its neighbours 1 and 2 ulps either side (m = 0: prev == var, the ratio
    exactly 1 and one ulp beside it).
    kind "search": m = 1 .. min(|n - floor|, n // 3) - 1 below 1 and 1 .. min(n // 3, init - n) - 1 above, prev0 and 4 ulps either
    side, the float32 rule against each of ANNEAL_MUTANTS: the first ANNEAL_SEARCH_KEEP inputs (m ascending, removal first, ulps
    ascending) on which a mutant decides otherwise.
    kind "special": prev NaN (nothing, the state becomes var), 1e-12 (the product finite and beyond 2^31), inf (first call).
    kind "var0": var == 0 on a set prev (the state stays).   kind "out_of_spec": prev == 0, the ratio infinite: the reference raises.
    Everything is a function of (float32 var, n, floor, init) alone."""
    var, n, floor, init = np.float32(var), int(n), int(floor), int(init)
    assert var > 0 and n >= 1
    gap = abs(n - floor)
    cases, seen = [], set()

    def add(tag, kind, prev, v=var):
        key = (int(f32_bits(prev)), int(f32_bits(v)))
        if key not in seen:
            seen.add(key)
            cases.append(dict(tag=tag, kind=kind, prev=np.float32(prev), var=np.float32(v)))

    for tag, p in (("nan", np.nan), ("tiny", 1e-12), ("first", np.inf)):
        add(tag, "special", np.float32(p))
    add("var0", "var0", np.float32(2.0) * var, np.float32(0.0))
    add("prev0", "out_of_spec", np.float32(0.0))
    targets = sorted({m for m in (0, 1, 2, n // 7, gap - 1, gap, gap + 1, n // 3 - 1, n // 3, n // 3 + 1, init - n - 1, init - n, init - n + 1)
                      if 0 <= m < n})
    for m in targets:
        for sign, sn in ((1, "-"), (-1, "+")):
            for d, p in zip((0, 1, -1, 2, -2), _ulp_steps(_prev_for(var, n, m, sign), (0, 1, -1, 2, -2))):
                add(f"m{sn}{m}{d:+d}", "target", p)
    # the discriminating search
    ms, sg = [], []
    for sign, top in ((1, min(gap, n // 3)), (-1, min(n // 3, init - n))):
        ms += list(range(1, max(top, 1)))
        sg += [sign] * (max(top, 1) - 1)
    if ms:
        order = np.lexsort((np.asarray(sg) < 0, np.asarray(ms)))  # m ascending, removal first
        ms, sg = np.asarray(ms)[order], np.asarray(sg)[order]
        steps = np.arange(-4, 5)
        prevs = _ulp_steps(_prev_for(var, n, ms, sg), steps)
        rule = anneal_rule(var, prevs, n, floor, init)
        for mut in ANNEAL_MUTANTS:
            other = anneal_rule(var, prevs, n, floor, init, mut)
            for j in np.flatnonzero((rule[0] != other[0]) | (rule[1] != other[1]))[:ANNEAL_SEARCH_KEEP]:
                add(f"s{'-' if sg[j // 9] > 0 else '+'}{ms[j // 9]}{steps[j % 9]:+d}", "search", prevs[j])
    return cases


def anneal_rule_separations(cases, n, floor, init):
    """How many of the recipe's cases (var > 0, finite prev) each mutant decides otherwise than the float32 rule."""
    live = [c for c in cases if c["var"] > 0 and np.isfinite(c["prev"]) and c["prev"] > 0]
    var = {int(f32_bits(c["var"])) for c in live}
    assert len(var) == 1  # (one frame's cases)
    var, prev = f32_from_bits(var.pop())[()], np.array([c["prev"] for c in live], dtype=np.float32)
    rule = anneal_rule(var, prev, n, floor, init)
    out = {}
    for mut in ANNEAL_MUTANTS:
        other = anneal_rule(var, prev, n, floor, init, mut)
        out[mut] = int(((rule[0] != other[0]) | (rule[1] != other[1])).sum())
    return out


def assert_anneal_recipe_conditions(cases, n, floor, init, what="", one_sided=False):
    """The conditions that keep a recipe honest (not measurements): at least ANNEAL_SEPARATE_MIN of its cases separate the float32
    rule from the float64 rule and from the reciprocal division, and - for sets of at most 300 particles - from the float64 product.
    one_sided: a set whose floor or init_particles cuts the rule's range on one side to under n // 3 (the regimes beside the main
    set: |n - floor| or init - n small) has too few integers in reach for the float64 product, which parts from the rule on about
    eight inputs per hundred integers scanned; the other two conditions hold there as well."""
    sep = anneal_rule_separations(cases, n, floor, init)
    assert sep["f64"] >= ANNEAL_SEPARATE_MIN and sep["reciprocal"] >= ANNEAL_SEPARATE_MIN, (what, sep)
    if n <= 300 and not one_sided:
        assert sep["f64_product"] >= ANNEAL_SEPARATE_MIN, (what, sep)
    return sep


# ---- the softmax guard: one dissenting slot in a cloud collapsed onto one score ---------------------------------------------------
# (tools/gen_softmax_guard.py writes G16 from these; tests/test_softmax_guard_reference.py on the CPU, tests/test_gpu_softmax_guard.py
# on the GPU; DESIGN.md, "The softmax guard's rule")
GUARD_WIDE = 0.4472135954999579               # 1 / sqrt(5): the cosine of e_0 and the float32 row (1, 2, 0, ...)
GUARD_BELOW32 = float(np.float32(1e-8))       # 9.99999993922529e-09: the float32 nearest 1e-8 lies BELOW the edge
GUARD_ABOVE32 = float(np.nextafter(np.float32(1e-8), np.float32(1.0)))   # 1.000000082740371e-08: the next float32, above it
# kind -> (the dissenter's score beside a base of +0.0, whether get_similarity applies the softmax)
GUARD_KINDS = {
    "wide_hi": (GUARD_WIDE, True), "wide_lo": (-GUARD_WIDE, True),
    "edge": (1e-8, False), "above": (float(np.nextafter(1e-8, 1.0)), True), "below": (float(np.nextafter(1e-8, 0.0)), False),
    "above32_hi": (GUARD_ABOVE32, True), "above32_lo": (-GUARD_ABOVE32, True),
    "below32_hi": (GUARD_BELOW32, False), "below32_lo": (-GUARD_BELOW32, False),
    "signed_zero": (-0.0, False), "nan": (float("nan"), True),
}
GUARD_WIDE_KINDS = ("wide_hi", "wide_lo")
GUARD_EDGE_KINDS = tuple(k for k in GUARD_KINDS if k not in GUARD_WIDE_KINDS)
# the kinds a float32 codebook row can produce: kind -> the first two entries of the row (the rest 0) under the code e_0
GUARD_ROWS = {
    "wide_hi": (1.0, 2.0), "wide_lo": (-1.0, 2.0),
    "above32_hi": (GUARD_ABOVE32, 1.0), "above32_lo": (-GUARD_ABOVE32, 1.0),
    "below32_hi": (GUARD_BELOW32, 1.0), "below32_lo": (-GUARD_BELOW32, 1.0),
    "nan": (float("nan"), 1.0),
}
GUARD_N = 12345                               # 3 * 4096 + 57: the last lane of the last group holds one live slot
GUARD_SLOTS = (0, 3, 63, 64, 255, 256, 1023, 1024, 4095, 4096, 8191, 10114, 12288, 12344)
GUARD_EDGE_SLOTS = (0, 10114, 12344)
GUARD_SMALL = (1, 2, 15, 16, 17)
GUARD_N66 = 65 * 4096 + 57                    # 266 297: 66 blocks, past the one-wave tables
GUARD_SLOTS66 = (63 * 4096 + 17, 64 * 4096, GUARD_N66 - 1)
GUARD_N258 = 257 * 4096 + 57                  # 1 052 729: 258 blocks, the second round of the 256-strided block loops
GUARD_SLOTS258 = (256 * 4096 - 1, 256 * 4096, GUARD_N258 - 1)
GUARD_K, GUARD_D = 800, 128


def recipe_guard_scores(N, kind, slot):
    """N float64 scores: +0.0 everywhere, x[slot] the dissenter of GUARD_KINDS[kind]."""
    x = np.zeros(int(N), dtype=np.float64)
    x[int(slot)] = GUARD_KINDS[kind][0]
    return x


def guard_applied(N, kind):
    """Whether get_similarity applies the softmax to recipe_guard_scores(N, kind, .): one particle alone is always raw - NaN too,
    as far as the weights go (max - min of a single NaN is NaN: the softmax of one NaN is NaN as well)."""
    return bool(GUARD_KINDS[kind][1]) and (int(N) > 1 or kind == "nan")


def guard_cases(edge_kinds=GUARD_EDGE_KINDS, big=(GUARD_N66,)):
    """(N, kind, slot) of the issue's list: GUARD_N at every slot with the wide kinds, its three edge slots with the edge kinds and
    NaN as well; N in 1, 2, 15, 16, 17 at every slot with every kind; the sizes of `big` at their three slots with every kind."""
    out = [(GUARD_N, k, s) for s in GUARD_SLOTS for k in GUARD_WIDE_KINDS]
    out += [(GUARD_N, k, s) for s in GUARD_EDGE_SLOTS for k in edge_kinds]
    out += [(n, k, s) for n in GUARD_SMALL for s in range(n) for k in GUARD_WIDE_KINDS + tuple(edge_kinds)]
    for n in big:
        slots = {GUARD_N66: GUARD_SLOTS66, GUARD_N258: GUARD_SLOTS258}[n]
        out += [(n, k, s) for s in slots for k in GUARD_WIDE_KINDS + tuple(edge_kinds)]
    return out


def guard_rule_torch(x):
    """particle_filter.get_similarity's tail (modules/particle_filter.py:459-468) restated on float64 scores: the softmax over dim 0
    unless isclose(max - min, a zero of the same dtype) with torch's default tolerances.  -> (weights, applied)."""
    import torch
    w = torch.as_tensor(np.asarray(x, dtype=np.float64))
    if w.numel() == 1:       # (.squeeze() of one target: a 0-dim tensor, max == min, returned as it is)
        return w.numpy().copy(), False
    close = bool(torch.isclose(w.max() - w.min(), torch.zeros(1, dtype=w.dtype)))
    if close:
        return w.numpy().copy(), False
    return torch.softmax(w, dim=0).numpy(), True


def guard_rows(kind, D=GUARD_D):
    """(base row, dissenting row) float32 (D,): (0, 1, 0, ...) and GUARD_ROWS[kind] - under the code e_0 their cosines are 0 and the
    kind's value exactly (the norm sqrt(1 + a^2) is 1.0 in float64 for the 1e-8 rows; 1 / sqrt(5) for the wide ones)."""
    base = np.zeros(D, dtype=np.float32)
    base[1] = 1.0
    row = np.zeros(D, dtype=np.float32)
    row[0], row[1] = GUARD_ROWS[kind]
    return base, row


_GUARD_WORLD = {}


def guard_world(d=GUARD_D):
    """The codebook the guard frames stand on, and per row k the row the pose of k lands on once it is moved 5 m off the surface
    (`moved`: a pruned particle still takes a nearest entry and its score counts in the guard) - by the oracle, once per process."""
    if d not in _GUARD_WORLD:
        from midastouch_amd.synthetic import make_codebook
        from oracle import oracle
        cb = make_codebook("004_sugar_box", K=GUARD_K, D=d, seed=1005)
        off = cb.poses.copy()
        off[:, :3, 3] += 5.0
        ofl = oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices, pen_max=0.5)
        assert np.array_equal(ofl.SE3_NN_idx(cb.poses), np.arange(GUARD_K)), "codebook poses that are not their own nearest entry"
        moved = ofl.SE3_NN_idx(off)
        dist_on, dist_off = oracle.nn3_dist(cb.poses, ofl.verts), oracle.nn3_dist(off, ofl.verts)
        assert (dist_on <= 0.5).all() and (dist_off > 0.5).all()
        _GUARD_WORLD[d] = (cb, moved)
    return _GUARD_WORLD[d]


_GUARD_FRAMES = {}


def guard_frame(N, kind, slot, pruned="none", d=GUARD_D, salt=0):
    """An engine frame whose scores are recipe_guard_scores(N, kind, slot): every codebook row (0, 1, 0, ...) but row k*, the kind's
    dissenting row; the code e_0; identity odometry, no motion noise, pen_max = 0.5; every particle on a codebook pose, the pruned
    ones 5 m off the surface.  pruned: "none", "half" (every other particle but the dissenter) or "dissenter" (the dissenting
    particle alone - it then starts on the pose whose moved copy lands on k*).  What is asserted here, on the CPU: the scores of
    the two rows are exactly the kind's; nn = the constructed nearest entries (guard_world's `moved` for the pruned) name k* at
    `slot` and nowhere else.  slot None: the flat twin for a batch row beside dissenting rows - the same codebook, nobody on k*, the
    code e_1: every particle scores exactly 1.0.  -> a namespace like tie_frame's with nn, mask, x (the scores per particle), kstar."""
    import types
    key = (N, kind, slot, pruned, d, salt)
    if key in _GUARD_FRAMES:
        return _GUARD_FRAMES[key]
    from oracle import oracle
    cb, moved = guard_world(d)
    K = GUARD_K
    flat = slot is None
    assert kind in GUARD_ROWS and (flat or 0 <= slot < N) and pruned in ("none", "half", "dissenter")
    assert pruned != "dissenter" or (GUARD_KINDS[kind][1] and not flat), "pruning the dissenter of a raw kind leaves every weight zero"
    mask = np.ones(N, dtype=bool)
    rng = np.random.default_rng([N, N if flat else slot, salt, 41 + flat])
    if pruned == "dissenter":
        mask[slot] = False
        home = 0
        kstar = int(moved[home])             # the entry the moved dissenter lands on
    else:
        if pruned == "half":
            mask[rng.random(N) < 0.5] = False
            mask[0 if flat else slot] = True
        kstar = int(np.setdiff1d(np.arange(K), moved)[0])   # an entry no moved pose lands on
        home = kstar
    others = np.setdiff1d(np.arange(K), [kstar, home])
    idx = others[rng.integers(0, others.shape[0], N)]
    if not flat:
        idx[slot] = home
    nn = np.where(mask, idx, moved[idx]).astype(np.int32)
    if flat:
        assert (nn != kstar).all(), "a flat frame with a particle on the dissenting row"
    else:
        assert nn[slot] == kstar and (np.delete(nn, slot) != kstar).all(), "the dissenting row is not the dissenter's alone"
    base, row = guard_rows(kind, d)
    emb = np.tile(base, (K, 1))
    emb[kstar] = row
    code = np.zeros(d)
    code[1 if flat else 0] = 1.0
    sc = oracle.score_codebook(emb, code)
    val = GUARD_KINDS[kind][0]
    if flat:
        assert (np.delete(sc, kstar) == 1.0).all()
    else:
        assert np.array_equal(sc[[kstar]], [val], equal_nan=True) and (np.delete(sc, kstar) == 0.0).all() and not np.signbit(np.delete(sc, kstar)).any()
    start = cb.poses[idx].copy()
    start[~mask, :3, 3] += 5.0
    x = sc[nn]
    assert np.array_equal(x, np.ones(N) if flat else recipe_guard_scores(N, kind, slot), equal_nan=True)
    fr = types.SimpleNamespace(key=("guard",) + key, N=N, kind=kind, slot=slot, pruned=pruned, emb=emb, code=code, odom=np.eye(4, dtype=np.float32),
                               start=start, kw=dict(sig_t=0.0, sig_r=0.0, pen_max=0.5, seed=4600), mask=mask, nn=nn, x=x, scores=sc,
                               kstar=kstar, applied=False if flat else guard_applied(N, kind), d=d, idx=idx)
    _GUARD_FRAMES[key] = fr
    return fr


def guard_expected(fr, shard=None):
    """What every engine must report for a guard frame, from its construction and the oracle's arithmetic alone (no nearest-neighbour
    search: the frame of a million particles is built this way too): e = softmax_numerators(x, shift = 1), S = the blocked sum of e
    over ALL particles, weights = e / S * mask, the CDF of e * mask and its status.  shard = (ranks, n_loc): the sums as `ranks`
    ranks of n_loc slots add them - every rank's slots in blocks of their own, +0.0 padded (tests/test_gpu_resample_pin.py)."""
    from oracle import oracle
    e, applied = oracle.softmax_numerators(fr.x, True, shift=1.0)
    assert applied == fr.applied, (fr.key, applied)
    em = e * fr.mask
    if shard is None:
        pad_of, keep = (lambda a: a), slice(None)
    else:
        ranks, n_loc = shard
        pad = (-n_loc) % 4096
        pad_of = lambda a: np.concatenate([np.concatenate([a[r * n_loc:(r + 1) * n_loc], np.zeros(pad)]) for r in range(ranks)])  # noqa: E731
        keep = np.concatenate([np.arange(n_loc) + r * (n_loc + pad) for r in range(ranks)])
    S = oracle.blocked_scan(pad_of(e))[1] if applied else 1.0
    c, status = oracle.cdf(pad_of(em))
    return dict(e=e, em=em, applied=applied, weights=e / S * fr.mask, cdf=c[keep], status=status, V=int(fr.mask.sum()), N=fr.N)
