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


# ---- DBSCAN at its edges: points on eps, counts at min_samples, single links ------------------------------------------------------
# (tools/gen_dbscan_edges.py writes G17 from these; tests/test_dbscan_edges_reference.py on the CPU, tests/test_gpu_dbscan_edges.py on
# the GPU; DESIGN.md, "DBSCAN's rule")
# Points on an integer lattice scaled by a power of two, x = V 2^-k with |V| < 2^24, and eps = m 2^-k: the coordinates are exact float32
# values, eps eps is exact in double and every squared distance is an integer times 2^-2k in any arithmetic, any order, fused or not.
# The predicate is |dV|^2 <= m^2 over integers; the reference is a brute-force DBSCAN on int64 with sklearn's scan order.
DB_CELL = 0.577            # cell side / eps (csrc/dbscan.hip DB_CELL)
DB_MAXDIM = 128            # cells per axis of the dense grid
DB_POPS = (1, 63, 64, 65, 255, 256, 257, 300)   # cell populations: the scans step by 64 (link, border) and by 256 (core count)
DB_ROUNDING_MUTANTS = ("reversed", "contracted", "f32")
DB_ROUNDING_MIN = 8        # cases per mutant a recipe must hold


def _db_labels(adj, ms):
    """Labels of sklearn's DBSCAN from the neighbour relation (itself included): clusters numbered by their first core point in index
    order, a border point takes the smallest number among the clusters whose core points reach it.  -> (labels, clusters, core)."""
    n = len(adj)
    core = adj.sum(axis=1) >= ms
    lab = np.full(n, -1, dtype=np.int64)
    cadj = adj & core[None, :]
    ncl = 0
    for i in range(n):
        if not core[i] or lab[i] >= 0:
            continue
        lab[i] = ncl
        stack = [i]
        while stack:
            j = stack.pop()
            nb = np.flatnonzero(cadj[j] & (lab < 0))
            lab[nb] = ncl
            stack.extend(nb.tolist())
        ncl += 1
    if n:
        big = np.iinfo(np.int64).max
        cand = np.where(cadj, lab[None, :], big).min(axis=1)
        border = ~core & (cand < big)
        lab[border] = cand[border]
    return lab, ncl, core


def db_int_dbscan(V, m2, ms):
    """Brute-force DBSCAN of the integer points V (N, d): neighbours <=> |dV|^2 <= m2, in int64."""
    V = np.asarray(V, dtype=np.int64).reshape(len(V), -1)
    V = V - V.min(axis=0) if len(V) else V
    sq = (V * V).sum(axis=1)
    d2 = sq[:, None] + sq[None, :] - 2 * (V @ V.T)
    return _db_labels(d2 <= m2, ms)


def db_f64_d2(X, variant="spec"):
    """Squared distances of all pairs of the float32 points X (N, 3) as the kernel's predicate adds them up - ((dx dx) + dy dy) + dz dz
    in double - or as a mutant does: "reversed" (dz first), "contracted" (the chain fused: fma(dz, dz, fma(dy, dy, dx dx))), "f32"."""
    X = np.asarray(X, dtype=np.float32)
    if variant == "f32":
        d = [X[:, None, a] - X[None, :, a] for a in range(3)]
        return ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(np.float64)
    Y = X.astype(np.float64)
    d = [Y[:, None, a] - Y[None, :, a] for a in range(3)]
    if variant == "spec":
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    if variant == "reversed":
        return (d[2] * d[2] + d[1] * d[1]) + d[0] * d[0]
    if variant == "contracted":
        return _fma(d[2], d[2], _fma(d[1], d[1], d[0] * d[0]))
    raise ValueError(variant)


def _fma(a, b, c):
    """fma(a, b, c) in double, exactly rounded, through rationals (small arrays only: the rounding sets hold four points)."""
    from fractions import Fraction
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.empty(a.shape, dtype=np.float64)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def db_f64_dbscan(X, eps, ms, variant="spec"):
    """The float64 restatement of the kernel's DBSCAN (and, by `variant`, of a mutant's)."""
    return _db_labels(db_f64_d2(X, variant) <= float(eps) * float(eps), ms)


def db_cells(X, eps):
    """Cell of every point, cells per axis and `hashed`, as k_db_setup and db_cell_coords do: floor((x - min) / (0.577 eps)) on the
    float32 bounds, in double; hashed when some axis has more than 128 cells."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    lo, h = X64.min(axis=0), float(eps) * DB_CELL
    dims = np.floor((X64.max(axis=0) - lo) / h) + 1.0
    c = np.clip(np.floor((X64 - lo) / h), 0.0, dims - 1.0).astype(np.int64)
    return c, dims.astype(np.int64), bool((dims > DB_MAXDIM).any())


def db_classes(X, eps, i):
    """The occupied cells as point i's core test and border pass see them: {cell offset: dict(pop, cls, on_min, on_max, single)}, cls
    "own", "within" (the tight box's far corner is within eps: counted without a distance), "cut" (exact tests), "beyond" (the near
    corner is beyond eps) or "far" (outside the 5 x 5 x 5 walk); on_min / on_max: the near / far corner lies exactly on eps."""
    c, _, _ = db_cells(X, eps)
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    r2 = float(eps) * float(eps)
    keys, inv = np.unique(c, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    p, out = X64[i], {}
    for ci, key in enumerate(keys):
        pts = X64[inv == ci]
        off = tuple(int(v) for v in key - c[i])
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        gmax = np.maximum(p - lo, hi - p)
        gmin = np.maximum(np.maximum(lo - p, p - hi), 0.0)
        mind2 = (gmin[0] * gmin[0] + gmin[1] * gmin[1]) + gmin[2] * gmin[2]
        maxd2 = (gmax[0] * gmax[0] + gmax[1] * gmax[1]) + gmax[2] * gmax[2]
        if off == (0, 0, 0):
            cls = "own"
        elif max(abs(v) for v in off) > 2:
            cls = "far"
        else:
            cls = "within" if maxd2 <= r2 else ("cut" if mind2 <= r2 else "beyond")
        out[off] = dict(pop=len(pts), cls=cls, on_min=bool(mind2 == r2), on_max=bool(maxd2 == r2), single=bool((lo == hi).all()))
    return out


def _db_case(name, sites, m, k, off, ms, seed, anchor, markers=False, fifth=False, first=None, dist=3):
    """A lattice case from `sites` {local integer site: multiplicity} (coincident particles, which resampling produces): the point
    `anchor`, at least 3 m below every site on every axis, is the grid's origin (it places the lattice on the cell grid); markers: a far point that
    gives the x axis more than 128 cells (the hashed table); fifth: far padding points, each alone in its cell, bring n // 5 onto ms
    (ms None: n // 5 as it falls); first: a local site whose copy is moved to index 0 of the shuffled order."""
    sites = {tuple(int(x) for x in s): int(c) for s, c in sites.items() if c > 0}
    pts = np.array([s for s, c in sites.items() for _ in range(c)], dtype=np.int64).reshape(-1, 3)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    a = np.asarray(anchor, dtype=np.int64)
    assert (a <= lo - dist * m).all(), (name, a, lo)
    extra = [a]
    side = int(np.ceil(DB_CELL * m))
    if markers:
        extra.append(np.array([a[0] + (DB_MAXDIM + 2) * side, a[1], a[2]]))
    n = len(pts) + len(extra)
    if fifth and ms is not None:
        assert n <= 5 * ms + 4, (name, n, ms)
        npad = max(5 * ms - n, 0)
        step, per = m + 1, 8   # more than eps apart: never neighbours, never cell-mates
        j = np.arange(npad)
        pad = np.stack([hi[0] + dist * m + step * (j // (per * per)), a[1] + step * (j // per % per), a[2] + step * (j % per)], axis=1)
        extra += list(pad)
    V = np.concatenate([pts, np.array(extra, dtype=np.int64).reshape(-1, 3)]) + np.asarray(off, dtype=np.int64)
    n = len(V)
    order = np.random.default_rng([17, seed]).permutation(n)
    if first is not None:
        f = int(np.flatnonzero((pts == np.asarray(first)).all(axis=1))[0])
        at = int(np.flatnonzero(order == f)[0])
        order[[0, at]] = order[[at, 0]]
    V = V[order]
    assert np.abs(V).max() < (1 << 24)
    X = (V.astype(np.float64) * 2.0 ** -k).astype(np.float32)
    assert np.array_equal(X.astype(np.float64) * 2.0 ** k, V)  # exact float32 values
    ms = n // 5 if ms is None else int(ms)
    if fifth:
        assert n // 5 == ms, (name, n, ms)
    eps = m * 2.0 ** -k
    lab, ncl, core = db_int_dbscan(V, m * m, ms)
    local = V - np.asarray(off, dtype=np.int64)
    c = dict(name=name, V=V, local=local, k=int(k), m=int(m), off=tuple(int(x) for x in off), ms=ms, eps=eps, X=X, labels=lab, ncl=ncl,
             core=core, fifth=bool(fifth), hashed=db_cells(X, eps)[2])
    assert c["hashed"] == bool(markers) or fifth, (name, db_cells(X, eps)[1])
    return c


def _db_site_index(c, site):
    return np.flatnonzero((c["local"] == np.asarray(site, dtype=np.int64)).all(axis=1))


def _db_cube(m, R):
    g = np.arange(-R, R + 1)
    S = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return S, (S * S).sum(axis=1)


def db_probe(m, k, off, r, pops, delta=0, markers=False, fifth=False, seed=0, own=1, cut_pops=None):
    """One site p (the local origin, `own` copies) and neighbours placed by class, so that p's neighbour count c is known: with
    min_samples = c + delta the core set is p's site alone (delta 0: every neighbour is a border point of cluster 0, the decoys are noise)
    or empty (delta 1: everything is noise) - any dropped or extra candidate flips the whole set.  Around p:
      corner   a point exactly on eps that is its cell's nearest corner to p, its cell-mate beyond eps (mind2 == r2 < maxd2): two cells
      cut      per entry P of `pops` a cell of P - 1 copies of a site within eps and one site beyond it (at m^2 + 1 where the cell has one)
      within   per entry P of `pops` a cell of P copies of one site well within eps
      decoy    sites at m^2 + 1, alone in their cells
      on       antipodal pairs exactly on eps, each alone in its cell (the box is the point: maxd2 == r2) - one pair more than there
               are points beyond eps, so that no site but p sees as many points as p does (no site is within eps of both v and -v).
    cut_pops: the cut cells' populations where they differ from `pops`; (): the two corner cells are then the only cells the upper bound
    of p's count can take its last points from - read as "beyond", p is dropped before any distance is looked at."""
    m2, hl = m * m, DB_CELL * m
    cutp = tuple(pops if cut_pops is None else cut_pops)
    a = 3 * m + (m + 2) + np.asarray(r, dtype=np.int64)        # the anchor lies this far below p: _db_case's, the cube reaches m + 2 down
    S, d2 = _db_cube(m, m + 2)
    cell = np.floor((S + a) / hl).astype(np.int64)
    cid = {}
    for i, key in enumerate(map(tuple, cell)):
        cid.setdefault(key, []).append(i)
    own_cell = tuple(np.floor(a / hl).astype(np.int64))
    used, sites, plan = {own_cell}, {(0, 0, 0): own}, {}
    outside = 0

    def take(key):
        used.add(key)

    # corner: v on eps, w = v one step further out on one axis, same cell
    corners = 0
    for i in np.flatnonzero(d2 == m2):
        key = tuple(cell[i])
        if key in used or corners == 2:
            continue
        v = S[i]
        best = None
        for ax in range(3):
            w = v.copy()
            w[ax] += 1 if v[ax] >= 0 else -1
            if (np.abs(w) <= m + 2).all() and tuple(np.floor((w + a) / hl).astype(np.int64)) == key:
                dw = int((w * w).sum())
                if best is None or dw < best[0]:
                    best = (dw, w)
        if best is None:
            continue
        sites[tuple(v)] = 1
        sites[tuple(best[1])] = 1
        plan[tuple(int(x) - int(y) for x, y in zip(key, own_cell))] = "corner"
        outside += 1
        corners += 1
        take(key)
    # cut cells, the farthest-reaching first (their box is cut whatever the alignment)
    cells = sorted((key for key in cid if key not in used), key=lambda key: -max(d2[i] for i in cid[key] if d2[i] <= m2) if any(d2[i] <= m2 for i in cid[key]) else 0)
    todo = list(cutp)
    for key in cells:
        if not todo:
            break
        idx = cid[key]
        ins = [i for i in idx if 0 < d2[i] < m2]
        outs = [i for i in idx if d2[i] > m2]
        if not ins or not outs or key in used:
            continue
        u = max(ins, key=lambda i: d2[i])
        w = min(outs, key=lambda i: d2[i])
        P = todo.pop(0)
        if P > 1:
            sites[tuple(S[u])] = P - 1
            sites[tuple(S[w])] = 1
            outside += 1
            plan[tuple(int(x) - int(y) for x, y in zip(key, own_cell))] = "cut"
        else:
            sites[tuple(S[u])] = 1   # a population of one: the box is the point
            plan[tuple(int(x) - int(y) for x, y in zip(key, own_cell))] = "within"
        take(key)
    assert not todo, ("cut cells", m, r)
    # within cells, the nearest first
    todo = list(pops)
    for key in sorted((key for key in cid if key not in used), key=lambda key: min(d2[i] for i in cid[key])):
        if not todo:
            break
        u = min(cid[key], key=lambda i: d2[i])
        if not 0 < d2[u] < m2:
            continue
        sites[tuple(S[u])] = todo.pop(0)
        plan[tuple(int(x) - int(y) for x, y in zip(key, own_cell))] = "within"
        take(key)
    assert not todo, ("within cells", m, r)
    # decoys at m^2 + 1, alone
    decoys = 0
    for i in np.flatnonzero(d2 == m2 + 1):
        key = tuple(cell[i])
        if key in used or decoys == 3:
            continue
        sites[tuple(S[i])] = 1
        plan[tuple(int(x) - int(y) for x, y in zip(key, own_cell))] = "decoy"
        outside += 1
        decoys += 1
        take(key)
    assert decoys >= 1
    # antipodal pairs on eps, alone
    pairs = 0
    for i in np.flatnonzero(d2 == m2):
        v = S[i]
        if tuple(v) < tuple(-v) or pairs == max(outside + 1, 3):
            continue
        k1, k2 = tuple(cell[i]), tuple(np.floor((-v + a) / hl).astype(np.int64))
        if k1 in used or k2 in used or k1 == k2:
            continue
        sites[tuple(v)] = 1
        sites[tuple(-v)] = 1
        for key in (k1, k2):
            plan[tuple(int(x) - int(y) for x, y in zip(key, own_cell))] = "on"
            take(key)
        pairs += 1
    assert pairs >= 3, ("antipodal pairs", pairs, outside)   # (fewer than outside + 1 may do: the conditions below are what counts)
    cnt = sum(n for s, n in sites.items() if sum(x * x for x in s) <= m2)
    name = f"probe/m{m}/r{'.'.join(map(str, r))}/off{'.'.join(map(str, off))}/{'hashed' if markers else 'dense'}/{'fifth' if fifth else 'ms'}/own{own}/pops{len(pops)}{'' if cut_pops is None else 'cut' + str(len(cutp))}/c{'+1' if delta else ''}"
    c = _db_case(name, sites, m, k, off, cnt + delta, seed, -a, markers=markers, fifth=fifth)
    # --- the conditions, on the case as built
    ip = _db_site_index(c, (0, 0, 0))
    assert len(ip) == own
    loc2 = (c["local"] * c["local"]).sum(axis=1)
    near = loc2 <= m2
    assert int(near.sum()) == cnt
    if delta == 0:
        assert np.array_equal(np.flatnonzero(c["core"]), ip), name          # the core set is exactly p's site
        assert c["ncl"] == 1 and (c["labels"][near] == 0).all() and (c["labels"][~near] == -1).all(), name
    else:
        assert not c["core"].any() and c["ncl"] == 0 and (c["labels"] == -1).all(), name
    cls = db_classes(c["X"], c["eps"], int(ip[0]))
    seen = {}
    for offc, what in plan.items():
        got = cls[offc]
        if what == "corner":
            assert got["cls"] == "cut" and got["on_min"] and not got["on_max"] and got["pop"] == 2, (name, offc, got)
        elif what == "cut":
            assert got["cls"] == "cut" and not got["on_min"], (name, offc, got)
        elif what == "within":
            assert got["cls"] == "within" and got["single"] and not got["on_max"], (name, offc, got)
        elif what == "decoy":
            assert got["cls"] == "beyond" and got["pop"] == 1, (name, offc, got)
        elif what == "on":
            assert got["cls"] == "within" and got["single"] and got["on_max"] and got["pop"] == 1, (name, offc, got)
        seen[what] = seen.get(what, 0) + 1
    assert cls[(0, 0, 0)]["cls"] == "own" and cls[(0, 0, 0)]["pop"] == own
    assert seen["corner"] == 2 and seen.get("cut", 0) + seen["within"] == len(pops) + len(cutp) and seen["on"] == 2 * pairs
    assert sorted(v["pop"] for o, v in cls.items() if plan.get(o) in ("cut", "within")) == sorted(list(pops) + list(cutp)), name
    if not cutp and delta == 0:   # the upper bound of p's count without the corner cells falls short of min_samples
        assert cnt - 2 < c["ms"] == cnt and sum(v["pop"] for v in cls.values() if v["cls"] in ("own", "within", "cut")) == cnt + 2, name
    c.update(p=int(ip[0]), count=cnt, plan=plan, classes=seen)
    return c


def db_own_cell(m, k, off, r, short, markers=False, seed=0, ms=64):
    """p's own cell decides: short 0 - the cell holds min_samples points exactly (core by population, no distance at all), decoys at
    m^2 + 1 around it; short 1 - the cell holds p (ms - 2 copies) and a second site p' (one copy), one short of min_samples, and the
    missing neighbour is one point exactly on eps of p, alone in its cell and beyond eps of p'.  The core set is p's site; with
    min_samples one higher it is empty."""
    m2, hl = m * m, DB_CELL * m
    out = []
    for rx in range(int(np.ceil(hl)) + 1):   # the alignment on x that puts p and p' into one cell
        ax = -(4 * m + 2 + r[0] + rx)
        if np.floor((0 - ax) / hl) == np.floor((1 - ax) / hl):
            break
    anchor = (ax, -(4 * m + 2 + r[1]), -(4 * m + 2 + r[2]))
    for delta in (0, 1):
        sites = {}
        S, d2 = _db_cube(m, m + 2)
        far = lambda s, o: sum((x - y) ** 2 for x, y in zip(s, o)) > m2  # noqa: E731
        dec = [tuple(S[i]) for i in np.flatnonzero(d2 == m2 + 1)]
        dec = [s for s in dec if far(s, (1, 0, 0)) and far(s, (-m, 0, 0))]      # decoys of p that no other site counts
        for s in dec[::max(len(dec) // 4, 1)][:4]:
            sites[s] = 1
        if short:
            sites[(0, 0, 0)] = ms - 2
            sites[(1, 0, 0)] = 1
            sites[(-m, 0, 0)] = 1
        else:
            sites[(0, 0, 0)] = ms
        name = f"own/m{m}/r{'.'.join(map(str, r))}/{'hashed' if markers else 'dense'}/short{short}/c{'+1' if delta else ''}"
        c = _db_case(name, sites, m, k, off, ms + delta, seed, anchor, markers=markers)
        ip = _db_site_index(c, (0, 0, 0))
        cls = db_classes(c["X"], c["eps"], int(ip[0]))
        assert cls[(0, 0, 0)]["pop"] == ms - short, (name, cls[(0, 0, 0)])
        if delta == 0:
            assert np.array_equal(np.flatnonzero(c["core"]), ip) and c["ncl"] == 1, name
        else:
            assert not c["core"].any(), name
        if short:
            on = [v for o, v in cls.items() if v["on_max"] and v["single"] and v["pop"] == 1]
            assert len(on) == 1, name
        c.update(p=int(ip[0]), count=ms)
        out.append(c)
    return out


def _db_plus_vector(m):
    """An integer vector of squared length m^2 + 1 whose first component is m (the next lattice point beside (m, 0, 0))."""
    return (m, 1, 0)


def db_bridge(m, k, off, r, on, kind, seed, markers=False, fifth=False, second_first=True):
    """Two blocks of core points joined by exactly one pair, a - b: exactly on eps (one cluster) or at m^2 + 1 (two).  kind "box": a
    and b are single-site cells of min_samples copies (the cells' boxes decide the link); "cut": the cell of a holds 65 copies of a and
    65 of a site one step further from b, the cell of b likewise (the link is found by the exact scan, a point against the other cell's
    core points); "one": a and b are single particles among 130 of their cells.  second_first: index 0 is a point of b's block, so the
    geometrically first block is not cluster 0."""
    # the cell-mates lie diagonally (a2 one step further in x and one up in y, b2 likewise on the other side): the two cells' boxes are
    # exactly eps apart in BOTH forms - the boxes never decide, the exact scan does - and a - b is the only pair that can be within eps
    b = (m, 0, 0) if on else _db_plus_vector(m)
    a2, b2 = (-1, 1, 0), (m + 1, 1 - b[1], 0)
    pop = {"box": None, "cut": (65, 65), "one": (1, 129)}[kind]
    ms = 5 if kind == "box" else 100
    hl = DB_CELL * m
    side = int(np.ceil(hl))
    for rx in range(side + 1):      # the alignment on x that puts a with a2, b with b2 and the two pairs apart; on y, 0 with 1
        lo = -1 - (3 * m + rx)
        cx = lambda x: int(np.floor((x - lo) / hl))  # noqa: E731
        if kind == "box" or (cx(0) == cx(-1) and cx(m) == cx(m + 1) and cx(0) != cx(m)):
            break
    else:
        raise AssertionError(("bridge alignment", m))
    for ry in range(side + 1):
        loy = -(3 * m + r[1] + ry)
        if np.floor((0 - loy) / hl) == np.floor((1 - loy) / hl):
            break
    if kind == "box":
        sites = {(0, 0, 0): ms, b: ms}
    else:
        sites = {(0, 0, 0): pop[0], a2: pop[1], b: pop[0], b2: pop[1]}
    name = f"bridge/m{m}/{kind}/{'on' if on else 'plus'}/r{rx}.{r[1]}.{r[2]}/{'hashed' if markers else 'dense'}/{'fifth' if fifth else 'ms'}/s{seed}"
    c = _db_case(name, sites, m, k, off, None if fifth else ms, seed, (lo, loy, -(3 * m + r[2])), markers=markers, fifth=fifth,
                 first=(b if second_first else (0, 0, 0)))
    ia, ib = _db_site_index(c, (0, 0, 0)), _db_site_index(c, b)
    d = c["local"][ia[0]] - c["local"][ib[0]]
    assert int((d * d).sum()) == m * m + (0 if on else 1)
    yz = (c["local"][:, 1] >= 0) & (c["local"][:, 1] <= 1) & (c["local"][:, 2] == 0)
    blockA = (c["local"][:, 0] <= 0) & (c["local"][:, 0] >= -1) & yz
    blockB = (c["local"][:, 0] >= m) & (c["local"][:, 0] <= m + 1) & yz
    assert c["core"][blockA | blockB].all() and int((blockA | blockB).sum()) == sum(sites.values()), name
    assert c["ncl"] == (1 if on else 2), name
    if not on:
        first_block = blockB if second_first else blockA
        assert (c["labels"][first_block] == 0).all() and (c["labels"][(blockA | blockB) & ~first_block] == 1).all(), name
    else:
        assert (c["labels"][blockA | blockB] == 0).all(), name
    # the pairs of the two blocks within eps: the bridge alone
    A, B = c["local"][blockA], c["local"][blockB]
    dd = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
    assert int((dd <= m * m).sum()) == (len(ia) * len(ib) if on else 0), name
    cells, _, _ = db_cells(c["X"], c["eps"])
    ca, cb = cells[ia[0]], cells[ib[0]]
    assert not np.array_equal(ca, cb)
    if kind != "box":
        assert (cells[blockA] == ca).all() and (cells[blockB] == cb).all(), name   # 130 points a cell
        cls = db_classes(c["X"], c["eps"], int(ia[0]))[tuple(int(v) for v in cb - ca)]
        assert cls["cls"] == "cut" and cls["on_min"] and cls["pop"] == 130, (name, cls)
    else:
        cls = db_classes(c["X"], c["eps"], int(ia[0]))[tuple(int(v) for v in cb - ca)]
        assert cls["single"] and cls["on_max"] == bool(on) and cls["cls"] == ("within" if on else "beyond"), (name, cls)
    return c


def db_border(m, k, off, r, mode, apop, seed, markers=False, fifth=False):
    """A non-core point x (the local origin).  Cluster 0 reaches it through ONE core point a exactly on eps (mode "on": label 0), or a
    lies at m^2 + 1 ("plus": label 1, x lies well inside cluster 1, whose core point b shares x's cell and is x's only neighbour of
    that cluster), or neither reaches it ("none": b is taken away as well, label -1).  apop 1: a is alone in its cell (the box decides);
    apop P > 1: a is one particle among P of its cell, the others one step beyond eps of x (the exact scan, 64 candidates at a time)."""
    ms = max(5, -(-(apop + 4 + int(markers)) // 4)) if fifth else 5     # fifth: n // 5 == ms is within the padding's reach
    a = (-m, 0, 0) if mode == "on" else tuple(-v for v in _db_plus_vector(m))
    sites = {(0, 0, 0): 1, a: 1}
    if apop > 1:
        sites[(a[0] - 1, a[1], a[2])] = apop - 1      # the cell-mates of a: core by their cell's population
    else:
        sites[(a[0] - 5 if m >= 5 else a[0] - m, a[1], a[2])] = ms   # what makes a a core point: within eps of a, beyond eps of x
    if mode != "none":
        sites[(1, 0, 0)] = 1                           # b, in x's cell
    sites[(1 + m, 0, 0)] = ms                          # b': exactly on eps of b, beyond eps of x
    hl = DB_CELL * m
    for rx in range(int(np.ceil(hl)) + 1):
        lo = min(s[0] for s in sites) - (3 * m + rx)
        cx = lambda x: int(np.floor((x - lo) / hl))  # noqa: E731
        if cx(0) == cx(1) and (apop == 1 or cx(a[0]) == cx(a[0] - 1)) and (apop > 1 or cx(a[0]) != cx(a[0] - 5 if m >= 5 else a[0] - m)):
            break
    else:
        raise AssertionError(("border alignment", m))
    name = f"border/m{m}/{mode}/apop{apop}/r{rx}.{r[1]}.{r[2]}/{'hashed' if markers else 'dense'}/{'fifth' if fifth else 'ms'}/s{seed}"
    first = (a[0] - 1, a[1], a[2]) if apop > 1 else (a[0] - 5 if m >= 5 else a[0] - m, a[1], a[2])   # cluster 0 is a's
    c = _db_case(name, sites, m, k, off, ms, seed, (lo, -(3 * m + 1 + r[1]), -(3 * m + r[2])), markers=markers, fifth=fifth, first=first)
    ix, ia = int(_db_site_index(c, (0, 0, 0))[0]), int(_db_site_index(c, a)[0])
    assert not c["core"][ix] and c["core"][ia] and c["labels"][ia] == 0, name
    want = {"on": 0, "plus": 1, "none": -1}[mode]
    assert c["labels"][ix] == want, (name, c["labels"][ix])
    assert c["ncl"] == 2, name
    cells, _, _ = db_cells(c["X"], c["eps"])
    cls = db_classes(c["X"], c["eps"], ix)
    ca = cls[tuple(int(v) for v in cells[ia] - cells[ix])]
    if mode == "on":
        assert ca["on_max" if apop == 1 else "on_min"] and ca["pop"] == apop and ca["cls"] == ("within" if apop == 1 else "cut"), (name, ca)
    else:
        assert ca["cls"] == "beyond" and ca["pop"] == apop, (name, ca)
    if mode != "none":
        ibb = int(_db_site_index(c, (1, 0, 0))[0])
        assert np.array_equal(cells[ibb], cells[ix]) and c["core"][ibb] and c["labels"][ibb] == 1 and cls[(0, 0, 0)]["pop"] == 2, name
        # b is x's only neighbour of cluster 1
        d2 = ((c["local"] - c["local"][ix]) ** 2).sum(axis=1)
        assert int(((d2 <= m * m) & c["core"] & (c["labels"] == 1)).sum()) == 1, name
    c.update(x=ix, want=want)
    return c


def db_corner(m, k, off, want, seed=0, markers=False):
    """Two points whose cells are two apart on every axis of `want` (a tuple of 0 / 2 per axis) and yet within eps: sqrt(3) 0.577 < 1
    leaves a sliver.  The recipe searches the alignment.  p, q = p + d and a cell-mate q' of q beyond eps of p (q's cell is cut: p's
    count needs the exact scan of a cell at the rim of the 5 x 5 x 5 walk), and a decoy at m^2 + 1 of p beside q.  Two cases: min_samples
    2 (p is a core point only through q) and 3 (p is a border point only through q)."""
    m2, hl = m * m, DB_CELL * m
    d, dplus = {(2, 2, 2): ((56, 56, 56), (55, 57, 56)), (2, 2, 0): ((72, 65, 0), (72, 65, 1)), (2, 0, 0): ((97, 0, 0), (97, 1, 0))}[tuple(want)]
    assert m == 97 and sum(x * x for x in d) in (m2, m2 - 1) and sum(x * x for x in dplus) == m2 + 1
    t = []
    for ax in range(3):       # p lies t cells-and-a-bit above the anchor: the smallest t that gives the wanted offsets
        for cand in range(3 * m, 3 * m + 40 * int(hl)):
            cp, cq, cq1 = (int(np.floor(v / hl)) for v in (cand, cand + d[ax], cand + d[ax] + (1 if ax == 0 else 0)))
            if cq - cp == want[ax] and cq1 == cq:
                t.append(cand)
                break
        else:
            raise AssertionError(("corner alignment", want, ax))
    q1 = (d[0] + 1, d[1], d[2])
    out = []
    for ms in (2, 3):
        name = f"corner/{'.'.join(map(str, want))}/{'hashed' if markers else 'dense'}/ms{ms}"
        sites = {(0, 0, 0): 1, d: 1, q1: 1, dplus: 1}
        c = _db_case(name, sites, m, k, off, ms, seed, tuple(-v for v in t), markers=markers)
        ip, iq = int(_db_site_index(c, (0, 0, 0))[0]), int(_db_site_index(c, d)[0])
        cells, _, _ = db_cells(c["X"], c["eps"])
        assert tuple(int(v) for v in cells[iq] - cells[ip]) == tuple(want), (name, cells[iq] - cells[ip])
        cls = db_classes(c["X"], c["eps"], ip)[tuple(want)]
        assert cls["cls"] == "cut" and cls["pop"] >= 2, (name, cls)
        assert c["core"][iq] and c["labels"][ip] == 0 and c["ncl"] == 1, name
        assert bool(c["core"][ip]) == (ms == 2), name
        # without q, p is noise
        keep = np.arange(len(c["V"])) != iq
        lab = db_int_dbscan(c["V"][keep], m2, ms)[0]
        assert lab[np.flatnonzero(keep) == ip][0] == -1, name
        c.update(p=ip)
        out.append(c)
    return out


def db_rounding_cases(mutant, seed=0, trials=6000):
    """The float64 predicate's rounding, a separate edge: pairs p, q whose differences carry more than 26 significant bits (p with
    components of magnitude 2^-30 .. 2^-12, q about eps away along unequal axes - and, for the float32 mutant, also pairs at |x| about
    0.3), and an eps with fl(eps eps) between the spec's sum ((dx dx) + dy dy) + dz dz and the mutant's.  Each pair is the bridge of a
    four-point set: p with a cell-mate 0.3 eps behind it, q with one 0.3 eps beyond it, min_samples 2 - every point is a core point by
    its cell's population, the two cells' boxes are cut and the pair p - q alone decides between one cluster and two.
    -> DB_ROUNDING_MIN cases on which the spec says "within" and the mutant does not, and as many the other way round."""
    rng = np.random.default_rng([23, seed, DB_ROUNDING_MUTANTS.index(mutant)])
    got = {True: [], False: []}
    for trial in range(trials):
        if all(len(v) >= DB_ROUNDING_MIN for v in got.values()):
            break
        eps0 = 1e-2 * rng.uniform(0.5, 1.5)
        if mutant == "f32" and trial % 2:
            p = rng.uniform(-0.3, 0.3, 3)
        else:
            p = rng.choice([-1.0, 1.0], 3) * np.ldexp(rng.uniform(1.0, 2.0, 3), -rng.integers(12, 31, 3))
        u = rng.uniform(0.2, 1.0, 3)
        u /= np.linalg.norm(u)
        X = np.stack([p, p - 0.3 * eps0 * u, p + eps0 * u, p + 1.3 * eps0 * u]).astype(np.float32)
        s, t = db_f64_d2(X[[0, 2]], "spec")[0, 1], db_f64_d2(X[[0, 2]], mutant)[0, 1]
        if s == t:
            continue
        lo, hi = min(s, t), max(s, t)
        eps = np.sqrt(lo)
        for _ in range(4):            # fl(eps eps) into [lo, hi)
            if eps * eps < lo:
                eps = np.nextafter(eps, np.inf)
        if not lo <= eps * eps < hi:
            continue
        within = bool(s <= eps * eps)
        if len(got[within]) >= DB_ROUNDING_MIN:
            continue
        cells, _, _ = db_cells(X, eps)
        if not (np.array_equal(cells[0], cells[1]) and np.array_equal(cells[2], cells[3]) and not np.array_equal(cells[0], cells[2])):
            continue
        lab, ncl, core = db_f64_dbscan(X, eps, 2)
        labm, nclm, _ = db_f64_dbscan(X, eps, 2, mutant)
        assert core.all() and ncl == (1 if within else 2) and nclm == (2 if within else 1), (mutant, trial)
        for v in DB_ROUNDING_MUTANTS + ("spec",):   # the other three cross pairs are far from the edge in every arithmetic
            d = db_f64_d2(X, v)
            assert min(d[0, 3], d[1, 2], d[1, 3]) > 1.5 * eps * eps
        cls = db_classes(X, eps, 0)[tuple(int(v) for v in cells[2] - cells[0])]
        assert cls["cls"] == ("cut" if within else "beyond") and cls["pop"] == 2
        got[within].append(dict(name=f"rounding/{mutant}/{'within' if within else 'beyond'}/{len(got[within])}", X=X, eps=float(eps), ms=2,
                                labels=lab, ncl=ncl, mutant=mutant, mutant_labels=labm, within=within, fifth=False, hashed=False))
    assert all(len(v) >= DB_ROUNDING_MIN for v in got.values()), (mutant, {k: len(v) for k, v in got.items()})
    return got[True] + got[False]


def db_rounding_separations(n=1000, seed=0):
    """Of n near-origin pairs, on how many does an eps exist that separates the spec's sum from each mutant's (the sums differ)."""
    rng = np.random.default_rng([29, seed])
    count = {v: 0 for v in DB_ROUNDING_MUTANTS}
    for _ in range(n):
        p = rng.choice([-1.0, 1.0], 3) * np.ldexp(rng.uniform(1.0, 2.0, 3), -rng.integers(12, 31, 3))
        u = rng.uniform(0.2, 1.0, 3)
        X = np.stack([p, p + 1e-2 * u / np.linalg.norm(u)]).astype(np.float32)
        s = db_f64_d2(X, "spec")[0, 1]
        for v in DB_ROUNDING_MUTANTS:
            count[v] += int(db_f64_d2(X, v)[0, 1] != s)
    return count


DB_TINY_SITES = ((0, 0, 0), (7, 0, 0), (14, 1, 0), (0, 0, 0), (300, 0, 0), (14, 8, 0), (-2, -3, -6), (300, 7, 0), (21, 1, 0))


def db_tiny_cases(m=7, k=10, off=(768, -300, 5000)):
    """n = 1 .. 9 points under min_samples = n // 5, which is 0 or 1: every point is a core point, the clusters are the components of
    "within eps" (on-eps links, a pair at m^2 + 1, a coincident pair).  n < 5 is out of spec: sklearn refuses min_samples = 0."""
    out = []
    for n in range(1, 10):
        V = np.array(DB_TINY_SITES[:n], dtype=np.int64) + np.asarray(off, dtype=np.int64)
        X = (V * 2.0 ** -k).astype(np.float32)
        lab, ncl, core = db_int_dbscan(V, m * m, n // 5)
        lab1, ncl1, _ = db_int_dbscan(V, m * m, 1)
        assert core.all() and np.array_equal(lab, lab1) and ncl == ncl1
        out.append(dict(name=f"tiny/n{n}", V=V, local=V - np.asarray(off), k=k, m=m, off=tuple(off), ms=n // 5, eps=m * 2.0 ** -k, X=X, labels=lab,
                        ncl=ncl, core=core, fifth=True, hashed=db_cells(X, m * 2.0 ** -k)[2]))
    assert out[8]["ncl"] == 3 and out[8]["labels"].tolist() == [0, 0, 1, 0, 2, 1, 0, 2, 1]
    return out


DB_POINTS_SIZES = (255, 256, 257, 513)


def db_points_case(dim, N, m=7, k=10, seed=0):
    """A float64 lattice in `dim` dimensions for the all-pairs kernel (midas_dbscan_points; the 256-column tile and its NaN padding at
    N = 255, 256, 257, 513).  Copies M = 4 a site, min_samples = 2 M:
      chain 1   12 sites along axis 0, exactly eps apart: an end site has 2 M neighbours (== min_samples, M of them on eps), and the
                smallest index is a copy of the far end - the cluster's number has to travel the whole chain (more than one spread step)
      chain 2   3 sites, the first at m^2 + 1 of chain 1's last site: a second cluster
      border    single points exactly on eps of one chain-1 site, along axis 1 and along the last axis: label 0; a decoy at m^2 + 1: noise
      filler    far single points, noise
    Copies of chain 1's end sites stand at the indices 255, 256 and N - 1.  dim != 3: the lattice lies at 2^33 + 5, beyond float32."""
    M, L = 4, 12
    e = lambda ax, v=1: tuple(v if i == ax else 0 for i in range(dim))  # noqa: E731
    add = lambda *vs: tuple(int(sum(x)) for x in zip(*vs))  # noqa: E731
    pts = []
    for j in range(L):
        pts += [e(0, j * m)] * M
    plus = add(e(0, m), e(1, 1))
    c2 = add(e(0, (L - 1) * m), plus)
    for j in range(3):
        pts += [add(c2, e(0, j * m))] * M
    pts += [add(e(0, 5 * m), e(1, m)), add(e(0, 3 * m), e(dim - 1, -m)), add(e(0, 7 * m), e(dim - 1, m), e(0 if dim == 2 else dim - 2, 1))]
    nfill = N - len(pts)
    assert nfill > 0
    pts += [add(e(0, 100 * m + 3 * m * j), e(1, -50 * m)) for j in range(nfill)]
    V = np.array(pts, dtype=np.int64)
    order = np.random.default_rng([31, dim, N, seed]).permutation(N)
    pos = {int(v): i for i, v in enumerate(order)}

    def put(at, src):  # the point `src` of the list goes to index `at`
        i = pos[src]
        o = int(order[at])
        order[at], order[i] = src, o
        pos[src], pos[o] = at, i
    put(0, (L - 1) * M)                     # a copy of chain 1's far end first
    put(N - 1, 0)                           # copies of its near end at N - 1 and around the tile boundary
    for at, src in ((255, 1), (256, 2)):
        if at < N - 1:
            put(at, src)
    V = V[order]
    off = (1 << 33) + 5 if dim != 3 else 768
    V = V + off
    X = V.astype(np.float64) * 2.0 ** -k
    assert np.array_equal(X * 2.0 ** k, V) and (dim == 3) == bool(np.array_equal(X.astype(np.float32).astype(np.float64), X))
    ms = 2 * M
    lab, ncl, core = db_int_dbscan(V, m * m, ms)
    cnt = (((V[:, None, :] - V[None, :, :]) ** 2).sum(axis=2) <= m * m).sum(axis=1)
    assert ncl == 2 and int((cnt == ms).sum()) == 4 * M and int(core.sum()) == (L + 3) * M, (dim, N)
    assert lab[0] == 0 and core[0] and sorted(np.unique(lab).tolist()) == [-1, 0, 1]
    assert int((~core & (lab == 0)).sum()) == 2 and int((lab == -1).sum()) == nfill + 1
    # with `<` for `<=` nothing is a core point
    assert not db_int_dbscan(V, m * m - 1, ms)[2].any()
    return dict(name=f"points/d{dim}/n{N}", V=V, k=k, m=m, ms=ms, eps=m * 2.0 ** -k, X=X, labels=lab, ncl=ncl, core=core, dim=dim)


DB_OFFSETS = ((768, -300, 5000), (-4096, 17, -1), (0, 0, 0))     # lattice offsets, some with negative coordinates
DB_ALIGN = ((0, 0, 0), (1, 2, 3), (3, 1, 2))                      # shifts of the lattice against the cell grid
DB_SMALL_POPS = (1, 63, 64, 65)
_DB_CASES = {}


def db_edge_cases():
    """Every lattice case, the rounding cases and the tiny sets, built once: {name: case}."""
    if _DB_CASES:
        return _DB_CASES
    out = []
    m, k = 7, 10
    for hashed in (False, True):
        for delta in (0, 1):
            out.append(db_probe(m, k, DB_OFFSETS[0], DB_ALIGN[1], DB_POPS, delta, markers=hashed, seed=1))
            out.append(db_probe(9, k, DB_OFFSETS[1], DB_ALIGN[2], DB_POPS, delta, markers=hashed, seed=2))
            for oi, off in enumerate(DB_OFFSETS):
                for ri, r in enumerate(DB_ALIGN):
                    out.append(db_probe(m, k, off, r, DB_SMALL_POPS, delta, markers=hashed, seed=10 * oi + ri, own=1 + 2 * ri))
            for ri in (0, 1):
                out.append(db_probe(m, k, DB_OFFSETS[ri + 1], DB_ALIGN[ri], DB_SMALL_POPS, delta, markers=hashed, seed=20 + ri, own=2, cut_pops=()))
            out.append(db_probe(m, k, DB_OFFSETS[0], DB_ALIGN[0], DB_SMALL_POPS, delta, markers=hashed, fifth=True, seed=5))
            out.append(db_probe(3, 9, DB_OFFSETS[2], DB_ALIGN[0], (1, 63, 64), delta, markers=hashed, fifth=True, seed=6))
        for short in (0, 1):
            for ri, r in enumerate(DB_ALIGN[:2]):
                out += db_own_cell(m, k, DB_OFFSETS[ri], r, short, markers=hashed, seed=ri)
        for on in (True, False):
            for kind in ("box", "cut", "one"):
                for s in range(16 if (kind == "one" and on) else 2):
                    out.append(db_bridge(m, k, DB_OFFSETS[s % 3], DB_ALIGN[s % 3], on, kind, s, markers=hashed, second_first=s % 4 != 3))
                out.append(db_bridge(m, k, DB_OFFSETS[1], DB_ALIGN[1], on, kind, 40, markers=hashed, fifth=True))
        for mode in ("on", "plus", "none"):
            for apop in (1, 65, 130):
                for s in range(2):
                    out.append(db_border(m, k, DB_OFFSETS[(s + apop) % 3], DB_ALIGN[s], mode, apop, s, markers=hashed))
                out.append(db_border(m, k, DB_OFFSETS[0], DB_ALIGN[2], mode, apop, 50, markers=hashed, fifth=True))
        for want in ((2, 2, 2), (2, 2, 0), (2, 0, 0)):
            out += db_corner(97, 13, DB_OFFSETS[0] if not hashed else DB_OFFSETS[1], want, markers=hashed)
    for mutant in DB_ROUNDING_MUTANTS:
        out += db_rounding_cases(mutant)
    out += db_tiny_cases()
    for c in out:
        assert c["name"] not in _DB_CASES, c["name"]
        _DB_CASES[c["name"]] = c
    return _DB_CASES


def db_fixture_cases():
    """The cases fixture G17 holds: those the reference's cluster_particles can be given - min_samples is n // 5 there, and at least 1."""
    return [c for c in db_edge_cases().values() if c["fifth"] and c["ms"] >= 1 and "V" in c]


# ---- the prune at its edges: vertices on the threshold sphere, the edges of the vertex lists ---------------------------------------
# (tools/gen_prune_edges.py writes G18 from these; tests/test_prune_edges_reference.py on the CPU, tests/test_gpu_prune_edges.py on
# the GPU; DESIGN.md, "The prune's rule")
# The rule is invalid = dist_to_nearest_vertex > pen_max in float64 (modules/particle_filter.py:379-403).  The world is an integer
# lattice with unit u = 2^-16 m: every vertex (float64), every codebook entry's and every particle's translation (float32) is an integer
# multiple of u below 2^24 in magnitude, so every value is exact in float32, every squared distance an integer times u^2 in any
# arithmetic, fused or not, in any order, and with thr = m u the predicate is |dV|^2 <= m^2 over int64.  One case = one particle, its
# own codebook entry (identity rotation) and its own vertices in its own region; regions stand PE_SPACING units apart and every point of
# a case lies within PE_REACH units of its region's origin, so no case sees another's vertices or entries (asserted from integers).
PE_K = 16
PE_U = 2.0 ** -PE_K
PE_M = 131                 # thr = 131 u = 1.99890 mm, next to the reference's 0.002
# squared_threshold(131 u) lies one ulp ABOVE (131 u)^2 - as for every m whose significand is below sqrt 2 -, so on that world a vertex
# exactly on the sphere has d2 < t2 and a `<` for the `<=` of a hit test goes unnoticed.  With a significand of sqrt 2 or more
# (113 = 1.77 * 64) t2 == (m u)^2 exactly: on the world of 113 u (1.72424 mm) an on-sphere vertex has d2 == t2 at every stage.
PE_M_STRICT = 113
PE_MS = (PE_M, PE_M_STRICT)
PE_SPACING = 4096          # units between the origins of neighbouring regions
PE_REACH = 600             # a case's entry, particle and vertices lie this close (per axis) to its region's origin
PE_DELTA = 450             # list-depth, tie and tree cases: the particle stands 450 u from its entry
PE_LIST = 256              # records of an entry's vertex list (csrc/midas_internal.hpp MESH_M)
PE_DEPTHS = (1, 8, 9, 16, 17, 32, 33, 80, 81, 144, 145, 256, 257, 300)   # the deciding vertex's rank by distance from the entry
PE_OFF = (37, -21, 12)     # the particle of an "off its entry" case, from the entry
PE_FIELD_DISTS = ("0", "1", "m/4", "m/2", "2m", "4m", "far")
PE_DEGENERATE = (0.0, float("inf"), -1e-3, float("nan"))
PE_D = 128
PE_AXES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def pe_squared_threshold(thr):
    """csrc/midas_internal.hpp squared_threshold restated: the largest float64 t2 with sqrt(t2) <= thr, so that sqrt(d2) > thr <=>
    d2 > t2; -1 for a negative or NaN threshold, +inf for +inf."""
    thr = float(thr)
    if not thr >= 0.0:
        return -1.0
    if np.isinf(thr):
        return float("inf")
    t = thr * thr
    while np.sqrt(t) > thr:
        t = float(np.nextafter(t, 0.0))
    while np.sqrt(np.nextafter(t, np.inf)) <= thr:
        t = float(np.nextafter(t, np.inf))
    return t


def pe_classes(m, off=0):
    """The direction classes (a, b, c), 0 <= a <= b <= c, with a^2 + b^2 + c^2 = m^2 + off, by enumeration."""
    import math
    t, out = m * m + off, []
    for a in range(m + 2):
        for b in range(a, m + 2):
            c2 = t - a * a - b * b
            if c2 < b * b:
                break
            c = math.isqrt(c2)
            if c * c == c2:
                out.append((a, b, c))
    return out


def pe_orbit(v):
    """Every distinct image of v under sign flips and axis permutations, sorted."""
    import itertools
    return sorted({tuple(s * x for s, x in zip(sg, p)) for p in itertools.permutations(v) for sg in itertools.product((1, -1), repeat=3)})


def _pe_case(name, family, m, P, verts, E=(0, 0, 0), decider=None, tie=False, kind=None):
    """A case in its region's own coordinates (integers): the entry E, the particle P, its vertices; `decider` the index of the
    vertex that decides it.  Works out the nearest vertex's squared distance d2 (-1: no vertex of its own), the mask d2 <= m^2, the
    deciding vertex's rank by distance from the entry (1 = the list's first record; asserted unambiguous unless `tie`) and whether
    the lists can settle the case at all."""
    P, E = np.asarray(P, dtype=np.int64), np.asarray(E, dtype=np.int64)
    V = np.asarray(verts, dtype=np.int64).reshape(-1, 3)
    assert np.abs(P).max() <= PE_REACH and np.abs(E).max() <= PE_REACH and (not len(V) or np.abs(V).max() <= PE_REACH), name
    assert len({tuple(v) for v in V}) == len(V), f"{name}: coincident vertices"
    dP = ((V - P) ** 2).sum(1)
    rho2 = ((V - E) ** 2).sum(1)
    d2 = int(dP.min()) if len(V) else -1
    c = dict(name=name, family=family, kind=kind, m=m, P=P, E=E, V=V, d2=d2, keep=bool(len(V) and d2 <= m * m), rank=0, decider=decider, tie=tie)
    if decider is not None:
        below, same = int((rho2 < rho2[decider]).sum()), int((rho2 == rho2[decider]).sum())
        assert same == (2 if tie else 1), f"{name}: {same} vertices at the deciding vertex's distance from the entry"
        c["rank"] = below + 1
        others = np.delete(dP, decider)
        assert not len(others) or others.min() > m * m + 1, f"{name}: a filler within reach of the particle"
    return c


def pe_sphere_cases(m):
    """On the sphere: one vertex at |dV|^2 = m^2 (kept), m^2 - 1 (kept) and m^2 + 1 (pruned) in every direction class under sign
    flips and axis permutations; the particle on its entry and PE_OFF off it (the m^2 cases both ways, the others alternating)."""
    out = []
    for off, kind in ((0, "on"), (-1, "in"), (1, "out")):
        i = 0
        for cl in pe_classes(m, off):
            for d in pe_orbit(cl):
                for delta in (((0, 0, 0), PE_OFF) if off == 0 else ((0, 0, 0),) if i % 2 else (PE_OFF,)):
                    P = np.array(delta)
                    c = _pe_case(f"sphere-{kind}-{d[0]}.{d[1]}.{d[2]}-{'on' if delta[0] == 0 else 'off'}", "sphere", m, P, [P + d], decider=0, kind=kind)
                    assert c["d2"] == m * m + off and c["rank"] == 1
                    out.append(c)
                i += 1
    return out


def pe_collinear_cases(m):
    """Entry, particle and vertex on one line, the vertex on the far side: rho_vertex = delta + d exactly, the tightest case of the
    triangle-inequality stop.  Along the six axes at d = m - 1, m, m + 1; along every direction class of the sphere at d = m."""
    out = []
    for a in PE_AXES:
        a = np.array(a)
        for r in (m - 1, m, m + 1):
            out.append(_pe_case(f"collinear-axis{a.tolist()}-{r}", "collinear", m, 200 * a, [(200 + r) * a], decider=0, kind="on" if r == m else "in" if r < m else "out"))
            assert out[-1]["d2"] == r * r
    for cl in pe_classes(m):
        d = np.array(pe_orbit(cl)[len(pe_orbit(cl)) // 3])
        out.append(_pe_case(f"collinear-{cl}", "collinear", m, 2 * d, [3 * d], decider=0, kind="on"))
        assert out[-1]["d2"] == m * m and int((9 * d * d).sum()) == 9 * m * m
    return out


def _pe_depth_vectors(m):
    """The deciding vertex from the particle, per kind: on the sphere (collinear with the entry: the stop's tightest case),
    at m^2 - 1 and at m^2 + 1."""
    v = {"on": (m, 0, 0), "in": pe_classes(m, -1)[-1][::-1], "out": (m, 1, 0)}
    assert sum(x * x for x in v["in"]) == m * m - 1 and sum(x * x for x in v["out"]) == m * m + 1
    return v


def pe_depth_cases(m):
    """List depth: the deciding vertex is the j-th by distance from the entry, j in PE_DEPTHS (257 and 300: not in the list - the
    header's rho must not stop the scan and the tree must find it).  The j - 1 fillers stand on the entry's far side at the radii
    1 .. j - 1, each at 450 + r > m + 1 from the particle.  Kind "none": the twin with no vertex within reach."""
    out, vec = [], _pe_depth_vectors(m)
    P = np.array((PE_DELTA, 0, 0))
    for j in PE_DEPTHS:
        fill = [(-r, 0, 0) for r in range(1, j)]
        for kind in ("on", "in", "out", "none"):
            if kind == "none":
                c = _pe_case(f"depth-{j}-none", "depth", m, P, fill, kind=kind)
                c["rank"] = j
                assert not c["keep"]
            else:
                c = _pe_case(f"depth-{j}-{kind}", "depth", m, P, fill + [P + vec[kind]], decider=j - 1, kind=kind)
                assert c["rank"] == j and c["keep"] == (kind != "out")
            out.append(c)
    return out


def pe_tie_cases(m):
    """Ties at the list's end: 255 fillers, then two vertices equidistant from the entry at ranks 256 / 257, one of them on the
    particle's sphere and the other on the far side.  Whichever the builder lists, the particle is kept."""
    out = []
    for a in PE_AXES:
        a = np.array(a)
        fill = [tuple(-r * a) for r in range(1, PE_LIST)]
        out.append(_pe_case(f"tie-{a.tolist()}", "tie", m, PE_DELTA * a, fill + [tuple(-(PE_DELTA + m) * a), tuple((PE_DELTA + m) * a)], decider=PE_LIST, tie=True, kind="on"))
    for c in out:   # (255 fillers at the radii 1 .. 255; the far-side twin and the deciding vertex share the ranks 256 and 257)
        assert len(c["V"]) == PE_LIST + 1 and c["rank"] == PE_LIST and c["keep"] and c["d2"] == m * m
    return out


def pe_tree_cases(m):
    """Tree edges: 256 fillers exhaust the list, the lone vertex within reach stands axis-aligned BETWEEN entry and particle, so a
    leaf whose box ends at it has box_dist2 == d2 == m^2 u^2 from the particle; and the same vertex one unit farther (pruned)."""
    out = []
    for a in PE_AXES:
        a = np.array(a)
        fill = [tuple(-r * a) for r in range(1, PE_LIST + 1)]
        for r, kind in ((m, "on"), (m + 1, "out")):
            c = _pe_case(f"tree-{a.tolist()}-{kind}", "tree", m, PE_DELTA * a, fill + [tuple((PE_DELTA - r) * a)], decider=PE_LIST, kind=kind)
            assert c["rank"] == PE_LIST + 1 and c["d2"] == r * r
            out.append(c)
    return out


def pe_field_cases(m):
    """Field-decided: the particle on its entry, its one vertex at 0, 1, m/4, m/2, 2m and 4m units; "far": no vertex of its own (the
    nearest stands in another region, beyond 20 m units)."""
    out = []
    for tag in PE_FIELD_DISTS:
        for a in PE_AXES[:2]:
            r = {"0": 0, "1": 1, "m/4": m // 4, "m/2": m // 2, "2m": 2 * m, "4m": 4 * m, "far": None}[tag]
            V = [] if r is None else [tuple(r * np.array(a))]
            out.append(_pe_case(f"field-{tag}-{a}", "field", m, (0, 0, 0), V, kind=tag))
            assert out[-1]["keep"] == (r is not None and r <= m)
    return out


_PE_WORLDS = {}


def pe_world(m=PE_M):
    """Every lattice case of threshold m u as the particles of ONE frame over ONE world.  -> a namespace: cases; per case (= per
    particle = per codebook entry) keep, d2, rank, the slice of its vertices; entries / parts / verts as int64 lattice coordinates;
    cb_poses, poses (identity rotations, float32), verts64, emb, code, thr.  Asserts the isolation of the regions, the exactness of
    every coordinate and, by an exact nearest-neighbour query over the whole world, that each case's nearest vertex is its own."""
    import types
    if m in _PE_WORLDS:
        return _PE_WORLDS[m]
    from scipy.spatial import cKDTree
    cases = pe_sphere_cases(m) + pe_collinear_cases(m) + pe_depth_cases(m) + pe_tie_cases(m) + pe_tree_cases(m) + pe_field_cases(m)
    n = len(cases)
    assert len({c["name"] for c in cases}) == n
    g = int(np.ceil(n ** (1.0 / 3.0)))
    i = np.arange(n)
    org = (np.stack([i % g, (i // g) % g, i // (g * g)], axis=1) - g // 2).astype(np.int64) * PE_SPACING
    # the first field case - particle, entry and vertex on one point - takes the region at the world's origin: its translation is
    # exactly (0, 0, 0), where the float32 screen's slack E vanishes (under thr = 0 its bounds collapse onto d2f = 0)
    zero, first = int(np.flatnonzero((org == 0).all(1))[0]), [c["family"] == "field" and c["kind"] == "0" for c in cases].index(True)
    org[[zero, first]] = org[[first, zero]]
    assert not org[first].any() and not cases[first]["P"].any() and not cases[first]["V"].any()
    assert PE_SPACING - 2 * PE_REACH > 4 * m + PE_REACH, "points of two regions within 4 m units + PE_REACH"
    entries = np.stack([c["E"] for c in cases]) + org
    parts = np.stack([c["P"] for c in cases]) + org
    at = np.cumsum([0] + [len(c["V"]) for c in cases])
    verts = np.concatenate([c["V"] + o for c, o in zip(cases, org)])
    owner = np.repeat(i, np.diff(at))
    for a in (entries, parts, verts):
        assert np.abs(a).max() < (1 << 24)
        f = (a * PE_U).astype(np.float32)
        assert np.array_equal(f.astype(np.float64) * 2.0 ** PE_K, a.astype(np.float64))
    # exact queries (integers below 2^24, squared distances below 2^53)
    vt, et = cKDTree(verts.astype(np.float64)), cKDTree(entries.astype(np.float64))
    dv, iv = vt.query(parts.astype(np.float64), k=1)
    de, ie = et.query(parts.astype(np.float64), k=2)
    assert np.array_equal(ie[:, 0], i) and (de[:, 1] > de[:, 0] + 2 * PE_REACH).all(), "a particle whose nearest entry is not its own"
    d2 = np.array([c["d2"] for c in cases], dtype=np.int64)
    got = np.rint(dv * dv).astype(np.int64)
    has = d2 >= 0
    assert np.array_equal(got[has], d2[has]) and np.array_equal(owner[iv[has]], i[has]), "a case whose nearest vertex is not its own"
    assert (got[~has] > (20 * m) ** 2).all(), "a case without vertices within 20 m units of another's"
    # the entry's list: its own vertices first, every foreign vertex farther than any of its own and beyond the stop's reach
    own_far = np.array([int(((c["V"] - c["E"]) ** 2).sum(1).max()) if len(c["V"]) else 0 for c in cases])
    assert ((PE_SPACING - 2 * PE_REACH) ** 2 > own_far).all() and PE_SPACING - 2 * PE_REACH > PE_DELTA + m + 4
    keep = np.array([c["keep"] for c in cases])
    assert np.array_equal(keep, has & (d2 <= m * m))
    ident = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    cb_poses, poses = ident.copy(), ident.copy()
    cb_poses[:, :3, 3] = (entries * PE_U).astype(np.float32)
    poses[:, :3, 3] = (parts * PE_U).astype(np.float32)
    rng = np.random.default_rng(1800 + m)
    emb = rng.standard_normal((n, PE_D)).astype(np.float32)
    w = types.SimpleNamespace(m=m, thr=m * PE_U, cases=cases, n=n, org=org, entries=entries, parts=parts, verts=verts, owner=owner, at=at,
                              keep=keep, d2=d2, rank=np.array([c["rank"] for c in cases]), family=np.array([c["family"] for c in cases]),
                              kind=np.array([str(c["kind"]) for c in cases]), cb_poses=cb_poses, poses=poses,
                              verts64=verts.astype(np.float64) * PE_U, emb=emb, code=rng.standard_normal(PE_D))
    nfill = np.diff(at) - np.array([c["decider"] is not None for c in cases]) - (w.family == "tie")
    # what neither the field nor the lists can settle and the tree must: a deciding vertex within a unit of the sphere behind the
    # list's end whose header cannot stop - the header's rho is the 257th vertex's distance from the entry: 450 - m or 450 - m - 1 in
    # the tree family, the 257th filler's 257 u under the 300th vertex, all far below delta + thr; only the 257th vertex at m^2 + 1
    # on the far side (rho^2 = (450 + m)^2 + 1) is stopped by it.  (The twins with no vertex within reach stand 451 u from their
    # nearest vertex: the field may decide them - `tree_open` - and without a field the tree does.)
    w.tree = ((w.rank > PE_LIST) & np.isin(w.kind, ("on", "in"))) | (w.family == "tree") | ((w.family == "depth") & (w.rank == 300) & (w.kind == "out"))
    w.tree_open = (w.kind == "none") & (nfill >= PE_LIST)
    w.shallow = (w.kind == "on") & (w.rank <= 16) & (w.rank >= 1) & np.isin(w.family, ("sphere", "collinear", "depth"))
    _PE_WORLDS[m] = w
    return w


def pe_frames(w):
    """The frames run over a world, as index lists into its cases: "all"; "small" (at most 512: every case outside the sphere
    family and every tenth of it - the two-kernel form's side of both engines' limits); "shallow" (only on-sphere cases decided
    within the first 16 records: nothing may reach the tree)."""
    i = np.arange(w.n)
    sph = i[w.family == "sphere"]
    small = np.sort(np.concatenate([i[w.family != "sphere"], sph[::10]]))
    small = small if len(small) % 2 == 0 else small[1:]     # (an even count: the sharded step takes no other)
    assert len(small) <= 512 < 2048 < w.n and w.n % 2 == 0
    shallow = i[w.shallow]
    return {"all": i, "small": small, "shallow": shallow[len(shallow) % 2:]}


def pe_degenerate_expected(w, thr, poses=None):
    """~(nn3_dist > thr) by the oracle for a degenerate threshold (0, +inf, negative, NaN) over the world's particles (or `poses`)."""
    from oracle import oracle
    d = oracle.nn3_dist(w.poses if poses is None else poses, w.verts64)
    with np.errstate(invalid="ignore"):
        return ~(d > thr)


def pe_nan_pose():
    P = np.eye(4, dtype=np.float32)
    P[0, 3] = np.nan
    return P


def _pe_brute_world(name, m, verts, parts):
    """A small world decided by brute force over int64: every particle stands on a codebook entry of its own (distinct
    positions: its nearest entry is itself, at distance 0), the mask is min |dV|^2 <= m^2.  -> a namespace like pe_world's."""
    import types
    verts, parts = np.asarray(verts, dtype=np.int64).reshape(-1, 3), np.asarray(parts, dtype=np.int64).reshape(-1, 3)
    n = len(parts)
    assert len({tuple(p) for p in parts}) == n and len({tuple(v) for v in verts}) == len(verts) and max(np.abs(verts).max(), np.abs(parts).max()) < (1 << 24)
    d2 = ((parts[:, None, :] - verts[None, :, :]) ** 2).sum(2).min(1)
    ident = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    ident[:, :3, 3] = (parts * PE_U).astype(np.float32)
    assert np.array_equal(ident[:, :3, 3].astype(np.float64) * 2.0 ** PE_K, parts.astype(np.float64))
    rng = np.random.default_rng(1900 + m + len(verts))
    cb_poses = _pe_with_far_entries(ident)
    return types.SimpleNamespace(name=name, m=m, thr=m * PE_U, n=n, parts=parts, verts=verts, d2=d2, keep=d2 <= m * m, cb_poses=cb_poses, poses=ident.copy(),
                                 verts64=verts.astype(np.float64) * PE_U, emb=rng.standard_normal((len(cb_poses), PE_D)).astype(np.float32),
                                 code=rng.standard_normal(PE_D))


PE_FAR_ENTRIES = 600


def _pe_with_far_entries(poses):
    """The small worlds' codebooks: an entry per particle, then PE_FAR_ENTRIES entries on a line 16 m away (nobody's nearest), so
    that the codebook has an ordinary size and only the MESH is tiny."""
    far = np.tile(np.eye(4, dtype=np.float32), (PE_FAR_ENTRIES, 1, 1))
    far[:, 0, 3] = 16.0 + np.arange(PE_FAR_ENTRIES, dtype=np.float32) * 2.0 ** -10
    far[:, 1, 3] = far[:, 2, 3] = 16.0
    assert np.abs(poses[:, :3, 3]).max() < 1.0
    return np.concatenate([poses, far])


PE_FACE_MS = (163, 164, 180)       # 2.4872 mm: "outside the grown grid = pruned" is armed (FIELD_EXPAND = 2.5 mm); 2.5024 mm and 2.7466 mm: it is not
PE_FACE_OUT = (170, 180, 181, 400)  # units outward that lie beyond the grown grid: FIELD_EXPAND 1.01 = 165.5 units plus a cell


def pe_face_world(m):
    """Mesh faces and the field's reach: a mesh of 15 vertices whose extreme vertex on each axis stands alone at +-100 units; a
    particle straight outward from it at m and m + 1 units (on the sphere, one unit beyond) and at PE_FACE_OUT units, beyond the
    grown grid.  Straight outward the extreme vertex is the nearest, so d is the offset itself (asserted): with m = 180 the particle
    at 170 and 180 units is outside the grid AND within thr - kept; with m = 163 every particle outside the grid is pruned."""
    R = 100
    verts = [(0, 0, 0)] + [tuple(R * np.array(a)) for a in PE_AXES] + [(sx * 40, sy * 40, sz * 40) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    outs = sorted({m, m + 1} | set(PE_FACE_OUT))
    parts = [tuple((R + o) * np.array(a)) for a in PE_AXES for o in outs]
    w = _pe_brute_world(f"face-{m}", m, verts, parts)
    assert np.array_equal(w.d2, np.array([o * o for _ in PE_AXES for o in outs]))
    assert FIELD_EXPAND_UNITS * 1.01 + 4 < min(PE_FACE_OUT) and (m != 180 or w.keep.reshape(6, -1)[:, :2].all())
    w.outside = np.array([o in PE_FACE_OUT for _ in PE_AXES for o in outs])
    return w


FIELD_EXPAND_UNITS = 0.0025 / PE_U   # csrc/tree.hip FIELD_EXPAND in lattice units: 163.84
PE_TINY_SIZES = (1, 2, 16, 17, 256, 257)


def pe_tiny_world(nv, m=PE_M):
    """Tiny meshes: nv vertices in all on a line, 3 units apart (lists padded with rho = inf records, a header rho = inf up to 256
    vertices, a tree of one leaf); particles around the first and the last vertex at m, m + 1 straight outward, on a direction
    class of the sphere, one at 0 and one far off."""
    verts = [(3 * i, 0, 0) for i in range(nv)]
    end = 3 * (nv - 1)
    a, b, c = pe_classes(m)[1]
    parts = [(-m, 0, 0), (-m - 1, 0, 0), (end + m, 0, 0), (end + m + 1, 0, 0), (-c, a, b), (-c, a, b + 1), (end + c, -b, a), (end + c, -b - 1, a),
             (0, 0, 0), (end, m, 0), (end, 0, -m - 1), (end + 20 * m, 7, 0)]
    w = _pe_brute_world(f"tiny-{nv}", m, verts, parts)
    assert w.keep.tolist() == [True, False, True, False, True, False, True, False, True, True, False, False], (nv, w.keep.tolist())
    return w


# the ulp family, off the lattice: float64 vertices and float32 particles whose spec distance d2 = fma(dz, dz, fma(dy, dy, dx dx))
# (csrc/tree_search.hpp dist2, oracle mo_nn3) is exactly t2 = squared_threshold(thr) - kept, and above fl(thr thr) for these
# thresholds - or the next double above t2 - pruned.
PE_ULP_THRS = (0.002, 1e-4, 0.004)
PE_ULP_PER_SIDE = 12


def _fma1(a, b, c):
    from fractions import Fraction
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def pe_ulp_d2(p, v, variant="spec"):
    """The squared distance of the float32 particle p (as float64) from the float64 vertex v as the spec adds it up, or as a mutant
    does: "reversed" (the chain from dz), "uncontracted" ((dx dx + dy dy) + dz dz with every product rounded)."""
    dx, dy, dz = (float(p[i]) - float(v[i]) for i in range(3))
    if variant == "spec":
        return _fma1(dz, dz, _fma1(dy, dy, dx * dx))
    if variant == "reversed":
        return _fma1(dx, dx, _fma1(dy, dy, dz * dz))
    if variant == "uncontracted":
        return (dx * dx + dy * dy) + dz * dz
    raise ValueError(variant)


_PE_ULP = {}


def pe_ulp_world(thr, per_side=PE_ULP_PER_SIDE, max_trials=4000):
    """Per side ("on": d2 == t2, kept; "above": d2 == the next double, pruned) `per_side` cases found by search: the particle a
    float32 point of a 2^-5 m grid in the plane z = 0 (its own entry), the vertex v = p - d with d drawn inside the sphere and dz
    stepped by ulps until the chain lands on the target exactly.  The cases of each side are chosen so that, where the search finds
    them, some separate the mutants: a reversed chain or an uncontracted sum puts them on the other side of t2 (`flips`, counted per
    variant; for all three thresholds of PE_ULP_THRS the search finds both within its first few hundred trials).  Asserts t2 !=
    thr thr, and that sqrt(d2) > thr agrees with d2 > t2 on every point."""
    import types
    if thr in _PE_ULP:
        return _PE_ULP[thr]
    t2 = pe_squared_threshold(thr)
    assert t2 != thr * thr and t2 == np.nextafter(thr * thr, np.inf), "a threshold whose t2 is thr thr: the family needs another"
    rng = np.random.default_rng(int(thr * 1e7) + 18)
    P, V, keep, flips = [], [], [], {"reversed": 0, "uncontracted": 0}
    for side, target in (("on", t2), ("above", float(np.nextafter(t2, np.inf)))):
        found, want_flip = [], {"reversed": 2, "uncontracted": 2}
        for trial in range(max_trials):
            if len(found) >= per_side:
                break
            i = len(P) + len(found)
            p = np.array([(i % 8 - 4) * 2.0 ** -5, (i // 8 - 3) * 2.0 ** -5, 0.0])
            ab = rng.uniform(-0.65, 0.65, 2) * thr
            v = np.array([p[0] - ab[0], p[1] - ab[1], 0.0])
            dx, dy = p[0] - v[0], p[1] - v[1]
            s = _fma1(dy, dy, dx * dx)
            z = float(np.sqrt(target - s)) * (1 if trial % 2 else -1)
            for k in range(-6, 7):
                zk = z
                for _ in range(abs(k)):
                    zk = float(np.nextafter(zk, np.inf if k > 0 else -np.inf))
                v[2] = -zk
                if pe_ulp_d2(p, v) == target:
                    fl = {var: (pe_ulp_d2(p, v, var) > t2) != (target > t2) for var in flips}
                    need = [var for var in fl if fl[var] and want_flip[var] > 0]
                    if need or len(found) < per_side - sum(want_flip.values()):
                        for var in need:
                            want_flip[var] -= 1
                        found.append((p.copy(), v.copy(), fl))
                    break
        assert len(found) == per_side, (thr, side, len(found))
        for p, v, fl in found:
            d2 = pe_ulp_d2(p, v)
            assert (np.sqrt(d2) > thr) == (d2 > t2) == (side == "above")
            P.append(p)
            V.append(v)
            keep.append(side == "on")
            for var in flips:
                flips[var] += fl[var]
    P, V = np.array(P), np.array(V)
    n = len(P)
    assert np.array_equal(P.astype(np.float32).astype(np.float64), P) and len({tuple(p) for p in P}) == n
    ident = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    ident[:, :3, 3] = P.astype(np.float32)
    w = types.SimpleNamespace(name=f"ulp-{thr}", thr=thr, t2=t2, n=n, keep=np.array(keep), cb_poses=_pe_with_far_entries(ident), poses=ident.copy(), verts64=V,
                              flips=flips, emb=rng.standard_normal((n + PE_FAR_ENTRIES, PE_D)).astype(np.float32), code=rng.standard_normal(PE_D))
    _PE_ULP[thr] = w
    return w


def pe_tiled(w, n):
    """The particles of a small world repeated up to n (several particles on one pose are ordinary): -> (poses, the case of each)."""
    idx = np.arange(n) % w.n
    return w.poses[idx], idx
