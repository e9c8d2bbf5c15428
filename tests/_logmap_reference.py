"""The yardstick of the log-map cluster centres (get_cluster_centers(method="logmap"), modules/particle_filter.py:153-206 with
pose.log_map_averaged, modules/pose.py:101-109; DESIGN.md 2, "The log-map centre's arithmetic") - not the kernel's twin:

  * omega of a particle from `oracle.so3_log` (the float32 spec function the device function is bit-identical to), widened;
  * everything else numpy float64 (numpy's sin / cos, not the device's), the formulas and thresholds of `pose.se3_log` / `se3_exp`;
  * every sum by math.fsum (exactly rounded sums of the float64 products), where the kernel adds in its butterfly / wave / block order;
  * the spread in two passes around the float32 centre translation, where the kernel closes one-pass moments;
  * the float32 weights, the flatten rule and the NaN rule as tests/_recipes.py::cluster_reference states them.

tests/test_logmap_reference.py holds it to a scipy restatement on the CPU; the GPU tests hold the kernels to it."""
import math

import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24
ROT_TOL = 2.0 ** -23  # two float32 roundings of an entry in [-1, 1] (the float64 error of an entry, ~1e-13, is far below)


def so3_log64(poses):
    """(n,3) float64: oracle.so3_log's float32 rotation vectors, widened."""
    from oracle import oracle as orc
    P = np.ascontiguousarray(np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4))
    return np.asarray(orc.so3_log(P), dtype=np.float32).reshape(-1, 3).astype(np.float64)


def se3_log_from(omega, t):
    """xi = [u, omega] (n,6) float64 from float64 omega and t: u = t - a / 2 + c (omega x a), a = omega x t,
    c = th > 1e-6 ? (1 - (th / 2) cos(th / 2) / sin(th / 2)) / th^2 : 1 / 12."""
    om, t = np.asarray(omega, dtype=np.float64).reshape(-1, 3), np.asarray(t, dtype=np.float64).reshape(-1, 3)
    th = np.sqrt((om * om).sum(axis=1))
    big = th > 1e-6
    h = 0.5 * np.where(big, th, 1.0)
    with np.errstate(all="ignore"):
        c = np.where(big, (1.0 - h * np.cos(h) / np.sin(h)) / np.where(big, th * th, 1.0), 1.0 / 12.0)
    c = np.where(np.isnan(th), np.nan, c)
    a = np.cross(om, t)
    u = t - 0.5 * a + c[:, None] * np.cross(om, a)
    return np.concatenate([u, om], axis=1)


def se3_log_reference(poses):
    """(n,6) float64 [u, omega] of float32 poses: the yardstick of `ops.se3_log`."""
    P = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
    return se3_log_from(so3_log64(P), P[:, :3, 3].astype(np.float64))


def se3_exp64(xi):
    """One tangent vector [u, omega] -> (4,4) float64: th <= 1e-8 ? A, B, C = 1, 1/2, 1/6 : sin th / th, (1 - cos th) / th^2,
    (th - sin th) / th^3; R = I + A W + B W^2, t = (I + B W + C W^2) u."""
    xi = np.asarray(xi, dtype=np.float64).reshape(6)
    u, om = xi[:3], xi[3:]
    th = float(np.sqrt(om @ om))
    if th <= 1e-8:
        A, B, Cc = 1.0, 0.5, 1.0 / 6.0
    else:
        A, B, Cc = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th), (th - math.sin(th)) / (th * th * th)
    W = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    W2 = W @ W
    T = np.zeros((4, 4))
    T[:3, :3] = np.eye(3) + A * W + B * W2
    T[:3, 3] = (np.eye(3) + B * W + Cc * W2) @ u
    T[3, 3] = 1.0
    return T


def se3_log_bound(xi_ref, poses):
    """Per entry bound (n,6) on `ops.se3_log` against se3_log_reference.  omega: 0 - the same float32 bits, widened.  u: both sides
    evaluate the same float64 formula on the same inputs and differ in the order of a few operations and in sin / cos (each within
    2 ulp).  With T = max abs(t) of the pose and th = abs(omega) <= pi: a component of a = omega x t is two products and a
    subtraction of magnitudes <= th T (error <= 4 u th T), of b = omega x a likewise on top of a's error (<= 12 u th^2 T);
    c = (1 - x) / th^2 with x = h cos h / sin h <= 1 known to 5 u gives abs(dc) <= 7 u / th^2 + 2 u c, and abs(b) <= th^2 T, c th^2 <= 1.1:
    d(c b) <= (7 + 15 * 1.1) u T < 24 u T; the two additions of t - a / 2 + c b round values <= (2 + th) T.  In all under
    32 u (1 + th) T on each side, 64 u (1 + th) T between the two."""
    P = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
    T = np.abs(P[:, :3, 3].astype(np.float64)).max(axis=1)
    th = np.sqrt((xi_ref[:, 3:] ** 2).sum(axis=1))
    b = np.zeros_like(xi_ref)
    b[:, :3] = (64.0 * U64 * (1.0 + th) * T)[:, None]
    return b


def logmap_cluster_reference(poses, w, labels, label_values=None):
    """Per label value (default: the sorted unique labels) a dict: center (4,4) f32, std (3,) f32, var (3,) float64 (two passes
    around the float32 centre translation), center64 (4,4), count, flat, nan, tmax (max abs(t) of the members), thmax (max
    abs(omega)), t (m,3) float64 and tw (m,) float64: the members' translations and effective weights, sw their fsum.  A NaN weight
    is never flat and makes rotation, translation and spread NaN, the bottom row stays 0 0 0 1; an empty cluster is NaN
    everywhere with count 0."""
    P = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
    w32 = np.asarray(w).astype(np.float32).reshape(-1)
    labels = np.asarray(labels).reshape(-1)
    values = np.unique(labels) if label_values is None else np.asarray(label_values).reshape(-1)
    xi_all = se3_log_reference(P)
    out = []
    for lab in values:
        sel = labels == lab
        n = int(sel.sum())
        rec = dict(label=int(lab), count=n, flat=False, nan=False, tmax=0.0, thmax=0.0,
                   center=np.full((4, 4), np.nan, dtype=np.float32), std=np.full(3, np.nan, dtype=np.float32),
                   var=np.full(3, np.nan), center64=np.full((4, 4), np.nan), t=None, tw=None, sw=float("nan"), thbar=0.0)
        out.append(rec)
        if n == 0:
            continue
        t, tw, xi = P[sel][:, :3, 3].astype(np.float64), w32[sel], xi_all[sel]
        rec["tmax"] = float(np.abs(t).max())
        rec["thmax"] = float(np.sqrt((xi[:, 3:] ** 2).sum(axis=1)).max())
        rec["center"][3] = (0.0, 0.0, 0.0, 1.0)
        if np.isnan(tw).any():
            rec["nan"] = True
            continue
        rec["flat"] = bool(abs(np.float32(tw.max() - tw.min())) <= 1e-8)
        tw = np.ones(n) if rec["flat"] else tw.astype(np.float64)
        sw = math.fsum(tw)
        xb = np.array([math.fsum(tw * xi[:, k]) for k in range(6)]) / sw
        with np.errstate(all="ignore"):
            C64 = se3_exp64(xb) if np.isfinite(xb).all() else np.full((4, 4), np.nan)
        rec["center64"] = C64
        rec["thbar"] = float(np.sqrt((xb[3:] ** 2).sum()))
        rec["center"][:3] = C64[:3]  # (rounded to float32 here)
        rec["t"], rec["tw"], rec["sw"] = t, tw, sw
        rec["var"] = spread_var(rec, rec["center"][:3, 3])
        with np.errstate(all="ignore"):
            rec["std"] = np.sqrt(rec["var"]).astype(np.float32)
    return out


def spread_var(rec, m32):
    """sum w (t - m)^2 / sum w per axis, two passes around the float32 translation m32, fsum."""
    d = rec["t"] - np.asarray(m32, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.array([math.fsum(rec["tw"] * (d[:, k] * d[:, k])) for k in range(3)]) / rec["sw"]


def spread_kappa(nblocks):
    return 4 * (int(nblocks) + 12) + 4


def translation_f64_term(rec, nblocks):
    """The float64 part of the translation bound.  The centre's translation is V(omega_bar) u_bar with u_bar = sum w u / sum w.
    With weights >= 0, T = max abs(t) and th = max abs(omega) of the members, abs(u) <= U = 1.2 (1 + th) T:
      * a particle's u differs by up to 64 u64 (1 + th) T between the two sides (se3_log_bound), and so does any weighted mean of it;
      * the kernel's sums go through six butterfly levels, three additions over the waves and a chain over the blocks - at most
        nblocks + 8 additions deep - of products with one rounding: numerator and denominator each within (nblocks + 10) u64 of
        the sum of magnitudes, the quotient one more: abs(d u_bar) <= (2 (nblocks + 10) + 1) u64 U; the reference's fsum sides: 3 u64 U;
      * omega_bar carries the same relative error; it enters V - I = B W + C W^2, of norm <= th / 2 + th^2 / 6 < 1 + th, applied to
        u_bar: another (2 (nblocks + 10) + 4) u64 (1 + th) U;
      * the closed forms of B and C (sin, cos within 2 ulp, the cancellations (1 - cos th) / th^2 and (th - sin th) / th^3 hold
        their absolute error: 1 - cos th is known to 2 u64, so B to 2 u64 / th_bar^2 and B W to 2 u64 / th_bar - at the threshold
        th_bar = 1e-8 that is 2e-8 of abs(u_bar), still under a float32 step; C W^2 to 2 u64) and the 3 x 3 product: under
        (40 (1 + th) + 2 / th_bar) u64 U on each side, the second part only for th_bar > 1e-8 (below, both sides take the constants).
    Sum: (4 (nblocks + 10) + 64 + 8 + 80) u64 (1 + th)^2 1.2 T, rounded up to (4 nblocks + 200) u64 1.2 (1 + th)^2 T, plus
    4 u64 / th_bar 1.2 (1 + th) T."""
    U = 1.2 * (1.0 + rec["thmax"]) * rec["tmax"]
    small = 4.0 * U64 / rec["thbar"] * U if rec["thbar"] > 1e-8 else 0.0
    return (4.0 * nblocks + 200.0) * U64 * (1.0 + rec["thmax"]) * U + small


def assert_logmap_cluster(got_c, got_s, ref, nblocks, tag="", log=None):
    """Centres (C,4,4) and spreads (C,3) of a device form against logmap_cluster_reference's records (nblocks = the 256-particle
    workgroups whose partials the finisher adds up).  Effective weights >= 0.

    Translation.  The kernel's float64 centre translation is within translation_f64_term of the reference's float64 value (derived
    there); each is rounded once to float32: within ONE float32 ulp of the reference's float32 entry plus that term.

    Rotation.  R = I + A W + B W^2 of omega_bar, whose float64 error is of the order (nblocks + 10) u64: every entry within 2^-23
    of the reference's float32 entry (two float32 roundings).

    Spread.  sd = sqrt(var), var = (S2 - 2 m S1 + m^2 S0) / S0 from the one-pass moments around the float32 centre translation m
    THE DEVICE REPORTS (within one ulp of the reference's by the line above; the log-map centre is not the weighted mean, so var
    depends on m to first order and the yardstick is taken around the same m: two passes, fsum).  The derivation is
    _recipes.assert_cluster's - the same moments, the same closed form: abs(var - var_ref) <= E = kappa u64 T^2 with
    kappa = 4 (nblocks + 12) + 4, abs(sd - sd_ref) <= E / (sd_ref + sqrt(E)) + 2^-23 sd_ref.  No slack beyond that.

    NaN and empty clusters: NaN where the reference is NaN (the bottom row of a cluster with members stays 0 0 0 1).
    -> what was seen: t_ulp (largest translation deviation in float32 ulps of the reference entry), t_exact / t_total, t_f64_frac
    (largest deviation beyond one ulp as a fraction of the float64 term; 0 when none exceeded an ulp), rot_dev, sd_frac (largest
    deviation as a fraction of its bound), sd_equal / sd_total, kappa_ratio (abs(sd^2 - var_ref) / (u64 T^2) after taking off
    2^-22 var_ref)."""
    got_c = np.asarray(got_c.detach().cpu().numpy() if hasattr(got_c, "detach") else got_c, dtype=np.float32).reshape(-1, 4, 4)
    got_s = np.asarray(got_s.detach().cpu().numpy() if hasattr(got_s, "detach") else got_s, dtype=np.float32).reshape(-1, 3)
    assert got_c.shape[0] == len(ref) and got_s.shape[0] == len(ref), (tag, got_c.shape, got_s.shape, len(ref))
    seen = dict(t_ulp=0.0, t_exact=0, t_total=0, t_f64_frac=0.0, rot_dev=0.0, sd_frac=0.0, sd_equal=0, sd_total=0, kappa_ratio=0.0)
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
        ulp = np.maximum(np.spacing(np.abs(rt)), np.spacing(np.abs(c[:3, 3]))).astype(np.float64)
        d64 = translation_f64_term(r, nblocks)
        dev = np.abs(c[:3, 3].astype(np.float64) - rt.astype(np.float64))
        seen["t_ulp"] = max(seen["t_ulp"], float((dev / ulp).max()))
        seen["t_exact"] += int((c[:3, 3] == rt).sum())
        seen["t_total"] += 3
        over = np.maximum(dev - ulp, 0.0)
        if d64 > 0.0:
            seen["t_f64_frac"] = max(seen["t_f64_frac"], float(over.max() / d64))
        assert (dev <= ulp + d64).all(), f"{what}: translation {c[:3, 3]!r} vs {rt!r}: off by {dev}, allow {ulp} + {d64:.3g}"
        # rotation
        dr = float(np.abs(c[:3, :3].astype(np.float64) - r["center"][:3, :3].astype(np.float64)).max())
        seen["rot_dev"] = max(seen["rot_dev"], dr)
        assert dr <= ROT_TOL, f"{what}: rotation off by {dr:.3g}\n{c[:3, :3]}\n{r['center'][:3, :3]}"
        # spread, around the translation the device reports
        var_ref = r["var"] if np.array_equal(c[:3, 3], rt) else spread_var(r, c[:3, 3])
        rs32 = np.sqrt(var_ref).astype(np.float32)
        rs = rs32.astype(np.float64)
        T2 = r["tmax"] ** 2
        E = kappa * U64 * T2
        bound = 2.0 ** -23 * rs + (E / (rs + np.sqrt(E)) if E > 0.0 else 0.0)
        d = np.abs(s.astype(np.float64) - rs)
        frac = np.where(d == 0.0, 0.0, d / np.where(bound > 0.0, bound, 1e-300))
        seen["sd_frac"] = max(seen["sd_frac"], float(frac.max()))
        seen["sd_equal"] += int((s == rs32).sum())
        seen["sd_total"] += 3
        if T2 > 0.0:
            ratio = np.maximum(np.abs(s.astype(np.float64) ** 2 - var_ref) - 2.0 ** -22 * var_ref, 0.0) / (U64 * T2)
            seen["kappa_ratio"] = max(seen["kappa_ratio"], float(ratio.max()))
        assert (d <= bound).all(), (f"{what}: spread {s!r} vs {rs32!r}: off by {d} where kappa = {kappa}, max|t| = {r['tmax']:.3g} "
                                    f"allow {bound}")
    if log is not None:
        for k, v in seen.items():
            log[k] = (log.get(k, 0) + v) if isinstance(v, int) else max(log.get(k, 0.0), v)
    return seen
