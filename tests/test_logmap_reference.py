"""The log-map yardstick (tests/_logmap_reference.py) on the CPU: against a scipy restatement of theseus' SE3.log_map / exp_map,
exp(log(T)) == T to rounding, the threshold branches on either side of 1e-6 and 1e-8, one cluster of one member."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from _logmap_reference import (assert_logmap_cluster, logmap_cluster_reference, se3_exp64, se3_log_from, se3_log_reference,
                               spread_var)


@pytest.fixture(scope="module", autouse=True)
def _built(oracle):
    return oracle


def _se3_log_np(P):
    """theseus SE3.log_map restated with scipy / numpy float64: xi = [V^-1 t, omega] (published formulas)."""
    R, t = P[:, :3, :3].astype(np.float64), P[:, :3, 3].astype(np.float64)
    om = Rotation.from_matrix(R).as_rotvec()
    out = np.zeros((len(P), 6))
    for k in range(len(P)):
        th = np.linalg.norm(om[k])
        W = np.array([[0, -om[k, 2], om[k, 1]], [om[k, 2], 0, -om[k, 0]], [-om[k, 1], om[k, 0], 0]])
        if th > 1e-6:
            Vinv = np.eye(3) - 0.5 * W + (1 - th * np.cos(th / 2) / (2 * np.sin(th / 2))) / th**2 * W @ W
        else:
            Vinv = np.eye(3) - 0.5 * W + W @ W / 12.0
        out[k, :3], out[k, 3:] = Vinv @ t[k], om[k]
    return out


def _se3_exp_np(xi):
    u, om = xi[:3], xi[3:]
    th = np.linalg.norm(om)
    W = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    A, B, C = (np.sin(th) / th, (1 - np.cos(th)) / th**2, (th - np.sin(th)) / th**3) if th > 1e-8 else (1.0, 0.5, 1.0 / 6.0)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * W + B * W @ W
    T[:3, 3] = (np.eye(3) + B * W + C * W @ W) @ u
    return T


def _poses(n, seed, spread_deg=40.0, dist=0.1):
    rng = np.random.default_rng(seed)
    P = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    P[:, :3, :3] = Rotation.from_rotvec(np.deg2rad(spread_deg) * rng.standard_normal((n, 3))).as_matrix().astype(np.float32)
    P[:, :3, 3] = rng.uniform(-dist, dist, (n, 3)).astype(np.float32)
    return P


def test_log_against_scipy():
    """omega comes from the float32 spec function (within a few float32 steps of scipy's float64 logarithm of the float32 matrix),
    so u agrees to that times abs(t); with scipy's omega put in, u agrees to float64 rounding."""
    P = _poses(500, 1)
    xi, ref = se3_log_reference(P), _se3_log_np(P)
    assert np.abs(xi[:, 3:] - ref[:, 3:]).max() < 2e-6
    assert np.abs(xi[:, :3] - ref[:, :3]).max() < 2e-6 * 0.1 * 2
    same = se3_log_from(ref[:, 3:], P[:, :3, 3])
    assert np.abs(same[:, :3] - ref[:, :3]).max() < 1e-15


def test_exp_of_log_is_the_pose():
    P = _poses(300, 2, spread_deg=60.0, dist=10.0)
    xi = se3_log_reference(P)
    for k in range(len(P)):
        T = se3_exp64(xi[k])
        assert np.abs(T - _se3_exp_np(xi[k])).max() < 1e-14 * 10.0
        assert np.abs(T[:3, 3] - P[k, :3, 3]).max() < 1e-13  # V V^-1 = I to float64 rounding, whatever omega is
        assert np.abs(T[:3, :3] - P[k, :3, :3]).max() < 3e-6  # (float32 omega of a float32 matrix)


@pytest.mark.parametrize("th", [0.5e-6, 0.999e-6, 1.001e-6, 2e-6])
def test_log_threshold_1e_6(th):
    """Either side of th = 1e-6 the two branches of c agree to 1e-4 relative (the closed form cancels there: 1e-16 / th^2), which
    moves u by th^2 T of it - nothing; the branch taken is the spec's."""
    om = np.array([[th, 0.0, 0.0]])
    t = np.array([[0.3, -0.2, 0.1]])
    xi = se3_log_from(om, t)
    a = np.cross(om, t)
    c = 1.0 / 12.0 if th <= 1e-6 else (1.0 - 0.5 * th * np.cos(0.5 * th) / np.sin(0.5 * th)) / (th * th)
    assert np.array_equal(xi[0, :3], (t - 0.5 * a + c * np.cross(om, a))[0])
    assert abs(c - 1.0 / 12.0) < 1e-3
    assert np.abs(xi[0, :3] - (t - 0.5 * a)[0]).max() < 1e-12


@pytest.mark.parametrize("th", [0.5e-8, 1e-8, 1.0000001e-8, 3e-8])
def test_exp_threshold_1e_8(th):
    xi = np.array([0.3, -0.2, 0.1, 0.0, th, 0.0])
    T = se3_exp64(xi)
    assert np.abs(T - _se3_exp_np(xi)).max() == 0.0 or th > 1e-8  # the restatement takes `>`: the same branch up to 1e-8
    W = np.array([[0, 0, th], [0, 0, 0], [-th, 0, 0]])
    first = np.eye(3) + W
    assert np.abs(T[:3, :3] - first).max() < 1e-15
    # just above the threshold cos(th) rounds to 1 and the closed form gives B = 0 where 1/2 is meant: the spec's formula, off by
    # up to th / 2 of abs(u) there - far under a float32 step of the centre (the bound's 1 / th_bar term, translation_f64_term)
    assert np.abs(T[:3, 3] - (np.eye(3) + 0.5 * W) @ xi[:3]).max() < (1e-15 if th <= 1e-8 else 0.5 * th * 0.4)


def test_one_member_is_its_pose():
    P = _poses(7, 3, spread_deg=50.0)
    for k in range(len(P)):
        (rec,) = logmap_cluster_reference(P[k:k + 1], np.array([0.25]), np.zeros(1, dtype=np.int64))
        assert rec["count"] == 1 and rec["flat"]
        assert np.array_equal(rec["center"][:3, 3], P[k, :3, 3])  # exp(log) returns the float32 translation itself
        assert np.abs(rec["center"][:3, :3] - P[k, :3, :3]).max() < 3e-6
        assert np.array_equal(rec["std"], np.zeros(3, dtype=np.float32))
        assert_logmap_cluster(rec["center"][None], rec["std"][None], [rec], 1, "itself")


def test_cluster_against_scipy_restatement():
    rng = np.random.default_rng(5)
    P = _poses(900, 4, spread_deg=8.0)
    labels = rng.integers(-1, 3, 900)
    w = rng.uniform(0.0, 1.0, 900)
    w[labels == 1] = 0.37  # flat
    ref = logmap_cluster_reference(P, w, labels, np.array([-1, 0, 1, 2, 9]))
    xi = _se3_log_np(P)
    w32 = w.astype(np.float32)
    for rec in ref[:4]:
        m = labels == rec["label"]
        tw = np.ones(m.sum()) if rec["flat"] else w32[m].astype(np.float64)
        assert rec["flat"] == (rec["label"] == 1)
        C = _se3_exp_np((xi[m] * tw[:, None]).sum(0) / tw.sum())
        assert np.abs(rec["center"] - C).max() < 2e-6
        sd = np.sqrt((((P[m, :3, 3].astype(np.float64) - C[:3, 3]) ** 2) * tw[:, None]).sum(0) / tw.sum())
        np.testing.assert_allclose(rec["std"], sd, rtol=1e-4)
        assert np.array_equal(rec["var"], spread_var(rec, rec["center"][:3, 3]))
    assert ref[4]["count"] == 0 and np.isnan(ref[4]["center"]).all() and np.isnan(ref[4]["std"]).all()


def test_nan_weight_rule():
    P = _poses(50, 6)
    w = np.full(50, 0.5)
    w[17] = np.nan
    (rec,) = logmap_cluster_reference(P, w, np.zeros(50, dtype=np.int64))
    assert rec["nan"] and not rec["flat"] and np.isnan(rec["center"][:3]).all() and np.isnan(rec["std"]).all()
    assert np.array_equal(rec["center"][3], np.float32([0, 0, 0, 1]))
