"""`ops.se3_log` (k_se3_log, cluster_logmap.hpp) against the yardstick of tests/_logmap_reference.py, entry by entry within the
bound derived there: omega the same bits as the float32 spec function, u within 64 u64 (1 + th) T."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from _logmap_reference import se3_log_bound, se3_log_reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _pose(rotvec=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)):
    P = np.eye(4, dtype=np.float32)
    P[:3, :3] = Rotation.from_rotvec(np.asarray(rotvec, dtype=np.float64)).as_matrix().astype(np.float32)
    P[:3, 3] = np.asarray(t, dtype=np.float32)
    return P


def _tiny(v, t):
    """I + hat((v, 0, 0)) in float32: so3_log's small-angle branch returns theta = v to a rounding."""
    P = _pose(t=t)
    P[2, 1], P[1, 2] = np.float32(v), np.float32(-v)
    return P


def _edges():
    t = (0.03, -0.07, 0.11)
    ax = np.array([1.0, 2.0, -2.0]) / 3.0
    out = [("identity", _pose(t=t)), ("identity at the origin", _pose()),
           ("theta 0.9e-6", _tiny(0.9e-6, t)), ("theta 0.999e-6", _tiny(0.999e-6, t)), ("theta 1.001e-6", _tiny(1.001e-6, t)),
           ("theta 1.1e-6", _tiny(1.1e-6, t)), ("theta 4.9e-3", _pose(ax * 4.9e-3, t)), ("theta 5.1e-3", _pose(ax * 5.1e-3, t)),
           ("theta 3.1", _pose(ax * 3.1, t)), ("theta pi", _pose(ax * np.pi, t)), ("t = 0", _pose(ax * 0.7)),
           ("abs(t) = 10", _pose(ax * 0.7, np.array([6.0, -8.0, 0.0]))), ("abs(t) = 10, theta 3.1", _pose(ax * 3.1, (0.0, 6.0, 8.0)))]
    # so3_log's cut at 1 + cos(theta) = 1e-2: theta = acos(-0.99), either side
    cut = float(np.arccos(-0.99))
    for d in (-1e-3, -1e-5, 1e-5, 1e-3):
        out.append((f"cut{d:+g}", _pose(ax * (cut + d), t)))
    return out


def _check(ops, P, tag):
    dev = torch.device("cuda", 0)
    got = ops.se3_log(torch.as_tensor(P).to(dev))
    assert got.shape == (len(P), 6) and got.dtype == torch.float64
    got = got.cpu().numpy()
    ref = se3_log_reference(P)
    bound = se3_log_bound(ref, P)
    assert np.array_equal(got[:, 3:], ref[:, 3:]), f"{tag}: omega is not the spec function's"
    dev_u = np.abs(got[:, :3] - ref[:, :3])
    frac = float((dev_u / np.where(bound[:, :3] > 0, bound[:, :3], 1e-300)).max())
    print(f"{tag}: largest u deviation {dev_u.max():.3g}, {frac:.3g} of its bound")
    assert (dev_u <= bound[:, :3]).all(), (tag, dev_u.max(), frac)
    return got


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_sizes(N):
    from midastouch_amd import ops
    rng = np.random.default_rng(N)
    P = np.stack([_pose(rng.standard_normal(3) * rng.uniform(0.0, 1.8), rng.uniform(-0.2, 0.2, 3)) for _ in range(N)])
    _check(ops, P, f"N = {N}")


def test_edges():
    from midastouch_amd import ops
    names, P = zip(*_edges())
    P = np.stack(P)
    got = _check(ops, P, "edges")
    xi = dict(zip(names, got))
    assert np.array_equal(xi["identity"], np.float64([np.float32(0.03), np.float32(-0.07), np.float32(0.11), 0, 0, 0]))
    assert np.array_equal(xi["identity at the origin"], np.zeros(6))
    assert np.array_equal(xi["t = 0"][:3], np.zeros(3)) and xi["t = 0"][3:].any()
    for k in ("theta 0.9e-6", "theta 0.999e-6"):  # c = 1 / 12 on this side
        assert 0.0 < np.linalg.norm(xi[k][3:]) <= 1e-6
    for k in ("theta 1.001e-6", "theta 1.1e-6"):
        assert np.linalg.norm(xi[k][3:]) > 1e-6
    assert abs(np.linalg.norm(xi["theta 3.1"][3:]) - 3.1) < 1e-5 and abs(np.linalg.norm(xi["theta pi"][3:]) - np.pi) < 1e-3


def test_nan_pose_gives_a_nan_row():
    from midastouch_amd import ops
    P = np.stack([_pose((0.1, 0.2, 0.3), (0.01, 0.02, 0.03))] * 3)
    P[1, 0, 0] = np.nan
    got = ops.se3_log(torch.as_tensor(P).to(torch.device("cuda", 0))).cpu().numpy()
    assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all() and np.array_equal(got[0], got[2])
