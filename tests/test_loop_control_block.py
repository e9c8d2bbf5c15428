"""The loop engines' control-block writers on the host (loop_engine.particles_block / annealing_block), for one trajectory
(lead ()) and for a batch (lead (3,)): what `set_particles` and `set_annealing_state` put into ctl_i / ctl_d.  No device."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from midastouch_amd import _lib  # noqa: E402
from midastouch_amd.loop_engine import annealing_block, particles_block  # noqa: E402

CAP = 64
KEPT = (_lib.LOOP_I_INIT, _lib.LOOP_I_VARSET, _lib.LOOP_I_FRAME)
COUNTS = (_lib.LOOP_I_N, _lib.LOOP_I_NSET, _lib.LOOP_I_NCL)


def _old(lead):
    """A block with every word set and different: word k of row r holds 100 (r + 1) + k."""
    rows = int(np.prod(lead, dtype=np.int64))
    return (100 * (torch.arange(rows, dtype=torch.int32)[:, None] + 1) + torch.arange(32, dtype=torch.int32)).reshape(lead + (32,))


def _expect(n, ncl, old=None):
    e = torch.zeros(32, dtype=torch.int32)
    e[_lib.LOOP_I_N] = e[_lib.LOOP_I_NSET] = n
    e[_lib.LOOP_I_NCL] = ncl
    if old is not None:
        for k in KEPT:
            e[k] = old[k]
    return e


@pytest.mark.parametrize("n", [1, CAP])
@pytest.mark.parametrize("reset", [True, False])
def test_particles_block_single(n, reset):
    old = _old(())
    for labels, ncl in ((None, 1), (torch.tensor([0, 4, 2]), 5)):
        ncl_in = 1 if labels is None else int(labels.max()) + 1
        ci = particles_block(n, ncl_in, None if reset else old, reset)
        assert ci.shape == (32,) and ci.dtype == torch.int32 and ci.device.type == "cpu"
        assert torch.equal(ci, _expect(n, ncl, None if reset else old))
    assert torch.equal(old, _old(()))  # the old block is read, not written


@pytest.mark.parametrize("reset", [True, False])
def test_particles_block_batch(reset):
    old = _old((3,))
    ns, ncl = [1, CAP, 17], [1, 5, 2]
    ci = particles_block(ns, ncl, None if reset else old, reset)
    assert ci.shape == (3, 32) and ci.dtype == torch.int32
    for b in range(3):  # every row is its own trajectory's block
        assert torch.equal(ci[b], _expect(ns[b], ncl[b], None if reset else old[b])), b
        assert torch.equal(ci[b], particles_block(ns[b], ncl[b], None if reset else old[b], reset)), b


def test_particles_block_reset_needs_no_old_block():
    """Annealing starts over: INIT, VARSET and FRAME are zero whatever the old block held (and it is not asked for)."""
    for old in (None, _old(())):
        ci = particles_block(5, 1, old, True)
        assert not ci[list(KEPT)].any()
        assert int(ci.sum()) == 5 + 5 + 1


def _state(lead):
    rows = int(np.prod(lead, dtype=np.int64))
    cd = (0.5 + torch.arange(rows * 16, dtype=torch.float64)).reshape(lead + (16,))
    return _old(lead), cd


def test_annealing_block_single():
    f32 = float(np.float32(0.1))
    assert f32 != 0.1
    for var, varset, prev in ((float("inf"), 0, 0.0), (0.1, 1, f32)):
        ci0, cd0 = _state(())
        ci, cd = annealing_block(ci0.clone(), cd0.clone(), var, 4321)
        assert ci.dtype == torch.int32 and cd.dtype == torch.float64
        assert int(ci[_lib.LOOP_I_VARSET]) == varset and int(ci[_lib.LOOP_I_INIT]) == 4321
        assert float(cd[_lib.LOOP_D_VARPREV]) == prev
        other_i = [k for k in range(32) if k not in (_lib.LOOP_I_VARSET, _lib.LOOP_I_INIT)]
        other_d = [k for k in range(16) if k != _lib.LOOP_D_VARPREV]
        assert torch.equal(ci[other_i], ci0[other_i]) and torch.equal(cd[other_d], cd0[other_d])


def test_annealing_block_batch_rows_are_independent():
    f32 = float(np.float32(0.1))
    ci0, cd0 = _state((3,))
    pv, ip = [0.1, float("inf"), 2.5], [64, 1, 1000]
    ci, cd = annealing_block(ci0.clone(), cd0.clone(), pv, ip)
    assert ci[:, _lib.LOOP_I_VARSET].tolist() == [1, 0, 1]
    assert ci[:, _lib.LOOP_I_INIT].tolist() == ip
    assert cd[:, _lib.LOOP_D_VARPREV].tolist() == [f32, 0.0, 2.5]
    for b in range(3):  # row b is what the single call makes of row b
        si, sd = annealing_block(ci0[b].clone(), cd0[b].clone(), pv[b], ip[b])
        assert torch.equal(ci[b], si) and torch.equal(cd[b], sd), b
    other_i = [k for k in range(32) if k not in (_lib.LOOP_I_VARSET, _lib.LOOP_I_INIT)]
    other_d = [k for k in range(16) if k != _lib.LOOP_D_VARPREV]
    assert torch.equal(ci[:, other_i], ci0[:, other_i]) and torch.equal(cd[:, other_d], cd0[:, other_d])
