"""BatchLoopEngine's state handling: the scratch reserved at construction holds every frame (no frame allocates), and a
`set_particles` call that is refused leaves the engine as it was."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def test_batch_loop_no_frame_allocates(dev):
    """The largest batch of the largest sets the tests can afford - 64 trajectories of MIDAS_LOOP_BATCH_MAX_CAP particles, where
    the per-trajectory part of the reservation (~118 MB) exceeds the slack the cell tables' round figure leaves - through a
    DBSCAN frame and two plain ones with ground truth (every phase, the RMSE partials included): MIDAS_SCRATCH_LOG reports every
    allocation on stderr, and after the constructor there is none.  (The switch is read once per process: a child process.)"""
    code = (
        "import sys, numpy as np, torch\n"
        "from midastouch_amd import BatchLoopEngine, _lib\n"
        "from midastouch_amd.synthetic import make_codebook, make_trajectory\n"
        "dev = torch.device('cuda', 0)\n"
        "B, cap = 64, _lib.LOOP_BATCH_MAX_CAP\n"
        "cb = make_codebook(K=3000, D=256, seed=1013, mesh_points=20000)\n"
        "tr = make_trajectory(cb, T=4, seed=2000)\n"
        "eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, cap, seed=4000, device=dev)\n"
        "sys.stderr.write('MARK\\n'); sys.stderr.flush()\n"
        "rng = np.random.default_rng(0)\n"
        "eng.set_particles(torch.as_tensor(cb.poses[rng.integers(0, 3000, (B, cap))]))\n"
        "for t in range(3):\n"
        "    rep = lambda a: torch.as_tensor(a[t + 1])[None].repeat(B, *([1] * a[t + 1].ndim)).contiguous()\n"
        "    eng.step(rep(tr.odoms), rep(tr.codes), gts=rep(tr.gt_poses))\n"
        "torch.cuda.synchronize()\n"
        "print('DONE', min(eng.n), max(eng.n))\n")
    env = dict(os.environ, MIDAS_SCRATCH_LOG="1", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "DONE" in r.stdout
    before, after = r.stderr.split("MARK")
    assert "reserved one chunk" in before and "[midas] scratch" not in after, r.stderr


def test_batch_loop_refused_set_particles_changes_nothing(dev):
    """A label set of the wrong length for the LAST trajectory is refused before anything is copied: poses, labels, hints and
    control blocks of every trajectory are what they were, and the engine steps on as if the call had not been made."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd._lib import MidasError
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    cb = make_codebook(K=3000, D=256, seed=1013, mesh_points=20000)
    tr = make_trajectory(cb, T=3, seed=2001)
    rng = np.random.default_rng(1)
    B, cap = 3, 700
    eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, cap, seed=4100, floor=100, device=dev)
    eng.set_particles([torch.as_tensor(cb.poses[rng.integers(0, 3000, n)]) for n in (700, 65, 300)])
    rep = lambda a: torch.as_tensor(a)[None].repeat(B, *([1] * a.ndim)).contiguous()  # noqa: E731
    eng.step(rep(tr.odoms[1]), rep(tr.codes[1]))
    state = lambda: [x.clone() for x in (eng._poses, eng._labels, eng._hint, eng.ctl_i, eng.ctl_d)]  # noqa: E731
    before, n_before = state(), list(eng.n)
    other = [torch.as_tensor(cb.poses[rng.integers(0, 3000, n)]) for n in (10, 20, 30)]
    with pytest.raises(MidasError):
        eng.set_particles(other, labels=[torch.zeros(10), torch.zeros(20), torch.zeros(31)])
    with pytest.raises(MidasError):
        eng.set_particles(other, labels=[torch.zeros(10), torch.zeros(20)])
    with pytest.raises(MidasError):
        eng.set_particles(other[:2] + [torch.as_tensor(cb.poses[rng.integers(0, 3000, cap + 1)])])
    for x, y in zip(before, state()):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert eng.n == n_before
    eng.step(rep(tr.odoms[2]), rep(tr.codes[2]))
    assert all(rec[0]["err"] == 0 for rec in eng.read_log(1, 2, strict=False))
