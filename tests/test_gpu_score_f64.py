"""Batched float64 scoring on the matrix cores (midas_score_batch_f64, k_score_mfma_f64): bit-identical to midas_score and to the
summation spec (oracle.score_codebook) for every code, both layouts (D in {128, 256, 512, 1024} and any other D), ragged K and B,
float32 and float64 embeddings, adversarial rows and codes; and the batch engine's dense float64 mode against the float64 oracle
pipeline.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from midastouch_amd import ops as o
    return o


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_case(K, D, B, dtype, seed):
    """(K, D) embeddings of `dtype` and (B, D) float64 codes with the adversarial rows and codes up front: a zero row and code
    (both clamps), negative zeros, a tiny row (its squared norm underflows to the clamp; float64: 1e-300) and a tiny code (subnormal
    products), a huge row, a cancellation-heavy row and code pair, a code equal to a row."""
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((K, D))
    codes = rng.standard_normal((B, D))
    f64 = dtype == np.float64
    alt = np.where(np.arange(D) % 2 == 0, 1.0, -1.0)
    rows = [np.zeros(D), -np.zeros(D), E[2 % K] * (1e-300 if f64 else 1e-30), E[3 % K] * (1e150 if f64 else 1e30),
            alt * 1e8 + rng.standard_normal(D), alt * (1.0 + 1e-9 * rng.standard_normal(D))]
    for r, v in enumerate(rows[:K - 1]):  # (one row stays random: a float64 codebook keeps a value float32 cannot hold)
        E[r] = v
    E = E.astype(dtype)
    cds = [np.zeros(D), -np.zeros(D), codes[2 % B] * (1e-290 if not f64 else 1e-20), alt.copy(), E[min(6, K - 1)].astype(np.float64)]
    for b, v in enumerate(cds[:B]):
        codes[b] = v
    if f64:
        assert not np.array_equal(E.astype(np.float32).astype(np.float64), E)  # ops.Codebook keeps it float64
    return E, codes


def check_bitwise(ops, oracle, dev, K, D, B, dtype, seed):
    E, codes = make_case(K, D, B, dtype, seed)
    cbk = ops.Codebook(T(E, dev))
    assert cbk.emb.dtype == (torch.float64 if dtype == np.float64 else torch.float32)
    got = cbk.score_batch(T(codes, dev), precision="f64").cpu().numpy()
    assert got.shape == (B, K)
    gemv = cbk.score(T(codes, dev)).cpu().numpy()
    ref = np.stack([oracle.score_codebook(E, c) for c in codes])
    assert np.array_equal(bits(gemv), bits(ref)), "midas_score vs the spec (precondition)"
    bad = np.argwhere(bits(got) != bits(ref))
    assert bad.size == 0, f"{len(bad)} scores differ from the spec, first (code, row) {bad[:5].tolist()}: " \
                          f"{got[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]!r}"
    assert np.array_equal(bits(got), bits(gemv))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D,B", [(128, 70), (256, 33), (512, 17), (1024, 15), (1, 16), (17, 129), (48, 64), (100, 1), (640, 33)])
def test_bitwise_every_layout(dev, ops, oracle, D, B, dtype):
    check_bitwise(ops, oracle, dev, 1037, D, B, dtype, seed=D * 7 + B)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 64, 70, 129])
@pytest.mark.parametrize("D,dtype", [(512, np.float32), (100, np.float64)], ids=["reg-f32", "strided-f64"])
def test_bitwise_batch_sizes(dev, ops, oracle, D, dtype, B):
    check_bitwise(ops, oracle, dev, 517, D, B, dtype, seed=B)


@pytest.mark.parametrize("K", [1, 17])
@pytest.mark.parametrize("D", [256, 48])
def test_bitwise_small_codebooks(dev, ops, oracle, K, D):
    check_bitwise(ops, oracle, dev, K, D, 17, np.float64, seed=K + D)
    check_bitwise(ops, oracle, dev, K, D, 5, np.float32, seed=K + D + 1)


def test_bitwise_c5_shape(dev, ops, oracle):
    """K 50 000 x D 512 x B 64 (the batch engine's c5 shape)."""
    check_bitwise(ops, oracle, dev, 50_000, 512, 64, np.float32, seed=5)


def test_golden_g1(dev, ops, golden):
    g = golden("g1_similarity")
    for tag in ("a", "b"):
        cbk = ops.Codebook(T(g[f"{tag}_C"], dev))
        q = T(np.atleast_2d(g[f"{tag}_q"].astype(np.float64)), dev)
        heat = cbk.score_batch(q, precision="f64")[0].cpu().numpy()
        assert np.array_equal(bits(heat), bits(cbk.score(q)[0].cpu().numpy()))
        np.testing.assert_allclose(heat, g[f"{tag}_heat"], rtol=0, atol=1e-14)


def test_errors(dev, ops):
    from midastouch_amd._lib import MidasError
    E, codes = make_case(100, 64, 3, np.float32, 0)
    cbk = ops.Codebook(T(E, dev))
    with pytest.raises(MidasError):
        cbk.score_batch(T(codes, dev), precision="f16")
    with pytest.raises(MidasError):
        cbk.score_batch(T(codes[:0], dev), precision="f64")  # B = 0
    with pytest.raises(MidasError):
        cbk.score_batch(T(codes[:, :63], dev), precision="f64")  # D mismatch
    with pytest.raises(MidasError):
        cbk.set_batch_precision("f16")
    # the float32 form keeps its float32 behaviour (rounded codes: not the float64 bits)
    f32 = cbk.score_batch(T(codes, dev)).cpu().numpy()
    f64 = cbk.score_batch(T(codes, dev), precision="f64").cpu().numpy()
    assert np.array_equal(f64, cbk.score(T(codes, dev)).cpu().numpy()) and not np.array_equal(f32, f64)


# ---- the batch engine's dense float64 mode ------------------------------------------------------------------------------------
def engine_case(D=256, emb64=False, scores="dense_f64", frames=5):
    """BatchFilterEngine(scores=...) against the oracle pipeline with the float64 spec scores (oracle.score_codebook) per
    trajectory: NN indices, resample indices and poses equal, weights bit-identical.  Returns the engine's per-frame state.
    (scores None: the constructor as called before the argument existed.)"""
    from midastouch_amd.engine import BatchFilterEngine
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    from oracle import oracle

    oracle.build()
    dev = torch.device("cuda", 0)
    B, N, K = 5, 1024, 3000
    cb = make_codebook("cotter-pin", K=K, D=D, seed=1004)
    E = cb.embeddings
    if emb64:  # values float32 cannot hold: the codebook stays float64
        E = E.astype(np.float64) * (1.0 + 1e-12 * np.random.default_rng(9).standard_normal(E.shape))
    trajs = [make_trajectory(cb, T=8, seed=2100 + b) for b in range(B)]
    ofl = oracle.OracleFilter(cb.poses, E, cb.mesh_vertices)
    kw = {} if scores is None else {"scores": scores}  # None: the constructor as called before the argument existed
    eng = BatchFilterEngine(cb.poses, E, cb.mesh_vertices, B, N, sig_t=1e-4, sig_r=0.5, seed=4000, device=dev, **kw)
    assert eng.codebook.emb.dtype == (torch.float64 if emb64 else torch.float32)
    # float64 scores on every path taken here: dense_f64; "auto" = sparse per trajectory on a float32 codebook with D in {128, 256,
    # 512, 1024}, the float64 GEMV pass on a float64 codebook
    assert eng.sparse_scores == (scores != "dense_f64" and not emb64 and D in (128, 256, 512, 1024))
    rng = np.random.default_rng(3)
    poses = np.stack([cb.poses[rng.integers(0, K, N)] for _ in range(B)])
    eng.set_particles(torch.as_tensor(poses))
    states = []
    for t in range(1, 1 + frames):
        odoms = torch.as_tensor(np.stack([tr.odoms[t] for tr in trajs])).to(dev)
        codes = torch.as_tensor(np.stack([tr.codes[t] for tr in trajs])).to(dev)
        gts = torch.as_tensor(np.stack([tr.gt_poses[t] for tr in trajs])).to(dev)
        eng.step(odoms, codes, gts)
        states.append([x.cpu().numpy().copy() for x in (eng.nn_idx, eng.ridx, eng.poses, eng.weights, eng.status, eng.rmse)])
        sc = np.stack([oracle.score_codebook(E, c) for c in codes.cpu().numpy()])
        tn_all, rot_all = oracle.philox_noise(B * N, 4000, t - 1, np.float32(1e-4), np.float32(0.5))
        u_all = oracle.philox_uniform64(B * N, 4000, t - 1)
        for b in range(B):
            sl = slice(b * N, (b + 1) * N)
            ref = ofl.step(poses[b], trajs[b].odoms[t], trajs[b].codes[t], tn_all[sl], rot_all[sl], u=u_all[sl], scores=sc[b])
            assert np.array_equal(eng.nn_idx[b].cpu().numpy(), ref["nn_idx"]), (t, b)
            assert np.array_equal(eng.weights[b].cpu().numpy(), ref["weights"]), (t, b)
            assert np.array_equal(eng.ridx[b].cpu().numpy(), ref["ridx"]), (t, b)
            assert np.array_equal(eng.poses[b].cpu().numpy(), ref["poses"]), (t, b)
            poses[b] = ref["poses"]
    return states


def _child(env_extra, call):
    env = dict(os.environ)
    env.pop("MIDAS_OVERLAP", None)
    env.pop("MIDAS_DENSE_SCORES", None)
    env.update(env_extra)
    code = f"import sys; sys.path[:0] = [{REPO!r}, {HERE!r}]; import test_gpu_score_f64 as t; {call}; print('case ok')"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "case ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("overlap", ["0", "1"])
def test_batch_engine_dense_f64_matches_float64_oracle(dev, overlap):
    """Serial form (MIDAS_OVERLAP=0) and side-stream overlap form (1) - the context reads the switch once: a fresh process each."""
    _child({"MIDAS_OVERLAP": overlap}, "t.engine_case()")


def test_batch_engine_dense_f64_float64_codebook(dev):
    engine_case(D=256, emb64=True, frames=3)


def test_batch_engine_dense_f64_strided_layout(dev):
    engine_case(D=100, frames=3)


def test_batch_engine_auto_is_todays_default(dev):
    """scores="auto" (and the constructor without the argument) keeps today's selection: sparse float64 scoring on a float32
    codebook, the float64 GEMV pass on a float64 one - each checked against the float64 oracle pipeline, frame by frame."""
    from midastouch_amd.engine import BatchFilterEngine
    from midastouch_amd._lib import MidasError
    a = engine_case(scores="auto", frames=3)
    b = engine_case(scores=None, frames=3)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert np.array_equal(x, y)
    engine_case(scores="auto", emb64=True, frames=2)
    with pytest.raises(MidasError):
        BatchFilterEngine(np.zeros((4, 4, 4), np.float32), np.zeros((4, 8), np.float32), np.zeros((4, 3)), 2, 16, device=dev,
                          scores="dense")
