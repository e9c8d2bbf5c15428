"""The codebook's float64 self-similarity on the matrix cores (midas_selfsim_panel_f64 / midas_selfsim_topn_f64,
k_selfsim_mfma_f64): panels bit-identical to midas_score and to the summation spec (oracle.score_codebook) for both layouts,
float32 and float64 codebooks, ragged panels and adversarial rows; top_n_error(fast=True, precision="f64") equal to the default
exact form (errors and indices) and to the reference's fixture G12; confusion_matrix against the float64 scores and against
the reference's function.  Needs an MI355X."""
import numpy as np
import pytest

from _recipes import sha

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


def make_emb(K, D, dtype, seed):
    """(K, D) embeddings with adversarial rows up front: zero and negative-zero rows (the norm clamp), a tiny row (its squared
    norm underflows; subnormal products against the others), a huge row (near overflow), a cancellation-heavy pair, a duplicate
    row (exact ties)."""
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((K, D))
    f64 = dtype == np.float64
    alt = np.where(np.arange(D) % 2 == 0, 1.0, -1.0)
    rows = [np.zeros(D), -np.zeros(D), E[2 % K] * (1e-300 if f64 else 1e-30), E[3 % K] * (1e150 if f64 else 1e30),
            alt * 1e8 + rng.standard_normal(D), alt * (1.0 + 1e-9 * rng.standard_normal(D)), E[7 % K] * (1e-160 if f64 else 1e-20)]
    for r, v in enumerate(rows[:K - 1]):  # (one row stays random: a float64 codebook keeps a value float32 cannot hold)
        E[r] = v
    if K > 12:
        E[12] = E[9]  # a duplicate: equal similarities everywhere
    return E.astype(dtype)


def check_panel(ops, oracle, dev, E, i0, R, oracle_rows=8):
    cbk = ops.Codebook(T(E, dev))
    assert cbk.emb.dtype == (torch.float64 if E.dtype == np.float64 else torch.float32)
    got = cbk.self_similarity(i0, R).cpu().numpy()
    assert got.shape == (R, E.shape[0])
    gemv = cbk.score(cbk.emb[i0:i0 + R].to(torch.float64)).cpu().numpy()
    bad = np.argwhere(bits(got) != bits(gemv))
    assert bad.size == 0, f"{len(bad)} values differ from midas_score, first (row, entry) {bad[:5].tolist()}: " \
                          f"{got[tuple(bad[0])]!r} vs {gemv[tuple(bad[0])]!r}"
    pick = sorted(set([0, R - 1] + list(range(0, R, max(1, R // oracle_rows)))))
    ref = np.stack([oracle.score_codebook(E, E[i0 + r].astype(np.float64)) for r in pick])
    assert np.array_equal(bits(got[pick]), bits(ref))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", [1, 3, 100, 128, 256, 512, 1024, 1100])
def test_panel_bitwise_every_layout(dev, ops, oracle, D, dtype):
    E = make_emb(1037, D, dtype, seed=D)
    check_panel(ops, oracle, dev, E, 0, 1037)


@pytest.mark.parametrize("K,i0,R", [(1, 0, 1), (2, 1, 1), (17, 3, 13), (70, 33, 37), (999, 517, 301), (5000, 2049, 2951)])
@pytest.mark.parametrize("D,dtype", [(256, np.float32), (100, np.float64), (512, np.float64), (48, np.float32)],
                         ids=["reg-f32", "strided-f64", "reg-f64", "strided-f32"])
def test_panel_ragged(dev, ops, oracle, K, i0, R, D, dtype):
    E = make_emb(K, D, dtype, seed=K + D)
    check_panel(ops, oracle, dev, E, i0, R, oracle_rows=4)


def test_panel_unaligned_codebook(dev, ops):
    """A float64 codebook view that is not 16-byte aligned: midas_score takes the strided layout for it (the spec's D = 256 order
    is the register layout: not these bits), and so must the panel."""
    E = make_emb(301, 256, np.float64, seed=3)
    base = torch.zeros(301 * 256 + 1, dtype=torch.float64, device=dev)
    view = base[1:].view(301, 256)
    view.copy_(T(E, dev))
    cbk = ops.Codebook(view)
    assert cbk.emb.data_ptr() % 16 != 0
    got = cbk.self_similarity().cpu().numpy()
    gemv = cbk.score(cbk.emb).cpu().numpy()
    assert np.array_equal(bits(got), bits(gemv))


# ---- top_n_error ----------------------------------------------------------------------------------------------------------------
def topn_case(K, D, dtype, seed):
    E = make_emb(K, D, dtype, seed)
    rng = np.random.default_rng(seed + 1)
    poses = rng.standard_normal((K, 3)) * 0.05
    return E, poses


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", [100, 256])
@pytest.mark.parametrize("K,n", [(20, 1), (20, 25), (20, 256), (700, 7), (700, 256), (2500, 25), (5000, 1), (5000, 25)])
def test_topn_equals_default(dev, K, n, D, dtype):
    from midastouch_amd.single_touch import top_n_error
    E, poses = topn_case(K, D, dtype, seed=K * 3 + n + D)
    emb, pz = T(E, dev), T(poses, dev)
    ref_err, ref_idx = top_n_error(emb, pz, n=n, want_idx=True)
    rows = -(-K // 3)  # three panels: both buffers and the hand-over between the streams
    err, idx = top_n_error(emb, pz, n=n, fast=True, precision="f64", want_idx=True, panel_rows=rows)
    assert np.array_equal(bits(err.cpu().numpy()), bits(ref_err.cpu().numpy()))
    assert np.array_equal(idx.cpu().numpy(), ref_idx.cpu().numpy())
    if n > K:
        assert (idx.cpu().numpy()[:, K:] == -1).all()
    # the default panel size (one panel here) and a repeat run: the same bits
    err2, idx2 = top_n_error(emb, pz, n=n, fast=True, precision="f64", want_idx=True)
    assert np.array_equal(bits(err2.cpu().numpy()), bits(err.cpu().numpy()))
    assert np.array_equal(idx2.cpu().numpy(), idx.cpu().numpy())
    err3 = top_n_error(emb, pz, n=n, fast=True, precision="f64", panel_rows=rows)
    assert np.array_equal(bits(err3.cpu().numpy()), bits(err.cpu().numpy()))


def test_topn_matches_reference_fixture(dev, golden):
    """G12 (eval/single_touch_test.top_n_error outputs written by the reference) through the float64 matrix-core path, with the
    assertions of the default path's fixture test."""
    from midastouch_amd.single_touch import top_n_error
    from midastouch_amd.synthetic import make_codebook
    g = golden("g12_topn")
    for tag in ("a", "b", "c"):
        K, D, n = int(g[f"{tag}_K"]), int(g[f"{tag}_D"]), int(g[f"{tag}_n"])
        cb = make_codebook(K=K, D=D, seed=int(g[f"{tag}_seed"]), mesh_points=2000)
        assert sha(cb.embeddings.astype(np.float32)) == str(g[f"{tag}_emb_sha"])
        poses = cb.poses[:, :3, 3].astype(np.float64)
        emb, pz = torch.as_tensor(cb.embeddings).to(dev), torch.as_tensor(poses).to(dev)
        err = top_n_error(emb, pz, n=n, fast=True, precision="f64", panel_rows=max(1, K // 3)).cpu().numpy()
        assert np.array_equal(bits(err), bits(top_n_error(emb, pz, n=n).cpu().numpy()))
        ref = g[f"{tag}_err"]
        same = np.isclose(err, ref, rtol=1e-12, atol=1e-15)
        assert same.mean() > 0.995, (tag, same.mean())
        X = cb.embeddings.astype(np.float64)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        C = X @ X.T
        np.fill_diagonal(C, 0)
        srt = -np.sort(-C, axis=1)
        clear = (srt[:, n - 1] - srt[:, n]) > 1e-12
        assert same[clear].all(), tag


# ---- confusion_matrix -----------------------------------------------------------------------------------------------------------
def reference_confusion(X, sz, batch_size):
    """modules/misc.py:78-108 restated in numpy: sklearn's cosine_similarity (rows scaled to unit norm, zero rows kept) in
    batch blocks, then (C - min) / ptp."""
    X = np.asarray(X, dtype=np.float64)[:sz]
    nrm = np.sqrt(np.einsum("ij,ij->i", X, X))
    nrm[nrm == 0.0] = 1.0
    Xn = X / nrm[:, None]
    C = np.full((sz, sz), np.nan)
    nb = sz // batch_size
    if nb == 0:
        C = Xn @ Xn.T
    else:
        for i in range(nb):
            ir = np.arange(i * batch_size, sz if i == nb - 1 else (i + 1) * batch_size)
            for j in range(nb):
                jr = np.arange(j * batch_size, sz if j == nb - 1 else (j + 1) * batch_size)
                C[ir[:, None], jr] = Xn[ir] @ Xn[jr].T
    return (C - np.min(C)) / np.ptp(C)


@pytest.mark.parametrize("K,sz,batch_size,D,dtype", [(300, 64, 100, 256, np.float32), (300, 250, 100, 100, np.float64),
                                                      (1037, 1037, 100, 128, np.float32), (700, 333, 64, 3, np.float64)])
def test_confusion_matrix(dev, ops, K, sz, batch_size, D, dtype):
    from midastouch_amd.single_touch import confusion_matrix
    rng = np.random.default_rng(K + sz)
    E = rng.standard_normal((K, D)).astype(dtype)
    E[5] = 0.0
    got = confusion_matrix(T(E, dev), sz, batch_size=batch_size)
    assert got.dtype == torch.float64 and got.shape == (sz, sz) and got.is_cuda
    got = got.cpu().numpy()
    cbk = ops.Codebook(T(E[:sz], dev))
    S = cbk.score(cbk.emb.to(torch.float64)).cpu().numpy()
    assert np.array_equal(bits(got), bits((S - S.min()) / (S.max() - S.min())))
    np.testing.assert_allclose(got, reference_confusion(E, sz, batch_size), rtol=0, atol=1e-12)
    assert np.array_equal(bits(confusion_matrix(T(E, dev), sz, batch_size=7).cpu().numpy()), bits(got))


def test_confusion_matrix_constant(dev):
    """ptp = 0: numpy's 0 / 0 = NaN everywhere."""
    from midastouch_amd.single_touch import confusion_matrix
    E = np.ones((5, 16), dtype=np.float32)
    got = confusion_matrix(T(E, dev)).cpu().numpy()
    assert np.isnan(got).all()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(dev, ops):
    from midastouch_amd._lib import MidasError
    from midastouch_amd.single_touch import confusion_matrix, top_n_error
    E, poses = topn_case(100, 64, np.float32, 0)
    emb, pz = T(E, dev), T(poses, dev)
    for n in (0, 257):
        with pytest.raises(MidasError):
            top_n_error(emb, pz, n=n, fast=True, precision="f64")
    with pytest.raises(MidasError):
        top_n_error(emb, T(np.zeros((100, 17)), dev), fast=True, precision="f64")  # d > 16
    with pytest.raises(MidasError):
        top_n_error(torch.as_tensor(E), torch.as_tensor(poses), fast=True, precision="f64")  # CPU tensors
    with pytest.raises(MidasError):
        top_n_error(emb, pz, fast=True, precision="f16")
    with pytest.raises(MidasError):
        top_n_error(emb, pz, precision="bf16")
    with pytest.raises(MidasError):
        confusion_matrix(torch.as_tensor(E))
    with pytest.raises(MidasError):
        confusion_matrix(emb, sz=101)
    cbk = ops.Codebook(emb)
    with pytest.raises(MidasError):
        cbk.self_similarity(90, 11)
    with pytest.raises(MidasError):
        cbk.self_similarity(0, 0)
