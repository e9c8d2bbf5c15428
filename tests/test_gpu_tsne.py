"""One-dimensional t-SNE on the device (midastouch_amd/tsne.py, csrc/tsne.hip) against sklearn 1.7's TSNE pieces: the kNN, the
perplexity search, the joint P, the exact gradient, the optimiser (bit for bit against sklearn's own _gradient_descent), the
initialisations, end-to-end quality, colours and the error cases.  DESIGN.md 4.6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _sk(name):
    t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    utils = pytest.importorskip("sklearn.manifold._utils")
    for mod in (t_sne, utils):
        if hasattr(mod, name):
            return getattr(mod, name)
    raise AssertionError(f"sklearn.manifold no longer has {name}")


def _codebook(K, D, seed=1):
    from midastouch_amd.synthetic import make_codebook

    return np.asarray(make_codebook(K=K, D=D, seed=seed).embeddings)


def _blobs(K, F, seed=0):
    from sklearn.datasets import make_blobs

    X, _ = make_blobs(n_samples=K, n_features=F, centers=8, cluster_std=2.0, random_state=seed)
    return X


def _sk_knn(X64, k):
    from sklearn.neighbors import NearestNeighbors

    G = NearestNeighbors(n_neighbors=k).fit(X64).kneighbors_graph(mode="distance")
    G.data **= 2
    return G


def _exact_kl(P, y):
    """One host evaluator: sum p_ij log(p_ij / (q_ij / Z)) over P's nonzeros, float64, the exact Z."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    P = P.tocoo()
    d = y[:, None] - y[None, :]
    q = 1.0 / (1.0 + d * d)
    np.fill_diagonal(q, 0.0)
    Z = q.sum()
    qq = q[P.row, P.col] / Z
    return float(np.sum(P.data * np.log(np.maximum(P.data, 1e-300) / np.maximum(qq, 1e-300))))


def _grad64(P, y, ex=1.0):
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    P = P.tocoo()
    K = y.shape[0]
    d = y[:, None] - y[None, :]
    q = 1.0 / (1.0 + d * d)
    np.fill_diagonal(q, 0.0)
    Z = q.sum()
    pos = np.zeros(K)
    pv = (P.data * ex).astype(np.float32).astype(np.float64)
    np.add.at(pos, P.row, pv * q[P.row, P.col] * (y[P.row] - y[P.col]))
    neg = (q * q * d).sum(1)
    grad = 4.0 * (pos - neg / Z)
    kl = float(np.sum(pv * np.log(np.maximum(pv, 1.1754944e-38) / np.maximum(q[P.row, P.col] / Z, 1.1754944e-38))))
    return grad, kl


# ---- kNN -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,F", [(2, 3), (50, 64), (122, 256), (1000, 1000), (5000, 3), (1000, 2000), (5000, 64)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_knn_against_sklearn(K, F, dtype):
    from midastouch_amd import tsne

    rng = np.random.default_rng(K * 7 + F)
    X = (rng.standard_normal((K, F)) if F != 256 else _codebook(K, F)).astype(dtype)
    k = min(K - 1, 121)
    idx, d2 = tsne.knn(torch.as_tensor(X, device=DEV), k)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    X64 = X.astype(np.float64)
    G = _sk_knn(X64, k)
    nrm = (X64 * X64).sum(1)
    for i in range(K):
        row = slice(G.indptr[i], G.indptr[i + 1])
        sk = dict(zip(G.indices[row], G.data[row]))
        assert set(idx[i]) == set(sk), f"row {i}: neighbour sets differ"
        assert np.all(np.diff(d2[i]) >= 0), f"row {i}: not ascending"
        ref = np.array([sk[j] for j in idx[i]])
        tol = 1e-9 * np.abs(ref) + 1e-12 * (nrm[i] + nrm[idx[i]])
        assert np.all(np.abs(d2[i] - ref) <= tol), f"row {i}: distances differ"


def test_knn_strided_view_and_duplicates():
    from midastouch_amd import tsne

    rng = np.random.default_rng(5)
    W = rng.standard_normal((600, 130))
    W[17] = W[3]
    W[250] = W[3]
    W[40] = W[41]
    Xt = torch.as_tensor(W, device=DEV)[:, 1:101]  # row stride 130, 100 columns
    assert not Xt.is_contiguous()
    k = 31
    idx, d2 = tsne.knn(Xt, k)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    X = W[:, 1:101]
    G = _sk_knn(X, k)
    dups = {3, 17, 250, 40, 41}
    for i in range(600):
        assert i not in set(idx[i])
        if i not in dups:  # (sklearn's own self-removal can keep a duplicated row itself and drop its twin)
            # copies of one point tie exactly; at the k-th place the device takes the smallest index, sklearn any of them
            canon = {17: 3, 250: 3, 41: 40}
            ours = sorted(canon.get(int(j), int(j)) for j in idx[i])
            ref = sorted(canon.get(int(j), int(j)) for j in G.indices[G.indptr[i]:G.indptr[i + 1]])
            assert ours == ref, f"row {i}"
    for i, j in ((3, 17), (3, 250), (17, 3), (40, 41), (41, 40)):
        assert idx[i][0] in (j, 3, 17, 250) and d2[i][0] == 0.0 and j in set(idx[i])
    assert list(idx[3][:2]) == [17, 250]  # zero-distance ties by index


def test_knn_confusion_matrix_route():
    from midastouch_amd import single_touch, tsne

    E = torch.as_tensor(_codebook(1500, 512), device=DEV)
    Cm = single_touch.confusion_matrix(E)
    idx, d2 = tsne.knn(Cm, 121)
    G = _sk_knn(Cm.cpu().numpy(), 121)
    idx = idx.cpu().numpy()
    same = sum(set(idx[i]) == set(G.indices[G.indptr[i]:G.indptr[i + 1]]) for i in range(1500))
    assert same == 1500


# ---- affinities ------------------------------------------------------------------------------------------------------------

def _sorted_rows(idx, d2):
    order = np.argsort(idx, axis=1)
    return np.take_along_axis(idx, order, 1), np.take_along_axis(d2, order, 1)


@pytest.mark.parametrize("perplexity", [5.0, 30.0, 40.0, 50.0])
def test_conditional_p_against_binary_search(perplexity):
    from midastouch_amd import tsne

    bsp = _sk("_binary_search_perplexity")
    X = _codebook(3000, 64)
    k = tsne.n_neighbors(3000, perplexity)
    idx, d2 = tsne.knn(torch.as_tensor(X, device=DEV), k)
    cols, ds = _sorted_rows(idx.cpu().numpy(), d2.cpu().numpy())
    d32 = ds.astype(np.float32)
    ref = bsp(d32, perplexity, 0)
    got = tsne.conditional_affinities(torch.as_tensor(d32, device=DEV), perplexity).cpu().numpy()
    bad = [i for i in range(3000) if not np.allclose(got[i], ref[i], rtol=1e-9, atol=0)]
    if bad:  # a last-ulp exp difference can flip one bisection step of a row; say which
        print(f"perplexity {perplexity}: rows off at rtol 1e-9: {bad}")
    assert len(bad) <= 3
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-12)


@pytest.mark.parametrize("perplexity", [5.0, 40.0])
def test_joint_p_against_sklearn(perplexity):
    from scipy.sparse import csr_matrix

    from midastouch_amd import tsne

    jp = _sk("_joint_probabilities_nn")
    X = _blobs(2000, 32)
    k = tsne.n_neighbors(2000, perplexity)
    idx, d2 = tsne.knn(torch.as_tensor(X, device=DEV), k)
    _, _, P = tsne.affinities(idx, d2, perplexity)
    i_np, d_np = idx.cpu().numpy(), d2.cpu().numpy()
    D = csr_matrix((d_np.ravel(), i_np.ravel().astype(np.int64), np.arange(0, 2000 * k + 1, k)), shape=(2000, 2000))
    ref = jp(D, perplexity, 0)
    ref.sort_indices()
    got = P.to_scipy()
    assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
    np.testing.assert_allclose(got.data, ref.data, rtol=1e-9, atol=0)


# ---- gradient and KL -------------------------------------------------------------------------------------------------------

def _graph(X, perplexity):
    from midastouch_amd import tsne

    k = tsne.n_neighbors(X.shape[0], perplexity)
    idx, d2 = tsne.knn(torch.as_tensor(X, device=DEV), k)
    return tsne.affinities(idx, d2, perplexity)[2]


@pytest.mark.parametrize("K", [3, 500, 3000])
@pytest.mark.parametrize("ex", [1.0, 12.0])
def test_gradient_exact(K, ex):
    from midastouch_amd import tsne

    kl_bh = _sk("_kl_divergence_bh")
    X = _blobs(K, 16, seed=K)
    P = _graph(X, 1.0 if K == 3 else 30.0)
    rng = np.random.default_rng(K)
    y = (rng.standard_normal(K) * 3.0).astype(np.float32)
    kl, g = tsne.gradient(P, torch.as_tensor(y, device=DEV), ex)
    g = g.cpu().numpy()
    g64, kl64 = _grad64(P.to_scipy(), y, ex)
    assert np.max(np.abs(g - g64)) <= 1e-5 * np.max(np.abs(g64))
    assert abs(kl - kl64) <= 1e-5 * abs(kl64) + 1e-12
    Ps = P.to_scipy()
    Ps.data *= ex
    e_bh, g_bh = kl_bh(y.reshape(-1, 1).copy(), Ps, 1, K, 1, angle=0.0, compute_error=True)
    np.testing.assert_allclose(g, g_bh, rtol=1e-4, atol=1e-4 * np.max(np.abs(g_bh)))
    assert abs(kl - e_bh) <= 1e-4 * abs(e_bh) + 1e-9


# ---- the optimiser, bit for bit --------------------------------------------------------------------------------------------

def _sklearn_schedule(P, y0, min_grad_norm, max_iter=1000):
    """TSNE._tsne's two _gradient_descent calls, with the device gradient as the objective."""
    from midastouch_amd import tsne

    gd = _sk("_gradient_descent")
    K = P.K
    Ps = P.to_scipy()

    def obj(p, Pm, dof, n, nc, compute_error=True, **kw):
        Pj = tsne.JointP(P.crow, P.col, torch.as_tensor(Pm.data, device=DEV), K)
        kl, g = tsne.gradient(Pj, torch.as_tensor(p, device=DEV))
        return (kl if compute_error else 0.0), g.cpu().numpy()

    lr = tsne.auto_learning_rate(K)
    opt = dict(it=0, n_iter_check=50, min_grad_norm=min_grad_norm, learning_rate=lr, verbose=0, kwargs={},
               args=[Ps, 1, K, 1], n_iter_without_progress=250, max_iter=250, momentum=0.5)
    Ps *= 12.0
    p, err, it = gd(obj, y0.copy(), **opt)
    Ps /= 12.0
    opt.update(max_iter=max_iter, it=it + 1, momentum=0.8, n_iter_without_progress=300)
    p, err, it = gd(obj, p, **opt)
    return p, err, it


@pytest.mark.parametrize("min_grad_norm", [1e-7, 1.0])
def test_optimizer_bitwise_against_gradient_descent(min_grad_norm):
    from midastouch_amd import tsne

    K = 500
    P = _graph(_codebook(K, 64), 40.0)
    y0 = tsne.random_init(K, 0).numpy()
    p_ref, err_ref, it_ref = _sklearn_schedule(P, y0, min_grad_norm)
    y, err, it, _ = tsne.optimize(P, torch.as_tensor(y0, device=DEV), min_grad_norm=min_grad_norm)
    assert it == it_ref
    assert err == err_ref
    assert np.array_equal(y.cpu().numpy().view(np.uint32), p_ref.astype(np.float32).view(np.uint32))
    if min_grad_norm == 1.0:
        assert it_ref < 999  # both stages stopped at their first check


# ---- initialisation --------------------------------------------------------------------------------------------------------

def test_init_random_bitwise():
    from sklearn.utils import check_random_state

    from midastouch_amd import tsne

    ref = 1e-4 * check_random_state(0).standard_normal(size=(777, 1)).astype(np.float32)
    got = tsne.random_init(777, 0).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_init_pca_against_sklearn(dtype):
    from sklearn.decomposition import PCA

    from midastouch_amd import tsne

    rng = np.random.default_rng(3)
    X = (rng.standard_normal((1200, 80)) * np.r_[8.0, 2.0, np.ones(78)] + 5.0).astype(dtype)
    ref = PCA(n_components=1, svd_solver="randomized", random_state=0).fit_transform(X).astype(np.float32, copy=False)
    ref = (ref / np.std(ref[:, 0]) * 1e-4)[:, 0]
    got = tsne.pca_init(torch.as_tensor(X, device=DEV)).cpu().numpy()
    assert got.dtype == np.float32
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.max(np.abs(ref)))


def test_init_pca_identical_rows_raise():
    from midastouch_amd import tsne
    from midastouch_amd.ops import MidasError

    X = torch.ones((300, 8), dtype=torch.float64, device=DEV)
    with pytest.raises(MidasError):
        tsne.pca_init(X)


# ---- end to end ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,D,route", [(500, 64, "emb"), (2000, 64, "emb"), (2000, 256, "emb"), (2000, 512, "confusion")])
def test_end_to_end_quality_against_sklearn(K, D, route):
    from sklearn.manifold import TSNE, trustworthiness

    from midastouch_amd import single_touch, tsne

    jp = _sk("_joint_probabilities_nn")
    E = torch.as_tensor(_codebook(K, D, seed=K + D), device=DEV)
    Xt = single_touch.confusion_matrix(E) if route == "confusion" else E
    X = Xt.cpu().numpy().astype(np.float64)
    y_sk = TSNE(n_components=1, perplexity=40, init="pca", random_state=0).fit_transform(X)[:, 0]
    y, info = tsne.tsne_1d(Xt, return_info=True)
    y = y.cpu().numpy()
    P = jp(_sk_knn(X, tsne.n_neighbors(K, 40.0)), 40.0, 0)
    kl_dev, kl_sk = _exact_kl(P, y), _exact_kl(P, y_sk)
    print(f"K {K} D {D} {route}: KL device {kl_dev:.5f} sklearn {kl_sk:.5f}, n_iter {info['n_iter']}")
    assert kl_dev <= 1.05 * kl_sk
    t_dev = trustworthiness(X, y[:, None], n_neighbors=10)
    t_sk = trustworthiness(X, y_sk[:, None], n_neighbors=10)
    assert t_dev >= t_sk - 0.01


def test_determinism():
    from midastouch_amd import tsne

    X = torch.as_tensor(_codebook(1500, 128), device=DEV)
    a = tsne.tsne_1d(X).cpu().numpy()
    b = tsne.tsne_1d(X).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- colours ---------------------------------------------------------------------------------------------------------------

def test_color_tsne_is_spectral_of_the_embedding():
    import matplotlib

    from midastouch_amd import single_touch, tsne

    X = torch.as_tensor(_codebook(800, 64), device=DEV)
    y = tsne.tsne_1d(X, nan_to_num=True).cpu().numpy()
    enc = (y - np.min(y)) / (np.max(y) - np.min(y))
    ref = matplotlib.colormaps["Spectral"](enc)[:, :3]
    got = single_touch.color_tsne(X).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, ref)


def test_codebook_colors_routes():
    from midastouch_amd import single_touch

    E = torch.as_tensor(_codebook(700, 512), device=DEV)
    got = single_touch.codebook_colors(E)
    assert torch.equal(got, single_touch.color_tsne(single_touch.confusion_matrix(E), "pca"))
    E2 = torch.as_tensor(_codebook(700, 64), device=DEV)
    assert torch.equal(single_touch.codebook_colors(E2), single_touch.color_tsne(E2, "pca"))
    assert single_touch.codebook_colors(E, sz=400).shape == (400, 3)


def test_color_tsne_nan_to_num_and_input_untouched():
    from midastouch_amd import single_touch

    # float32: nan_to_num's +-FLT_MAX squares finitely in float64 (float64 infinities become +-DBL_MAX, whose squares overflow -
    # there sklearn fails as well)
    for dtype, with_inf in ((torch.float32, True), (torch.float64, False)):
        C = torch.as_tensor(_codebook(600, 64), device=DEV).to(dtype)
        C[5, 3] = float("nan")
        C[250, :] = float("nan")
        if with_inf:
            C[17, 0] = float("inf")
            C[100, 10] = -float("inf")
        before = C.clone()
        got = single_touch.color_tsne(C)
        assert torch.equal(torch.isnan(C), torch.isnan(before)) and torch.equal(torch.nan_to_num(C), torch.nan_to_num(before))
        ref = single_touch.color_tsne(torch.nan_to_num(before))
        assert torch.equal(got, ref)
        assert bool(torch.isfinite(got).all())


# ---- full size -------------------------------------------------------------------------------------------------------------

def test_full_size_codebook_colors_50k():
    import time

    from midastouch_amd import single_touch, tsne

    E = torch.as_tensor(_codebook(50000, 512, seed=7), device=DEV)
    t0 = time.perf_counter()
    colors = single_touch.codebook_colors(E)
    torch.cuda.synchronize()
    print(f"codebook_colors K 50000 D 512: {time.perf_counter() - t0:.1f} s")
    c = colors.cpu().numpy()
    assert c.shape == (50000, 3) and np.all(np.isfinite(c)) and c.min() >= 0.0 and c.max() <= 1.0
    # the same stages by hand, for the KL of the initial embedding
    Cm = single_touch.confusion_matrix(E)
    idx, d2 = tsne.knn(Cm, 121, nan_to_num=True)
    _, _, P = tsne.affinities(idx, d2, 40.0)
    y0 = tsne.pca_init(Cm, nan_to_num=True)
    kl0, _ = tsne.gradient(P, y0)
    y, kl, it, _ = tsne.optimize(P, y0)
    print(f"K 50000: KL {kl0:.4f} -> {kl:.4f}, n_iter {it}")
    assert kl < kl0 and it > 0
    assert torch.equal(tsne.spectral_colors(y), colors)


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_error_cases():
    from midastouch_amd import tsne
    from midastouch_amd.ops import MidasError

    X = torch.as_tensor(_codebook(100, 64), device=DEV)
    with pytest.raises(MidasError):
        tsne.tsne_1d(X.cpu())
    with pytest.raises(MidasError):
        tsne.tsne_1d(X, perplexity=100.0)
    with pytest.raises(MidasError):
        tsne.tsne_1d(X, perplexity=0.0)
    with pytest.raises(MidasError):
        tsne.tsne_1d(X, perplexity=-3.0)
    with pytest.raises(MidasError):
        tsne.tsne_1d(torch.as_tensor(_codebook(400, 64), device=DEV), perplexity=90.0)  # k = 271 > 256
    with pytest.raises(MidasError):
        tsne.tsne_1d(X[0])
    with pytest.raises(MidasError):
        tsne.knn(X, 300)
