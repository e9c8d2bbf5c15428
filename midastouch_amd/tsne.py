"""One-dimensional t-SNE on the device: sklearn `TSNE(n_components=1, perplexity=40, init="pca", random_state=0)` as
`modules/misc.py:111-129` (`color_tsne`) calls it, with the exact O(K^2) gradient in place of Barnes-Hut.  DESIGN.md 4.6.

Stages (sklearn/manifold/_t_sne.py `TSNE._fit` / `_tsne`):
  knn         `midas_tsne_knn`: the k = min(K - 1, int(3 perplexity + 1)) nearest rows, squared euclidean in float64 on the matrix
              cores, ascending (d2, index)
  affinities  `midas_tsne_perplexity` (`_binary_search_perplexity`) on the float32 distances in sklearn's sorted column order,
              then `_joint_probabilities_nn`'s P = cond + cond^T, / max(sum, DBL_EPSILON), as a CSR in sorted order (torch plumbing)
  init        "pca": the first principal component score by subspace iteration (torch matmuls), sklearn's sign rule, float32,
              / std * 1e-4; "random": sklearn's RandomState draw; or a given (K,) tensor
  optimize    `midas_tsne_optimize`: `_gradient_descent` twice, as `_tsne` schedules it (early exaggeration 12 for 250 iterations at
              momentum 0.5, then momentum 0.8), on the exact gradient (`midas_tsne_gradient`)
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import MidasError, _ptr

EXPLORATION_MAX_ITER = 250  # TSNE._EXPLORATION_MAX_ITER
N_ITER_CHECK = 50  # TSNE._N_ITER_CHECK
MAX_NEIGHBORS = 256


class JointP(NamedTuple):
    """The joint probabilities as a K x K CSR on the device: crow (K + 1,) int64, col (nnz,) int32, val (nnz,) float64."""

    crow: torch.Tensor
    col: torch.Tensor
    val: torch.Tensor
    K: int

    @staticmethod
    def from_scipy(P, device) -> "JointP":
        P = P.tocsr()
        P.sort_indices()
        return JointP(torch.as_tensor(P.indptr.astype(np.int64), device=device),
                      torch.as_tensor(P.indices.astype(np.int32), device=device),
                      torch.as_tensor(P.data.astype(np.float64), device=device), P.shape[0])

    def to_scipy(self):
        from scipy.sparse import csr_matrix

        return csr_matrix((self.val.cpu().numpy(), self.col.cpu().numpy(), self.crow.cpu().numpy()), shape=(self.K, self.K))


def _check_x(X) -> torch.Tensor:
    if not isinstance(X, torch.Tensor):
        raise MidasError("t-SNE needs a torch tensor on a HIP device")
    if not X.is_cuda:
        raise MidasError("t-SNE needs X on a HIP device; there is no CPU fallback")
    if X.dim() != 2:
        raise MidasError(f"t-SNE needs a 2-D X (K, F), got shape {tuple(X.shape)}")
    if X.dtype not in (torch.float32, torch.float64):
        X = X.to(torch.float64)
    if X.shape[1] >= 1 and X.stride(1) != 1:
        X = X.contiguous()
    return X


def n_neighbors(K: int, perplexity: float) -> int:
    """TSNE._fit's neighbour count, after its perplexity check."""
    if not perplexity > 0:
        raise MidasError(f"perplexity must be positive, got {perplexity}")
    if perplexity >= K:
        raise MidasError(f"perplexity must be less than n_samples ({K}), got {perplexity}")
    k = min(K - 1, int(3.0 * perplexity + 1))
    if k > MAX_NEIGHBORS:
        raise MidasError(f"{k} neighbours (perplexity {perplexity}): at most {MAX_NEIGHBORS} are supported")
    return k


def knn(X: torch.Tensor, k: int, nan_to_num: bool = False, rows_per_panel: int = 0):
    """(idx (K, k) int32, d2 (K, k) float64): each row's k nearest other rows by squared euclidean distance, ascending
    (d2, index).  X (K, F) float32 or float64 on the device, any row stride; nan_to_num: np.nan_to_num on every element as it is
    read (X itself is not written)."""
    X = _check_x(X)
    K, F = X.shape
    if K < 2 or F < 1:
        raise MidasError(f"knn needs at least 2 rows and 1 column, got {tuple(X.shape)}")
    if not 1 <= k <= min(MAX_NEIGHBORS, K - 1):
        raise MidasError(f"k = {k} outside 1 .. min({MAX_NEIGHBORS}, K - 1 = {K - 1})")
    ctx = _lib.context(X.device)
    idx = torch.empty((K, k), dtype=torch.int32, device=X.device)
    d2 = torch.empty((K, k), dtype=torch.float64, device=X.device)
    dtype = _lib.MIDAS_F32 if X.dtype == torch.float32 else _lib.MIDAS_F64
    ctx.call("midas_tsne_knn", _ptr(X), dtype, K, F, X.stride(0), int(bool(nan_to_num)), int(k), int(rows_per_panel),
             _ptr(idx), _ptr(d2))
    return idx, d2


def conditional_affinities(d2_sorted: torch.Tensor, perplexity: float) -> torch.Tensor:
    """`_binary_search_perplexity` on (K, k) distances (rounded to float32 here, as `_joint_probabilities_nn` does): (K, k)
    float64 conditional P, row by row in the given column order."""
    if not d2_sorted.is_cuda:
        raise MidasError("conditional_affinities needs the distances on a HIP device; there is no CPU fallback")
    d = d2_sorted.to(torch.float32).contiguous()
    K, k = d.shape
    if not 1 <= k <= MAX_NEIGHBORS:
        raise MidasError(f"k = {k} outside 1 .. {MAX_NEIGHBORS}")
    out = torch.empty((K, k), dtype=torch.float64, device=d.device)
    _lib.context(d.device).call("midas_tsne_perplexity", _ptr(d), K, k, float(np.float32(perplexity)), _ptr(out))
    return out


def affinities(idx: torch.Tensor, d2: torch.Tensor, perplexity: float):
    """(cond, P): `_joint_probabilities_nn` on the kNN graph.  The rows are taken in sklearn's sorted column order
    (`distances.sort_indices()`); cond (K, k) float64 is in that order (`cond_cols` gives its columns); P = (cond + cond^T) /
    max(sum, DBL_EPSILON) as a `JointP` in sorted CSR order.  Returns (cond, cond_cols, P)."""
    K, k = idx.shape
    order = torch.argsort(idx, dim=1)
    cols = torch.gather(idx, 1, order)
    cond = conditional_affinities(torch.gather(d2, 1, order), perplexity)
    rows = torch.arange(K, device=idx.device, dtype=torch.int64).repeat_interleave(k)
    c = cols.reshape(-1).to(torch.int64)
    key = torch.cat([rows * K + c, c * K + rows])
    v = torch.cat([cond.reshape(-1), cond.reshape(-1)])
    uk, inv = torch.unique(key, sorted=True, return_inverse=True)
    # at most two terms a key (p_j|i and p_i|j): their sum does not depend on the order they arrive in
    val = torch.zeros(uk.shape[0], dtype=torch.float64, device=idx.device).index_add_(0, inv, v)
    total = torch.clamp(val.sum(), min=float(np.finfo(np.float64).eps))
    val = val / total
    r = uk // K
    crow = torch.zeros(K + 1, dtype=torch.int64, device=idx.device)
    crow[1:] = torch.cumsum(torch.bincount(r, minlength=K), 0)
    return cond, cols, JointP(crow, (uk % K).to(torch.int32), val, K)


def _val32(P: JointP, exaggeration: float = 1.0) -> torch.Tensor:
    val = P.val if exaggeration == 1.0 else P.val * float(exaggeration)
    return val.to(torch.float32).contiguous()


def gradient(P: JointP, y: torch.Tensor, exaggeration: float = 1.0):
    """(KL, grad): `_kl_divergence_bh(y, P * exaggeration, 1, K, 1, angle=0, compute_error=True)` - the exact one-dimensional
    gradient (K,) float32 and the error of compute_gradient_positive (a Python float)."""
    y = y.reshape(-1).to(torch.float32).contiguous()
    if not y.is_cuda:
        raise MidasError("gradient needs y on a HIP device; there is no CPU fallback")
    K = y.shape[0]
    if K != P.K or K < 2:
        raise MidasError(f"y has {K} rows, P is {P.K} x {P.K}")
    val = _val32(P, exaggeration)
    grad = torch.empty_like(y)
    kl = torch.empty(1, dtype=torch.float64, device=y.device)
    _lib.context(y.device).call("midas_tsne_gradient", K, _ptr(y), _ptr(P.crow), _ptr(P.col), _ptr(val), _ptr(grad), _ptr(kl))
    return float(kl.item()), grad


def auto_learning_rate(K: int, early_exaggeration: float = 12.0):
    """TSNE._fit's learning_rate="auto": a numpy float64 scalar."""
    return np.maximum(K / early_exaggeration / 4, 50)


def gradient_descent(P: JointP, y: torch.Tensor, val: torch.Tensor, it: int, max_iter: int, momentum: float, learning_rate,
                     n_iter_without_progress: int, min_grad_norm: float, n_iter_check: int = N_ITER_CHECK):
    """One `_gradient_descent` call in place on y (K,) float32 with P's values `val` (float32): (error, last iteration)."""
    res = (C.c_double * 2)()
    lr_f32 = 0 if isinstance(learning_rate, np.floating) and np.asarray(learning_rate).dtype == np.float64 else 1
    _lib.context(y.device).call("midas_tsne_optimize", P.K, _ptr(y), _ptr(P.crow), _ptr(P.col), _ptr(val), int(it), int(max_iter),
                                float(momentum), float(learning_rate), lr_f32, int(n_iter_check), int(n_iter_without_progress),
                                float(min_grad_norm), C.cast(res, C.c_void_p))
    return float(res[0]), int(res[1])


def optimize(P: JointP, y0: torch.Tensor, early_exaggeration: float = 12.0, learning_rate="auto", max_iter: int = 1000,
             n_iter_without_progress: int = 300, min_grad_norm: float = 1e-7):
    """`TSNE._tsne`: (y (K,) float32, KL, n_iter, learning rate used).  Stage 1 on P * early_exaggeration at momentum 0.5 for up to 250 iterations,
    stage 2 on (P * early_exaggeration) / early_exaggeration at momentum 0.8 from the next iteration up to max_iter.
    learning_rate "auto" is max(K / early_exaggeration / 4, 50) as a numpy float64 (float64 updates, as numpy 2 promotes them);
    a number is a Python float (float32 updates)."""
    y = y0.reshape(-1).to(torch.float32).clone()
    if not y.is_cuda:
        raise MidasError("optimize needs y0 on a HIP device; there is no CPU fallback")
    if y.shape[0] != P.K:
        raise MidasError(f"y0 has {y.shape[0]} rows, P is {P.K} x {P.K}")
    lr = auto_learning_rate(P.K, early_exaggeration) if isinstance(learning_rate, str) and learning_rate == "auto" else float(learning_rate)
    ee = float(early_exaggeration)
    pe = P.val * ee
    err, it = gradient_descent(P, y, pe.to(torch.float32), 0, EXPLORATION_MAX_ITER, 0.5, lr, EXPLORATION_MAX_ITER, min_grad_norm)
    remaining = max_iter - EXPLORATION_MAX_ITER
    if it < EXPLORATION_MAX_ITER or remaining > 0:
        err, it = gradient_descent(P, y, (pe / ee).to(torch.float32), it + 1, max_iter, 0.8, lr, n_iter_without_progress,
                                   min_grad_norm)
    return y, err, it, lr


def _row_chunks(X: torch.Tensor, nan_to_num: bool, rows: int):
    for a in range(0, X.shape[0], rows):
        c = X[a:a + rows]
        if nan_to_num:
            c = torch.nan_to_num(c)  # in X's dtype, as np.nan_to_num (a copy of the chunk; X is not written)
        yield c.to(torch.float64)


def _orth(W: torch.Tensor) -> torch.Tensor:
    """Orthonormal columns spanning W (Householder QR of the thin F x b block on the host)."""
    Q, _ = np.linalg.qr(W.cpu().numpy())
    return torch.as_tensor(Q, device=W.device)


def pca_init(X: torch.Tensor, nan_to_num: bool = False, max_iter: int = 300, block: int = 8) -> torch.Tensor:
    """sklearn's init="pca" for one component: the first principal component score of the centred X (sign: the component's
    entry of largest magnitude positive, svd_flip(u_based_decision=False)), cast to float32, / np.std * 1e-4.  The component
    comes from subspace iteration on X_c^T X_c, one pass over X an iteration, until the top Ritz vector settles."""
    X = _check_x(X)
    K, F = X.shape
    rows = max(1, min(K, (1 << 26) // max(F, 1)))
    mu = torch.zeros(F, dtype=torch.float64, device=X.device)
    for c in _row_chunks(X, nan_to_num, rows):
        mu += c.sum(0)
    mu /= K
    b = max(1, min(block, F, K))
    g = torch.Generator(device="cpu").manual_seed(0)
    V = _orth(torch.randn(F, b, generator=g, dtype=torch.float64).to(X.device))
    v_prev = None
    for _ in range(max_iter):
        W = torch.zeros_like(V)
        for c in _row_chunks(X, nan_to_num, rows):
            cc = c - mu
            W += cc.T @ (cc @ V)
        w, U = np.linalg.eigh((V.T @ W).cpu().numpy())
        v = V @ torch.as_tensor(U[:, -1], device=X.device)
        v = v / torch.linalg.vector_norm(v)
        if v_prev is not None and 1.0 - abs(float(v @ v_prev)) < 1e-15:
            break
        v_prev = v
        V = _orth(W)
    if float(v[torch.argmax(torch.abs(v))]) < 0:
        v = -v
    score = torch.cat([(c - mu) @ v for c in _row_chunks(X, nan_to_num, rows)])
    y = score.to(torch.float32)
    s = y.to(torch.float64).std(unbiased=False).to(torch.float32)
    if not float(s) > 0:
        raise MidasError("init='pca': the first principal component score has zero spread (every row of X is the same); "
                         "sklearn divides 0 by 0 here")
    return y / s * 1e-4


def random_init(K: int, random_state: int = 0, device=None) -> torch.Tensor:
    """sklearn's init="random": `1e-4 * RandomState(random_state).standard_normal((K, 1)).astype(np.float32)`."""
    y = 1e-4 * np.random.RandomState(random_state).standard_normal(size=(K, 1)).astype(np.float32)
    return torch.as_tensor(y.reshape(-1), device=device)


def tsne_1d(X: torch.Tensor, perplexity: float = 40.0, early_exaggeration: float = 12.0, learning_rate="auto",
            max_iter: int = 1000, n_iter_without_progress: int = 300, min_grad_norm: float = 1e-7, init="pca",
            random_state: int = 0, return_info: bool = False, nan_to_num: bool = False):
    """`TSNE(n_components=1, ...).fit_transform(X)[:, 0]` on the device: (K,) float32 (and `info` with n_iter, kl_divergence,
    learning_rate when return_info).  X (K, F) float32 / float64 on a HIP device, any row stride; nan_to_num: np.nan_to_num
    semantics on the fly (X is read, not rewritten).  The gradient is the exact one (Barnes-Hut at angle 0)."""
    X = _check_x(X)
    K = X.shape[0]
    if max_iter < EXPLORATION_MAX_ITER:
        raise MidasError(f"max_iter must be at least {EXPLORATION_MAX_ITER}, got {max_iter}")
    k = n_neighbors(K, perplexity)
    idx, d2 = knn(X, k, nan_to_num=nan_to_num)
    _, _, P = affinities(idx, d2, perplexity)
    if isinstance(init, str) and init == "pca":
        y0 = pca_init(X, nan_to_num=nan_to_num)
    elif isinstance(init, str) and init == "random":
        y0 = random_init(K, random_state, X.device)
    elif isinstance(init, (torch.Tensor, np.ndarray)):
        y0 = torch.as_tensor(init).reshape(-1).to(X.device, torch.float32)
        if y0.shape[0] != K:
            raise MidasError(f"init has {y0.shape[0]} entries, X has {K} rows")
    else:
        raise MidasError(f"init must be 'pca', 'random' or a (K,) array, got {init!r}")
    y, kl, it, lr = optimize(P, y0, early_exaggeration, learning_rate, max_iter, n_iter_without_progress, min_grad_norm)
    if return_info:
        return y, {"n_iter": it, "kl_divergence": kl, "learning_rate": float(lr)}
    return y


def spectral_colors(y: torch.Tensor) -> torch.Tensor:
    """`plt.cm.Spectral((y - min) / (max - min))[:, :3]` on the device: (K, 3) float64.  The 256-entry table is matplotlib's,
    read at run time; the index rule is Colormap.__call__'s (x * N truncated, x == 1 -> N - 1, under / over / bad entries)."""
    import matplotlib

    cmap = matplotlib.colormaps["Spectral"]
    N = cmap.N
    lut = np.concatenate([cmap(np.arange(N)), [cmap.get_under(), cmap.get_over(), cmap.get_bad()]])
    lut = torch.as_tensor(lut[:, :3], dtype=torch.float64, device=y.device)
    lo, hi = y.min(), y.max()
    enc = (y - lo) / (hi - lo)
    xa = enc * N
    xa = torch.where(xa == N, torch.full_like(xa, N - 1), xa)
    under, over, bad = xa < 0, xa >= N, torch.isnan(xa)
    ix = torch.nan_to_num(xa, nan=0.0, posinf=0.0, neginf=0.0).to(torch.int64)
    ix = torch.where(under, N, torch.where(over, N + 1, ix))
    ix = torch.where(bad, N + 2, ix)
    return lut[ix]
