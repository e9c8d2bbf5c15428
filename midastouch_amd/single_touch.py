"""Single-touch evaluation of a codebook: `eval/single_touch_test.py:35-91` on the device.

`top_n_error` is the reference's K x K self-similarity of the embeddings followed by a per-row top-25 and the best pose
error among them.  Here the similarity rows come from the scoring kernels tile by tile (exact float64 GEMV rows by default;
`fast=True`: the self-similarity as a float32 GEMM on the matrix cores, `midas_selfsim_topn` - panels of `panel_rows`
queries against all K entries; `fast=True, precision="f64"`: the same panels in float64 on the matrix cores,
`midas_selfsim_topn_f64` - the default path's values bit for bit, any embedding dtype and D) and the selection kernel
(`midas_topn_pose_error`) consumes each tile in one pass - the K x K matrix (20 GB at K = 50 k) never exists.
`confusion_matrix` is `modules/misc.py:78-108` (`eval/viz_codebook.py:37`): the same float64 panels, this time materialised.
`color_tsne` is `modules/misc.py:111-129` (sklearn's one-dimensional t-SNE of the nan_to_num'd matrix, min-max scaled, through
`plt.cm.Spectral`) on the device (`tsne.tsne_1d`); `codebook_colors` is the compute of `eval/viz_codebook.py:34-40`.
The heat-map of `filter/filter.py:213-215` is `particle_filter.get_similarity(code, codebook.get_embeddings(), softmax=False)`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

NUM_NEIGHBORS = 25  # single_touch_test.py:32
F64_PANEL_ROWS = 2048  # MIDAS_SELFSIM_F64_ROWS: two float64 panels of 2048 x K (1.6 GB at K = 50 k)


def top_n_error(embeddings: torch.Tensor, poses: torch.Tensor, n: int = NUM_NEIGHBORS, fast: bool = False,
                tile: int = 256, want_idx: bool = False, panel_rows: int | None = None, precision: str = "f32"):
    """(K,) float64: for every codebook entry the smallest |pose_j - pose_i| among its n most similar entries
    (diagonal similarity set to 0 like `np.fill_diagonal(C, 0)`).  embeddings (K, D) and poses (K, d) on a HIP device.

    Default: exact float64 rows (one `Codebook.score` GEMV pass per entry).  `fast=True` (precision "f32"): the float32 GEMM
    panels of `midas_selfsim_topn` (float32 embeddings, D % 32 == 0; panels of `panel_rows`, default 4096), else float32
    `score_batch` tiles - close to the exact result, not equal.  `fast=True, precision="f64"`: `midas_selfsim_topn_f64`, float64
    panels on the matrix cores for any embedding dtype and D - errors and indices EQUAL to the default form's, bit for bit
    (panels of `panel_rows`, default 2048: two panels of 2048 x K float64 in scratch, 1.6 GB at K = 50 k).  The precision only
    selects among the fast forms; without `fast` the default form runs."""
    if precision not in ("f32", "f64"):
        raise ops.MidasError(f"precision must be 'f32' or 'f64', got {precision!r}")
    emb = embeddings if isinstance(embeddings, torch.Tensor) else torch.as_tensor(embeddings)
    if not emb.is_cuda:
        raise ops.MidasError("top_n_error needs the embeddings on a HIP device; there is no CPU fallback")
    cb = ops.Codebook(emb)
    feat = torch.as_tensor(poses).to(emb.device, torch.float64).reshape(emb.shape[0], -1)
    K = emb.shape[0]
    out = torch.empty((K,), dtype=torch.float64, device=emb.device)
    idx_all = torch.empty((K, n), dtype=torch.int32, device=emb.device) if want_idx else None
    if fast and precision == "f64":
        # the float64 self-similarity on the matrix cores (midas_selfsim_topn_f64), panel by panel: the default path's values
        feat = feat.contiguous()
        cb.ctx.call("midas_selfsim_topn_f64", cb.h, int(n), ops._ptr(feat), int(feat.shape[1]),
                    int(panel_rows) if panel_rows is not None else F64_PANEL_ROWS, ops._ptr(out), ops._ptr(idx_all))
        return (out, idx_all) if want_idx else out
    panel_rows = 4096 if panel_rows is None else panel_rows
    if fast and cb.emb.dtype == torch.float32 and cb.D % 32 == 0:
        # the whole K x K x D self-similarity as a float32 GEMM on the matrix cores (midas_selfsim_topn), panel by panel
        cb.ctx.call("midas_selfsim_topn", cb.h, int(n), ops._ptr(feat), int(feat.shape[1]), int(panel_rows), ops._ptr(out),
                    ops._ptr(idx_all))
        return (out, idx_all) if want_idx else out
    tile = min(int(tile), 64) if fast else int(tile)
    for i0 in range(0, K, tile):
        q = cb.emb[i0:i0 + tile].to(torch.float64)
        scores = cb.score_batch(q) if fast else cb.score(q)
        r = ops.topn_pose_error(scores, i0, n, feat, want_idx=want_idx)
        if want_idx:
            out[i0:i0 + tile], idx_all[i0:i0 + tile] = r
        else:
            out[i0:i0 + tile] = r
    return (out, idx_all) if want_idx else out


def confusion_matrix(embeddings: torch.Tensor, sz: int | None = None, batch_size: int = 100) -> torch.Tensor:
    """`modules/misc.py:78-108` on the device: the cosine similarities of the first sz embeddings against each other, scaled to
    [0, 1] as `(C - C.min()) / np.ptp(C)` in float64 (ptp = 0: 0 / 0 = NaN, as numpy).  Every similarity is a float64 panel value
    of `Codebook.self_similarity` - `Codebook.score`'s, bit for bit - written straight into the (sz, sz) float64 device tensor that
    is returned.  The matrix is materialised, as in the reference: 8 sz^2 bytes (20 GB at sz = 50 k).  sz None: all rows.
    batch_size is accepted for the reference's signature; it does not change the result."""
    del batch_size
    emb = embeddings if isinstance(embeddings, torch.Tensor) else torch.as_tensor(embeddings)
    if not emb.is_cuda:
        raise ops.MidasError("confusion_matrix needs the embeddings on a HIP device; there is no CPU fallback")
    sz = emb.shape[0] if sz is None else int(sz)
    if sz < 1 or sz > emb.shape[0]:
        raise ops.MidasError(f"confusion_matrix: sz = {sz} outside 1 .. {emb.shape[0]}")
    cb = ops.Codebook(emb[:sz])
    C = torch.empty((sz, sz), dtype=torch.float64, device=emb.device)
    cb.ctx.call("midas_selfsim_panel_f64", cb.h, 0, sz, ops._ptr(C), sz)
    lo, hi = C.min(), C.max()
    return (C - lo) / (hi - lo)


def color_tsne(C: torch.Tensor, TSNE_init: str = "pca") -> torch.Tensor:
    """`modules/misc.py:111-129` on the device: TSNE(n_components=1, perplexity=40, init=TSNE_init, random_state=0) of
    np.nan_to_num(C) (applied as C is read - C is not modified), min-max scaled, `plt.cm.Spectral(...)[:, :3]`: (K, 3) float64.
    The t-SNE uses the exact gradient (tsne.tsne_1d)."""
    from . import tsne

    X = C if isinstance(C, torch.Tensor) else torch.as_tensor(C)
    if not X.is_cuda:
        raise ops.MidasError("color_tsne needs C on a HIP device; there is no CPU fallback")
    y = tsne.tsne_1d(X, perplexity=40.0, init=TSNE_init, random_state=0, nan_to_num=True)
    return tsne.spectral_colors(y)


def codebook_colors(embeddings: torch.Tensor, sz: int | None = None) -> torch.Tensor:
    """The compute of `eval/viz_codebook.py:34-40`: (sz, 3) float64 colours of the codebook entries.  D > 256:
    color_tsne(confusion_matrix(embeddings, sz), "pca") - the sz x sz matrix is materialised, 8 sz^2 bytes; otherwise
    color_tsne on the embeddings."""
    emb = embeddings if isinstance(embeddings, torch.Tensor) else torch.as_tensor(embeddings)
    if not emb.is_cuda:
        raise ops.MidasError("codebook_colors needs the embeddings on a HIP device; there is no CPU fallback")
    if emb.shape[1] > 256:
        return color_tsne(confusion_matrix(emb, sz), "pca")
    return color_tsne(emb, "pca")


def get_random_error(poses, n: int = NUM_NEIGHBORS, rng=None) -> float:
    """Mean best error of n random picks per entry (single_touch_test.py:76-91); host arithmetic, numpy draws."""
    poses = np.asarray(torch.as_tensor(poses).cpu(), dtype=np.float64).reshape(len(poses), -1)
    rng = np.random if rng is None else rng
    N = poses.shape[0]
    err = np.zeros(N)
    for i in range(N):
        pred = rng.choice(N, size=n)
        err[i] = np.min(np.linalg.norm(poses[pred] - poses[i], axis=1))
    return float(np.mean(err))
