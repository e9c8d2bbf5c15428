"""Tensor-level wrappers over the C ABI (one function per kernel group).

Inputs/outputs are torch tensors on a HIP device; torch only owns the memory.  Each function
cites the reference arithmetic it replaces (paths relative to /root/reference/midastouch).
"""
from __future__ import annotations

import ctypes as C
import sys

import torch

from . import _lib
from ._lib import MidasError, _ptr


def _ctx(t: torch.Tensor):
    if not t.is_cuda:
        raise MidasError("midastouch_amd kernels need tensors on a HIP device; there is no CPU fallback")
    return _lib.context(t.device)


def _poses(p: torch.Tensor) -> torch.Tensor:
    p = p[None] if p.dim() == 2 else p
    if p.dtype != torch.float32 or not p.is_contiguous():
        p = p.float().contiguous()
    return p


class Codebook:
    """midas_codebook handle over a (K, D) embedding matrix kept in HBM (float32 when lossless)."""

    def __init__(self, embeddings: torch.Tensor):
        ctx = _ctx(embeddings)
        emb = embeddings.contiguous()
        if emb.dtype == torch.float64:
            e32 = emb.float()
            # the TCN emits float32 codes cast to float64 (contrib/tcn_minkloc/tcn.py:148): store them
            # as float32 when that loses nothing, float64 otherwise
            if bool((e32.double() == emb).all()):
                emb = e32
        elif emb.dtype != torch.float32:
            emb = emb.float()
        self.emb = emb
        self.K, self.D = emb.shape
        self.ctx = ctx
        h = C.c_void_p()
        dtype = _lib.MIDAS_F32 if emb.dtype == torch.float32 else _lib.MIDAS_F64
        ctx.call("midas_codebook_create", self.K, self.D, _ptr(emb), dtype, C.byref(h))
        self.h = h

    def score(self, codes: torch.Tensor) -> torch.Tensor:
        """cos(code_b, C_k) for every row: (B, K) float64 (particle_filter.py:455-457, filter.py:213-215)."""
        codes = torch.atleast_2d(codes).to(self.emb.device, torch.float64).contiguous()
        if codes.shape[1] != self.D:
            raise MidasError(f"tactile code has {codes.shape[1]} dims, codebook has {self.D}")
        out = torch.empty((codes.shape[0], self.K), dtype=torch.float64, device=self.emb.device)
        self.ctx.call("midas_score", self.h, codes.shape[0], _ptr(codes), _ptr(out))
        return out

    def score_batch(self, codes: torch.Tensor, precision: str = "f32") -> torch.Tensor:
        """(B, K) scores of B codes in one pass over the codebook on the matrix cores.

        precision "f32" (`midas_score_batch`): the codes rounded to float32, float32 fma chains - within ~1e-7 of `score`, equal to
        `oracle.score_codebook_batch`; float32 embeddings with D % 16 == 0 only.  "f64" (`midas_score_batch_f64`): float64 codes and
        arithmetic in the summation spec's order - bit-identical to `score` and `oracle.score_codebook`; any embeddings and D."""
        entry = {"f32": "midas_score_batch", "f64": "midas_score_batch_f64"}.get(precision)
        if entry is None:
            raise MidasError(f"precision must be 'f32' or 'f64', got {precision!r}")
        codes = torch.atleast_2d(codes).to(self.emb.device, torch.float64).contiguous()
        if codes.shape[1] != self.D:
            raise MidasError(f"tactile code has {codes.shape[1]} dims, codebook has {self.D}")
        out = torch.empty((codes.shape[0], self.K), dtype=torch.float64, device=self.emb.device)
        self.ctx.call(entry, self.h, codes.shape[0], _ptr(codes), _ptr(out))
        return out

    def self_similarity(self, i0: int = 0, rows: int | None = None) -> torch.Tensor:
        """(rows, K) float64: cos(E_i, E_j) for the entries i in [i0, i0 + rows) against all K entries (`midas_selfsim_panel_f64`,
        float64 chains on the matrix cores) - bit-identical to `score(self.emb[i0:i0 + rows].double())`.  rows None: to the end."""
        i0 = int(i0)
        rows = self.K - i0 if rows is None else int(rows)
        if i0 < 0 or rows < 1 or i0 + rows > self.K:
            raise MidasError(f"self_similarity rows [{i0}, {i0 + rows}) outside the codebook's {self.K} entries")
        out = torch.empty((rows, self.K), dtype=torch.float64, device=self.emb.device)
        self.ctx.call("midas_selfsim_panel_f64", self.h, i0, rows, _ptr(out), self.K)
        return out

    def set_batch_precision(self, precision: str) -> None:
        """Precision of the dense batch scoring pass inside `midas_filter_step_batch` ("f32": today's default, "f64": the
        float64 kernel of `score_batch(..., "f64")`, bit-identical to `score`)."""
        dtype = {"f32": _lib.MIDAS_F32, "f64": _lib.MIDAS_F64}.get(precision)
        if dtype is None:
            raise MidasError(f"precision must be 'f32' or 'f64', got {precision!r}")
        self.ctx.check(self.ctx.lib.midas_codebook_set_batch_precision(self.h, dtype))

    def __del__(self, _finalizing=sys.is_finalizing):  # pragma: no cover  # (bound at import: module globals are gone by then)
        if _finalizing():  # the process is going away: the HIP runtime may be gone already (its calls would abort, not raise)
            return
        try:
            if self.h:
                self.ctx.lib.midas_codebook_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Tree:
    """Static KD-tree handle: dim 6 (float32 pose features) or dim 3 (float64 mesh vertices)."""

    def __init__(self, points: torch.Tensor):
        ctx = _ctx(points)
        dim = points.shape[1]
        if dim == 6:
            pts = points.float().contiguous()
        elif dim == 3:
            pts = points.double().contiguous()
        else:
            raise MidasError("Tree needs (K,6) float32 or (K,3) float64 points")
        self.dim, self.K, self.ctx = dim, pts.shape[0], ctx
        h = C.c_void_p()
        ctx.call("midas_tree_build", dim, self.K, _ptr(pts), C.byref(h))
        self.h = h

    def attach_mesh(self, mesh_tree: "Tree", cb_poses: torch.Tensor):
        """Per-codebook-entry mesh vertex lists: the prune of the fused step then rarely walks the mesh tree."""
        if self.dim != 6 or mesh_tree.dim != 3:
            raise MidasError("attach_mesh: self must be the 6-d codebook tree, mesh_tree the 3-d vertex tree")
        cb_poses = cb_poses.to(torch.float32).contiguous()
        self.ctx.call("midas_tree_attach_mesh", self.h, mesh_tree.h, _ptr(cb_poses))
        self._mesh = mesh_tree  # keep the mesh tree alive while the lists refer to it

    def export(self, what: str):
        """Host copy (numpy uint8 / float32 / int32) of one of the per-entry lists: "nbrs" (K, 513, 32) bytes, "rho_out" (K,),
        "twin" (K,), "vlist" (K, 257, 32) bytes.  For tests and inspection (midas_tree_export)."""
        import numpy as np
        code, shape, dt = {"nbrs": (0, (self.K, 513, 32), np.uint8), "rho_out": (1, (self.K,), np.float32),
                           "twin": (2, (self.K,), np.int32), "vlist": (3, (self.K, 257, 32), np.uint8)}[what]
        out = np.empty(shape, dtype=dt)
        self.ctx.call("midas_tree_export", self.h, code, C.c_void_p(out.ctypes.data), out.nbytes)
        return out

    def __del__(self, _finalizing=sys.is_finalizing):  # pragma: no cover  # (bound at import: module globals are gone by then)
        if _finalizing():  # the process is going away: the HIP runtime may be gone already (its calls would abort, not raise)
            return
        try:
            if self.h:
                self.ctx.lib.midas_tree_destroy(self.h)
                self.h = None
        except Exception:
            pass


class ObjectSet:
    """midas_object_set handle: the objects the rows of one batch frame stand on (BatchLoopEngine.for_objects).  objects: per object
    its `codebook`, `tree6` (with `tree3`'s vertex lists attached), `tree3` and float32 `cb_poses` on the device; row_object: the
    object of every row.  The handles are kept alive with the set."""

    def __init__(self, ctx, objects, row_object):
        self.ctx, self.objects, n, B = ctx, list(objects), len(objects), len(row_object)
        arr = lambda hs: (C.c_void_p * n)(*[h.value if isinstance(h, C.c_void_p) else h for h in hs])  # noqa: E731
        cbs, t6s, t3s = (arr([getattr(o, k).h for o in self.objects]) for k in ("codebook", "tree6", "tree3"))
        poses = arr([o.cb_poses.data_ptr() for o in self.objects])
        rows = (C.c_int32 * B)(*[int(i) for i in row_object])
        h = C.c_void_p()
        ctx.call("midas_object_set_create", n, cbs, t6s, t3s, poses, B, rows, C.byref(h))
        self.h = h

    def __del__(self, _finalizing=sys.is_finalizing):  # pragma: no cover  # (bound at import: module globals are gone by then)
        if _finalizing():
            return
        try:
            if self.h:
                self.ctx.lib.midas_object_set_destroy(self.h)
                self.h = None
        except Exception:
            pass


def _counts(ns, B: int):
    """B host counts as the C ABI reads them."""
    ns = [int(v) for v in ns]
    if len(ns) != B:
        raise MidasError(f"{len(ns)} particle counts for {B} rows")
    return (C.c_int32 * B)(*ns)


def init_particles_batch(poses: torch.Tensor, gts: torch.Tensor, sigmas: torch.Tensor, ns, seed: int = 0, draw: int = 0,
                         tn: torch.Tensor | None = None, rot: torch.Tensor | None = None) -> torch.Tensor:
    """init_filter (modules/particle_filter.py:129-145) for B rows in one launch, in place: poses (B, cap, 4, 4) float32, slots
    [0, ns[b]) of row b := gts[b] @ T(from_euler('zyx', rot, degrees), tn); the slots behind stay.  gts (B, 4, 4); sigmas (B, 2): row
    b's init_noise (metres, degrees).  tn / rot (B, cap, 3) float32, already scaled: the caller's draws; None: Philox normals keyed
    (seed + b, 0xFFFFFFFF - draw) (`midas_init_particles_batch`)."""
    if poses.dim() != 4 or poses.dtype != torch.float32 or not poses.is_contiguous():
        raise MidasError("init_particles_batch writes in place: contiguous float32 poses (B, cap, 4, 4)")
    if (tn is None) != (rot is None):
        raise MidasError("tn and rot (the start's draws) come together or not at all")
    if not 0 <= int(draw) <= 0xFFFFFFFF:
        raise MidasError("draw counts the starts so far: 0 .. 2^32 - 1")
    B, cap, d = poses.shape[0], poses.shape[1], poses.device
    n_host = _counts(ns, B)
    gts = gts.to(d, torch.float32).contiguous()
    sigmas = sigmas.to(d, torch.float32).contiguous()
    if tuple(gts.shape) != (B, 4, 4) or tuple(sigmas.shape) != (B, 2):
        raise MidasError(f"expected gts ({B},4,4) and sigmas ({B},2), got {tuple(gts.shape)} and {tuple(sigmas.shape)}")
    if tn is not None:
        tn, rot = (t.to(d, torch.float32).contiguous() for t in (tn, rot))
        if tuple(tn.shape) != (B, cap, 3) or tuple(rot.shape) != (B, cap, 3):
            raise MidasError(f"expected tn and rot ({B},{cap},3), got {tuple(tn.shape)} and {tuple(rot.shape)}")
    _ctx(poses).call("midas_init_particles_batch", B, cap, n_host, _ptr(gts), _ptr(sigmas), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw),
                     _ptr(tn), _ptr(rot), _ptr(poses))
    return poses


def project_batch(poses: torch.Tensor, hint: torch.Tensor, ns, tree6: "Tree" = None, codebook: "Codebook" = None,
                  cb_poses: torch.Tensor | None = None, object_set: "ObjectSet" = None) -> torch.Tensor:
    """particles.poses, _, _ = codebook.SE3_NN(particles.poses) (filter/filter.py:159-160) for B rows in one launch, in place: slots
    [0, ns[b]) of poses (B, cap, 4, 4) := the nearest codebook pose, of hint (B, cap) int32 := its index - on object_set's object of
    the row, or on (tree6, codebook, cb_poses) for every row.  Row b holds the bits of gather_rows(cb_poses, nn6(tree6,
    se3_feature(poses[b, :ns[b]]))) (`midas_project_batch`)."""
    if poses.dim() != 4 or poses.dtype != torch.float32 or not poses.is_contiguous():
        raise MidasError("project_batch writes in place: contiguous float32 poses (B, cap, 4, 4)")
    B, cap = poses.shape[0], poses.shape[1]
    if hint.dtype != torch.int32 or not hint.is_contiguous() or tuple(hint.shape) != (B, cap) or hint.device != poses.device:
        raise MidasError(f"project_batch writes in place: contiguous int32 hints ({B}, {cap}) beside the poses")
    n_host = _counts(ns, B)
    if object_set is None:
        if tree6 is None or codebook is None or cb_poses is None:
            raise MidasError("project_batch needs an object set, or a tree, its codebook and the codebook's poses")
        if cb_poses.dtype != torch.float32 or not cb_poses.is_contiguous() or cb_poses.device != poses.device:
            raise MidasError("project_batch reads contiguous float32 codebook poses on the particles' device")
        if cb_poses.numel() != 16 * tree6.K:
            raise MidasError(f"{cb_poses.shape[0]} codebook poses for a tree over {tree6.K} entries")
        args = (None, codebook.h, tree6.h, _ptr(cb_poses))
    else:
        args = (object_set.h, None, None, None)
    _ctx(poses).call("midas_project_batch", *args, B, cap, n_host, _ptr(poses), _ptr(hint))
    return hint


def se3_feature(poses: torch.Tensor, w: float = 0.01) -> torch.Tensor:
    """R3_SE3 (tactile_tree/tactile_tree.py:73-77)."""
    poses = _poses(poses)
    out = torch.empty((poses.shape[0], 6), dtype=torch.float32, device=poses.device)
    _ctx(poses).call("midas_se3_feature", poses.shape[0], _ptr(poses), float(w), _ptr(out))
    return out


def nn6(tree: Tree, feat: torch.Tensor, hint: torch.Tensor | None = None, want_d2: bool = False):
    feat = feat.float().contiguous()
    n = feat.shape[0]
    idx = torch.empty(n, dtype=torch.int32, device=feat.device)
    d2 = torch.empty(n, dtype=torch.float32, device=feat.device) if want_d2 else None
    if hint is not None:
        hint = hint.to(torch.int32).contiguous()
    _ctx(feat).call("midas_nn6", tree.h, n, _ptr(feat), _ptr(hint), _ptr(idx), _ptr(d2))
    return (idx, d2) if want_d2 else idx


def knn6(tree: Tree, feat: torch.Tensor, k: int, want_d2: bool = False):
    """(N, k) int32 indices of the k nearest codebook entries per query, by (distance, index); exact (tactile_tree.py:50-52
    with n_neighbors = k)."""
    feat = feat.float().contiguous()
    n = feat.shape[0]
    idx = torch.empty((n, k), dtype=torch.int32, device=feat.device)
    d2 = torch.empty((n, k), dtype=torch.float32, device=feat.device) if want_d2 else None
    _ctx(feat).call("midas_knn6", tree.h, n, _ptr(feat), int(k), _ptr(idx), _ptr(d2))
    return (idx, d2) if want_d2 else idx


def nn6_stats(tree: Tree, feat: torch.Tensor, hint: torch.Tensor | None = None):
    """Diagnostic: (leaves visited, nodes visited) per query."""
    feat = feat.float().contiguous()
    n = feat.shape[0]
    leaves = torch.empty(n, dtype=torch.int32, device=feat.device)
    nodes = torch.empty(n, dtype=torch.int32, device=feat.device)
    if hint is not None:
        hint = hint.to(torch.int32).contiguous()
    _ctx(feat).call("midas_nn6_stats", tree.h, n, _ptr(feat), _ptr(hint), _ptr(leaves), _ptr(nodes))
    return leaves, nodes


def nn3_dist(tree: Tree, poses: torch.Tensor) -> torch.Tensor:
    poses = _poses(poses)
    dist = torch.empty(poses.shape[0], dtype=torch.float64, device=poses.device)
    _ctx(poses).call("midas_nn3", tree.h, poses.shape[0], _ptr(poses), _ptr(dist))
    return dist


def propagate(poses, odom, tn=None, rot=None, std_t=0.0, std_r=0.0, seed=0, step=0) -> torch.Tensor:
    """poses @ (odom @ Tn) (particle_filter.py:319-345,370-375); tn/rot None -> device Philox draws."""
    poses = _poses(poses)
    dev = poses.device
    odom = odom.to(dev, torch.float32).contiguous()
    out = torch.empty_like(poses)
    if tn is not None:
        tn = tn.to(dev, torch.float32).contiguous()
        rot = rot.to(dev, torch.float32).contiguous()
    _ctx(poses).call("midas_propagate", poses.shape[0], _ptr(poses), _ptr(out), _ptr(odom), _ptr(tn), _ptr(rot),
                     float(std_t), float(std_r), int(seed), int(step))
    return out


def check_poses(poses):
    poses = _poses(poses)
    flag = torch.empty(poses.shape[0], dtype=torch.uint8, device=poses.device)
    count = torch.zeros(1, dtype=torch.int32, device=poses.device)
    _ctx(poses).call("midas_check_poses", poses.shape[0], _ptr(poses), _ptr(flag), _ptr(count))
    return flag, count


def gather_f64(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    table = table.double().contiguous()
    idx = idx.to(torch.int32).contiguous()
    out = torch.empty(idx.shape[0], dtype=torch.float64, device=table.device)
    _ctx(table).call("midas_gather_f64", idx.shape[0], _ptr(table), _ptr(idx), _ptr(out))
    return out


def softmax_weights(x: torch.Tensor, softmax: bool = True) -> torch.Tensor:
    """get_similarity tail (particle_filter.py:459-468)."""
    x = x.double().contiguous()
    w = torch.empty_like(x)
    _ctx(x).call("midas_softmax", x.shape[0], _ptr(x), int(bool(softmax)), _ptr(w))
    return w


def prune_(w: torch.Tensor, dist: torch.Tensor, thr: float) -> torch.Tensor:
    """In place w *= !(dist > thr) (particle_filter.py:394-402); returns the kept count (device int32[1])."""
    if w.dtype != torch.float64 or not w.is_contiguous():
        raise MidasError("prune_ needs a contiguous float64 weight tensor (it is modified in place)")
    nvalid = torch.zeros(1, dtype=torch.int32, device=w.device)
    _ctx(w).call("midas_prune", w.shape[0], _ptr(w), _ptr(dist.double().contiguous()), float(thr), _ptr(nvalid))
    return nvalid


def cdf(w: torch.Tensor):
    w = w.double().contiguous()
    out = torch.empty_like(w)
    status = torch.zeros(1, dtype=torch.int32, device=w.device)
    _ctx(w).call("midas_cdf", w.shape[0], _ptr(w), _ptr(out), _ptr(status))
    return out, status


def resample_search(cdf_t: torch.Tensor, M: int, mode: int, u=None, u32: float = -1.0, seed=0, step=0) -> torch.Tensor:
    idx = torch.empty(M, dtype=torch.int32, device=cdf_t.device)
    if u is not None:
        u = u.to(cdf_t.device, torch.float64).contiguous()
    _ctx(cdf_t).call("midas_resample_search", cdf_t.shape[0], _ptr(cdf_t), M, mode, _ptr(u), float(u32), int(seed),
                     int(step), _ptr(idx))
    return idx


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """src[idx] along dim 0 (particle_filter.py:246-248; tactile_tree.py:54-58)."""
    src = src.contiguous()
    idx = idx.to(torch.int32).contiguous()
    out = torch.empty((idx.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    row_bytes = src.element_size()
    for s in src.shape[1:]:
        row_bytes *= s
    if idx.shape[0] and row_bytes:
        _ctx(src).call("midas_gather_rows", idx.shape[0], _ptr(idx), _ptr(src), _ptr(out), row_bytes)
    return out


def rmse(poses: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    poses = _poses(poses)
    gt = gt.to(poses.device, torch.float32).contiguous()
    out = torch.empty(2, dtype=torch.float64, device=poses.device)
    _ctx(poses).call("midas_rmse", poses.shape[0], _ptr(poses), _ptr(gt), _ptr(out))
    return out


CLUSTER_CENTER_ENTRIES = {"quat_avg": "midas_cluster_centers", "logmap": "midas_cluster_centers_logmap"}


def se3_log(poses: torch.Tensor) -> torch.Tensor:
    """(N,4,4) -> (N,6) float64 tangent vectors [V^-1 t, omega] (midas_se3_log; theseus `SE3.log_map`, pose.py:105-106): what the
    log-map cluster centres average."""
    poses = _poses(poses)
    out = torch.empty((poses.shape[0], 6), dtype=torch.float64, device=poses.device)
    _ctx(poses).call("midas_se3_log", poses.shape[0], _ptr(poses), _ptr(out))
    return out


def cluster_centers(poses: torch.Tensor, weights: torch.Tensor, labels: torch.Tensor, label_values: torch.Tensor,
                    method: str = "quat_avg"):
    """K9: (centres (C,4,4) f32, stds (C,3) f32, members (C,) i64) of the clusters `label_values`: method "quat_avg"
    (midas_cluster_centers) or "logmap" (midas_cluster_centers_logmap), get_cluster_centers' two (particle_filter.py:153-206)."""
    entry = CLUSTER_CENTER_ENTRIES.get(method)
    if entry is None:
        raise MidasError(f"method must be 'quat_avg' or 'logmap', got {method!r}")
    poses = _poses(poses)
    dev = poses.device
    labels = labels.to(dev, torch.int64).contiguous()
    label_values = label_values.to(dev, torch.int64).contiguous()
    weights = weights.to(dev).contiguous()
    if weights.dtype not in (torch.float32, torch.float64):
        weights = weights.double()
    C = int(label_values.shape[0])
    centers = torch.empty((C, 4, 4), dtype=torch.float32, device=dev)
    stds = torch.empty((C, 3), dtype=torch.float32, device=dev)
    counts = torch.empty((C,), dtype=torch.int64, device=dev)
    w64 = _ptr(weights) if weights.dtype == torch.float64 else None
    w32 = _ptr(weights) if weights.dtype == torch.float32 else None
    _ctx(poses).call(entry, poses.shape[0], _ptr(poses), w64, w32, _ptr(labels), C, _ptr(label_values),
                     _ptr(centers), _ptr(stds), _ptr(counts))
    return centers, stds, counts


def pose_estimate(poses_prop: torch.Tensor, weights: torch.Tensor):
    """The per-frame pose estimate of B particle sets by one call (midas_pose_estimate; filter/filter.py:184-186 on a set nobody
    has clustered): poses_prop (B,N,4,4), weights (B,N) -> (centres (B,4,4) f32, stds (B,3) f32).  Row b is bit for bit
    `cluster_centers(poses_prop[b], weights[b], zeros(N), [0])[:2]` with float64 weights."""
    if poses_prop.dim() != 4 or tuple(poses_prop.shape[2:]) != (4, 4) or tuple(weights.shape) != tuple(poses_prop.shape[:2]):
        raise MidasError(f"pose_estimate: expected (B,N,4,4) poses and (B,N) weights, got {tuple(poses_prop.shape)} and {tuple(weights.shape)}")
    poses = _poses(poses_prop)
    dev = poses.device
    ctx = _ctx(poses)
    weights = weights.to(dev, torch.float64).contiguous()
    B, N = int(poses.shape[0]), int(poses.shape[1])
    centers = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    stds = torch.empty((B, 3), dtype=torch.float32, device=dev)
    a = _lib.EstimateArgs()
    a.N, a.B = N, B
    a.poses_prop, a.weights, a.centers, a.stds = _ptr(poses), _ptr(weights), _ptr(centers), _ptr(stds)
    ctx.call("midas_pose_estimate", C.byref(a))
    return centers, stds


def dbscan(poses: torch.Tensor, eps: float = 1e-2, min_samples: int = -1):
    """cluster_particles(method="euclidean") labels (particle_filter.py:208-217): DBSCAN of the translations on the device.
    min_samples < 0 -> N // 5.  Returns (labels int32 (N,), info int32 (2,) = [clusters, limit flag])."""
    poses = _poses(poses)
    labels = torch.empty(poses.shape[0], dtype=torch.int32, device=poses.device)
    info = torch.zeros(2, dtype=torch.int32, device=poses.device)
    _ctx(poses).call("midas_dbscan", poses.shape[0], _ptr(poses), float(eps), int(min_samples), _ptr(labels), _ptr(info))
    return labels, info


def dbscan_batch(poses: torch.Tensor, counts=None, eps: float = 1e-2, min_samples: int = -1, max_clusters: int = 0, out=None):
    """cluster_particles(method="euclidean") labels (particle_filter.py:208-217) of B particle sets in one set of launches
    (midas_dbscan_batch): poses (B, N, 4, 4); counts None (every row holds N points) or B live counts (int tensor or sequence,
    0 .. N each); min_samples < 0 -> n_b // 5 per row; max_clusters 0 = any number, 1 .. 62 = a row with more reports flag 2.
    Returns (labels int32 (B, N), info int32 (B, 2) = per row [clusters, flags]); row b holds `dbscan(poses[b, :n_b])`'s labels,
    slots beyond n_b are left as they are (-1 in a fresh tensor; `out`: a (B, N) int32 tensor of the caller's to write into).
    B * N is bounded by `_lib.DBSCAN_BATCH_MAX_POINTS` (the rows share one set of cell tables)."""
    if poses.dim() != 4 or tuple(poses.shape[2:]) != (4, 4):
        raise MidasError(f"expected (B,N,4,4) poses, got {tuple(poses.shape)}")
    B, N = int(poses.shape[0]), int(poses.shape[1])
    if B < 1 or N < 1:
        raise MidasError(f"dbscan_batch needs at least one row and one slot, got {B} x {N}")
    if B * N > _lib.DBSCAN_BATCH_MAX_POINTS:
        raise MidasError(f"dbscan_batch holds at most DBSCAN_BATCH_MAX_POINTS = {_lib.DBSCAN_BATCH_MAX_POINTS} points in all, not {B} x {N} "
                         "(cluster the rows one by one with dbscan)")
    ctx = _ctx(poses)
    if poses.dtype != torch.float32 or not poses.is_contiguous():
        poses = poses.float().contiguous()
    if counts is not None:
        counts = torch.as_tensor(counts).to(poses.device, torch.int32).contiguous().reshape(-1)
        if counts.numel() != B:
            raise MidasError(f"{counts.numel()} counts for {B} rows")
    if out is None:
        out = torch.full((B, N), -1, dtype=torch.int32, device=poses.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (B, N) or not out.is_contiguous() or out.device != poses.device:
        raise MidasError(f"out must be a contiguous ({B},{N}) int32 tensor on {poses.device}")
    info = torch.zeros((B, 2), dtype=torch.int32, device=poses.device)
    ctx.call("midas_dbscan_batch", B, N, _ptr(counts), 1, _ptr(poses), float(eps), int(min_samples), _ptr(out), _ptr(info), int(max_clusters))
    return out, info


def dbscan_points(points: torch.Tensor, eps: float = 1e-2, min_samples: int = -1):
    """DBSCAN labels of N points in 2 .. 6 dimensions (cluster_particles(method="logmap"), particle_filter.py:218-223: the
    6-d SE(3) logarithms), all pairs on the device in float64 - sklearn's predicate and numbering.
    Returns (labels int32 (N,), info int32 (2,) = [clusters, spread steps or -1])."""
    pts = points.to(torch.float64).contiguous()
    if not pts.is_cuda:
        raise MidasError("midastouch_amd kernels need tensors on a HIP device; there is no CPU fallback")
    labels = torch.empty(pts.shape[0], dtype=torch.int32, device=pts.device)
    info = torch.zeros(2, dtype=torch.int32, device=pts.device)
    _ctx(pts).call("midas_dbscan_points", pts.shape[0], int(pts.shape[1]), _ptr(pts), float(eps), int(min_samples), _ptr(labels), _ptr(info))
    return labels, info


def anneal_select(weights: torch.Tensor, mode: int, k: int, ties: str = "index", info: torch.Tensor = None) -> torch.Tensor:
    """Index list of the annealed particle set (particle_filter.py:421-446): mode 1 = without the k smallest weights (order
    kept), mode 2 = everybody followed by the k largest (largest first).  ties: "index" = to the smaller index (torch's CUDA
    kernel), "aten_cpu" = the members / the order `torch.topk` returns on the CPU (topk_aten.hip).  info: optional int32[1]
    the call adds its depth-limit fallbacks to."""
    w = weights.double().contiguous()
    n = w.shape[0]
    src = torch.empty(n + (k if mode == 2 else 0), dtype=torch.int32, device=w.device)
    rule = {"index": _lib.TOPK_TIES_INDEX, "aten_cpu": _lib.TOPK_TIES_ATEN_CPU}[ties]
    _ctx(w).call("midas_anneal_select_ties", n, _ptr(w), int(mode), int(k), rule, _ptr(src), _ptr(info))
    return src[:n - k] if mode == 1 else src


def topn_pose_error(scores: torch.Tensor, row0: int, n: int, feat: torch.Tensor, want_idx: bool = False):
    """Per row of `scores` (B, K) f64 - row b = similarities of entry row0 + b - the best pose error among its n
    best-scoring entries, diagonal zeroed (midas_topn_pose_error; eval/single_touch_test.py:35-73)."""
    scores = scores.to(torch.float64).contiguous()
    feat = feat.to(scores.device, torch.float64).contiguous()
    B, K = scores.shape
    err = torch.empty((B,), dtype=torch.float64, device=scores.device)
    idx = torch.empty((B, n), dtype=torch.int32, device=scores.device) if want_idx else None
    _ctx(scores).call("midas_topn_pose_error", B, K, _ptr(scores), int(row0), int(n), _ptr(feat), int(feat.shape[1]), _ptr(err),
                      _ptr(idx))
    return (err, idx) if want_idx else err
