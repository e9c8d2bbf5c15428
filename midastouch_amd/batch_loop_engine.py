"""BatchLoopEngine: B trajectories' whole loop bodies (`filter/filter.py:150-190`: measurement update, DBSCAN, cluster centres,
annealing of the particle count, resample) per set of launches - `midas_loop_step_batch`.

BatchFilterEngine / PipelinedBatchFilterEngine batch the fixed-N part of the frame; a sweep over seeds, logs or objects stacked
onto them never clusters or anneals.  Here every trajectory is a LoopEngine's particle set - its own live count in its own control
block, its own labels, cluster rows and log ring - and the kernels of the small-set frame run with the trajectory as grid.y.
Trajectory b draws from the Philox streams keyed (seed + b, frame): frame for frame it holds the bits of a LoopEngine built with
seed + b and stepped with row b of the operands.

The first version covers the small-set regime only: at most 16 384 particles per trajectory (`_lib.LOOP_BATCH_MAX_CAP`), device
Philox draws, ties of annealing's top-k by index, a float32 codebook scored sparsely.  Host draws (`tn` / `rot` / `u`), seeded torch
streams, the ATen tie rule, larger sets and sharding stay with LoopEngine and the sharded engine.  DBSCAN frames run the single
pass once per trajectory, one after the other on the stream, on one shared set of cell tables.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops
from ._lib import LoopArgs, MidasError, _ptr
from .engine import RESAMPLE_MODES, advance_epoch, codebook_index, frame_operands, sparse_scoring
from .loop_engine import ALL_PHASES, log_records


class BatchLoopEngine:
    def __init__(self, cb_poses, cb_embeddings, mesh_vertices, batch: int, num_particles: int, *, sig_t=2e-4, sig_r=0.5,
                 pen_max=0.002, seed=4000, softmax=True, resample="weighted_random", floor: int = 1000, eps: float = 1e-2,
                 cluster: bool = True, cluster_every: int = 50, log_frames: int = 4096, device=None):
        self.B, self.cap = B, cap = int(batch), int(num_particles)
        if B < 1 or B > 65535:
            raise MidasError("BatchLoopEngine holds 1 .. 65535 trajectories")
        if cap < 1 or cap > _lib.LOOP_BATCH_MAX_CAP:
            raise MidasError(f"BatchLoopEngine holds 1 .. {_lib.LOOP_BATCH_MAX_CAP} particles per trajectory (larger sets: LoopEngine)")
        self.ctx, self.cb_poses, self.cb_feat, self.tree6, self.codebook, self.tree3 = codebook_index(
            cb_poses, cb_embeddings, mesh_vertices, device)
        self.device = d = self.ctx.device
        self.K, self.D = self.codebook.K, self.codebook.D
        if not sparse_scoring(self.codebook, switch=False):
            raise MidasError("BatchLoopEngine scores sparsely: a float32 codebook with D in {128, 256, 512, 1024}")
        self.sig_t, self.sig_r, self.pen_max = float(sig_t), float(sig_r), float(pen_max)
        self.seed, self.softmax, self.floor, self.eps = int(seed), bool(softmax), int(floor), float(eps)
        self.cluster, self.cluster_every = bool(cluster), max(int(cluster_every), 1)
        self.mode = RESAMPLE_MODES[resample]
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=d)  # noqa: E731
        self.ctl_i, self.ctl_d = z((B, 32), torch.int32), z((B, 16), torch.float64)
        self._poses, self.poses_prop = z((B, cap, 4, 4), torch.float32), z((B, cap, 4, 4), torch.float32)
        self._hint = torch.full((B, cap), -1, dtype=torch.int32, device=d)
        self._nn_idx, self._valid = z((B, cap), torch.int32), z((B, cap), torch.uint8)
        self._x, self._e, self._w, self._w_res = (z((B, cap), torch.float64) for _ in range(4))
        self._labels, self._labels_next = z((B, cap), torch.int32), z((B, cap), torch.int32)
        self._labels_prev = self._labels
        self._src, self._ridx = z((B, cap), torch.int32), z((B, cap), torch.int32)
        self._scores = z((B, self.K), torch.float64)
        self._part_rmse = z((B, 2 * ((cap + 63) // 64)), torch.float64)
        self._cl_poses = z((B, _lib.LOOP_MAX_CLUSTERS, 4, 4), torch.float32)
        self._cl_stds = z((B, _lib.LOOP_MAX_CLUSTERS, 3), torch.float32)
        self.log_frames = int(log_frames)
        self._log = z((B, self.log_frames, _lib.LOOP_LOG_DOUBLES), torch.float64)
        self.telemetry = z(16, torch.int64)  # (cumulative over the batch)
        self._stamps, self._epoch = z((B, self.K), torch.int32), 0  # sparse scoring per trajectory (include/midas_hip.h score_stamps_dev)
        self.step_count = 0   # frames enqueued (Philox counter, log row)
        self._n_host = None   # the B live counts as last read (None: ask the device)
        # what never changes between frames
        a = self._args = LoopArgs()
        a.cap = cap
        a.ctl_i, a.ctl_d = _ptr(self.ctl_i), _ptr(self.ctl_d)
        a.poses, a.poses_prop = _ptr(self._poses), _ptr(self.poses_prop)
        a.hint, a.nn_idx, a.valid = _ptr(self._hint), _ptr(self._nn_idx), _ptr(self._valid)
        a.x, a.e, a.weights, a.weights_out = _ptr(self._x), _ptr(self._e), _ptr(self._w), _ptr(self._w_res)
        a.src, a.ridx, a.scores = _ptr(self._src), _ptr(self._ridx), _ptr(self._scores)
        a.cb_poses = _ptr(self.cb_poses)
        a.cluster_poses, a.cluster_stds = _ptr(self._cl_poses), _ptr(self._cl_stds)
        a.seed, a.prune_thr, a.softmax, a.resample_mode = self.seed, self.pen_max, int(self.softmax), self.mode
        a.floor, a.eps = self.floor, self.eps
        a.telemetry, a.score_stamps = _ptr(self.telemetry), _ptr(self._stamps)
        a.topk_ties = _lib.TOPK_TIES_INDEX
        # The scratch every phase combination of a batch frame asks for, reserved now so that no frame allocates: per trajectory the
        # hand-over records of the front (32 B a particle), the block results, the cluster-moment partials (64 x 36 doubles per 256
        # particles) and cluster rows, the resample's prefix values; once, DBSCAN's cell tables (84 MB + 41 B a particle).
        nb, nb256 = (cap + 4095) // 4096, (cap + 255) // 256
        per_traj = (32 * cap + 32 * nb + 8 * 64 * 10 + 8 * 36 * 64 * nb256 + 4 * 64 * 16 + 4 * 64 * 3 + 8 * 64 + 8 * (cap + 16) + 12 * nb)
        self.ctx.call("midas_scratch_reserve", (128 << 20) + 256 * cap + B * per_traj + 64 * 256)

    # ---- state ----------------------------------------------------------------------------------------------------
    def set_particles(self, poses, labels=None):
        """Start (or restart) every trajectory: poses (B, n, 4, 4), or a list of B tensors (n_b, 4, 4) with n_b <= capacity each;
        labels likewise, default 0 like `Particles` (particle_filter.py:47).  Annealing starts over."""
        if isinstance(poses, (list, tuple)):
            poses = [torch.as_tensor(p).to(self.device, torch.float32).reshape(-1, 4, 4) for p in poses]
        else:
            poses = torch.as_tensor(poses).to(self.device, torch.float32)
            if poses.dim() != 4:
                raise MidasError(f"expected ({self.B},n,4,4) poses or a list of {self.B} sets, got {tuple(poses.shape)}")
            poses = list(poses.reshape(poses.shape[0], -1, 4, 4))
        if len(poses) != self.B:
            raise MidasError(f"{len(poses)} particle sets for a batch of {self.B} trajectories")
        if labels is not None and len(labels) != self.B:
            raise MidasError(f"{len(labels)} label sets for a batch of {self.B} trajectories")
        ns = [int(p.shape[0]) for p in poses]
        for b, n in enumerate(ns):
            if n < 1 or n > self.cap:
                raise MidasError(f"trajectory {b}: {n} particles do not fit the engine's capacity of {self.cap}")
        if labels is not None:  # every check in front of the first copy: a refused call leaves the engine as it was
            labels = [torch.as_tensor(lb).to(self.device).to(torch.int32).reshape(-1) for lb in labels]
            for b, (lb, n) in enumerate(zip(labels, ns)):
                if lb.numel() != n:
                    raise MidasError(f"trajectory {b}: {lb.numel()} labels for {n} particles")
        ci = torch.zeros((self.B, 32), dtype=torch.int32)
        self._hint.fill_(-1)
        self._labels.zero_()
        for b, (p, n) in enumerate(zip(poses, ns)):
            self._poses[b, :n].copy_(p)
            ncl = 1  # label 0 everywhere
            if labels is not None:
                self._labels[b, :n].copy_(labels[b])
                ncl = int(labels[b].max().item()) + 1
            ci[b, _lib.LOOP_I_N] = n
            ci[b, _lib.LOOP_I_NSET] = n
            ci[b, _lib.LOOP_I_NCL] = ncl
        self.ctl_d.zero_()
        self.ctl_i.copy_(ci)
        self._n_host = ns

    def project_to_codebook(self):
        """poses := codebook pose nearest to each particle (filter/filter.py:159-160), every trajectory's live set."""
        for b, n in enumerate(self.n):
            idx = ops.nn6(self.tree6, ops.se3_feature(self._poses[b, :n]))
            self._poses[b, :n].copy_(ops.gather_rows(self.cb_poses, idx))
            self._hint[b, :n].copy_(idx)

    @property
    def n(self):
        """The B live particle counts (one read-back when the host does not know them)."""
        if self._n_host is None:
            self._n_host = [int(v) for v in self.ctl_i[:, _lib.LOOP_I_N].cpu()]
        return self._n_host

    def frame_view(self, b: int):
        """Trajectory b's latest completed frame as LoopEngine.frame_view gives it (one synchronisation): its log record plus
        views of its per-particle arrays before annealing, of the annealed set and of the resampled set."""
        if self.step_count == 0:
            raise MidasError("frame_view needs a completed frame")
        if not 0 <= b < self.B:
            raise MidasError(f"trajectory {b} of a batch of {self.B}")
        rec = self.read_log(self.step_count - 1, self.step_count, rows=(b,))[0][0]
        nb, ns = rec["n"], rec["n_after"]
        rec.update(poses_prop=self.poses_prop[b, :nb], nn_idx=self._nn_idx[b, :nb], valid=self._valid[b, :nb], weights=self._w[b, :nb],
                   labels_frame=self._labels_prev[b, :nb], src=self._src[b, :ns], ridx=self._ridx[b, :ns], poses=self._poses[b, :ns],
                   weights_res=self._w_res[b, :ns], labels=self._labels[b, :ns], hint=self._hint[b, :ns],
                   ctl_i=self.ctl_i[b].cpu().numpy(), ctl_d=self.ctl_d[b].cpu().numpy())
        return rec

    # ---- one batch frame ------------------------------------------------------------------------------------------
    def step(self, odoms, codes, gts=None, u32=-1.0, multiplier: float = 1.0, dbscan=None, unit_weights: bool = False):
        """Enqueues one frame of every trajectory and reads nothing back: odoms (B,4,4), codes (B,D), gts (B,4,4) or None.
        dbscan: None = on every `cluster_every`-th frame (filter.py:182), True / False to force - for all trajectories alike."""
        phases = ALL_PHASES
        if not self.cluster:
            phases &= ~(_lib.LOOP_DBSCAN | _lib.LOOP_ANNEAL)
        elif dbscan is False or (dbscan is None and self.step_count % self.cluster_every != 0):
            phases &= ~_lib.LOOP_DBSCAN
        odoms, codes, gts = frame_operands(self.device, (self.B,), self.D, odoms, codes, gts)
        a = self._args
        a.labels, a.labels_out = _ptr(self._labels), _ptr(self._labels_next)
        a.log = C.c_void_p(self._log.data_ptr() + (self.step_count % self.log_frames) * _lib.LOOP_LOG_DOUBLES * 8)
        a.odom16, a.code, a.gt16 = _ptr(odoms), _ptr(codes), _ptr(gts)
        a.part_rmse = _ptr(self._part_rmse) if gts is not None else None
        a.u32 = float(u32)
        mul = max(float(multiplier), 1.0)
        a.std_t, a.std_r = mul * self.sig_t, mul * self.sig_r
        a.step = self.step_count
        a.unit_weights = int(bool(unit_weights))
        a.score_epoch = advance_epoch(self)
        self._keep = (odoms, codes, gts)  # keep operands alive until the stream has consumed them
        self.ctx.bind_current_stream()
        self.ctx.check(self.ctx.lib.midas_loop_step_batch(self.ctx.h, self.codebook.h, self.tree6.h, self.tree3.h, C.byref(a), int(phases),
                                                          self.B, self.log_frames * _lib.LOOP_LOG_DOUBLES))
        self._labels_prev = self._labels
        self._labels, self._labels_next = self._labels_next, self._labels
        self.step_count += 1
        self._n_host = None

    # ---- results --------------------------------------------------------------------------------------------------
    def read_log(self, first: int = 0, last: int = None, strict: bool = True, rows=None):
        """Per trajectory, LoopEngine.read_log's records of frames [first, last) - a list of B lists, one read-back - with its
        handling of the frames' condition bits.  rows: only these trajectories (a list in their order)."""
        last = self.step_count if last is None else min(last, self.step_count)
        first = max(first, last - self.log_frames)
        which = range(self.B) if rows is None else rows
        log = (self._log if rows is None else self._log[list(rows)]).cpu().numpy()
        return [log_records(log[i], first, last, strict=strict, who=f"trajectory {b}, ") for i, b in enumerate(which)]
