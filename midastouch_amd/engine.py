"""Device-resident filter engine: the reference's per-frame loop body as ONE C-ABI call per frame.

`FilterEngine.step()` is the fast path behind the north-star aliases `step()/update_weights()/
resample()` (midastouch_amd/filter.py): score codebook -> propagate -> feature -> NN -> gather score ->
softmax -> prune -> CDF -> resample -> gather, all on the GPU with no host synchronisation
(reference loop body: filter/filter.py:150-190, clustering/annealing excluded = fixed N).  With `estimate=True` an engine also
leaves the frame's pose estimate (filter.py:184-186 on the unclustered set: `eng.estimate`), one more C call behind the frame.

Two random-draw modes:
  * parity mode  - the caller supplies the host draws of the reference (torch CPU mt19937:
                   tn, rot from torch.normal in that order, then N float64 uniforms);
  * device mode  - the kernels draw from the Philox spec streams keyed by (seed, step).

The frame setup every engine form shares (single, batch, loop, shard: midastouch_amd/loop_engine.py, dist.py) lives here too:
`codebook_index`, `RESAMPLE_MODES`, `sparse_scoring`, `advance_epoch` and the operand checks.  The fixed-N engines share `_Engine`
below; the two loop engines share `loop_engine._LoopBase` (state table, cached `LoopArgs`, control-block writers, seeded frame).
"""
from __future__ import annotations

import ctypes as C
import numbers
import os

import numpy as np
import torch

from . import _lib, ops
from ._lib import EstimateArgs, LazyArgs, LazyFlushArgs, MidasError, StepArgs, _ptr


EPOCH_LIMIT = 0x3FFFFFF0  # (bits 31:30 of a stamp count the frames a listed row went unused: csrc/midas_internal.hpp)

# the reference's `resample` option -> the kernels' draw rule
RESAMPLE_MODES = {"weighted_random": _lib.RESAMPLE_MULTINOMIAL, "low_var": _lib.RESAMPLE_SYSTEMATIC,
                  "low_var_batch": _lib.RESAMPLE_SYSTEMATIC}


def advance_epoch(eng, n: int = 1) -> int:
    """First of n consecutive sparse-scoring epochs of an engine or a shard's state (`_epoch`, `_stamps`, optionally
    `_score_list`): non-zero, spaced by 2 when the holder keeps a prediction list (the value between two epochs tags the listed
    rows), never reused while the stamps live - before the 32-bit counter could wrap (2.5 days at 20k frames/s) the stamps and
    the list lengths are zeroed and the count restarts, so a stale stamp can never equal a current epoch."""
    lst = getattr(eng, "_score_list", None)
    inc = 2 if lst is not None else 1
    if eng._epoch + inc * n >= EPOCH_LIMIT:
        eng._stamps.zero_()
        if lst is not None:
            lst[:2].zero_()
        eng._epoch = 0
    first = eng._epoch + inc
    eng._epoch += inc * n
    return first


def sparse_scoring(codebook, switch: bool = True) -> bool:
    """Whether the particle kernels can score `codebook`'s rows themselves (sparse scoring, include/midas_hip.h
    score_stamps_dev: float32 rows, D in {128, 256, 512, 1024}) - and, with `switch`, whether MIDAS_DENSE_SCORES=1 (read at
    every call) leaves them to: with it every row is scored every frame.  Same scores either way."""
    return (codebook.emb.dtype == torch.float32 and codebook.D in (128, 256, 512, 1024) and
            not (switch and os.environ.get("MIDAS_DENSE_SCORES", "0") == "1"))


def codebook_index(cb_poses, cb_embeddings, mesh_vertices, device, *, rows=None, share=None):
    """The codebook as the kernels read it -> (context, float32 poses, 6-d features, NN index, embeddings, mesh index).

    cb_poses may be a tactile_tree already on the device (cb_embeddings None: its index is shared) and mesh_vertices an ops.Tree.
    share: another engine or shard backend of the same process and codebook whose poses, features, NN index and mesh index are
    used as they are (only the embeddings are built).  rows = (rank, world): only that rank's contiguous slice of the embedding
    rows (codebook-row sharding)."""
    ctx = _lib.context(torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
    d = ctx.device
    if hasattr(cb_poses, "SE3_NN") and cb_embeddings is None:  # a tactile_tree already on the device: share its index
        tt = cb_poses
        poses, feat, tree6, codebook = tt.poses, tt.logmap_pose, tt.tree, tt.codebook
    else:
        if share is not None:
            poses, feat, tree6 = share.cb_poses, share.cb_feat, share.tree6
        else:
            poses = torch.as_tensor(cb_poses).to(d, torch.float32).contiguous()
            feat = ops.se3_feature(poses)
            tree6 = ops.Tree(feat)
        emb = torch.as_tensor(cb_embeddings)
        if rows is not None:
            r, w = rows
            if emb.shape[0] % w:
                raise MidasError("codebook-row sharding needs K divisible by the number of ranks")
            k = emb.shape[0] // w
            emb = emb[r * k:(r + 1) * k]
        codebook = ops.Codebook(emb.to(d))
    if share is not None:
        tree3 = share.tree3
    else:
        tree3 = mesh_vertices if isinstance(mesh_vertices, ops.Tree) else ops.Tree(torch.as_tensor(mesh_vertices).to(d, torch.float64))
    if getattr(tree6, "_mesh", None) is not tree3:  # vertex lists of this mesh not yet on the codebook index
        tree6.attach_mesh(tree3, poses)
    return ctx, poses, feat, tree6, codebook, tree3


def operand(t, name: str, dtype, shape, device):
    """A frame operand as the C ABI reads it: on `device`, `dtype`, contiguous, exactly `shape` elements (the kernels
    take raw pointers and check nothing).  Host tensors (the reference's CPU-generator draws), float32 tactile codes
    (what the TCN emits before its .double()) and strided views are converted; a wrong element count raises."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == device and t.shape == tuple(shape) and t.is_contiguous():
        return t  # (already what the kernels read: the common case of a run() fed from device tensors)
    t = torch.as_tensor(t)
    n = 1
    for s_ in shape:
        n *= int(s_)
    if t.numel() != n:
        raise MidasError(f"{name}: expected shape {tuple(shape)} ({n} values), got {tuple(t.shape)}")
    if t.device != device or t.dtype != dtype:
        t = t.to(device=device, dtype=dtype)
    return t.contiguous().reshape(shape)


def frame_specs(lead, D):
    """(name, dtype, shape) of the odometry, tactile code and ground truth of one frame (lead = ()), or of T frames / B
    trajectories (lead = (T,) / (B,))."""
    s = "s" if lead else ""
    return (("odom" + s, torch.float32, lead + (4, 4)), ("tactile code" + s, torch.float64, lead + (D,)),
            ("gt pose" + s, torch.float32, lead + (4, 4)))


def frame_operands(device, lead, D, odom, code, gt):
    """Odometry, tactile code and ground truth (or None) as the C ABI reads them (frame_specs)."""
    so, sc, sg = frame_specs(lead, D)
    return operand(odom, *so, device), operand(code, *sc, device), operand(gt, *sg, device)


def check_motion_draws(tn, rot):
    if (tn is None) != (rot is None):
        raise MidasError("tn and rot (the motion model's host draws) come together or not at all")


class _Engine:
    """What FilterEngine and BatchFilterEngine share: the codebook index, the filter's parameters, the particle set of one
    trajectory or of B (`_lead` = (N,) or (B, N)) and the eager frame."""

    def _setup(self, cb_poses, cb_embeddings, mesh_vertices, device, lead, sig_t, sig_r, pen_max, seed, softmax, resample):
        self.ctx, self.cb_poses, self.cb_feat, self.tree6, self.codebook, self.tree3 = codebook_index(
            cb_poses, cb_embeddings, mesh_vertices, device)
        self.device = self.ctx.device
        self.K, self.D = self.codebook.K, self.codebook.D
        self.sig_t, self.sig_r, self.pen_max = float(sig_t), float(sig_r), float(pen_max)
        self.seed, self.softmax = int(seed), bool(softmax)
        self.mode = RESAMPLE_MODES[resample]
        self._lead = lead
        self.N = lead[-1]
        # what _operands makes of a frame's odom, code, gt, tn, rot and u (per trajectory for a batch)
        self._specs = frame_specs(lead[:-1], self.D) + (("tn", torch.float32, lead + (3,)), ("rot", torch.float32, lead + (3,)),
                                                        ("u", torch.float64, lead))
        self.step_count = 0
        self.use_hint = True
        # sparse scoring: only the rows that are some particle's nearest entry are scored, by the particle kernels
        # themselves (stamps of the frame that last scored a row; include/midas_hip.h score_stamps_dev).  Same scores.
        self.sparse_scores = sparse_scoring(self.codebook)
        self._epoch = 0

    def _alloc_state(self):
        """The particle set and the latest frame's outputs (the pipelined engines keep theirs double-buffered)."""
        lead, bz, d = self._lead, self._lead[:-1], self.device
        f32, f64, i32 = dict(dtype=torch.float32, device=d), dict(dtype=torch.float64, device=d), dict(dtype=torch.int32, device=d)
        self.poses = torch.zeros(lead + (4, 4), **f32)
        self.poses_prop = torch.zeros(lead + (4, 4), **f32)
        self.weights = torch.zeros(lead, **f64)      # pre-resample, masked
        self.weights_res = torch.ones(lead, **f64)   # gathered by resample
        self.nn_idx = torch.zeros(lead, **i32)
        self.hint = torch.full(lead, -1, **i32)
        self.hint_next = torch.full(lead, -1, **i32)
        self.ridx = torch.zeros(lead, **i32)
        self.status = torch.zeros(bz + (2,), **i32)
        self.rmse = torch.zeros(bz + (2,), **f64)

    # ---- per-frame pose estimate (estimate=True) -------------------------------------------------------
    def _alloc_estimate(self, on):
        """estimate=True: every frame leaves its pose estimate (filter/filter.py:184-186: the quaternion-mean centre and the
        per-axis spread of the propagated particles under the masked pre-resample weights) by one midas_pose_estimate behind the
        frame.  The output rows are allocated here, once; off, the engine holds nothing for it."""
        self._estimate_on = bool(on)
        if not on:
            return
        bz, d = self._lead[:-1], self.device
        B = bz[0] if bz else 1
        self._est_rows = (torch.zeros(bz + (4, 4), dtype=torch.float32, device=d), torch.zeros(bz + (3,), dtype=torch.float32, device=d))
        self._est = self._est_rows  # what `estimate` returns: these rows, or the last rows of a run()'s log
        a = EstimateArgs()
        a.N, a.B = self.N, B
        a.centers, a.stds = _ptr(self._est_rows[0]), _ptr(self._est_rows[1])
        self._est_args = a
        # the block partials of the moments come from the context's scratch: held before the first frame asks
        self.ctx.call("midas_scratch_reserve", B * ((self.N + 255) // 256) * 36 * 8 + 256)

    @property
    def estimate(self):
        """(centre (4,4), stds (3,)) - (B,4,4), (B,3) for a batch - float32 device tensors of the latest frame; no synchronisation
        and, on the pipelined engines, no flush.  Needs estimate=True at construction."""
        if not self._estimate_on:
            raise MidasError("the engine was built without estimate=True")
        return self._est

    def _enqueue_estimate(self, poses_prop, weights=None, tables=None, valid=None):
        a = self._est_args
        a.poses_prop, a.weights, a.tables, a.valid = _ptr(poses_prop), _ptr(weights), _ptr(tables), _ptr(valid)
        a.softmax = int(self.softmax)
        self.ctx.check(self.ctx.lib.midas_pose_estimate(self.ctx.h, C.byref(a)))
        self._est = self._est_rows

    # ---- state ----------------------------------------------------------------------------------
    def set_particles(self, poses):
        poses = torch.as_tensor(poses).to(self.device, torch.float32)
        if tuple(poses.shape) != self._lead + (4, 4):
            raise MidasError(f"expected ({','.join(map(str, self._lead))},4,4) poses, got {tuple(poses.shape)}")
        self.poses.copy_(poses)
        self.hint.fill_(-1)

    def project_to_codebook(self):
        """poses := codebook pose nearest to each particle (filter/filter.py:159-160)."""
        poses = self.poses
        idx = ops.nn6(self.tree6, ops.se3_feature(poses.view(-1, 4, 4)))
        poses.copy_(ops.gather_rows(self.cb_poses, idx).view_as(poses))
        self.hint.copy_(idx.view_as(self.hint))
        return idx

    # ---- systematic offsets in device memory ------------------------------------------------------
    def _offset_rows(self, vals):
        """One systematic offset per trajectory as the kernels read it under u32 = MIDAS_U32_FROM_U: a tensor of `u`'s shape whose
        first double of every trajectory's row holds the float32 value (the rest is never read).  vals: one value per trajectory,
        on the host or the device; enqueued on the current stream, nothing read back."""
        bz = self._lead[:-1]
        v = torch.as_tensor(vals)
        n = 1
        for b in bz:
            n *= b
        if v.numel() != n:
            raise MidasError(f"u32: expected one offset or {n} (one per trajectory), got {v.numel()}")
        buf = torch.empty(self._lead, dtype=torch.float64, device=self.device)
        buf[..., 0] = v.to(self.device).to(torch.float32).to(torch.float64).reshape(bz)
        return buf

    def _u32_rows(self, u, u32):
        """A frame's `u32` as given -> (u, u32) as the C ABI takes them: a number is the offset of every trajectory (< 0: Philox, keyed
        by seed + trajectory) - today's meaning; B values (a host or device tensor, a list) are one offset per trajectory, handed
        over in device memory: row b resamples as if run alone with u32 = values[b]."""
        if isinstance(u32, numbers.Real) or (isinstance(u32, (torch.Tensor, np.ndarray)) and u32.ndim == 0):
            return u, float(u32)
        if self.mode != _lib.RESAMPLE_SYSTEMATIC:
            raise MidasError("u32 per trajectory is the systematic resampler's offset: resample='low_var' / 'low_var_batch' only")
        return self._offset_rows(u32), _lib.U32_FROM_U

    # ---- one frame ------------------------------------------------------------------------------
    def _operands(self, odom, code, gt, tn, rot, u):
        """A frame's operands as the C ABI reads them: per trajectory odom (4,4), code (D,), gt (4,4), tn / rot (N,3), u (N,)."""
        check_motion_draws(tn, rot)
        d, (so, sc, sg, st, sr, su) = self.device, self._specs
        return (operand(odom, *so, d), operand(code, *sc, d), operand(gt, *sg, d), operand(tn, *st, d), operand(rot, *sr, d),
                operand(u, *su, d))

    def _eager_step(self, call, odom, code, gt, tn, rot, u, u32, std_t, std_r, *batch):
        """The frame by one C call (midas_filter_step / midas_filter_step_batch, whose trailing argument is B)."""
        odom, code, gt, tn, rot, u = self._operands(odom, code, gt, tn, rot, u)
        a = StepArgs()
        a.N = self.N
        a.poses_in, a.poses_prop, a.poses_out = _ptr(self.poses), _ptr(self.poses_prop), _ptr(self.poses)
        a.weights, a.weights_out = _ptr(self.weights), _ptr(self.weights_res)
        a.hint_in = _ptr(self.hint) if self.use_hint else None
        a.nn_idx, a.hint_out, a.ridx = _ptr(self.nn_idx), _ptr(self.hint_next), _ptr(self.ridx)
        a.odom16, a.code, a.gt16 = _ptr(odom), _ptr(code), _ptr(gt)
        a.rmse = _ptr(self.rmse) if gt is not None else None
        a.tn, a.rot, a.u, a.u32 = _ptr(tn), _ptr(rot), _ptr(u), float(u32)
        a.std_t, a.std_r, a.seed, a.step = std_t, std_r, self.seed, self.step_count
        a.prune_thr, a.softmax, a.resample_mode = self.pen_max, int(self.softmax), self.mode
        a.status, a.telemetry = _ptr(self.status), _ptr(self.telemetry)
        if self.sparse_scores:
            a.score_stamps, a.score_epoch = _ptr(self._stamps), advance_epoch(self)
        self._keep = (odom, code, gt, tn, rot, u)  # keep operands alive until the stream has consumed them
        self.ctx.bind_current_stream()
        self.ctx.check(call(self.ctx.h, self.codebook.h, self.tree6.h, self.tree3.h, C.byref(a), *batch))
        if self._estimate_on:
            self._enqueue_estimate(self.poses_prop, weights=self.weights)
        self.hint, self.hint_next = self.hint_next, self.hint
        self.step_count += 1


class FilterEngine(_Engine):
    def __init__(self, cb_poses, cb_embeddings, mesh_vertices, num_particles: int, *, sig_t=2e-4, sig_r=0.5,
                 pen_max=0.002, seed=4000, softmax=True, resample="weighted_random", device=None, estimate: bool = False):
        N = int(num_particles)
        self._setup(cb_poses, cb_embeddings, mesh_vertices, device, (N,), sig_t, sig_r, pen_max, seed, softmax, resample)
        # 16 cumulative counters ([0], [1] = tree-search fallbacks); with MIDAS_ABLATE=4 (profiling) the kernel
        # also keeps 16 statistics slots per wave behind them
        extra = 16 * ((N + 15) // 16) if int(os.environ.get("MIDAS_ABLATE", "0")) & 4 else 0
        self.telemetry = torch.zeros(16 + extra, dtype=torch.int64, device=self.device)
        self._stamps = torch.zeros(self.K, dtype=torch.int32, device=self.device)
        self._alloc_state()
        self._alloc_estimate(estimate)

    # ---- one frame ------------------------------------------------------------------------------
    def step(self, odom, code, gt=None, tn=None, rot=None, u=None, u32=-1.0, multiplier: float = 1.0):
        """Runs one frame; results stay on the device (self.poses, self.weights, self.ridx ...)."""
        mul = max(float(multiplier), 1.0)  # motionModel clamps multiplier >= 1 (particle_filter.py:365-366)
        self._eager_step(self.ctx.lib.midas_filter_step, odom, code, gt, tn, rot, u, u32, mul * self.sig_t, mul * self.sig_r)

    # ---- profiling --------------------------------------------------------------------------------
    def profile(self, on, only_slot: int = None):
        """HIP-event timing of the step's kernels: all of them, or only slot `only_slot` (least perturbation)."""
        self.ctx.call("midas_profile_enable", 0 if not on else (1 if only_slot is None else 2 + int(only_slot)))

    def profile_read(self, reset=True):
        ms = (C.c_double * _lib.PROF_SLOTS)()
        calls = C.c_int64()
        self.ctx.call("midas_profile_read", ms, C.byref(calls), int(reset))
        names = [self.ctx.lib.midas_profile_slot_name(i).decode() for i in range(_lib.PROF_SLOTS)]
        return {n: ms[i] for i, n in enumerate(names) if n}, calls.value


def _materialised(name):
    """Attribute that belongs to the resampled particle set: reading it materialises a pending resample first."""

    def get(self):
        self.flush()
        return getattr(self, "_" + name)

    def put(self, value):
        setattr(self, "_" + name, value)

    return property(get, put)


class _FoldedResample:
    """The folded-resample state machine of PipelinedFilterEngine and PipelinedBatchFilterEngine, written for one trajectory or B
    (`_lead` = (N,) or (B, N)) and the entry points `_lazy_calls` names (the batch ones take B as their trailing argument).

    The resampled particle set of the latest frame exists only implicitly (tables + draws) until somebody reads it: `poses`,
    `weights`, `weights_res`, `hint`, `ridx` and `status` materialise it on access (`flush()`); `nn_idx`, `poses_prop` and `rmse`
    of the latest frame are always there (double buffers, `_cur` is the latest frame's set)."""

    poses = _materialised("poses")
    weights = _materialised("weights")
    weights_res = _materialised("weights_res")
    hint = _materialised("hint")
    ridx = _materialised("ridx")

    @property
    def status(self):
        self.flush()
        return self._st[self._cur]

    @property
    def nn_idx(self):
        return self._nn[self._cur]

    @property
    def poses_prop(self):
        return self._prop[self._cur]

    @property
    def rmse(self):
        """rmse of the latest frame's propagated particles (filter.py:164): written by the frame itself, no materialisation."""
        return self._rmse_last[..., :2] if self._pending else self._rmse

    def _alloc_state(self):
        lead, bz, N, d = self._lead, self._lead[:-1], self.N, self.device
        f32, f64, i32 = dict(dtype=torch.float32, device=d), dict(dtype=torch.float64, device=d), dict(dtype=torch.int32, device=d)
        self._poses = torch.zeros(lead + (4, 4), **f32)
        self._weights = torch.zeros(lead, **f64)
        self._weights_res = torch.ones(lead, **f64)
        self._hint = torch.full(lead, -1, **i32)
        self._ridx = torch.zeros(lead, **i32)
        self._rmse = torch.zeros(bz + (2,), **f64)
        self._prop = [torch.zeros(lead + (4, 4), **f32) for _ in range(2)]
        self._nn = [torch.zeros(lead, **i32) for _ in range(2)]
        self._st = [torch.zeros(bz + (2,), **i32) for _ in range(2)]
        self._valid = torch.zeros(lead, dtype=torch.uint8, device=d)
        lib = self.ctx.lib
        B = bz[0] if bz else 1
        self._tables = torch.zeros(B * int(lib.midas_lazy_tables_doubles(N)), **f64)  # one block per trajectory
        # guide tables of the folded resample's search (midas_lazy_args.guide_dev, one trajectory; MIDAS_GUIDE=0: the three-line
        # search alone)
        self._guide = (torch.zeros(int(lib.midas_lazy_guide_bytes(N)), dtype=torch.uint8, device=d)
                       if not bz and os.environ.get("MIDAS_GUIDE", "1") != "0" else None)
        self._scores = torch.zeros(bz + (self.K,), **f64)
        self._part_rmse = torch.zeros(bz + (2 * ((N + 63) // 64),), **f64)
        self._rmse_frame = torch.zeros(bz + (3,), **f64)
        self._rmse_last = self._rmse_frame   # where the latest frame left {rmse_t, rmse_r, clock}: _rmse_frame or a row of the run log
        # prediction lists of the sparse scoring (include/midas_hip.h score_list_dev, one trajectory): the rows a frame used are
        # scored for the next frame by streaming workgroups of its front launch.  MIDAS_SCORE_LIST=0: every row by its first particle.
        self._score_list = torch.zeros(2 + 2 * self.K, **i32) \
            if not bz and self.sparse_scores and os.environ.get("MIDAS_SCORE_LIST", "1") != "0" and N >= 16 else None
        self._lazy_step, self._lazy_flush = (getattr(lib, name) for name in self._lazy_calls)
        self._batch = bz
        self._cur, self._draw, self._had_gt = 0, (None, -1.0, 0), False
        self._pending, self._flushed = False, True

    def set_particles(self, poses):
        self._pending, self._flushed = False, True
        super().set_particles(poses)

    def project_to_codebook(self):
        self.flush()
        idx = super().project_to_codebook()
        if self._score_list is not None:
            # every particle's nearest entry is known: the first frame's rows go on the prediction list right away (they would
            # otherwise all be claimed by whichever particle wave touches them first - up to 64 rows a wave after a wide start)
            self.ctx.bind_current_stream()
            self.ctx.call("midas_score_list_seed", self.K, _ptr(self._stamps), advance_epoch(self), _ptr(self._score_list), self.N, _ptr(idx))
        return idx

    def _wait_draws(self):
        """The pending frame's draws may still be in flight on the generator's stream (TorchCpuStream(s)): order this stream
        behind them."""
        ev = getattr(self, "_draw_event", None)
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
            self._draw_event = None

    def _lazy_args(self, cur):
        """The buffers of a frame that follows the frame on buffer set `cur` (no per-frame values)."""
        nxt = cur ^ 1
        a = LazyArgs()
        a.N = self.N
        a.poses_prop_prev, a.nn_idx_prev, a.status_prev = _ptr(self._prop[cur]), _ptr(self._nn[cur]), _ptr(self._st[cur])
        a.poses_prop, a.nn_idx, a.valid, a.status = _ptr(self._prop[nxt]), _ptr(self._nn[nxt]), _ptr(self._valid), _ptr(self._st[nxt])
        a.tables, a.scores, a.guide = _ptr(self._tables), _ptr(self._scores), _ptr(self._guide)
        a.poses_in, a.telemetry = _ptr(self._poses), _ptr(self.telemetry)
        return a

    def _lazy_frame(self, odom, code, gt, tn, rot, u, u32, own_u, u_event, std_t, std_r):
        """One frame on the other buffer set with the pending resample folded in.  u: this frame's resample draws, consumed by
        the next frame or by flush() - a caller's tensor is copied (it may be mutated before then), one generated here (own_u)
        is kept as it is; u_event: their event on the generator's stream."""
        self._wait_draws()
        odom, code, gt, tn, rot, u = self._operands(odom, code, gt, tn, rot, u)
        cur = self._cur
        fold = self._pending and not self._flushed
        a = self._lazy_args(cur)
        a.part_rmse = _ptr(self._part_rmse) if gt is not None else None
        a.resample_prev = int(fold)
        a.hint_in = _ptr(self._hint) if self.use_hint else None
        pu, pu32, pstep = self._draw
        a.resample_mode, a.u_prev, a.u32_prev, a.step_prev = self.mode, _ptr(pu), float(pu32), int(pstep)
        a.ridx = _ptr(self._ridx) if fold else None
        a.odom16, a.code, a.gt16 = _ptr(odom), _ptr(code), _ptr(gt)
        a.tn, a.rot = _ptr(tn), _ptr(rot)
        a.std_t, a.std_r, a.seed, a.step = std_t, std_r, self.seed, self.step_count
        a.prune_thr, a.softmax = self.pen_max, int(self.softmax)
        if self.sparse_scores:
            a.score_stamps, a.score_epoch, a.score_list = _ptr(self._stamps), advance_epoch(self), _ptr(self._score_list)
        a.rmse = _ptr(self._rmse_frame) if gt is not None else None
        self._keep = (odom, code, gt, tn, rot, pu)
        self.ctx.bind_current_stream()
        self.ctx.check(self._lazy_step(self.ctx.h, self.codebook.h, self.tree6.h, self.tree3.h, C.byref(a), *self._batch))
        if self._estimate_on:  # from where the frame left its weights (the tables): nothing is materialised
            self._enqueue_estimate(self._prop[cur ^ 1], tables=self._tables, valid=self._valid)
        self._draw = (None if u is None else (u if own_u else u.clone()), float(u32), self.step_count)
        self._draw_event = u_event
        self._rmse_last = self._rmse_frame
        self._had_gt = gt is not None
        self._pending, self._flushed, self._cur = True, False, cur ^ 1
        self.step_count += 1

    def flush(self):
        """Materialise the latest frame's resample (poses, weights, weights_res, hint, ridx, status, rmse)."""
        if not self._pending or self._flushed:
            return
        self._wait_draws()
        cur = self._cur
        u, u32, stp = self._draw
        a = LazyFlushArgs()
        a.N = self.N
        a.tables, a.valid, a.nn_idx, a.poses_prop = _ptr(self._tables), _ptr(self._valid), _ptr(self._nn[cur]), _ptr(self._prop[cur])
        a.status = _ptr(self._st[cur])
        a.part_rmse = _ptr(self._part_rmse) if self._had_gt else None
        a.softmax, a.resample_mode, a.u, a.u32 = int(self.softmax), self.mode, _ptr(u), float(u32)
        a.seed, a.step = self.seed, int(stp)
        a.weights, a.ridx, a.poses_out = _ptr(self._weights), _ptr(self._ridx), _ptr(self._poses)
        a.weights_out, a.hint_out = _ptr(self._weights_res), _ptr(self._hint)
        a.rmse = _ptr(self._rmse) if self._had_gt else None
        self.ctx.bind_current_stream()
        self.ctx.check(self._lazy_flush(self.ctx.h, C.byref(a), *self._batch))
        self._flushed = True


class PipelinedFilterEngine(_FoldedResample, FilterEngine):
    """FilterEngine with the resample of frame t folded into the front kernel of frame t+1 (midas_lazy_step).

    Slot n of the next frame is particle src(n) of this one, a per-slot dependence: the resampler's search and
    gather run as a prologue of the next particle update, the resampled poses never travel through HBM and a
    frame is two launches instead of three.  The resampled particle set of the latest frame therefore exists only
    implicitly (tables + draws) until somebody reads it: `poses`, `weights`, `weights_res`, `hint`, `ridx`, `status`
    and `rmse` materialise it on access (`flush()`, the same kernel as the eager engine's tail - bit-identical
    results); `nn_idx` and `poses_prop` of the latest frame are always there.  A caller that looks at the particles
    every frame gets the eager engine's launches; one that only steps gets the pipelined ones.
    Needs a float32 codebook with D in {128, 256, 512, 1024} and N <= 1 M (MidasError otherwise: use FilterEngine).
    """

    _lazy_calls = ("midas_lazy_step", "midas_lazy_flush")

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not sparse_scoring(self.codebook, switch=False) or self.N > (1 << 20):
            raise MidasError("PipelinedFilterEngine needs a float32 codebook with D in {128,256,512,1024} and N <= 2^20")

    def check(self):
        """Raises if a frame's tail reported its tables undefined (status bit 4, value 16: a wave of the grouped tail waited
        0.2 s for its block's records - include/midas_hip.h, midas_lazy_args.status_dev).  One small read-back."""
        st = torch.stack([self._st[0][0], self._st[1][0]]).cpu()
        if int(st[0]) & 16 or int(st[1]) & 16:
            raise MidasError("grouped tail: a wave did not receive its block's records in time - the frame's CDF tables are undefined "
                             "(foreign work on the device?); MIDAS_TAIL_GROUPED=0 selects the form without waits")

    def seed_torch_stream(self, seed, motion: bool = False):
        """Resample draws from the device replica of torch's CPU generator under torch.manual_seed(seed) (torch_rng.py):
        every step() without explicit `u` then resamples with the uniforms torch.multinomial would consume
        (modules/particle_filter.py:245) - with resample="low_var" every step() without an explicit `u32 >= 0` takes the systematic
        resampler's one float32 `torch.rand(1)` (:291) instead, which stays in device memory (MIDAS_U32_FROM_U).  With host motion noise (tn, rot given) the stream first steps over the words those
        two torch.normal calls took, so it stays aligned with a host generator seeded alike.
        motion=True: the motion noise comes from the stream too - `torch.normal(0, sig_t, (N, 3))`, `torch.normal(0, sig_r, (N, 3))`
        in front of the resampler's uniforms, the reference's order (:326-335, :245) - i.e. EVERY draw of a frame is the one a
        seeded run of the reference takes, generated on the device (unit normals a frame ahead, scaled where they are used).
        The stream draws its N uniforms (or its one offset) EVERY frame, a frame ahead of the status they are used under: the reference's resampler draws
        none on a frame whose weights are all zero or hold a NaN (:237-241), so behind such a guard frame this stream is no longer
        the reference's (LoopEngine.seed_torch_stream skips the draw there).
        seed=None: back to Philox."""
        from .torch_rng import TorchCpuStream
        self.torch_stream = None if seed is None else TorchCpuStream(seed, self.device)
        self.torch_motion = bool(motion) and seed is not None
        self._unit_noise = None  # (tn, rot, event): unit normals of the NEXT frame, drawn behind this frame's uniforms
        return self.torch_stream

    def step(self, odom, code, gt=None, tn=None, rot=None, u=None, u32=-1.0, multiplier: float = 1.0):
        stream = getattr(self, "torch_stream", None)
        own_u, u_event = False, None  # own_u: generated here (a buffer nobody else holds): kept for the folded frame without a copy
        systematic = self.mode == _lib.RESAMPLE_SYSTEMATIC
        if stream is not None and (float(u32) < 0.0 if systematic else u is None):
            stream_motion = False
            # the resampler's draw of this frame: N float64 uniforms, or the systematic resampler's one float32 offset
            draw = ("rand32",) if systematic else ("rand64", self.N)
            if tn is not None:
                stream.skip_normal(3 * self.N).skip_normal(3 * self.N)
            elif getattr(self, "torch_motion", False):
                stream_motion = True
                # the frame's own normals: std = 1 draws scaled here - fl(n x std) is what ATen's fused multiply-add with mean 0 gives -
                # so that they can be drawn a frame ahead whatever `multiplier` the caller passes then
                if self._unit_noise is None:
                    a, _ = stream.normal_async(0.0, 1.0, (self.N, 3))
                    b, ev = stream.normal_async(0.0, 1.0, (self.N, 3))
                    self._unit_noise = (a, b, ev)
                a, b, ev = self._unit_noise
                if ev is not None:
                    torch.cuda.current_stream(self.device).wait_event(ev)
                mul = max(float(multiplier), 1.0)
                tn, rot = a * (mul * self.sig_t), b * (mul * self.sig_r)
            # this frame's draws are consumed by the NEXT launch (the folded resample) or by flush(): generated beside this
            # frame's kernels on the generator's own stream, waited for where they are read
            own_u = True
            if stream_motion:
                # ... together with the next frame's unit normals, which follow them in the stream: one walk of the generator
                # (midas_mt19937_draws) instead of three
                (u, a, b), ev = stream.draws_async([draw, ("normal", 0.0, 1.0, (self.N, 3)), ("normal", 0.0, 1.0, (self.N, 3))])
                u_event = ev
                self._unit_noise = (a, b, ev)
            elif systematic:
                (u,), u_event = stream.draws_async([draw])
            else:
                u, u_event = stream.rand64_async(self.N)
            if systematic:  # the offset into the row the kernels read, on this stream behind the draw
                if u_event is not None:
                    torch.cuda.current_stream(self.device).wait_event(u_event)
                u, u32, u_event = self._offset_rows(u), _lib.U32_FROM_U, None
        mul = max(float(multiplier), 1.0)
        self._lazy_frame(odom, code, gt, tn, rot, u, u32, own_u, u_event, mul * self.sig_t, mul * self.sig_r)

    def run(self, odoms, codes, gts=None):
        """T frames by ONE C-ABI call (midas_lazy_run; device draws): odoms (T,4,4) f32, codes (T,D) f64, gts (T,4,4) f32 or
        None.  Returns the (T,3) float64 device tensor of per-frame {rmse_t, rmse_r, device clock in us at the frame's end}
        when gts is given.  Equivalent to T
        calls of step() - same kernels, same results - without the per-frame turn-around through Python."""
        d = self.device
        T = int(torch.as_tensor(odoms).shape[0])
        odoms, codes, gts = frame_operands(d, (T,), self.D, odoms, codes, gts)
        cur, nxt = self._cur, self._cur ^ 1
        fold = self._pending and not self._flushed
        # the argument block with every pointer that does not change from call to call, one per buffer parity, built once (the
        # timed region of a caller starts before this call: what is set up here is time the device idles)
        # (keyed on the buffers' addresses: a caller that rebinds one - `eng.poses = t`, `eng.telemetry = ...` - gets a fresh block)
        bufs = (self._prop[cur], self._nn[cur], self._st[cur], self._prop[nxt], self._nn[nxt], self._valid, self._st[nxt], self._tables,
                self._scores, self._guide, self._poses, self.telemetry)
        sig = tuple(0 if b is None else b.data_ptr() for b in bufs)
        cache = self.__dict__.setdefault("_run_args", {})
        a, have = cache.get(cur, (None, None))
        if have != sig:
            a = self._lazy_args(cur)  # (ridx and u_prev stay NULL: device draws, the ridx of a folded frame are not kept)
            cache[cur] = (a, sig)
        a.part_rmse = _ptr(self._part_rmse) if gts is not None else None
        a.resample_prev = int(fold)
        a.hint_in = _ptr(self._hint) if self.use_hint else None
        self._wait_draws()
        pu, pu32, pstep = self._draw
        if pu is not None:
            raise MidasError("run() continues with device draws: the pending frame was stepped with host uniforms - flush() first")
        a.resample_mode, a.u32_prev, a.step_prev = self.mode, float(pu32), int(pstep)
        a.odom16, a.code, a.gt16 = _ptr(odoms), _ptr(codes), _ptr(gts)
        a.std_t, a.std_r = self.sig_t, self.sig_r
        a.seed, a.step = self.seed, self.step_count
        a.prune_thr, a.softmax = self.pen_max, int(self.softmax)
        if self.sparse_scores:  # (a caller may switch the scoring form between calls)
            a.score_stamps, a.score_epoch, a.score_list = _ptr(self._stamps), advance_epoch(self, T), _ptr(self._score_list)
        else:
            a.score_stamps, a.score_epoch, a.score_list = None, 0, None
        # a FRESH tensor per call (caching allocator: no launch, no fill - every row is written by its frame): the log belongs
        # to the caller and stays valid across later run() / step() calls; the engine keeps a reference for `rmse`
        log = torch.empty((T, 3), dtype=torch.float64, device=d) if gts is not None else None
        self._keep = (odoms, codes, gts, log)
        self.ctx.bind_current_stream()
        if self._estimate_on:  # every frame's estimate, enqueued behind its tail inside the same call; fresh tensors like the log
            ec = torch.empty((T, 4, 4), dtype=torch.float32, device=d)
            es = torch.empty((T, 3), dtype=torch.float32, device=d)
            self.ctx.check(self.ctx.lib.midas_lazy_run_estimate(self.ctx.h, self.codebook.h, self.tree6.h, self.tree3.h, C.byref(a), T,
                                                                _ptr(log), _ptr(ec), _ptr(es)))
            self.estimate_log = (ec, es)
            self._est = (ec[T - 1], es[T - 1])
        else:
            self.ctx.check(self.ctx.lib.midas_lazy_run(self.ctx.h, self.codebook.h, self.tree6.h, self.tree3.h, C.byref(a), T, _ptr(log)))
        self.step_count += T
        if log is not None:
            self._rmse_last = log[T - 1]
        self._draw = (None, -1.0, self.step_count - 1)
        self._had_gt = gts is not None
        self._pending, self._flushed = True, False
        self._cur = nxt if T % 2 else cur
        return log


class BatchFilterEngine(_Engine):
    """B independent trajectories against one codebook, one C-ABI call per frame of the whole batch
    (BASELINE config 5, "throughput mode": SURVEY.md 8(e) batch mode).

    State tensors carry a leading batch dimension; everything but the scoring is the same kernels as the single-trajectory
    engine with the trajectory as grid.y.  Device-mode Philox streams are keyed by b*N + n.

    `scores` chooses how the B tactile codes of a frame are scored:
    - "auto" (default): sparse per trajectory (score stamps: the particle waves score the rows they need with the float64
      arithmetic of the single-trajectory step - exact to `oracle.score_codebook`) for a float32 codebook with D in
      {128, 256, 512, 1024}, unless MIDAS_DENSE_SCORES=1; otherwise one dense pass over the codebook - on the matrix cores in
      float32 (`midas_score_batch`, exact to `oracle.score_codebook_batch`, ~1e-7 from the float64 scores) where it applies,
      the float64 GEMV loop otherwise.
    - "dense_f64": one dense pass on the matrix cores in float64 (`midas_score_batch_f64`) for any codebook - bit-identical
      to `oracle.score_codebook` and to the single-trajectory engine's scores.
    """

    def __init__(self, cb_poses, cb_embeddings, mesh_vertices, batch: int, num_particles: int, *, sig_t=1e-4, sig_r=0.5,
                 pen_max=0.002, seed=4000, softmax=True, resample="weighted_random", device=None, scores="auto",
                 estimate: bool = False):
        if scores not in ("auto", "dense_f64"):
            raise MidasError(f"scores must be 'auto' or 'dense_f64', got {scores!r}")
        B, N = int(batch), int(num_particles)
        self._setup(cb_poses, cb_embeddings, mesh_vertices, device, (B, N), sig_t, sig_r, pen_max, seed, softmax, resample)
        self.B = B
        extra = 16 * B * ((N + 63) // 64) if int(os.environ.get("MIDAS_ABLATE", "0")) & 4 else 0  # per-wave statistics (profiling)
        self.telemetry = torch.zeros(16 + extra, dtype=torch.int64, device=self.device)
        # sparse scoring per trajectory (B x K stamps): the particle waves score the rows their trajectory needs with the
        # float64 arithmetic of the single-trajectory step; MIDAS_DENSE_SCORES=1 keeps the matrix-core pass over all rows
        if scores == "dense_f64":  # no stamps: every frame is one float64 pass over all rows on the matrix cores
            self.sparse_scores = False
            self.codebook.set_batch_precision("f64")
        self._stamps = torch.zeros((B, self.K), dtype=torch.int32, device=self.device) if self.sparse_scores else None
        self._alloc_state()
        self._alloc_estimate(estimate)

    def seed_torch_streams_low_var(self, seeds, motion: bool = False, pieces: int = 0):
        """seed_torch_streams for an engine built with resample="low_var" / "low_var_batch": the resampler's draw of trajectory b is
        stream b's one float32 `torch.rand(1)` a frame, the systematic resampler's offset (particle_filter.py:291), which stays in
        device memory (MIDAS_U32_FROM_U); `motion`, the word skipping for host tn / rot and the limitation behind guard frames are
        seed_torch_streams'.  A method of its own: seed_torch_streams on a systematic engine refuses, as it always did."""
        return self.seed_torch_streams(seeds, motion, pieces, _systematic=True)

    def seed_torch_streams(self, seeds, motion: bool = False, pieces: int = 0, _systematic: bool = False):
        """Trajectory b draws from the device replica of torch's CPU generator under torch.manual_seed(seeds[b]) - B seeded runs of
        the reference, one process each (TorchCpuStreams; PipelinedFilterEngine.seed_torch_stream for one trajectory).  `seeds`: B
        ints, or B torch.Generators continued where they stand (from_host), or None: back to Philox.
        motion=False: every step() without `u` resamples trajectory b with the uniforms torch.multinomial(w_b.double(), N, True)
        would consume on stream b (modules/particle_filter.py:245) - after seed_torch_streams_low_var (an engine built with
        resample="low_var"; this method refuses such an engine, as it always did) every step() without offsets of the
        caller's (`u32` >= 0 or B values) with stream b's one float32 `torch.rand(1)`, the systematic resampler's offset (:291), which
        stays in device memory; with host tn / rot the streams first step over the words of the
        two torch.normal((N, 3)) calls.  motion=True: tn, rot and u all come from the streams in the reference's order
        (torch.normal(0, sig_t, (N, 3)), torch.normal(0, sig_r, (N, 3)), N float64 uniforms: :326-335, :245) - unit normals, scaled
        by sig_t / sig_r where they are used (fl(n x std): ATen's fused multiply-add with mean 0) - and explicit tn / rot / u are an
        error.  One walk of the generators per frame; the context's scratch for it is reserved here.  `pieces` (TorchCpuStreams'):
        0 by default - the jump costs B x pieces x 39 workgroups of 78 KB LDS, and at c5 (B = 64) it takes 0.42 ms where the 64
        sequential walks, side by side, take 37 us (the mt19937 paragraph).
        The streams draw their N uniforms (or their one offset) EVERY frame, a frame ahead of the status they are used under: the reference's resampler draws
        none on a frame whose weights are all zero or hold a NaN (:237-241), so behind such a guard frame a row's stream is no longer
        the reference's (BatchLoopEngine.seed_torch_streams skips the draw there, per row).
        After a run, `torch_streams.to_host(b, g)` hands stream b back to a host generator."""
        self._unit_noise = None  # (tn, rot, event): unit normals of the NEXT frame (the pipelined engine draws them a frame ahead)
        if seeds is None:
            self.torch_streams, self.torch_motion = None, False
            return None
        seeds = list(seeds)
        if len(seeds) != self.B:
            raise MidasError(f"seed_torch_streams: {len(seeds)} seeds for {self.B} trajectories")
        if _systematic != (self.mode == _lib.RESAMPLE_SYSTEMATIC):
            if _systematic:
                raise MidasError("seed_torch_streams_low_var is the systematic resampler's: resample='low_var' / 'low_var_batch' only")
            raise MidasError("seeded torch streams reproduce torch.multinomial's draws: resample='weighted_random' only - the systematic "
                             "resampler's one float32 torch.rand(1) a frame: seed_torch_streams_low_var")
        from .torch_rng import TorchCpuStreams
        st = TorchCpuStreams(seeds, self.device, pieces=pieces)
        N = self.N
        frame = [("normal", 0.0, 1.0, (N, 3)), ("normal", 0.0, 1.0, (N, 3)), self._resampler_draw()] if motion else [self._resampler_draw()]
        st.reserve(frame)
        self.torch_streams, self.torch_motion = st, bool(motion)
        return st

    def _resampler_draw(self):
        """The resampler's draw of one frame as a TorchCpuStreams item: N float64 uniforms (torch.multinomial, particle_filter.py:245)
        or the systematic resampler's one float32 offset (torch.rand(1), :291)."""
        return ("rand64", self.N) if self.mode == _lib.RESAMPLE_MULTINOMIAL else ("rand32",)

    def _resampler_rows(self, u, ev):
        """What the streams drew for the resampler -> (u, u32, event) as the frame takes them: the uniforms as they are, or the B
        offsets in the rows the kernels read (MIDAS_U32_FROM_U), written on this stream behind the draw."""
        if self.mode == _lib.RESAMPLE_MULTINOMIAL:
            return u, -1.0, ev
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
        return self._offset_rows(u), _lib.U32_FROM_U, None

    def _stream_draws(self, tn, rot, u, u32=-1.0):
        """This frame's draws from the seeded streams (seed_torch_streams): (tn, rot, u, u32, event of u or None); without streams
        the caller's, `u32` as _u32_rows makes it."""
        st = getattr(self, "torch_streams", None)
        systematic = self.mode == _lib.RESAMPLE_SYSTEMATIC
        own = not (isinstance(u32, numbers.Real) and float(u32) < 0.0) if systematic else u is not None  # the caller's resampler draws
        if st is None or (own and not self.torch_motion):
            # (no streams, or the caller's uniforms / offsets: the streams are not used this frame)
            return (tn, rot) + self._u32_rows(u, u32) + (None,)
        B, N = self.B, self.N
        if self.torch_motion:
            if tn is not None or rot is not None or u is not None or own:
                raise MidasError("seed_torch_streams(motion=True): the streams draw tn, rot and u (the systematic offset too) - passing "
                                 "them would desynchronise the streams from the reference's")
            return self._seeded_frame()
        if tn is not None:
            st.skip_normal(3 * N).skip_normal(3 * N)
        (u,), ev = st.draws_async([self._resampler_draw()])
        return (tn, rot) + self._resampler_rows(u, ev)

    def _seeded_frame(self):
        """motion=True: the frame's normals and uniforms by one walk (the eager step reads all three at once)."""
        N = self.N
        (a, b, u), ev = self.torch_streams.draws_async([("normal", 0.0, 1.0, (N, 3)), ("normal", 0.0, 1.0, (N, 3)), self._resampler_draw()])
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
        return (a * self.sig_t, b * self.sig_r) + self._resampler_rows(u, None)

    def step(self, odoms, codes, gts=None, tn=None, rot=None, u=None, u32=-1.0):
        """odoms (B,4,4) f32, codes (B,D) f64, gts (B,4,4) f32 or None; optional host draws tn/rot (B,N,3), u (B,N); u32: the
        systematic offset of every trajectory (a number; < 0: Philox) or B of them, one per trajectory (_u32_rows)."""
        check_motion_draws(tn, rot)  # (before the streams draw)
        tn, rot, u, u32, ev = self._stream_draws(tn, rot, u, u32)
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
        self._eager_step(self.ctx.lib.midas_filter_step_batch, odoms, codes, gts, tn, rot, u, u32, self.sig_t, self.sig_r, self.B)


class PipelinedBatchFilterEngine(_FoldedResample, BatchFilterEngine):
    """BatchFilterEngine with every trajectory's resample folded into the next frame's front kernel (midas_lazy_step_batch):
    two launches per batch frame - the front with the trajectory as grid.y (one-wave workgroups, per-wave resample tables)
    and the LDS-free tail - instead of particle update + tail + resample-gather.  As with PipelinedFilterEngine the
    resampled particle set of the latest frame is implicit until somebody reads it: `poses`, `weights`, `weights_res`,
    `hint`, `ridx`, `status` materialise it (`flush()`, bit-identical to BatchFilterEngine's), `nn_idx` / `poses_prop` /
    `rmse` of the latest frame are always there.  Needs sparse scoring (float32 codebook, D in {128, 256, 512, 1024}) and
    16 <= N <= 262144 particles per trajectory."""

    _lazy_calls = ("midas_lazy_step_batch", "midas_lazy_flush_batch")

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.sparse_scores or self.N < 16 or self.N > 262144:
            raise MidasError("PipelinedBatchFilterEngine needs a float32 codebook with D in {128,256,512,1024} (sparse scoring) "
                             "and 16 <= N <= 262144")

    def _seeded_frame(self):
        """motion=True: this frame's normals were drawn a frame ahead, behind the previous frame's uniforms; this frame's uniforms
        (consumed by the NEXT launch's folded resample or by flush()) and the next frame's normals follow them in one walk, beside
        this frame's kernels on the generators' own stream."""
        N, st = self.N, self.torch_streams
        if self._unit_noise is None:
            (a, b), ev = st.draws_async([("normal", 0.0, 1.0, (N, 3)), ("normal", 0.0, 1.0, (N, 3))])
            self._unit_noise = (a, b, ev)
        a, b, ev = self._unit_noise
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
        tn, rot = a * self.sig_t, b * self.sig_r
        (u, a, b), ev = st.draws_async([self._resampler_draw(), ("normal", 0.0, 1.0, (N, 3)), ("normal", 0.0, 1.0, (N, 3))])
        self._unit_noise = (a, b, ev)
        return (tn, rot) + self._resampler_rows(u, ev)

    def step(self, odoms, codes, gts=None, tn=None, rot=None, u=None, u32=-1.0):
        check_motion_draws(tn, rot)  # (before the streams draw)
        own_u = u is None
        tn, rot, u, u32, u_event = self._stream_draws(tn, rot, u, u32)
        own_u = own_u and u is not None  # generated here (a tensor nobody else holds): kept for the folded resample without a copy
        self._lazy_frame(odoms, codes, gts, tn, rot, u, u32, own_u, u_event, self.sig_t, self.sig_r)
