"""LoopEngine: the reference's whole loop body (`filter/filter.py:150-190`) as one C-ABI call per frame, on a particle
set whose size lives in device memory.

FilterEngine / PipelinedFilterEngine run the fixed-N part of the frame (motion, NN, similarity, prune, resample).  The
reference's loop also clusters (DBSCAN every 50th frame, `particle_filter.py:208-228`), takes the cluster centres
(:153-206) and anneals the particle count on their spread (:405-447) between the update and the resample, so N changes
every frame.  `midas_loop_step` does all of it on the device - DBSCAN included, top-k selection / compaction /
duplication included - with the live count in the control block, every array sized to the initial particle count
(annealing never grows the set beyond it, :439-440), so a frame is enqueued without reading anything back.  Per-frame
results (rmse, N, cluster centres ...) go to a device log that is read once, when somebody asks.

Draws: device Philox streams keyed by (seed, frame) by default; `tn` / `rot` / `u` take the host draws of the reference
(torch CPU generator, its order: tn, rot, then the resampler's uniforms) - the host then has to know the particle count,
i.e. `n` (one small read-back per frame), and may split the frame with `phases` to draw the uniforms once the annealed
size is known, as the reference does.  Such a replay also wants `topk_ties="aten_cpu"`: inside a tie (the normal case:
particles on one codebook entry share a weight) annealing's `torch.topk` keeps whomever ATen's CPU kernel happens to reach,
and the device then walks that kernel's algorithm (topk_aten.hip) instead of its own radix select (ties by index).
`seed_torch_stream(seed)` takes those same draws from torch's CPU stream on the device, sized by the counts in the control
block: the replay without the read-backs and without splitting the frame by hand.

BatchLoopEngine (batch_loop_engine.py) is this engine for B trajectories; what the two share - the set-up, the state table and
the constant part of `LoopArgs` made from it, the phase mask, the control-block writers, `frame_view`, the seeded streams' set-up
and frame, the frame's scalars and its completion - is `_LoopBase`, by a lead shape: () here, (B,) there.
"""
from __future__ import annotations

import ctypes as C
import numbers
import os
import time
import warnings

import numpy as np
import torch

from . import _lib, ops
from ._lib import LoopArgs, MidasError, _ptr
from .engine import RESAMPLE_MODES, advance_epoch, check_motion_draws, codebook_index, frame_operands, operand, sparse_scoring

ALL_PHASES = _lib.LOOP_FRONT | _lib.LOOP_DBSCAN | _lib.LOOP_ANNEAL | _lib.LOOP_RESAMPLE
TOPK_TIES = {"index": _lib.TOPK_TIES_INDEX, "aten_cpu": _lib.TOPK_TIES_ATEN_CPU}
# get_cluster_centers' two methods as the bit ANNEAL's calls carry (one value for the engine, chosen on the host like the resample mode)
CENTER_FORMS = {"quat_avg": 0, "logmap": _lib.LOOP_CENTERS_LOGMAP}


def state_table(cap: int, K: int, log_frames: int, ctl_d: int = 16):
    """The state of one trajectory: (attribute, LoopArgs field or None, shape behind the lead, dtype, fill).  A field named here
    never changes between frames (`labels` / `labels_out` swap when a frame completes; LoopEngine hands `score_stamps` over only
    on the calls that score sparsely)."""
    f32, f64, i32, n, ncl = torch.float32, torch.float64, torch.int32, (cap,), _lib.LOOP_MAX_CLUSTERS
    return (("ctl_i", "ctl_i", (32,), i32, 0), ("ctl_d", "ctl_d", (ctl_d,), f64, 0),
            ("_poses", "poses", (cap, 4, 4), f32, 0), ("poses_prop", "poses_prop", (cap, 4, 4), f32, 0),
            ("_hint", "hint", n, i32, -1), ("_nn_idx", "nn_idx", n, i32, 0), ("_valid", "valid", n, torch.uint8, 0),
            ("_x", "x", n, f64, 0), ("_e", "e", n, f64, 0), ("_w", "weights", n, f64, 0), ("_w_res", "weights_out", n, f64, 0),
            ("_labels", "labels", n, i32, 0), ("_labels_next", "labels_out", n, i32, 0), ("_src", "src", n, i32, 0), ("_ridx", "ridx", n, i32, 0),
            ("_scores", "scores", (K,), f64, 0), ("_part_rmse", None, (2 * ((cap + 63) // 64),), f64, 0),  # (handed over with a ground truth)
            ("_cl_poses", "cluster_poses", (ncl, 4, 4), f32, 0), ("_cl_stds", "cluster_stds", (ncl, 3), f32, 0),
            ("_log", None, (log_frames, _lib.LOOP_LOG_DOUBLES), f64, 0),  # (a frame gets its row)
            ("telemetry", "telemetry", (16,), torch.int64, 0),  # (no lead: cumulative over a batch)
            ("_stamps", "score_stamps", (K,), i32, 0))  # sparse scoring (include/midas_hip.h score_stamps_dev)


def particles_block(n, ncl, old, reset_annealing: bool):
    """The control block(s) `set_particles` writes, on the host: n, ncl = live count and cluster count (label maximum + 1) of one
    trajectory or of B -> (32,) or (B, 32) int32 with N = NSET = n, NCL = ncl and, unless annealing starts over, INIT, VARSET and
    FRAME of `old` (the block as it stands, on the host); every other word 0."""
    n = torch.as_tensor(n, dtype=torch.int32)
    ci = torch.zeros(n.shape + (32,), dtype=torch.int32)
    if not reset_annealing:
        for k in (_lib.LOOP_I_INIT, _lib.LOOP_I_VARSET, _lib.LOOP_I_FRAME):
            ci[..., k] = old[..., k]
    ci[..., _lib.LOOP_I_N] = ci[..., _lib.LOOP_I_NSET] = n
    ci[..., _lib.LOOP_I_NCL] = torch.as_tensor(ncl, dtype=torch.int32)
    return ci


def annealing_block(ci, cd, particle_var, init_particles):
    """`set_annealing_state` on the host copies of ctl_i / ctl_d (one row or B, changed in place and returned):
    particle_filter.particle_var as annealing keeps it - float32, "unset" while infinite - and init_particles."""
    pv = np.asarray(particle_var, dtype=np.float64)
    unset = np.isinf(pv)
    ci[..., _lib.LOOP_I_VARSET] = torch.as_tensor(np.where(unset, 0, 1), dtype=torch.int32)
    ci[..., _lib.LOOP_I_INIT] = torch.as_tensor(init_particles, dtype=torch.int32)
    cd[..., _lib.LOOP_D_VARPREV] = torch.as_tensor(np.where(unset, 0.0, pv.astype(np.float32)), dtype=torch.float64)
    return ci, cd


class _LoopBase:
    """What LoopEngine and BatchLoopEngine share: the codebook index, the filter's parameters, the state of one trajectory or of B
    (`_lead` = () or (B,)) with the `LoopArgs` that point at it, and the host's part of a frame."""

    def _setup(self, cb_poses, cb_embeddings, mesh_vertices, device, sig_t, sig_r, pen_max, seed, softmax, resample, floor, eps,
               cluster, cluster_every, log_frames, centers="quat_avg"):
        if centers not in CENTER_FORMS:  # (before a context is asked for)
            raise MidasError(f"centers must be one of {sorted(CENTER_FORMS)}, got {centers!r}")
        self.centers = centers
        self.ctx, self.cb_poses, self.cb_feat, self.tree6, self.codebook, self.tree3 = codebook_index(
            cb_poses, cb_embeddings, mesh_vertices, device)
        self.device = self.ctx.device
        self.K, self.D = self.codebook.K, self.codebook.D
        self.sig_t, self.sig_r, self.pen_max = float(sig_t), float(sig_r), float(pen_max)
        self.seed, self.softmax, self.floor, self.eps = int(seed), bool(softmax), int(floor), float(eps)
        self.cluster, self.cluster_every = bool(cluster), max(int(cluster_every), 1)
        self.mode = RESAMPLE_MODES[resample]
        self.log_frames = int(log_frames)
        self.step_count = 0   # frames enqueued (Philox counter, log row)
        self.starts = 0       # start() calls so far (the step word of a start's draws: 0xFFFFFFFF - starts)
        self._n_host = None   # live count(s) as last known by the host (None: ask the device)
        self._epoch = 0

    def _alloc_state(self, lead, topk_ties: str, ctl_d: int = 16):
        """The state table's tensors behind `lead`, and `_args`: what never changes between frames."""
        self._lead, self._state = lead, state_table(self.cap, self.K, self.log_frames, ctl_d)
        a = self._args = LoopArgs()
        for attr, field, shape, dt, fill in self._state:
            t = torch.full((() if attr == "telemetry" else lead) + shape, fill, dtype=dt, device=self.device)
            setattr(self, attr, t)
            if field is not None:
                setattr(a, field, _ptr(t))
        self._labels_prev = self._labels
        a.cap, a.cb_poses, a.topk_ties = self.cap, _ptr(self.cb_poses), TOPK_TIES[topk_ties]
        self._write_params()

    def _write_params(self):
        a = self._args
        a.seed, a.prune_thr, a.softmax, a.resample_mode = self.seed, self.pen_max, int(self.softmax), self.mode
        a.floor, a.eps = self.floor, self.eps

    # ---- state ----------------------------------------------------------------------------------------------------
    def _write_particles_block(self, n, ncl, reset_annealing: bool):
        """set_particles' control block(s) to the device; returned as written."""
        ci = particles_block(n, ncl, None if reset_annealing else self.ctl_i.cpu(), reset_annealing)
        if reset_annealing:
            self.ctl_d.zero_()
        self.ctl_i.copy_(ci)
        return ci

    def _write_annealing_state(self, particle_var, init_particles):
        ci, cd = annealing_block(self.ctl_i.cpu(), self.ctl_d.cpu(), particle_var, init_particles)
        self.ctl_i.copy_(ci)
        self.ctl_d.copy_(cd)

    def start(self, gts, init_noise, n=None, project: bool = True, tn=None, rot=None, reset_annealing=None):
        """Start (or restart) every trajectory on the device - `init_filter` and the projection onto the codebook that the reference
        runs on each frame seen while prev_idx == 0 (filter/filter.py:156-160; particle_filter.py:129-145) - without a host draw, an
        upload of poses or a read-back: two launches for all rows (`midas_init_particles_batch`, `midas_project_batch`).
        gts: (4,4), or (B,4,4) for a batch; init_noise: `particle_filter.init_noise` - (sigma_t in metres, sigma_r in degrees), or B
        such pairs, a row's sigma_t being its object's; n: the live count(s) to start with (None: the capacity).  tn / rot: the
        caller's draws, lead + (cap, 3) float32 already scaled (both or neither); None: Philox normals keyed (seed + b, 0xFFFFFFFF -
        starts) - `starts` counts the calls, so a second start draws fresh numbers as the reference's second init_filter does, on a
        step word no frame uses.  project=False leaves the particles off the codebook (hints -1).
        Poses, hints, labels 0 and the control blocks come out as `set_particles(poses, reset_annealing=...)` leaves them;
        reset_annealing None: the engine's first start resets annealing, later ones keep particle_var, init_particles and the frame
        count (filter/filter.py re-initialises without touching them)."""
        B = self._lead[0] if self._lead else 1
        cap, d = self.cap, self.device
        reset = self.starts == 0 if reset_annealing is None else bool(reset_annealing)
        ns = [cap] * B if n is None else ([int(n)] * B if isinstance(n, numbers.Integral) else [int(v) for v in n])
        if len(ns) != B or min(ns) < 1 or max(ns) > cap:
            raise MidasError(f"start: {B} live counts within 1 .. {cap} expected, got {ns if len(ns) <= 8 else len(ns)}")
        gts = operand(gts, "gt poses", torch.float32, (B, 4, 4), d)
        sig = torch.as_tensor(init_noise, dtype=torch.float32).reshape(-1, 2)
        sig = operand(sig.expand(B, 2) if sig.shape[0] == 1 else sig, "init_noise", torch.float32, (B, 2), d)
        check_motion_draws(tn, rot)
        if tn is not None:
            tn, rot = operand(tn, "tn", torch.float32, (B, cap, 3), d), operand(rot, "rot", torch.float32, (B, cap, 3), d)
        poses, hint = self._poses.view(B, cap, 4, 4), self._hint.view(B, cap)
        hint.fill_(-1)
        self._labels.zero_()
        ops.init_particles_batch(poses, gts, sig, ns, seed=self.seed, draw=self.starts, tn=tn, rot=rot)
        if project:
            if getattr(self, "_set", None) is not None:
                ops.project_batch(poses, hint, ns, object_set=self._set)
            else:
                ops.project_batch(poses, hint, ns, tree6=self.tree6, codebook=self.codebook, cb_poses=self.cb_poses)
        # particles_block on the device: N = NSET = n, NCL = 1 (label 0 everywhere) and, unless annealing starts over, the INIT,
        # VARSET and FRAME that stand there; every other word 0
        ci = torch.zeros_like(self.ctl_i)
        if reset:
            self.ctl_d.zero_()
        else:
            keep = [_lib.LOOP_I_INIT, _lib.LOOP_I_VARSET, _lib.LOOP_I_FRAME]
            ci[..., keep] = self.ctl_i[..., keep]
        n_dev = torch.tensor(ns, dtype=torch.int32).to(d).reshape(self._lead)
        ci[..., _lib.LOOP_I_N] = n_dev
        ci[..., _lib.LOOP_I_NSET] = n_dev
        ci[..., _lib.LOOP_I_NCL] = 1
        self.ctl_i.copy_(ci)
        self.starts += 1
        self._started(ns, reset)

    def _started(self, ns, reset: bool):
        """The host's bookkeeping behind start()."""
        self._n_host = ns

    def _frame_view(self, rec, b):
        """rec: the log record of the latest completed frame of trajectory b (() for the only one) -> with the views of its arrays."""
        nb, ns = rec["n"], rec["n_after"]
        rec.update(poses_prop=self.poses_prop[b][:nb], nn_idx=self._nn_idx[b][:nb], valid=self._valid[b][:nb], weights=self._w[b][:nb],
                   labels_frame=self._labels_prev[b][:nb], src=self._src[b][:ns], ridx=self._ridx[b][:ns], poses=self._poses[b][:ns],
                   weights_res=self._w_res[b][:ns], labels=self._labels[b][:ns], hint=self._hint[b][:ns],
                   ctl_i=self.ctl_i[b].cpu().numpy(), ctl_d=self.ctl_d[b].cpu().numpy())
        return rec

    def _log_window(self, first: int, last):
        """[first, last) clamped to the frames enqueued and to what the log ring still holds."""
        last = self.step_count if last is None else min(last, self.step_count)
        return max(first, last - self.log_frames), last

    # ---- seeded runs ----------------------------------------------------------------------------------------------
    def _seed_streams(self, cls, seeds, systematic: bool = False):
        """The device replica(s) of torch's CPU generator (torch_rng `cls`) with their tables uploaded now, not by the first frame,
        and the buffers a seeded frame draws into -> (streams, scratch bytes of the generator's two counted calls at capacity)."""
        if systematic != (self.mode == _lib.RESAMPLE_SYSTEMATIC):
            if systematic:
                raise MidasError("the _low_var seeding is the systematic resampler's: resample='low_var' / 'low_var_batch' only")
            raise MidasError("a seeded torch stream reproduces torch.multinomial's draws: resample='weighted_random' only - the "
                             "systematic resampler's one float32 torch.rand(1) a frame: seed_torch_stream_low_var / seed_torch_streams_low_var")
        st = cls(seeds, self.device, overlap=False, pieces=0)
        st._normal_tables()
        lead, cap, d = self._lead, self.cap, self.device
        self._tn, self._rot = (torch.zeros(lead + (cap, 3), dtype=torch.float32, device=d) for _ in range(2))
        self._u = torch.zeros(lead + (cap,), dtype=torch.float64, device=d)
        self._mt_status = torch.zeros(lead + (self.log_frames,), dtype=torch.int32, device=d)  # the counted calls' status, a word per log row
        ci = (self.ctl_i, _lib.LOOP_I_N)
        return st, max(st.counted_scratch_bytes([("normal", 0.0, 1.0, *ci, 3, cap)] * 2), st.counted_scratch_bytes([("rand64", *ci, cap)]),
                       st.counted_scratch_bytes([("rand32", *ci, cap)]))

    def _seeded_frame(self, st, stds, bound: int, u_bound: int, front, resample, status=()):
        """One frame with the stream's draws: the motion noise sized by the live count (stds = None: none), the frame up to
        annealing (`front()`), the resampler's draw - the uniforms sized by the annealed count (torch.multinomial,
        particle_filter.py:245), or the one float32 offset of the systematic resampler (torch.rand(1), :291), which lands in the first
        slot of every row of `_u` - and the resample (`resample()`): four enqueues, the counts never leave the device."""
        slot, ci = self.step_count % self.log_frames, self.ctl_i
        if slot == 0:
            self._mt_status.zero_()  # (the ring starts over, as the log's rows do)
        status = (self._mt_status, slot) + status
        if stds is not None:
            st.draws_counted_async([("normal", 0.0, stds[0], ci, _lib.LOOP_I_N, 3, bound), ("normal", 0.0, stds[1], ci, _lib.LOOP_I_N, 3, bound)],
                                   outs=[self._tn, self._rot], status=status)
        front()
        # NDRAW, not NSET: the resampler returns its input before it draws when the weights are all zero or hold a NaN
        # (particle_filter.py:237-241) - the stream must not move on such a frame (a zero count consumes nothing)
        kind = "rand64" if self.mode == _lib.RESAMPLE_MULTINOMIAL else "rand32"  # (rand32: NDRAW as a switch, 0 or 1 values)
        st.draws_counted_async([(kind, ci, _lib.LOOP_I_NDRAW, u_bound)], outs=[self._u], status=status)
        resample()

    # ---- one frame ------------------------------------------------------------------------------------------------
    def _phase_mask(self, phases: int, dbscan) -> int:
        """`phases` without what this frame does not run: no clustering at all, or DBSCAN on every `cluster_every`-th frame only."""
        if not self.cluster:
            return phases & ~(_lib.LOOP_DBSCAN | _lib.LOOP_ANNEAL)
        if phases & _lib.LOOP_ANNEAL:  # the form of the centres travels with the phase that takes them
            phases |= CENTER_FORMS[self.centers]
        if dbscan is False or (dbscan is None and self.step_count % self.cluster_every != 0):
            return phases & ~_lib.LOOP_DBSCAN
        return phases

    def _seeded_u32(self, u32) -> float:
        """The `u32` of a seeded frame: the stream draws the systematic offset, as it draws `u` - a caller's own is refused."""
        if self.mode != _lib.RESAMPLE_SYSTEMATIC:
            return float(u32)
        if float(u32) >= 0.0:
            raise MidasError("seeded torch stream: the stream draws the systematic offset - passing u32 would desynchronise the stream "
                             "from the reference's")
        return _lib.U32_FROM_U

    def _frame_scalars(self, u32, multiplier, unit_weights, std_override=None, score: bool = True):
        """What every call of a frame is told: its log row, the scalars, and - when it scores sparsely - its epoch."""
        a = self._args
        a.log = C.c_void_p(self._log.data_ptr() + (self.step_count % self.log_frames) * _lib.LOOP_LOG_DOUBLES * 8)
        a.u32 = float(u32)
        mul = max(float(multiplier), 1.0)
        a.std_t, a.std_r = (mul * self.sig_t, mul * self.sig_r) if std_override is None else std_override
        a.step = self.step_count
        a.unit_weights = int(bool(unit_weights))
        a.score_stamps, a.score_epoch = (_ptr(self._stamps), advance_epoch(self)) if score else (None, 0)
        return a

    def _frame_done(self, n_host=None):
        self._labels_prev = self._labels
        self._labels, self._labels_next = self._labels_next, self._labels
        a = self._args
        a.labels, a.labels_out = a.labels_out, a.labels
        self.step_count += 1
        self._n_host = n_host


class LoopEngine(_LoopBase):
    def __init__(self, cb_poses, cb_embeddings, mesh_vertices, num_particles: int, *, sig_t=2e-4, sig_r=0.5, pen_max=0.002,
                 seed=4000, softmax=True, resample="weighted_random", floor: int = 1000, eps: float = 1e-2, cluster: bool = True,
                 cluster_every: int = 50, log_frames: int = 4096, device=None,
                 topk_ties: str = "index", centers: str = "quat_avg"):
        self._setup(cb_poses, cb_embeddings, mesh_vertices, device, sig_t, sig_r, pen_max, seed, softmax, resample, floor, eps,
                    cluster, cluster_every, log_frames, centers)
        self.cap = cap = int(num_particles)
        if cap < 1 or cap > (1 << 20):
            raise MidasError("LoopEngine holds 1 .. 2^20 particles")
        # whom annealing's torch.topk takes inside a tie: "index" (torch's CUDA rule, the radix select) or "aten_cpu" (the
        # reference as it runs on the CPU - the rule of a seeded replay; topk_aten.hip)
        self.topk_ties = TOPK_TIES[topk_ties]
        self._alloc_state((), topk_ties, ctl_d=104 if os.environ.get("MIDAS_ANNEAL_CLOCKS") else 16)  # (104: profiling builds)
        self.sparse_scores = sparse_scoring(self.codebook)
        # {frames completed, live count} as the device last reported them, in pinned host memory: lets step() size its launches
        # to the live set without waiting for anything (an upper bound is all it needs, see _count_bound)
        self._mirror = torch.zeros(2, dtype=torch.int32).pin_memory()
        self._args.host_mirror = C.c_void_p(self._mirror.data_ptr())
        self._frames_at_reset, self._n_at_reset, self._steps_at_reset, self._grid_n = 0, cap, 0, cap
        self.max_ahead = 1         # frames the host may enqueue ahead of the device's last report (None: no limit)
        self.allow_frozen = True   # see _frozen()
        self._init_known = None    # init_particles as the host knows it (None: annealing's first call will take the live count)
        self._pending_phases = 0
        self.use_hint = True
        self.torch_stream = None   # seed_torch_stream
        # the scratch every phase combination of a frame at this capacity can ask for (DBSCAN's cell tables 84 MB + 41 B per
        # particle, the cluster-centre partials 72 B per particle, selection tables) reserved now: no frame of the run
        # allocates (MIDAS_SCRATCH_LOG=1 prints nothing after this line; the cold frame of BENCH_r03's floor_N run)
        self.ctx.call("midas_scratch_reserve", (128 << 20) + 256 * cap)

    # ---- state ----------------------------------------------------------------------------------------------------
    def set_particles(self, poses: torch.Tensor, labels: torch.Tensor = None, reset_annealing: bool = True):
        """Start (or restart) from `poses` (n <= capacity); labels default to 0 like `Particles` (particle_filter.py:47)."""
        poses = torch.as_tensor(poses).to(self.device, torch.float32).reshape(-1, 4, 4)
        n = poses.shape[0]
        if n < 1 or n > self.cap:
            raise MidasError(f"{n} particles do not fit the engine's capacity of {self.cap}")
        self._poses[:n].copy_(poses)
        self._hint.fill_(-1)
        if labels is None:
            self._labels.zero_()
            ncl = 1  # label 0 everywhere
        else:
            labels = torch.as_tensor(labels).to(self.device).to(torch.int32)
            self._labels[:n].copy_(labels)
            ncl = int(labels.max().item()) + 1
        ci = self._write_particles_block(n, ncl, reset_annealing)
        self._init_known = int(ci[_lib.LOOP_I_INIT]) if int(ci[_lib.LOOP_I_VARSET]) else None  # (both 0 once annealing starts over)
        self._n_host = n
        self._pending_phases = 0
        torch.cuda.current_stream(self.device).synchronize()  # the control block is in place, nothing older is in flight
        self._mirror[0], self._mirror[1] = int(ci[_lib.LOOP_I_FRAME]), n
        self._frames_at_reset, self._n_at_reset, self._steps_at_reset = int(ci[_lib.LOOP_I_FRAME]), n, self.step_count

    def _started(self, ns, reset: bool):
        """set_particles' bookkeeping without its read of the control block: annealing's init_particles, once a frame has taken it,
        is the count that frame started from (annealing's first call takes the live count, particle_filter.py:413-417), and the frame
        count is what the device last reported - all of it, once the stream has drained.
        Assumption behind `_init_known`: since the last reset either no frame ran, or whole frames with the ANNEAL phase did (what
        filter() and filter_sweep enqueue).  A caller that stepped partial phase masks without ANNEAL, or wrote
        set_annealing_state() (which sets `_init_known` itself), is not second-guessed here; `_init_known` only feeds `_frozen()`,
        whose claim the device checks (log row err bit 7), so a wrong guess is reported, never silent."""
        n = ns[0]
        if reset:
            self._init_known = None
        elif self._init_known is None and self.cluster and self.step_count > self._steps_at_reset:
            self._init_known = self._n_at_reset
        self._n_host = n
        self._pending_phases = 0
        torch.cuda.current_stream(self.device).synchronize()  # the control block is in place, nothing older is in flight
        frame = 0 if reset else int(self._mirror[0])
        self._mirror[0], self._mirror[1] = frame, n
        self._frames_at_reset, self._n_at_reset, self._steps_at_reset = frame, n, self.step_count

    def _count_bound(self) -> int:
        """An upper bound of the live count at the start of the frame about to be enqueued, from what the device reported
        last: annealing adds at most n // 3 particles per frame (particle_filter.py:437) and never exceeds the capacity."""
        if not self.cluster:
            return self._n_at_reset
        enq = self.step_count - self._steps_at_reset
        # stay at most `max_ahead` frames in front of the device: the bound below grows by 4/3 per unreported frame, and a
        # host that runs dozens of frames ahead could only ever assume the full capacity.  One frame in the queue while the
        # next is being enqueued keeps the device busy (enqueueing a frame takes less than running it); the wait is a look
        # at pinned memory.
        if self.max_ahead is not None and enq - (int(self._mirror[0]) - self._frames_at_reset) > self.max_ahead:
            t0 = time.perf_counter()
            while enq - (int(self._mirror[0]) - self._frames_at_reset) > self.max_ahead and time.perf_counter() - t0 < 0.05:
                pass
        done = int(self._mirror[0]) - self._frames_at_reset   # frames of this run the device has finished
        n = int(self._mirror[1]) if done > 0 else self._n_at_reset
        lag = (self.step_count - self._steps_at_reset) - max(done, 0)  # frames enqueued since that report
        for _ in range(max(lag, 0)):
            n += n // 3
            if n >= self.cap:
                return self.cap
        return min(n, self.cap)

    def _frozen(self) -> bool:
        """Annealing cannot change the set: the live count equals `floor` and the count annealing starts (started) from
        (particle_filter.py:421-446: a removal needs |n - floor| > 0, a duplication k + n <= init_particles) - true from a start with
        n == floor on, for good.  The ANNEAL phase then runs its decision only, not the selection's ten launches; the device checks
        the statement (log row err bit 7).  `allow_frozen = False` keeps the launches (tests)."""
        if not (self.cluster and self.allow_frozen):
            return False
        n0 = self._n_at_reset
        return self.floor == n0 and self._init_known in (None, n0)

    def set_annealing_state(self, particle_var: float, init_particles: int):
        """particle_filter.particle_var / init_particles (particle_filter.py:413-417) - for restarts and tests."""
        self._init_known = int(init_particles)
        self._write_annealing_state(float(particle_var), int(init_particles))

    def project_to_codebook(self):
        """poses := codebook pose nearest to each particle (filter/filter.py:159-160)."""
        n = self.n
        idx = ops.nn6(self.tree6, ops.se3_feature(self._poses[:n]))
        self._poses[:n].copy_(ops.gather_rows(self.cb_poses, idx))
        self._hint[:n].copy_(idx)
        return idx

    @property
    def n(self) -> int:
        """Live particle count (reads the control block when the host does not know it)."""
        if self._n_host is None:
            self._n_host = int(self.ctl_i[_lib.LOOP_I_N].item())
        return self._n_host

    # views of the live particle set / the latest frame (each reads the count: a synchronisation)
    poses = property(lambda self: self._poses[:self.n])
    weights_res = property(lambda self: self._w_res[:self.n])
    labels = property(lambda self: self._labels[:self.n])
    hint = property(lambda self: self._hint[:self.n])
    ridx = property(lambda self: self._ridx[:self.n])

    def frame_view(self):
        """The latest COMPLETED frame, for tests and inspection (one synchronisation): its log record plus views of the
        per-particle arrays - before annealing (n entries: poses_prop, nn_idx, valid, weights, labels_frame), the annealed set
        (n_after entries: src, ridx) and the resampled particle set (n_after entries: poses, weights_res, labels, hint)."""
        if self.step_count == 0 or self._pending_phases:
            raise MidasError("frame_view needs a completed frame")
        rec = self._frame_view(self.read_log(self.step_count - 1, self.step_count)[0], ())
        self._n_host = rec["n_after"]
        return rec

    # ---- seeded runs ----------------------------------------------------------------------------------------------
    def seed_torch_stream_low_var(self, seed):
        """seed_torch_stream for an engine built with resample="low_var" / "low_var_batch": the resampler's draw of a frame is then
        the one float32 `torch.rand(1)` of the systematic resampler (particle_filter.py:291), gated by ctl_i[LOOP_I_NDRAW] like the
        uniforms, left in device memory and read there by the resample (MIDAS_U32_FROM_U); a caller's `u32 >= 0` on such a frame is
        refused.  A method of its own: seed_torch_stream on a systematic engine refuses, as it always did."""
        return self.seed_torch_stream(seed, _systematic=True)

    def seed_torch_stream(self, seed, _systematic: bool = False):
        """Every draw of a frame from the device replica of torch's CPU generator under torch.manual_seed(seed) (torch_rng.py),
        in the reference's order and with the reference's sizes: `torch.normal(0, mul * sig_t, (n, 3))`, `torch.normal(0, mul *
        sig_r, (n, 3))` with n the live count (add_noise_to_odom, particle_filter.py:326-335) and, behind annealing, n_set float64
        uniforms (the resampler's torch.multinomial, :245) or - seed_torch_stream_low_var on an engine built with
        resample="low_var" (this method refuses such an engine, as it always did: it means multinomial's draws) - the one
        float32 `torch.rand(1)` of the systematic resampler (:291) - none on a frame whose weights are all zero or hold a NaN, where the
        resampler returns before it draws (:237-241; ctl_i[LOOP_I_NDRAW]).  The counts are read on the device (midas_mt19937_draws_counted): a
        step() without tn / rot / u enqueues the whole frame and reads nothing back.  A run that also draws on the host (init_filter)
        hands the stream over with the returned TorchCpuStream's from_host() / to_host().  seed=None: back to Philox.
        The generator runs on the engine's stream, in front of the kernels that read its numbers; its scratch at the engine's
        capacity is reserved here, so no frame allocates.  A live count below 6 (fewer than 16 normal values: ATen's scalar path,
        not modelled) is reported by read_log()."""
        if seed is None:
            self.torch_stream = None
            return None
        from .torch_rng import TorchCpuStream
        st, need = self._seed_streams(TorchCpuStream, seed, _systematic)
        self._no_noise = torch.zeros_like(self._tn)
        self.ctx.call("midas_scratch_reserve", max((128 << 20) + 256 * self.cap, need))  # (the generator shares the engine's context)
        self.torch_stream = st
        return st

    def _seeded_step(self, odom, code, gt, u32, multiplier, dbscan, std_override, unit_weights, motion_draws):
        """_seeded_frame with draws bounded by _count_bound(), and by what annealing can make of it; motion_draws=False draws no
        motion noise."""
        if self._pending_phases:
            raise MidasError("a seeded frame is enqueued whole: finish the frame in progress first")
        u32 = self._seeded_u32(u32)
        b = self._count_bound()
        tn, rot, stds = self._no_noise, self._no_noise, None
        if motion_draws:
            mul = max(float(multiplier), 1.0)
            tn, rot, stds = self._tn, self._rot, (mul * self.sig_t, mul * self.sig_r) if std_override is None else std_override
        self._seeded_frame(
            self.torch_stream, stds, b, min(self.cap, b + b // 3),
            lambda: self._enqueue(odom, code, gt, tn, rot, None, u32, multiplier, dbscan, _lib.LOOP_FRONT | _lib.LOOP_DBSCAN | _lib.LOOP_ANNEAL,
                                  std_override, unit_weights, bound=b, stream_draws=True),
            lambda: self._enqueue(None, None, None, None, None, self._u, u32, multiplier, dbscan, _lib.LOOP_RESAMPLE, std_override,
                                  unit_weights, stream_draws=True))

    # ---- one frame ------------------------------------------------------------------------------------------------
    def step(self, odom, code, gt=None, tn=None, rot=None, u=None, u32=-1.0, multiplier: float = 1.0, dbscan=None,
             phases: int = None, std_override=None, unit_weights: bool = False, motion_draws: bool = True, stream_draws: bool = False):
        """Enqueues one frame (or the given phases of it).  dbscan: None = on every `cluster_every`-th frame (count % 50 ==
        0, filter.py:182), True / False to force.  Host draws tn / rot (n, 3) and u (>= n_set,) as in FilterEngine.step.
        With seed_torch_stream the draws are the stream's and the engine splits the frame itself: tn / rot / u / phases are then an
        error; motion_draws=False draws no motion noise and propagates with zeros (the frames the reference starts from, where it
        does not call motionModel).
        stream_draws: the host splits the frame in front of RESAMPLE to draw `u` from a stream that has to stay the reference's - set
        on both calls: the first then leaves in ctl_i[LOOP_I_NDRAW] how many uniforms the reference's resampler draws on this frame
        (n_set, or 0 where it returns its input before drawing: all-zero or NaN weights), the second checks itself against it."""
        if self.torch_stream is None:
            return self._enqueue(odom, code, gt, tn, rot, u, u32, multiplier, dbscan, phases, std_override, unit_weights,
                                 stream_draws=stream_draws)
        if tn is not None or rot is not None or u is not None or phases is not None:
            raise MidasError("seed_torch_stream: the stream draws tn, rot and u and the engine splits the frame - passing them would "
                             "desynchronise the stream from the reference's")
        self._seeded_step(odom, code, gt, u32, multiplier, dbscan, std_override, unit_weights, motion_draws)

    def _enqueue(self, odom, code, gt, tn, rot, u, u32, multiplier, dbscan, phases, std_override, unit_weights, bound: int = None,
                 stream_draws: bool = False):
        """bound: the frame's _count_bound() when the caller has taken it already; tn / rot are then the engine's own capacity-sized
        buffers (tn[3 i + j] for particle i, as the kernels index them)."""
        d = self.device
        frame_start = self._pending_phases == 0
        if phases is None:
            phases = ALL_PHASES & ~self._pending_phases if not frame_start else ALL_PHASES
        phases = self._phase_mask(phases, dbscan)
        # the cached struct: a call reads NULL / 0 in an operand or switch as "not given", so every field that is not the state
        # table's is written on every call - what this call does not hand over as None or 0, never left from the call before
        front = bool(phases & _lib.LOOP_FRONT)
        if front:
            check_motion_draws(tn, rot)
            odom, code, gt = frame_operands(d, (), self.D, odom, code, gt)
            if tn is not None and bound is None:
                n = self.n
                tn, rot = operand(tn, "tn", torch.float32, (n, 3), d), operand(rot, "rot", torch.float32, (n, 3), d)
        else:
            odom = code = gt = tn = rot = None
        u = torch.as_tensor(u).to(d, torch.float64).contiguous().reshape(-1) if phases & _lib.LOOP_RESAMPLE and u is not None else None
        a = self._frame_scalars(u32, multiplier, unit_weights, std_override, score=self.sparse_scores and front)
        a.odom16, a.code, a.gt16, a.tn, a.rot, a.u = _ptr(odom), _ptr(code), _ptr(gt), _ptr(tn), _ptr(rot), _ptr(u)
        a.part_rmse = _ptr(self._part_rmse) if gt is not None else None
        self._write_params()  # (floor, eps ... stay settable between frames)
        if frame_start:
            self._grid_n = self._count_bound() if bound is None else bound
        a.grid_n, a.anneal_small, a.anneal_frozen = self._grid_n, int(self._grid_n <= 16384), int(self._frozen())
        a.topk_ties, a.stream_draws = self.topk_ties, int(bool(stream_draws))
        self._keep = [odom, code, gt, tn, rot, u]  # the operands of the call in flight
        self.ctx.bind_current_stream()
        self.ctx.check(self.ctx.lib.midas_loop_step(self.ctx.h, self.codebook.h, self.tree6.h, self.tree3.h, C.byref(a), int(phases)))
        self._pending_phases |= phases
        if phases & _lib.LOOP_RESAMPLE:  # frame complete
            self._pending_phases = 0
            self._frame_done(n_host=None if self.cluster else self._n_host)

    # ---- results --------------------------------------------------------------------------------------------------
    def read_log(self, first: int = 0, last: int = None, strict: bool = True):
        """Per-frame records of frames [first, last) as a list of dicts (one read-back): frame, n (before annealing),
        n_after, rmse_t, rmse_r, kept, drifted, status, mode, k, clusters, var, cluster_poses (C,4,4), cluster_stds (C,3), err.
        Conditions that leave a frame's particles or labels UNDEFINED (err bit 2: the live count exceeded the bound the launches
        were sized for; bits 5 / 6: DBSCAN's cell structure did not apply; a seeded stream's counted draw that set its status)
        raise MidasError once every row is parsed (the records are attached to the exception as `.records`); strict=False reports
        them as warnings like the benign ones (cluster limits)."""
        first, last = self._log_window(first, last)
        rows = self._log.cpu().numpy()
        mt = self._mt_status.cpu().numpy() if self.torch_stream is not None else None  # (seed_torch_stream: the counted draws' status)
        return log_records(rows, first, last, mt=mt, strict=strict)


def log_records(rows, first: int, last: int, mt=None, strict: bool = True, who: str = ""):
    """Frames [first, last) of a log ring `rows` (log_frames x LOOP_LOG_DOUBLES, on the host) as LoopEngine.read_log's records,
    with its handling of the frames' condition bits; mt: the counted draws' status words of a seeded stream, a word per row;
    who: what the messages call the ring's owner (a batch's "trajectory b, ")."""
    log_frames = rows.shape[0]
    out, fatal = [], []
    for f in range(first, last):
        L = rows[f % log_frames]
        npres = int(L[10])
        cl = L[16:16 + 19 * min(npres, 8)].reshape(-1, 19)
        err = int(L[15])
        # condition bits of THIS frame (the device clears the word once the row holds it)
        if err & (1 | 2):
            warnings.warn(f"{who}frame {f}: more than {_lib.LOOP_MAX_CLUSTERS - 2} clusters in one frame - the labels beyond that limit, and the "
                          "annealing driven by them, are not the reference's (min_samples = n / 5 allows about five)")
        if err & 8:
            warnings.warn(f"{who}frame {f}: {npres} cluster labels present, the log row keeps the centres of the first 8")
        if err & 4:
            fatal.append(f"{who}frame {f}: the live particle count exceeded the bound the launches were sized for; "
                         "the particles beyond it were not processed in this frame")
        if err & 32:
            fatal.append(f"{who}frame {f}: DBSCAN saw non-finite particle translations or a cloud of more than 2^21 cells per axis; labels undefined")
        if err & 64:
            fatal.append(f"{who}frame {f}: DBSCAN on a cloud wider than 128 cells per axis with more than 2^20 particles (hash table capacity); labels undefined")
        if err & 128:
            fatal.append(f"{who}frame {f}: the engine stated that annealing could not act (live count == floor == init_particles) and the "
                         "rule wanted to: the set was left as it was")
        if err & _lib.LOOP_ERR_NDRAW:
            fatal.append(f"{who}frame {f}: the resample's status disagrees with the count its stream's uniforms were drawn by "
                         "(ctl_i[NDRAW]): the stream is no longer the reference's")
        bits = int(mt[f % log_frames]) if mt is not None else 0
        if bits:
            why = [w for b, w in ((_lib.MT_STATUS_COUNT_RANGE, "a count exceeded the bound its draw was sized for"),
                                  (_lib.MT_STATUS_NORMAL_SHORT, "a live count below 6 - fewer than 16 normal values, ATen's scalar path"))
                   if bits & b]
            fatal.append(f"{who}frame {f}: the seeded stream drew nothing ({'; '.join(why)}): the frame's draws are undefined")
        out.append(dict(frame=f, n=int(L[1]), n_after=int(L[2]), rmse_t=float(L[3]), rmse_r=float(L[4]), kept=int(L[5]),
                        drifted=bool(L[6]), status=int(L[7]), mode=int(L[8]), k=int(L[9]), clusters=npres, var=float(L[11]),
                        S=float(L[12]), raw=bool(L[13]), ncl=int(L[14]), err=int(L[15]),
                        cluster_poses=cl[:, :16].reshape(-1, 4, 4).astype(np.float32), cluster_stds=cl[:, 16:].astype(np.float32)))
    if fatal and strict:
        e = MidasError("; ".join(fatal))
        e.records = out
        raise e
    for msg in fatal:
        warnings.warn(msg)
    return out
