"""BatchLoopEngine: B trajectories' whole loop bodies (`filter/filter.py:150-190`: measurement update, DBSCAN, cluster centres,
annealing of the particle count, resample) per set of launches - `midas_loop_step_batch`.

BatchFilterEngine / PipelinedBatchFilterEngine batch the fixed-N part of the frame; a sweep over seeds, logs or objects stacked
onto them never clusters or anneals.  Here every trajectory is a LoopEngine's particle set - its own live count in its own control
block, its own labels, cluster rows and log ring - and the kernels of the small-set frame run with the trajectory as grid.y.
Trajectory b draws from the Philox streams keyed (seed + b, frame): frame for frame it holds the bits of a LoopEngine built with
seed + b and stepped with row b of the operands.  The host side is LoopEngine's too: `loop_engine._LoopBase` with the lead (B,) -
its state table, control-block writers, phase mask, seeded frame and frame completion; what stands here is the batch's own (the
regimes, the scratch, the three entry points, list inputs and per-trajectory results).

The regime is the small set: at most 16 384 particles per trajectory (`_lib.LOOP_BATCH_MAX_CAP`; `wide=True`, below: 131 072), a
float32 codebook scored sparsely.  Sharding stays with the sharded engine.  A DBSCAN frame clusters all B trajectories in ONE pass
(`midas_dbscan_batch`'s launches: every trajectory in its own region of the one set of cell tables, the same labels as its own pass)
whenever B x capacity <= 2^20 (`_lib.DBSCAN_BATCH_MAX_POINTS`); beyond that - or with `batched_dbscan=False` - it runs the single
pass once per trajectory, one after the other on the stream.  Plain, seeded and wide engines alike.

Seeded runs: `seed_torch_streams(seeds)` makes trajectory b a process of the reference under `torch.manual_seed(seeds[b])` - its
motion noise and its resampler's uniforms come from a device replica of torch's CPU generator (torch_rng.TorchCpuStreams), sized by
the live and annealed counts in ITS control block, and ties of annealing's `torch.topk` go to the members ATen's CPU kernel keeps
(`topk_ties = "aten_cpu"`, settable on its own too).  Row b then holds, frame for frame, the bits of a LoopEngine built with
`topk_ties="aten_cpu"` and `seed_torch_stream(seeds[b])` - the reference's particles - through `midas_loop_step_batch_draws`; a frame
is four enqueues and reads nothing back.

Wide sets: `BatchLoopEngine(..., wide=True)` holds up to 131 072 particles per trajectory (`_lib.LOOP_BATCH_WIDE_MAX_CAP`, with
B x capacity <= 2^24) - the reference's own `num_particles: 50000` (config/expt/ycb.yaml) and the headline's 100 000 - through
`midas_loop_step_batch_wide`: beyond 16 384 annealing's selection is LoopEngine's radix select with the trajectory as grid.y, on
per-trajectory state reserved at construction.  Row b holds the bits of a LoopEngine built with seed + b as before; up to 16 384 a
wide engine runs the launches of a plain one.  Open follow-up: `seed_torch_streams` and `topk_ties = "aten_cpu"` raise on a wide
engine - the one-wave walk of ATen's top-k takes 1.4 - 11 ms at 100 000 particles per trajectory, which a batch frame cannot carry;
seeded replays at these sizes stay with LoopEngine.

Rows on different objects: `BatchLoopEngine.for_objects(objects, row_object, num_particles, ...)` - the object axis of the reference's
sweep (`bash/run_filter.sh`: objects x logs x trials) in ONE batch.  Every object gets its own codebook index on the one context, an
object set (`midas_object_set_create`) tells the front which record a row's workgroups read, and a frame goes through
`midas_loop_step_batch_objects`: one launch set for all rows, whatever they stand on.  Row b holds the bits of a LoopEngine built on
object row_object[b] with seed + b.  Scores and stamps are (B, K_max).

The filter's parameters per row: `sig_t`, `sig_r`, `pen_max`, `floor` and `softmax` are each one value for the batch or B values,
`step(unit_weights=)` a bool or B bools, `set_row_params(**kw)` changes them between frames - two datasets' configs
(config/expt/ycb.yaml, mcmaster.yaml), the two runners' presets (filter/filter.py, filter_real.py) or a parameter grid as rows of ONE
batch.  A frame with any per-row value goes through `midas_loop_step_batch_rows` with a table of B `midas_loop_row_params` on the
device (built on the host when a frame's inputs are not among the last ROW_TABLES_KEPT, sent without a stall after the first, kept resident) - the same number of launches, nothing read back;
row b then holds the bits of a LoopEngine built with row b's parameters and seed + b.  With scalars only the engine takes the entries
above, unchanged.  Shared by all rows still: `eps`, the DBSCAN flag and cadence, the resample mode, `multiplier` and `step_still`'s
`std_override`; seeded streams and the ATen tie rule refuse per-row values (their counted draws carry one std per segment).
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, ops
from ._lib import MidasError, _ptr
from .engine import codebook_index, frame_operands, sparse_scoring
from .loop_engine import ALL_PHASES, TOPK_TIES, _LoopBase, log_records


# the constructor's keywords and their defaults: what `for_objects` takes as **kw (tests hold __init__'s signature to this table)
DEFAULTS = dict(sig_t=2e-4, sig_r=0.5, pen_max=0.002, seed=4000, softmax=True, resample="weighted_random", floor=1000, eps=1e-2,
                cluster=True, cluster_every=50, log_frames=4096, device=None, wide=False, batched_dbscan=None, centers="quat_avg")


ROW_PARAMS = ("sig_t", "sig_r", "pen_max", "floor", "softmax")  # what a row may hold for itself (set_row_params' keywords)
ROW_TABLES_KEPT = 16  # resident parameter tables (40 B a row each): a sweep alternates between two (still / moving frames), rows with
#                        different update cadences cycle through lcm(frequencies) unit-weight patterns (BatchLoopEngine._row_table)


def squared_threshold(thr: float) -> float:
    """csrc/midas_internal.hpp squared_threshold on the host: the largest float64 t2 with sqrt(t2) <= thr, so that sqrt(d2) > thr <=>
    d2 > t2 exactly; -1 for a negative or NaN threshold, +inf for +inf.  (IEEE square roots on both sides: the same double.)"""
    thr = float(thr)
    if not thr >= 0.0:
        return -1.0
    if math.isinf(thr):
        return math.inf
    t = thr * thr
    while math.sqrt(t) > thr:
        t = math.nextafter(t, 0.0)
    while math.sqrt(math.nextafter(t, math.inf)) <= thr:
        t = math.nextafter(t, math.inf)
    return t


def row_values(name: str, value, B: int):
    """One of ROW_PARAMS (or `unit_weights`) as given -> (scalar, None) or (None, list of B), checked: a sequence of another length,
    a negative or NaN sigma, a floor below 1.  Nothing else is looked at (a threshold may be NaN or infinite, as a scalar may)."""
    if isinstance(value, (torch.Tensor, np.ndarray)):
        value = value.tolist()
    seq = isinstance(value, (list, tuple))
    vals = list(value) if seq else [value]
    if seq and len(vals) != B:
        raise MidasError(f"{name}: {len(vals)} values for a batch of {B} rows (one value, or one per row)")
    conv = {"sig_t": float, "sig_r": float, "pen_max": float, "floor": int, "softmax": bool, "unit_weights": bool}[name]
    try:
        vals = [conv(v) for v in vals]
    except (TypeError, ValueError) as e:
        raise MidasError(f"{name}: {e}") from e
    for b, v in enumerate(vals):
        where = f"row {b}: " if seq else ""
        if name in ("sig_t", "sig_r") and not v >= 0.0:
            raise MidasError(f"{where}{name} = {v}: a motion noise is a standard deviation, >= 0")
        if name == "floor" and v < 1:
            raise MidasError(f"{where}floor = {v}: annealing's floor is at least 1 particle")
    return (None, vals) if seq else (vals[0], None)


def row_params_table(B: int, std_t, std_r, pen_max, floor, softmax, unit_weights) -> np.ndarray:
    """B `midas_loop_row_params` on the host from six columns, each a scalar or B values; std_t / std_r as float32 already."""
    tab = np.zeros(B, dtype=_lib.LOOP_ROW_PARAMS_DTYPE)
    tab["std_t"], tab["std_r"] = std_t, std_r
    tab["prune_thr"] = pen_max
    t2 = {}
    tab["prune_t2"] = [t2.setdefault(float(v).hex(), squared_threshold(v)) for v in tab["prune_thr"]]  # (one search per distinct threshold)
    tab["floor"], tab["softmax"], tab["unit_weights"] = floor, np.asarray(softmax, dtype=bool), np.asarray(unit_weights, dtype=bool)
    return tab


class BatchLoopEngine(_LoopBase):
    def __init__(self, cb_poses, cb_embeddings, mesh_vertices, batch: int, num_particles: int, *, sig_t=2e-4, sig_r=0.5,
                 pen_max=0.002, seed=4000, softmax=True, resample="weighted_random", floor: int = 1000, eps: float = 1e-2,
                 cluster: bool = True, cluster_every: int = 50, log_frames: int = 4096, device=None, wide: bool = False,
                 batched_dbscan=None, centers: str = "quat_avg"):
        self._init([(cb_poses, cb_embeddings, mesh_vertices)], None, batch, num_particles, sig_t=sig_t, sig_r=sig_r, pen_max=pen_max,
                   seed=seed, softmax=softmax, resample=resample, floor=floor, eps=eps, cluster=cluster, cluster_every=cluster_every,
                   log_frames=log_frames, device=device, wide=wide, batched_dbscan=batched_dbscan, centers=centers)

    def _init(self, objects, row_object, batch, num_particles, *, sig_t, sig_r, pen_max, seed, softmax, resample, floor, eps, cluster,
              cluster_every, log_frames, device, wide, batched_dbscan, centers="quat_avg"):
        """The one initialiser behind the constructor (one object, row_object None) and `for_objects`: the bounds, the set-up on the
        first row's object, for an object batch every object's index and the object set, then the state and the scratch."""
        self._check_regime(batch, num_particles, wide, batched_dbscan)
        # each of ROW_PARAMS: one value for the batch, or B - the set-up then gets row 0's as the shared value (midas_loop_args'
        # field only has to pass the argument check) and the rows' own go into the parameter table of every frame
        given = {k: row_values(k, v, self.B) for k, v in dict(sig_t=sig_t, sig_r=sig_r, pen_max=pen_max, floor=floor, softmax=softmax).items()}
        rows = {k: v[1] for k, v in given.items()}
        sig_t, sig_r, pen_max, floor, softmax = (given[k][0] if rows[k] is None else rows[k][0] for k in ROW_PARAMS)
        first = 0 if row_object is None else row_object[0]  # the handles `_LoopBase` names (ctx, cb_poses, tree6, codebook, tree3): row 0's object
        self._setup(*objects[first], device, sig_t, sig_r, pen_max, seed, softmax, resample, floor, eps, cluster, cluster_every, log_frames,
                    centers)
        if not sparse_scoring(self.codebook, switch=False):
            raise MidasError("BatchLoopEngine scores sparsely: a float32 codebook with D in {128, 256, 512, 1024}")
        self.objects = self.row_object = self.Ks = self._set = None  # (for_objects)
        if row_object is not None:
            self.objects = []
            for i, o in enumerate(objects):
                if i == first:
                    ix = (self.ctx, self.cb_poses, self.cb_feat, self.tree6, self.codebook, self.tree3)
                else:
                    ix = codebook_index(*o, self.device)
                if ix[0] is not self.ctx:
                    raise MidasError("for_objects: every object's index lives on the engine's context")
                if not sparse_scoring(ix[4], switch=False):
                    raise MidasError(f"object {i}: BatchLoopEngine scores sparsely: a float32 codebook with D in {{128, 256, 512, 1024}}")
                self.objects.append(SimpleNamespace(cb_poses=ix[1], cb_feat=ix[2], tree6=ix[3], codebook=ix[4], tree3=ix[5]))
            self.row_object, self.Ks = list(row_object), [int(o.codebook.K) for o in self.objects]
            self._set = ops.ObjectSet(self.ctx, self.objects, row_object)
            self.K = max(self.Ks)  # scores and stamps are (B, K_max): row b touches the first Ks[row_object[b]] slots of its rows
        self._rows, self._rows_version, self._row_set, self._row_tables = rows, 0, self._set, {}
        self.row_table_uploads = 0  # parameter tables sent to the device so far (a sweep: two)
        self._alloc_batch()

    def _check_regime(self, batch, num_particles, wide, batched_dbscan):
        """The constructor's bounds, checked before a context is asked for."""
        self.B, self.cap = B, cap = int(batch), int(num_particles)
        self.wide = bool(wide)
        if B < 1 or B > 65535:
            raise MidasError("BatchLoopEngine holds 1 .. 65535 trajectories")
        # one DBSCAN pass for the batch (None: whenever its cell tables hold the batch) or one per trajectory
        if batched_dbscan and B * cap > _lib.DBSCAN_BATCH_MAX_POINTS:
            raise MidasError(f"batched_dbscan=True holds at most DBSCAN_BATCH_MAX_POINTS = {_lib.DBSCAN_BATCH_MAX_POINTS} particles in all, "
                             f"not {B} x {cap} (None or False: one pass per trajectory there)")
        self.batched_dbscan = B * cap <= _lib.DBSCAN_BATCH_MAX_POINTS if batched_dbscan is None else bool(batched_dbscan)
        if self.wide:
            if cap < 1 or cap > _lib.LOOP_BATCH_WIDE_MAX_CAP:
                raise MidasError(f"a wide BatchLoopEngine holds 1 .. {_lib.LOOP_BATCH_WIDE_MAX_CAP} particles per trajectory (larger sets: LoopEngine)")
            if B * cap > 1 << 24:
                raise MidasError(f"a wide BatchLoopEngine holds at most 2^24 particles in all, not {B} x {cap}")
        elif cap < 1 or cap > _lib.LOOP_BATCH_MAX_CAP:
            raise MidasError(f"BatchLoopEngine holds 1 .. {_lib.LOOP_BATCH_MAX_CAP} particles per trajectory (larger sets: LoopEngine)")

    def _alloc_batch(self):
        """The state of B trajectories behind the set-up (self.K scores and stamps a row) and the frames' scratch."""
        B, cap = self.B, self.cap
        self._topk_ties = "index"
        self._alloc_state((B,), self._topk_ties)
        self._args.dbscan_batched = int(self.batched_dbscan)
        self.torch_streams = None  # seed_torch_streams
        self._std_override = None  # set for the length of one step_still() only
        # The scratch every phase combination of a batch frame asks for, reserved now so that no frame allocates: per trajectory the
        # hand-over records of the front (32 B a particle), the block results, the cluster-moment partials (64 x 36 doubles per 256
        # particles) and cluster rows, the resample's prefix values, a wide engine's select state; once, DBSCAN's cell tables (84 MB +
        # 41 B a particle) - the batched pass: the same tables, 41 B for every particle of the batch, and per trajectory its record, root
        # list and bounds partials.
        per_traj = self._per_traj()
        self._scratch = (128 << 20) + 256 * cap + B * per_traj + (64 + 32 * self.batched_dbscan) * 256
        self.ctx.call("midas_scratch_reserve", self._scratch)

    @classmethod
    def for_objects(cls, objects, row_object, num_particles: int, **kw):
        """A batch whose rows stand on different objects - the reference's sweep over objects, logs and trials (bash/run_filter.sh) as
        one engine.  objects: a list of (cb_poses, cb_embeddings, mesh_vertices) triples, or of (tactile_tree, None, ops.Tree) as the
        constructor takes them; row_object: for each of the B rows the index of its object, in any order; **kw: the constructor's
        keywords (wide, batched_dbscan, seed, floor, ...), shared by all rows.  Every object's codebook index is built on one context;
        all codebooks are float32 with one D.  New attributes: `objects` (per object: cb_poses, cb_feat, tree6, codebook, tree3),
        `row_object` and `Ks` (the objects' codebook sizes; `K` is the largest, the extent of a row's scores)."""
        objects, row_object = list(objects), [int(i) for i in row_object]
        if not objects:
            raise MidasError("for_objects needs at least one object")
        if not row_object:
            raise MidasError("for_objects needs at least one row")
        for b, i in enumerate(row_object):
            if not 0 <= i < len(objects):
                raise MidasError(f"row {b}: object index {i} outside the {len(objects)} objects")

        def dim(o):  # D of an object's codebook as given, without touching a device
            return int(o[0].codebook.D) if o[1] is None else int(torch.as_tensor(o[1]).shape[-1])
        Ds = [dim(o) for o in objects]
        if len(set(Ds)) > 1:
            raise MidasError(f"for_objects needs codebooks of one D, got {Ds}")
        unknown = sorted(set(kw) - set(DEFAULTS))
        if unknown:
            raise MidasError(f"for_objects: unknown keyword(s) {unknown}; the constructor's are {sorted(DEFAULTS)}")
        self = cls.__new__(cls)
        self._init(objects, row_object, len(row_object), num_particles, **{**DEFAULTS, **kw})
        return self

    # ---- the filter's parameters per row ---------------------------------------------------------------------------------
    @property
    def per_row(self):
        """The ROW_PARAMS that hold a value per row at the moment (a tuple of names; empty: every parameter is shared)."""
        return tuple(k for k in ROW_PARAMS if self._rows[k] is not None)

    def row_params(self):
        """ROW_PARAMS as the rows hold them now: name -> list of B values."""
        return {k: list(self._rows[k]) if self._rows[k] is not None else [getattr(self, k)] * self.B for k in ROW_PARAMS}

    def set_row_params(self, **kw):
        """Changes `sig_t`, `sig_r`, `pen_max`, `floor` and / or `softmax` between frames: each one value for the batch or B values
        (a scalar makes the parameter shared again).  Every value is checked before any is taken: a refused call - another length than
        B, a negative or NaN sigma, a floor below 1, per-row values on an engine with seeded streams or the ATen tie rule - leaves the
        engine as it was.  Nothing is enqueued; the next frame's table carries the new values."""
        unknown = sorted(set(kw) - set(ROW_PARAMS))
        if unknown:
            raise MidasError(f"set_row_params: unknown keyword(s) {unknown}; a row's parameters are {list(ROW_PARAMS)}")
        new = {k: row_values(k, v, self.B) for k, v in kw.items()}
        rows = dict(self._rows, **{k: v[1] for k, v in new.items()})
        if any(v is not None for v in rows.values()):
            self._check_rows_regime()
        for k, (scalar, _) in new.items():
            if scalar is not None:
                setattr(self, k, scalar)
        self._rows = rows
        self._rows_version += 1  # (the resident tables are keyed by it: none of them is this setting's)
        self._write_params()

    def _check_rows_regime(self):
        if self.torch_streams is not None or self._topk_ties == "aten_cpu":
            raise MidasError("per-row filter parameters need device draws and ties by index: a seeded frame's counted draw carries one std "
                             "per segment, and the ATen tie rule stays shared-parameter (seed_torch_streams(None) / topk_ties = 'index' first)")

    def _row_plan(self, multiplier, unit_weights, std_override):
        """What a frame's parameter table is made from, checked - nothing is built, uploaded or changed here: -> (key, shared
        unit_weights).  key is None when every parameter and `unit_weights` are shared (the frame takes the entries it always took);
        else (version of the rows' parameters, the five shared attributes as they stand, multiplier, std_override, unit_weights as a
        bool or a tuple of B) - the table is a
        function of the key, so a steady frame looks its table up without building anything."""
        unit = row_values("unit_weights", unit_weights, self.B)
        if unit[1] is None and not self.per_row:
            return None, unit[0]
        self._check_rows_regime()
        override = None if std_override is None else (float(std_override[0]), float(std_override[1]))
        shared = tuple(getattr(self, k) for k in ROW_PARAMS)  # (a shared parameter may be set as an attribute, as on the shared frame)
        return (self._rows_version, shared, max(float(multiplier), 1.0), override, unit[0] if unit[1] is None else tuple(unit[1])), False

    def _row_table(self, key):
        """The table of `_row_plan`'s key on the device.  The last ROW_TABLES_KEPT keys' tables stay resident; a key that is not among
        them builds its table on the host - a row's std is float32(max(multiplier, 1) * sig_b), the product formed in float64 as
        LoopEngine forms it - and sends it from pinned memory without waiting for the copy (40 B a row; the engine's first miss allocates the page-locked
        buffer, which may synchronise - later misses take it from torch's host cache; the stream orders the copy in
        front of the frame, and a replaced table's memory behind the frames that read it).  A sweep builds two (still and moving
        frames); rows with different `update_freq` cycle through lcm(frequencies) unit-weight patterns - beyond ROW_TABLES_KEPT of
        them every frame that misses builds and sends its table again (O(B) host work, no stall)."""
        dev = self._row_tables.pop(key, None)
        if dev is None:
            _, _, mul, override, unit = key
            col = self.row_params()
            if override is None:
                std_t, std_r = ((mul * np.asarray(col[k], dtype=np.float64)).astype(np.float32) for k in ("sig_t", "sig_r"))
            else:
                std_t, std_r = np.float32(override[0]), np.float32(override[1])
            tab = row_params_table(self.B, std_t, std_r, col["pen_max"], col["floor"], col["softmax"], unit)
            dev = torch.from_numpy(tab.view(np.uint8)).pin_memory().to(self.device, non_blocking=True)
            while len(self._row_tables) >= ROW_TABLES_KEPT:
                self._row_tables.pop(next(iter(self._row_tables)))  # (the least recently used)
            self.row_table_uploads += 1
        self._row_tables[key] = dev  # (most recently used last)
        if self._row_set is None:  # one codebook: the rows entry reads objects from a set - one object, every row on it
            me = SimpleNamespace(cb_poses=self.cb_poses, cb_feat=self.cb_feat, tree6=self.tree6, codebook=self.codebook, tree3=self.tree3)
            self._row_set = ops.ObjectSet(self.ctx, [me], [0] * self.B)
        return dev

    # whom annealing's torch.topk takes inside a tie: "index" (torch's CUDA rule, the radix select: midas_loop_step_batch as ever) or
    # "aten_cpu" (the reference as it runs on the CPU, topk_aten.hip: midas_loop_step_batch_draws); settable between frames
    @property
    def topk_ties(self):
        return self._topk_ties

    @topk_ties.setter
    def topk_ties(self, rule):
        if rule == "aten_cpu" and self.wide:
            raise MidasError("a wide BatchLoopEngine breaks ties by index: the ATen tie rule beyond 16 384 particles stays with LoopEngine")
        if rule == "aten_cpu" and self.per_row:
            raise MidasError(f"the ATen tie rule stays shared-parameter: {list(self.per_row)} hold a value per row (set_row_params with scalars first)")
        self._args.topk_ties = TOPK_TIES[rule]
        if rule == "aten_cpu":  # the walk's queue, stopper lists, marks and block counts per trajectory, beside the frame's own
            cap = self.cap
            self._scratch = max(self._scratch, (128 << 20) + 256 * cap + self.B * (self._per_traj() + 25 * cap + 4 * ((cap + 4095) // 4096)) + 80 * 256)
            self.ctx.call("midas_scratch_reserve", self._scratch)
        self._topk_ties = rule

    def _per_traj(self):
        cap = self.cap
        nb, nb256 = (cap + 4095) // 4096, (cap + 255) // 256
        frame = 32 * cap + 32 * nb + 8 * 64 * 10 + 8 * 36 * 64 * nb256 + 4 * 64 * 16 + 4 * 64 * 3 + 8 * 64 + 8 * (cap + 16) + 12 * nb
        if self.wide and cap > _lib.LOOP_BATCH_MAX_CAP:
            # the radix selection per trajectory (anneal.hip select_scratch): 6 x 2048 histogram words, 32 state words, two block counts
            # a summation block, and cap / 3 + 1 (key, index) pairs twice - selected, then sorted
            frame += 4 * 6 * 2048 + 4 * 32 + 2 * 4 * nb + 2 * (8 + 4) * (cap // 3 + 1)
        if self.batched_dbscan:
            # dbscan.hip launch_dbscan_batch: cell, sorted position, point, core flag, parent, worklist, cell list and rank per particle;
            # a record (96 B), 64 roots and up to 64 x 6 bounds partials per trajectory
            frame += 41 * cap + 96 + 4 * 64 + 24 * min(nb256, 64)
        return frame

    # ---- state ----------------------------------------------------------------------------------------------------
    def set_particles(self, poses, labels=None, reset_annealing: bool = True):
        """Start (or restart) every trajectory: poses (B, n, 4, 4), or a list of B tensors (n_b, 4, 4) with n_b <= capacity each;
        labels likewise, default 0 like `Particles` (particle_filter.py:47).  Annealing starts over, unless reset_annealing=False:
        every trajectory then keeps its particle_var, init_particles and frame count, as LoopEngine.set_particles does."""
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
        self._hint.fill_(-1)
        self._labels.zero_()
        ncl = [1] * self.B  # label 0 everywhere
        for b, (p, n) in enumerate(zip(poses, ns)):
            self._poses[b, :n].copy_(p)
            if labels is not None:
                self._labels[b, :n].copy_(labels[b])
                ncl[b] = int(labels[b].max().item()) + 1
        self._write_particles_block(ns, ncl, reset_annealing)
        self._n_host = ns

    def set_annealing_state(self, particle_vars, init_particles):
        """particle_filter.particle_var / init_particles (particle_filter.py:413-417) of every trajectory, B of each - for restarts
        and replays, as LoopEngine.set_annealing_state per row."""
        pv, ip = [float(v) for v in particle_vars], [int(v) for v in init_particles]
        if len(pv) != self.B or len(ip) != self.B:
            raise MidasError(f"{len(pv)} variances and {len(ip)} counts for a batch of {self.B} trajectories")
        self._write_annealing_state(pv, ip)

    # ---- seeded runs ----------------------------------------------------------------------------------------------
    def seed_torch_streams_low_var(self, seeds):
        """seed_torch_streams for an engine built with resample="low_var" / "low_var_batch": behind annealing row b draws the one
        float32 `torch.rand(1)` of the systematic resampler (particle_filter.py:291) - none on a frame where the resampler returns
        before it draws (NDRAW = 0: the row's stream stands still) - and the resample reads row b's offset from device memory
        (MIDAS_U32_FROM_U).  Row b is bit for bit a LoopEngine with seed_torch_stream_low_var(seeds[b]).  A method of its own:
        seed_torch_streams on a systematic engine refuses, as it always did."""
        return self._seed_torch_streams(seeds, True)

    def seed_torch_streams(self, seeds):
        return self._seed_torch_streams(seeds, False)

    def _seed_torch_streams(self, seeds, systematic: bool):
        """Trajectory b draws as a process of the reference under torch.manual_seed(seeds[b]) (or continues the torch.Generator
        seeds[b]): `torch.normal(0, mul * sig_t, (n_b, 3))`, `torch.normal(0, mul * sig_r, (n_b, 3))` with n_b ITS live count
        (add_noise_to_odom, particle_filter.py:326-335) and, behind annealing, n_set_b float64 uniforms (the resampler's
        torch.multinomial, :245) or - seed_torch_streams_low_var on an engine built with resample="low_var" -
        its one float32 offset (torch.rand(1), :291) - none for a row whose weights are all zero or hold a NaN on that frame, where the resampler returns
        before it draws (:237-241; ctl_i[b][LOOP_I_NDRAW]) - all counts read on the device (midas_mt19937_draws_counted_batch); ties of annealing's top-k follow
        ATen's CPU kernel (`topk_ties` becomes "aten_cpu").  Returns the TorchCpuStreams (manual_seed / from_host / to_host per
        row).  seeds=None: back to Philox draws and ties by index.
        The generator runs on the engine's stream; its scratch and the walk's are reserved here, so no frame allocates.  A live
        count below 6 (fewer than 16 normal values: ATen's scalar path, not modelled) or beyond the capacity is reported per
        trajectory by read_log()."""
        if seeds is None:
            self.torch_streams = None
            self.topk_ties = "index"
            return None
        if self.wide:
            raise MidasError("a wide BatchLoopEngine draws from Philox: seeded torch streams beyond 16 384 particles stay with LoopEngine")
        if self.per_row:
            raise MidasError(f"seeded torch streams stay shared-parameter (one std per counted draw): {list(self.per_row)} hold a value per "
                             "row (set_row_params with scalars first)")
        seeds = list(seeds)
        if len(seeds) != self.B:
            raise MidasError(f"{len(seeds)} seeds for a batch of {self.B} trajectories")
        from .torch_rng import TorchCpuStreams
        st, need = self._seed_streams(TorchCpuStreams, seeds, systematic)
        self.topk_ties = "aten_cpu"
        self._scratch = max(self._scratch, need)
        self.ctx.call("midas_scratch_reserve", self._scratch)  # (the generator shares the engine's context)
        self.torch_streams = st
        return st

    def project_to_codebook(self):
        """poses := codebook pose nearest to each particle (filter/filter.py:159-160), every trajectory's live set - on the codebook
        of its own object."""
        for b, n in enumerate(self.n):
            o = self if self.objects is None else self.objects[self.row_object[b]]
            idx = ops.nn6(o.tree6, ops.se3_feature(self._poses[b, :n]))
            self._poses[b, :n].copy_(ops.gather_rows(o.cb_poses, idx))
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
        return self._frame_view(self.read_log(self.step_count - 1, self.step_count, rows=(b,))[0][0], b)

    # ---- one batch frame ------------------------------------------------------------------------------------------
    def step(self, odoms, codes, gts=None, u32=-1.0, multiplier: float = 1.0, dbscan=None, unit_weights=False):
        """Enqueues one frame of every trajectory and reads nothing back: odoms (B,4,4), codes (B,D), gts (B,4,4) or None.
        dbscan: None = on every `cluster_every`-th frame (filter.py:182), True / False to force - for all trajectories alike.
        unit_weights: a frame without measurement update (filter_real.py:205-212) - a bool, or B bools: the rows' own cadences.
        u32: the systematic resampler's offset (resample="low_var") - a number for every row (< 0: Philox, keyed by seed + row), or B
        values (a host or device tensor, a list): row b resamples with its own, as a LoopEngine stepped with u32 = values[b] does.
        The B values go to device memory (MIDAS_U32_FROM_U) through the entry that takes draws: not for a wide engine or per-row
        parameters, and not on a seeded frame, where the streams draw the offsets.
        A frame with another motion noise than multiplier x (sig_t, sig_r) - LoopEngine.step's `std_override` - is `step_still`."""
        row_key, unit_weights = self._row_plan(multiplier, unit_weights, self._std_override)  # (checks only)
        u32_rows = None if isinstance(u32, numbers.Real) else self._u32_rows(u32, row_key)  # (checks, then a (B,) column write)
        u32 = _lib.U32_FROM_U if u32_rows is not None else u32
        u32_seeded = self._seeded_u32(u32) if self.torch_streams is not None else None  # (a check as well)
        phases = self._phase_mask(ALL_PHASES, dbscan)
        odoms, codes, gts = frame_operands(self.device, (self.B,), self.D, odoms, codes, gts)
        rows = None if row_key is None else self._row_table(row_key)  # (behind every refusal: a refused frame has changed nothing)
        a = self._frame_scalars(u32, multiplier, unit_weights, self._std_override)
        a.odom16, a.code, a.gt16 = _ptr(odoms), _ptr(codes), _ptr(gts)
        a.part_rmse = _ptr(self._part_rmse) if gts is not None else None
        self._keep = (odoms, codes, gts)  # keep operands alive until the stream has consumed them
        st, log_stride = self.torch_streams, self.log_frames * _lib.LOOP_LOG_DOUBLES

        def call(entry, ph):
            self.ctx.bind_current_stream()
            if rows is not None:  # the filter's parameters per row: the objects frame by the kernels that read the table
                self.ctx.check(self.ctx.lib.midas_loop_step_batch_rows(self.ctx.h, self._row_set.h, C.byref(a), _ptr(rows), int(ph), self.B,
                                                                       log_stride, int(self.wide)))
                return
            if self._set is not None:  # rows on different objects: one entry, the regime of `entry` by its `wide` flag
                self.ctx.check(self.ctx.lib.midas_loop_step_batch_objects(self.ctx.h, self._set.h, C.byref(a), int(ph), self.B, log_stride,
                                                                          int(self.wide)))
                return
            self.ctx.check(entry(self.ctx.h, self.codebook.h, self.tree6.h, self.tree3.h, C.byref(a), int(ph), self.B, log_stride))

        if st is not None:
            # the stream's draws, every row's sized by ITS live and annealed counts: a row whose weights are all zero or hold a NaN
            # draws no uniforms on this frame - its stream stays where it is, the other rows' move on
            a.tn, a.rot, a.u = _ptr(self._tn), _ptr(self._rot), _ptr(self._u)
            a.stream_draws = 1
            a.u32 = u32_seeded
            try:
                self._seeded_frame(st, (a.std_t, a.std_r), self.cap, self.cap,
                                   lambda: call(self.ctx.lib.midas_loop_step_batch_draws, phases & ~_lib.LOOP_RESAMPLE),
                                   lambda: call(self.ctx.lib.midas_loop_step_batch_draws, _lib.LOOP_RESAMPLE), status=(self.log_frames,))
            finally:
                a.tn = a.rot = a.u = None
                a.stream_draws = 0
        elif u32_rows is not None:  # the rows' own offsets, read from the first slot of each row of uniforms
            a.u = _ptr(u32_rows)
            try:
                call(self.ctx.lib.midas_loop_step_batch_draws, phases)
            finally:
                a.u = None
        elif self._topk_ties == "aten_cpu":
            call(self.ctx.lib.midas_loop_step_batch_draws, phases)  # (Philox draws, the ATen tie rule)
        elif self.wide:
            call(self.ctx.lib.midas_loop_step_batch_wide, phases)
        else:
            call(self.ctx.lib.midas_loop_step_batch, phases)
        self._frame_done()

    def _u32_rows(self, u32, row_key):
        """B systematic offsets as a frame reads them from device memory: the first double of every row of a (B, cap) buffer of the
        engine's, rewritten per frame on the stream (the float32 values, exactly)."""
        if self.mode != _lib.RESAMPLE_SYSTEMATIC:
            raise MidasError("u32 per row is the systematic resampler's offset: resample='low_var' / 'low_var_batch' only")
        if self.torch_streams is not None:
            raise MidasError("seed_torch_streams: the streams draw the systematic offsets - passing u32 would desynchronise them from the "
                             "reference's")
        if self.wide or row_key is not None:
            raise MidasError("u32 per row goes through the entry that takes draws: not on a wide engine, not with per-row parameters "
                             "or unit_weights")
        v = torch.as_tensor(u32)
        if v.numel() != self.B:
            raise MidasError(f"u32: expected one offset or {self.B} (one per row), got {v.numel()}")
        if getattr(self, "_u32_buf", None) is None:
            self._u32_buf = torch.zeros((self.B, self.cap), dtype=torch.float64, device=self.device)
        self._u32_buf[:, 0] = v.to(self.device).to(torch.float32).to(torch.float64).reshape(self.B)
        return self._u32_buf

    def step_still(self, odoms, codes, gts=None, std_override=(0.0, 0.0), **kw):
        """`step()` with this one frame's motion noise (std_t, std_r) in place of multiplier x (sig_t, sig_r), shared by the rows, as
        LoopEngine.step(std_override=...) - by default (0.0, 0.0): the frames the reference starts from, where it does not call
        motionModel (filter/filter.py:152-160).  The override holds for this call alone, also when the call raises."""
        self._std_override = (float(std_override[0]), float(std_override[1]))
        try:
            self.step(odoms, codes, gts, **kw)
        finally:
            self._std_override = None

    # ---- results --------------------------------------------------------------------------------------------------
    def read_log(self, first: int = 0, last: int = None, strict: bool = True, rows=None):
        """Per trajectory, LoopEngine.read_log's records of frames [first, last) - a list of B lists, one read-back - with its
        handling of the frames' condition bits, a seeded stream's short or out-of-range draw included (reported for the trajectory
        it happened to).  rows: only these trajectories (a list in their order)."""
        first, last = self._log_window(first, last)
        which = range(self.B) if rows is None else rows
        log = (self._log if rows is None else self._log[list(rows)]).cpu().numpy()
        mt = None
        if self.torch_streams is not None:  # (seed_torch_streams: the counted draws' status, a word per trajectory and row)
            mt = (self._mt_status if rows is None else self._mt_status[list(rows)]).cpu().numpy()
        return [log_records(log[i], first, last, mt=None if mt is None else mt[i], strict=strict, who=f"trajectory {b}, ")
                for i, b in enumerate(which)]
