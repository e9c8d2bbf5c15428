"""torch's CPU random stream, reproduced on the device (csrc/mt19937.hip, include/midas_hip.h midas_mt19937_*).

The reference resamples with `WeightedRandomSampler` -> `torch.multinomial(weights.double(), N, True)` on torch's default
CPU generator (modules/particle_filter.py:245): under `torch.manual_seed(s)` the N draws are the stream of
`torch.rand(N, dtype=float64)`.  `TorchCpuStream(seed)` keeps that generator's state in device memory and hands out the
same uniforms without a host generator or a per-frame upload; `skip_normal(numel)` steps over the outputs a
`torch.normal(..., size)` of float32 values would have taken (add_noise_to_odom, :326-335), so a caller that still draws
its motion noise on the host generator stays aligned with the reference's stream.

`TorchCpuStreams(seeds)` holds B such streams - B seeded runs of the reference, one trajectory each, as a batch engine runs
them - and draws a frame of all of them by one call (midas_mt19937_draws_batch), or, where every trajectory's particle count is its own and changes every frame
(BatchLoopEngine.seed_torch_streams), with the sizes read from B control blocks on the device (midas_mt19937_draws_counted_batch).
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import _ptr


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def normal_words(numel: int) -> int:
    """32-bit generator outputs one CPU torch.normal of `numel` float32 values consumes (ATen normal_fill: one per value,
    the last 16 drawn again when numel is not a multiple of 16).  Sizes below 16 take ATen's scalar path: not modelled."""
    if numel < 16:
        raise _lib.MidasError("torch.normal of fewer than 16 values uses another code path of ATen: not modelled")
    return numel + (16 if numel % 16 else 0)


def counted_segment_words(kind: int, per: int, bound: int) -> int:
    """Raw words a counted call's scratch holds for one segment at its bound (csrc/mt19937.hip mt_counted_raw_words)."""
    if kind == _lib.MT_SEGMENT_RAND64:
        return 2 * per * bound
    return 1 if kind == _lib.MT_SEGMENT_RAND32 else per * bound + 16


def rand32_words(n: int = 1) -> int:
    """32-bit generator outputs one CPU torch.rand(n) of float32 values consumes: one per value (its low 24 bits times 2^-24).
    Only the single draw of the reference's systematic resampler (particle_filter.py:291) is modelled."""
    if int(n) != 1:
        raise _lib.MidasError("torch.rand of float32 values is modelled for the single draw torch.rand(1) only")
    return 1


_F64_KINDS = (_lib.MT_SEGMENT_RAND64, _lib.MT_SEGMENT_RAND32)  # (a rand32 value leaves the generator as the float64 that holds it)


# ---- torch's host generator state <-> a device state row ----------------------------------------------------------------
# Layout of the host state (CPUGeneratorImpl's legacy pod, 5056 bytes): uint64 seed | int32 left | int32 seeded | uint64 next |
# uint64 state[624] | ..; a device row is the 624 words of the current block and the number of them consumed (csrc/mt19937.hip).
def _host_state_row(generator: torch.Generator | None):
    """The device state row (626 int32, host) that continues `generator` (None: torch's default CPU generator) where it stands."""
    import numpy as np
    b = (torch.get_rng_state() if generator is None else generator.get_state()).numpy()
    if b.size != 5056:
        raise _lib.MidasError("unexpected layout of torch's CPU generator state")
    left = int(np.frombuffer(b[8:12].tobytes(), dtype=np.int32)[0])
    nxt = int(np.frombuffer(b[16:24].tobytes(), dtype=np.uint64)[0])
    words = np.frombuffer(b[24:24 + 624 * 8].tobytes(), dtype=np.uint64).astype(np.uint32)
    # at::mt19937 twists when --left reaches 0: left == 1 means "a new block is due" whatever next says (fresh seeds: left 1, next 0)
    pos = 624 if left == 1 else nxt
    return np.concatenate([words, np.array([pos, 0], dtype=np.uint32)]).view(np.int32)


def _set_host_state(st, generator: torch.Generator | None):
    """Make `generator` (None: torch's default CPU generator) continue where the device state row `st` (626 uint32, host) stands."""
    import numpy as np
    pos = int(st[624])
    g = torch.default_generator if generator is None else generator
    b = g.get_state().numpy().copy()
    if b.size != 5056:
        raise _lib.MidasError("unexpected layout of torch's CPU generator state")
    # pos words of the stored block are consumed: next = pos, left = 624 - pos + 1 (the twist happens when --left hits 0)
    b[8:12] = np.frombuffer(np.int32(624 - pos + 1).tobytes(), dtype=np.uint8)
    b[12:16] = np.frombuffer(np.int32(1).tobytes(), dtype=np.uint8)
    b[16:24] = np.frombuffer(np.uint64(pos if pos < 624 else 0).tobytes(), dtype=np.uint8)
    b[24:24 + 624 * 8] = np.frombuffer(st[:624].astype(np.uint64).tobytes(), dtype=np.uint8)
    g.set_state(torch.from_numpy(b))


class _GeneratorSide:
    """What TorchCpuStream and TorchCpuStreams share: the generator's stream and context, the jump-polynomial cache with its
    chaining policy (`chain_after`, `pieces_for`) and the torch.normal tables."""

    def _setup(self, device, overlap: bool, pieces: int):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = _lib.context(dev).device
        self.overlap = bool(overlap)
        if self.overlap:
            self.side = torch.cuda.Stream(self.device)
            with torch.cuda.stream(self.side):
                self.ctx = _lib.Context(self.device)  # bound to the side stream for good (never re-bound)
        else:
            self.side = None
            self.ctx = _lib.context(dev)
        self.pending_skip = 0
        self.pieces = int(pieces)
        self.chain_after = 2  # occurrences of a (previous size, skip, size) pattern before its jump polynomials are computed (1: at once)
        self._hist_words = 0   # words the call that wrote _hist handed out (0: no history)
        self._polys = {}       # (previous words, skip, words) -> device table of the pieces' polynomials

    def _enter(self):
        """Orders the generator's stream behind the caller's current stream (state, buffers and seeds are shared with it)."""
        if self.side is None:
            self.ctx.bind_current_stream()
            return
        self.side.wait_stream(torch.cuda.current_stream(self.device))

    def _call(self, name, *args):
        self.ctx.check(getattr(self.ctx.lib, name)(self.ctx.h, *args))

    def skip_words(self, n: int):
        """Step over n 32-bit outputs (applied with the next draw)."""
        self.pending_skip += int(n)
        return self

    def skip_normal(self, numel: int):
        """Step over what torch.normal(mean, std, size) with `numel` float32 values takes."""
        return self.skip_words(normal_words(numel))

    def skip_rand32(self, n: int = 1):
        """Step over what torch.rand(1) of a float32 value takes (a systematic resampler's offset drawn on the host)."""
        return self.skip_words(rand32_words(n))

    def _chain_polys(self, words: int, pieces: int | None = None):
        """The jump polynomials of a call of `words` words, or None (no history / too short: the sequential walk)."""
        pieces = self.pieces if pieces is None else pieces
        if pieces > 0 and self._hist_words and words >= _lib.MT19937_HIST_WORDS:
            # the polynomials cost the host ~10 ms each: worth it for a pattern of sizes that REPEATS (a fixed-N engine: the same
            # three calls every frame), not for a particle count that changes every frame (the annealing loop: 100 ms a frame of
            # host arithmetic when every call asked for its own set) - a (previous size, skip, size) is served in pieces from its
            # second occurrence on
            key = (self._hist_words, self.pending_skip, words, pieces)
            if key in self._polys:
                return self._polys[key]
            seen = self.__dict__.setdefault("_seen", {})
            if len(seen) > 256:
                seen.clear()
            seen[key] = seen.get(key, 0) + 1
            if seen[key] >= self.chain_after:
                return self._piece_polys(self._hist_words, self.pending_skip, words, pieces)
        return None

    def _drawn(self, words: int, out):
        # (a call too short to leave a history, or a pure skip, breaks the chain: the next call walks sequentially)
        self._hist_words = words if words >= _lib.MT19937_HIST_WORDS else 0
        self.pending_skip = 0
        if self.side is None:
            return out, None
        ev = torch.cuda.Event()
        ev.record(self.side)
        return out, ev

    def _normal_tables(self):
        """The three 2^24-entry tables of torch.normal's float32 path on this machine (torch_normal.py), on the device."""
        tabs = getattr(self, "_ntab", None)
        if tabs is None:
            from . import torch_normal
            with torch.cuda.stream(self.side) if self.side is not None else _null():
                tabs = tuple(torch.from_numpy(a).to(self.device) for a in torch_normal.host_tables())
            self._ntab = tabs
        return tabs

    def pieces_for(self, words: int) -> int:
        """Pieces a call of `words` words is cut into: `pieces` for a draw of 2 x 10^5 words (N = 10^5 uniforms), more for longer calls
        so that a piece stays ~54 blocks of 624 words (the walk of a piece is the sequential part; a jump costs ~2 us a piece)."""
        if self.pieces <= 0:
            return 0
        return max(self.pieces, min(48, -(-words // (54 * 624))))

    def _piece_polys(self, prev_words: int, skip: int, words: int, pieces: int | None = None):
        pieces = self.pieces if pieces is None else pieces
        key = (prev_words, skip, words, pieces)
        tab = self._polys.get(key)
        if tab is None:
            import numpy as np

            from . import mt_jump
            nblocks = -(-words // 624)
            bpc = -(-nblocks // pieces)
            rows = []
            for c in range(pieces):
                J = prev_words + skip + c * bpc * 624
                if not mt_jump.check(J):
                    raise _lib.MidasError(f"mt19937 jump polynomial for distance {J} failed its check against the reference generator")
                rows.append(mt_jump.jump_words(J))
            host = torch.from_numpy(np.stack(rows).view(np.int32))
            if len(self._polys) >= 16:
                self._polys.clear()
            # uploaded on the generator's stream (the caller is inside _enter() .. the launch)
            with torch.cuda.stream(self.side) if self.side is not None else _null():
                tab = host.to(self.device)
            self._polys[key] = tab
        return tab


class TorchCpuStream(_GeneratorSide):
    """`overlap=True` (default): the generator runs on a stream and a library context of its own - its single-workgroup block
    recurrence (one CU, ~100 us for a frame's 2 N words at N = 100k: 321 blocks of 624 words at 310 ns) then runs BESIDE the frame kernels of the caller's stream
    instead of in front of them.  `rand64()` orders the result behind the caller's stream as before; `rand64_async()` returns
    (tensor, event) and leaves the wait to the consumer (the pipelined engine: the draws of frame t are consumed by frame
    t + 1's launch).  The output buffers rotate (3): a buffer is rewritten two calls later, after the side stream has waited
    for the caller's stream as of THAT call - whoever consumed it was enqueued before.

    `pieces` (default 6; 0 = always the sequential walk): a call's 2 N words are generated in that many pieces side by side once
    the previous call has left MIDAS_MT19937_HIST_WORDS of its words on the device - mt19937 is linear over GF(2), the words
    that start a piece follow from those by one polynomial per piece (mt_jump.py; computed on the host once per distinct
    (previous size, skip, size), ~10 ms each, checked against a reference generator before use).  Same numbers, bit for bit;
    321 sequential blocks (86 us at N = 100k) become 54: 12 us for the jump, 15 for the blocks, 4 for the conversion - the seeded
    step at c2 goes from 10.8k to 22.7k frames/s (4 / 6 / 8 / 12 pieces: 21.7 / 22.7 / 21.7 / 21.8k; tools/bench_parity_mode.py)."""

    def __init__(self, seed: int, device=None, overlap: bool = True, pieces: int = 6):
        self._setup(device, overlap, pieces)
        self.state = torch.zeros(626, dtype=torch.int32, device=self.device)
        self._hist = torch.zeros(_lib.MT19937_HIST_WORDS, dtype=torch.int32, device=self.device)
        self._bufs, self._turn = [None, None, None], 0
        self.manual_seed(seed)

    def manual_seed(self, seed: int):
        """torch.manual_seed(seed) for this stream."""
        self._enter()
        self._call("midas_mt19937_seed", int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(self.state))
        self.pending_skip = 0
        self._hist_words = 0
        self._mark = None
        return self

    # ---- hand-over between torch's host generator and this stream --------------------------------------------------
    # A caller that draws some numbers on the host (init_filter, particle_filter.py:129-145) and the per-frame ones here keeps
    # ONE stream: from_host() continues the host generator where it stands, to_host() gives it back (_host_state_row /
    # _set_host_state: the layout of the host state).
    def from_host(self, generator: torch.Generator | None = None):
        """Continue `generator` (default: torch's default CPU generator) on the device: the next draw here is the number the host
        generator would have produced next."""
        host = _host_state_row(generator)
        self._enter()
        with torch.cuda.stream(self.side) if self.side is not None else _null():
            self.state.copy_(torch.from_numpy(host.copy()), non_blocking=False)
        self.pending_skip = 0
        self._hist_words = 0
        self._mark = None
        return self

    def to_host(self, generator: torch.Generator | None = None):
        """Give the stream back: `generator` (default: torch's default CPU generator) continues where this stream stands
        (pending skips applied).  Synchronises with the generator's stream."""
        import numpy as np
        if self.pending_skip:
            self._enter()
            self._call("midas_mt19937_rand64_chunked", _ptr(self.state), self.pending_skip, 0, None, None, None, 0)
            self.pending_skip = 0
            self._hist_words = 0
        if self.side is not None:
            self.side.synchronize()
        else:
            torch.cuda.current_stream(self.device).synchronize()
        _set_host_state(self.state.cpu().numpy().view(np.uint32), generator)
        return self

    def rand64_async(self, N: int, out: torch.Tensor | None = None):
        """The next N values of torch.rand(N, dtype=torch.float64), enqueued on the generator's stream: (tensor, event or None).
        The consumer waits for the event on its stream before it reads the tensor (None: same stream, already ordered).
        Without `out` the tensor is one of THREE rotating internal buffers: ONE consumer, which has enqueued its use of a buffer
        before the third following call (the engines: one draw per frame, consumed by that frame) - anybody who keeps the
        tensor longer, or shares the stream object between engines, passes `out` (or calls rand64, which allocates)."""
        N = int(N)
        own = out is None
        fresh = False
        if out is None:
            i = self._turn
            self._turn = (i + 1) % 3
            if self._bufs[i] is None or self._bufs[i].numel() != N:
                fresh = True  # (see below: a new block may be memory the caller's stream is still using)
                # (a buffer dropped here may still be being written on the generator's stream: the allocator learns of that stream
                # at allocation, so the block is not handed out again before the write is done)
                self._bufs[i] = torch.empty(N, dtype=torch.float64, device=self.device)
                if self.side is not None:
                    self._bufs[i].record_stream(self.side)
            out = self._bufs[i]
        if own and self.side is not None:
            # A rotating buffer was last handed out three calls ago and, by the contract above, its consumer was enqueued before the
            # call after that one: the generator waits for the caller's stream as it stood at the PREVIOUS call, not as it stands
            # now - it may run a whole frame ahead of the kernels that are being enqueued (state and history are its own).
            cur = torch.cuda.current_stream(self.device)
            mark = torch.cuda.Event()
            mark.record(cur)
            prev, self._mark = getattr(self, "_mark", None), mark
            # (a buffer allocated in THIS call is a block the allocator may have taken back from the caller's stream a moment ago -
            # kernels enqueued there since the previous mark may still read it: the full wait, once per buffer)
            if prev is None or fresh:
                self.side.wait_stream(cur)
            else:
                self.side.wait_event(prev)
        else:
            self._enter()
        words = 2 * N
        polys = self._chain_polys(words)
        self._call("midas_mt19937_rand64_chunked", _ptr(self.state), self.pending_skip, N, _ptr(out), _ptr(self._hist), _ptr(polys),
                   self.pieces if polys is not None else 0)
        return self._drawn(words, out)

    def normal_async(self, mean: float, std: float, size, out: torch.Tensor | None = None):
        """torch.normal(mean, std, size=size) of float32 values - the reference's motion-noise draws (particle_filter.py:326-335) -
        from this stream, enqueued on the generator's stream: (tensor, event or None) as rand64_async.  The result is a fresh tensor
        unless `out` is given (float32, contiguous, numel elements); at least 16 values (ATen's scalar path below that is not
        modelled)."""
        shape = tuple(size) if hasattr(size, "__len__") else (int(size),)
        numel = 1
        for d in shape:
            numel *= int(d)
        if numel < 16:
            raise _lib.MidasError("torch.normal of fewer than 16 values uses another code path of ATen: not modelled")
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
            if self.side is not None:
                out.record_stream(self.side)
        R, Ct, S = self._normal_tables()
        self._enter()
        words = normal_words(numel)
        polys = self._chain_polys(words) if numel >= _lib.MT19937_HIST_WORDS else None
        self._call("midas_mt19937_normal32", _ptr(self.state), self.pending_skip, numel, float(mean), float(std), _ptr(R), _ptr(Ct), _ptr(S),
                   _ptr(out), _ptr(self._hist), _ptr(polys), self.pieces if polys is not None else 0)
        return self._drawn(words if numel >= _lib.MT19937_HIST_WORDS else 0, out)

    def normal(self, mean: float, std: float, size, out: torch.Tensor | None = None) -> torch.Tensor:
        """torch.normal(mean, std, size=size) (float32), ordered behind the caller's current stream."""
        z, ev = self.normal_async(mean, std, size, out)
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
        return z

    def draws_async(self, spec):
        """Several consecutive draws by ONE walk of the generator (midas_mt19937_draws): spec = sequence of ("rand64", N),
        ("normal", mean, std, size) and ("rand32",) in the stream's order - a seeded frame of the reference is normal (N, 3) twice and
        rand64 N (particle_filter.py:326-335, :245), or with the systematic resampler one rand32: torch.rand(1), a float32 value that
        comes back as the one-element float64 tensor holding it exactly, as the resample kernels take it (:291).  Returns ([tensors], event or None): the numbers of the separate calls, fresh tensors,
        enqueued on the generator's stream behind the caller's current stream."""
        import ctypes as C
        outs, segs, words, need_tables = [], [], 0, False
        for item in spec:
            if item[0] == "rand64":
                n = int(item[1])
                out = torch.empty(n, dtype=torch.float64, device=self.device)
                segs.append((_lib.MT_SEGMENT_RAND64, n, 0.0, 1.0, out))
                words += 2 * n
            elif item[0] == "rand32":
                n = rand32_words(item[1] if len(item) > 1 else 1)
                out = torch.empty(n, dtype=torch.float64, device=self.device)
                segs.append((_lib.MT_SEGMENT_RAND32, n, 0.0, 1.0, out))
                words += n
            elif item[0] == "normal":
                _, mean, std, size = item
                shape = tuple(size) if hasattr(size, "__len__") else (int(size),)
                numel = 1
                for d in shape:
                    numel *= int(d)
                if numel < 16:
                    raise _lib.MidasError("torch.normal of fewer than 16 values uses another code path of ATen: not modelled")
                out = torch.empty(shape, dtype=torch.float32, device=self.device)
                segs.append((_lib.MT_SEGMENT_NORMAL32, numel, float(mean), float(std), out))
                words += normal_words(numel)
                need_tables = True
            else:
                raise ValueError(f"unknown draw {item[0]!r}")
            if self.side is not None:
                out.record_stream(self.side)
            outs.append(out)
        R, Ct, S = self._normal_tables() if need_tables else (None, None, None)
        self._enter()
        arr = (_lib.MtSegment * len(segs))()
        for a, (kind, count, mean, std, out) in zip(arr, segs):
            a.kind, a.count, a.mean, a.std, a.out_dev = kind, count, mean, std, out.data_ptr()
        pieces = self.pieces_for(words)
        polys = self._chain_polys(words, pieces)
        self._call("midas_mt19937_draws", _ptr(self.state), self.pending_skip, len(segs), C.cast(arr, C.c_void_p), _ptr(R), _ptr(Ct), _ptr(S),
                   _ptr(self._hist), _ptr(polys), pieces if polys is not None else 0)
        _, ev = self._drawn(words, None)
        return outs, ev

    @staticmethod
    def _counted_items(spec):
        """spec of draws_counted_async -> [(kind, mean, std, count tensor, index, per, bound)]."""
        items = []
        for item in spec:
            if item[0] == "rand64":
                _, cnt, idx, bound = item
                items.append((_lib.MT_SEGMENT_RAND64, 0.0, 1.0, cnt, int(idx), 1, int(bound)))
            elif item[0] == "rand32":  # (the count is a control word: one value when it is not zero; `bound` is its range and the row of `outs`)
                _, cnt, idx, bound = item
                items.append((_lib.MT_SEGMENT_RAND32, 0.0, 1.0, cnt, int(idx), 1, int(bound)))
            elif item[0] == "normal":
                _, mean, std, cnt, idx, per, bound = item
                items.append((_lib.MT_SEGMENT_NORMAL32, float(mean), float(std), cnt, int(idx), int(per), int(bound)))
            else:
                raise ValueError(f"unknown draw {item[0]!r}")
            if cnt.dtype != torch.int32 or not cnt.is_cuda or not cnt.is_contiguous() or not 0 <= int(idx) < cnt.numel():
                raise _lib.MidasError("a counted draw takes its size from element `index` of a contiguous int32 device tensor")
        return items

    @classmethod
    def counted_scratch_bytes(cls, spec) -> int:
        """Scratch one draws_counted_async(spec) call takes of the generator's context (sized by the bounds)."""
        words = 3 * 624
        for kind, _, _, _, _, per, bound in cls._counted_items(spec):
            words += counted_segment_words(kind, per, bound)
        return (4 * words + 255) // 256 * 256 + 256

    def draws_counted_async(self, spec, outs=None, status=None):
        """draws_async for draws whose sizes stand in device memory (midas_mt19937_draws_counted): spec = sequence of
        ("rand64", count_tensor, index, bound), ("normal", mean, std, count_tensor, index, per, bound) and ("rand32", word_tensor,
        index, bound) - torch.rand(1) when word_tensor[index] is not zero, nothing when it is zero: the systematic resampler's offset
        on a frame where the resampler draws (ctl_i[LOOP_I_NDRAW]); the value is written to the first of `bound` float64 - in the stream's order -
        the draw takes per x count_tensor[index] values (rand64: per = 1) as that element stands when the kernels run, `bound` is
        what the host knows it cannot exceed.  The reference's loop, whose particle count annealing changes every frame: normal
        (n, 3) twice, then rand64 n_set (particle_filter.py:326-335, :245), enqueued without reading either count back.
        Returns ([tensors], event or None): flat tensors of per x bound elements (float64 / float32) of which the first
        per x count hold the draw and the rest are left as they were; `outs` gives the tensors to write into (each at least that
        long).  A count beyond its bound or a normal draw of 1 .. 15 values cannot raise here: the call then draws nothing and
        sets _lib.MT_STATUS_* bits in `status` = (int32 device tensor, index), by default the stream's own word, which
        counted_status() reads.  Always the sequential walk; the next draw of any kind walks sequentially too."""
        import ctypes as C
        items = self._counted_items(spec)
        if not 1 <= len(items) <= 8:
            raise _lib.MidasError("1 .. 8 draws a call")
        if status is None:
            if getattr(self, "_status", None) is None:
                self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
            status = (self._status, 0)
        outs = [None] * len(items) if outs is None else list(outs)
        arr = (_lib.MtCountedSegment * len(items))()
        need_tables = False
        for i, (a, (kind, mean, std, cnt, idx, per, bound)) in enumerate(zip(arr, items)):
            if outs[i] is None:
                outs[i] = torch.empty(per * bound, dtype=torch.float64 if kind in _F64_KINDS else torch.float32, device=self.device)
                if self.side is not None:
                    outs[i].record_stream(self.side)
            elif (outs[i].dtype != (torch.float64 if kind in _F64_KINDS else torch.float32) or outs[i].numel() < per * bound
                  or not outs[i].is_contiguous() or outs[i].device != self.device):
                raise _lib.MidasError(f"draw {i}: `outs` wants a contiguous device tensor of at least {per * bound} values of the draw's type")
            need_tables |= kind == _lib.MT_SEGMENT_NORMAL32
            a.kind, a.per, a.count_dev, a.bound, a.mean, a.std = kind, per, cnt.data_ptr() + 4 * idx, bound, mean, std
            a.out_dev = outs[i].data_ptr()
        R, Ct, S = self._normal_tables() if need_tables else (None, None, None)
        self._enter()
        self._call("midas_mt19937_draws_counted", _ptr(self.state), self.pending_skip, len(items), C.cast(arr, C.c_void_p), _ptr(R), _ptr(Ct),
                   _ptr(S), C.c_void_p(status[0].data_ptr() + 4 * int(status[1])))
        _, ev = self._drawn(0, None)  # (no history: the next call walks sequentially)
        return outs, ev

    def counted_status(self) -> int:
        """The _lib.MT_STATUS_* bits draws_counted_async calls have set in the stream's own status word (one small read-back)."""
        st = getattr(self, "_status", None)
        return 0 if st is None else int(st.item())

    def rand32(self) -> torch.Tensor:
        """The next torch.rand(1) (float32, one generator output), ordered behind the caller's current stream: a fresh (1,) float32
        tensor.  No read-back: the value stays on the device."""
        (u,), ev = self.draws_async([("rand32",)])
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
        return u.to(torch.float32)

    def rand64(self, N: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """The next N values of torch.rand(N, dtype=torch.float64) (== the draws of torch.multinomial(w64, N, True)), ordered
        behind the caller's current stream; a fresh tensor unless `out` is given."""
        if out is None:
            out = torch.empty(int(N), dtype=torch.float64, device=self.device)
            if self.side is not None:
                out.record_stream(self.side)  # written on the generator's stream: the allocator must know
        u, ev = self.rand64_async(N, out)
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
        return u


class TorchCpuStreams(_GeneratorSide):
    """B of torch's CPU streams, drawn together: stream b is a process of the reference under torch.manual_seed(seeds[b]) (or a
    host generator continued by from_host), and one call (midas_mt19937_draws_batch) hands out the same draws of every stream -
    a batch engine's frame of B seeded trajectories (BatchFilterEngine.seed_torch_streams).

    `device`, `overlap`, `pieces`, `chain_after` and `pieces_for` are TorchCpuStream's; the jump polynomials are shared by all
    streams (a distance from the first word of the previous call's history, the same for every stream).  draws_async returns
    fresh (B, ...) tensors written on the generator's stream and an event every read orders behind - no rotating buffers."""

    def __init__(self, seeds, device=None, overlap: bool = True, pieces: int = 6):
        seeds = list(seeds)
        if not seeds:
            raise _lib.MidasError("TorchCpuStreams needs at least one stream")
        self.B = len(seeds)
        self._setup(device, overlap, pieces)
        self.state = torch.zeros((self.B, 626), dtype=torch.int32, device=self.device)
        self._hist = torch.zeros((self.B, _lib.MT19937_HIST_WORDS), dtype=torch.int32, device=self.device)
        if all(isinstance(s, torch.Generator) for s in seeds):
            self.from_host(seeds)
        else:
            self.manual_seed(seeds)

    def _count(self, items, what):
        items = list(items)
        if len(items) != self.B:
            raise _lib.MidasError(f"{what}: expected {self.B} (one per stream), got {len(items)}")
        return items

    def _restart(self):
        self.pending_skip = 0
        self._hist_words = 0

    def manual_seed(self, seeds):
        """torch.manual_seed(seeds[b]) for stream b."""
        seeds = self._count(seeds, "seeds")
        self._enter()
        for b, s in enumerate(seeds):
            self._call("midas_mt19937_seed", int(s) & 0xFFFFFFFFFFFFFFFF, _ptr(self.state[b]))
        self._restart()
        return self

    def from_host(self, generators):
        """Stream b continues the host generator generators[b] where it stands."""
        import numpy as np
        rows = np.stack([_host_state_row(g) for g in self._count(generators, "generators")])
        self._enter()
        with torch.cuda.stream(self.side) if self.side is not None else _null():
            self.state.copy_(torch.from_numpy(rows), non_blocking=False)
        self._restart()
        return self

    def to_host(self, b: int, generator: torch.Generator | None = None):
        """Give stream b back: `generator` (default: torch's default CPU generator) continues where stream b stands (pending skips
        applied to every stream).  Synchronises with the generator's stream."""
        import numpy as np
        b = int(b)
        if not 0 <= b < self.B:
            raise _lib.MidasError(f"stream {b} of {self.B}")
        if self.pending_skip:
            self._enter()
            self._batch_call([(_lib.MT_SEGMENT_RAND64, 0, 0.0, 1.0, None)], None)
            self._restart()
        if self.side is not None:
            self.side.synchronize()
        else:
            torch.cuda.current_stream(self.device).synchronize()
        _set_host_state(self.state[b].cpu().numpy().view(np.uint32), generator)
        return self

    def _batch_call(self, segs, polys, pieces: int = 0, tables=(None, None, None)):
        import ctypes as C
        arr = (_lib.MtSegment * len(segs))()
        for a, (kind, count, mean, std, out) in zip(arr, segs):
            a.kind, a.count, a.mean, a.std, a.out_dev = kind, count, mean, std, None if out is None else out.data_ptr()
        R, Ct, S = tables
        self._call("midas_mt19937_draws_batch", self.B, _ptr(self.state), self.pending_skip, len(segs), C.cast(arr, C.c_void_p), _ptr(R),
                   _ptr(Ct), _ptr(S), _ptr(self._hist), _ptr(polys), pieces if polys is not None else 0)

    def _segments(self, spec):
        """spec -> ([(kind, count, mean, std, shape)], words per stream)."""
        segs, words = [], 0
        for item in spec:
            if item[0] == "rand64":
                n = int(item[1])
                segs.append((_lib.MT_SEGMENT_RAND64, n, 0.0, 1.0, (n,)))
                words += 2 * n
            elif item[0] == "rand32":
                n = rand32_words(item[1] if len(item) > 1 else 1)
                segs.append((_lib.MT_SEGMENT_RAND32, n, 0.0, 1.0, (n,)))
                words += n
            elif item[0] == "normal":
                _, mean, std, size = item
                shape = tuple(int(d) for d in size) if hasattr(size, "__len__") else (int(size),)
                numel = 1
                for d in shape:
                    numel *= d
                if numel < 16:
                    raise _lib.MidasError("torch.normal of fewer than 16 values uses another code path of ATen: not modelled")
                segs.append((_lib.MT_SEGMENT_NORMAL32, numel, float(mean), float(std), shape))
                words += normal_words(numel)
            else:
                raise ValueError(f"unknown draw {item[0]!r}")
        return segs, words

    def draws_async(self, spec):
        """The draws of `spec` (TorchCpuStream.draws_async's format: ("rand64", N), ("normal", mean, std, size), in the stream's order)
        from every stream by ONE call: ([tensors of shape (B, ...)], event or None) - row b of each is what TorchCpuStream.draws_async
        gives on stream b.  Fresh tensors, written on the generator's stream behind the caller's current stream: the consumer waits
        for the event before it reads them (None: the same stream, already ordered)."""
        segs, words = self._segments(spec)
        outs, call = [], []
        for kind, count, mean, std, shape in segs:
            dt = torch.float64 if kind in _F64_KINDS else torch.float32
            out = torch.empty((self.B,) + shape, dtype=dt, device=self.device)
            if self.side is not None:
                out.record_stream(self.side)
            outs.append(out)
            call.append((kind, count, mean, std, out))
        tables = self._normal_tables() if any(k == _lib.MT_SEGMENT_NORMAL32 for k, *_ in segs) else (None, None, None)
        self._enter()
        pieces = self.pieces_for(words)
        polys = self._chain_polys(words, pieces)
        self._batch_call(call, polys, pieces, tables)
        _, ev = self._drawn(words, None)
        return outs, ev

    def scratch_bytes(self, spec) -> int:
        """Scratch one draws_async(spec) call takes of the generator's context, sequential or in pieces (the larger)."""
        _, words = self._segments(spec)
        r = lambda b: (b + 255) // 256 * 256  # noqa: E731  (the allocator's rounding)
        seq = r(self.B * (words + 3 * 624) * 4) + r(max(self.B, 16) * 4)
        pieces = self.pieces_for(words)
        nblocks = -(-words // 624)
        chunked = r(self.B * (nblocks + 1) * 624 * 4) + r(self.B * pieces * 624 * 4) if pieces > 0 else 0
        return max(seq, chunked)

    def reserve(self, *specs):
        """Reserve the generator context's scratch for the largest of these per-frame calls up front, so that no frame allocates
        device memory (synchronises the generator's stream)."""
        need = max(self.scratch_bytes(s) for s in specs)
        self.ctx.check(self.ctx.lib.midas_scratch_reserve(self.ctx.h, need))
        return self

    # ---- draws whose sizes stand in device memory, a count per stream ------------------------------------------------
    def _counted_items(self, spec):
        items = TorchCpuStream._counted_items(spec)
        for _, _, _, cnt, idx, _, _ in items:
            if cnt.dim() != 2 or cnt.shape[0] != self.B or not 0 <= idx < cnt.shape[1]:
                raise _lib.MidasError(f"a counted draw of {self.B} streams takes stream b's size from [b, index] of a ({self.B}, stride) int32 tensor")
        return items

    def counted_scratch_bytes(self, spec) -> int:
        """Scratch one draws_counted_async(spec) call takes of the generator's context: B x TorchCpuStream's at the same bounds."""
        words = 3 * 624
        for kind, _, _, _, _, per, bound in self._counted_items(spec):
            words += counted_segment_words(kind, per, bound)
        r = lambda b: (b + 255) // 256 * 256  # noqa: E731  (the allocator's rounding)
        return r(4 * words * self.B) + r(8 * 17 * self.B)

    def draws_counted_async(self, spec, outs=None, status=None):
        """TorchCpuStream.draws_counted_async for every stream by ONE call (midas_mt19937_draws_counted_batch), with its spec:
        ("rand64", count_tensor, index, bound) and ("normal", mean, std, count_tensor, index, per, bound) - here count_tensor is
        (B, stride) int32 and stream b draws per x count_tensor[b, index] values, as that element stands when the kernels run (B
        control blocks of a BatchLoopEngine).  Returns ([tensors], event or None): (B, per x bound) tensors, row b's first
        per x count values hold stream b's draw, the rest is left as it was; `outs` gives the tensors to write into (contiguous,
        B x per x bound values each).  Stream b is, number for number, TorchCpuStream.draws_counted_async on it alone: a count of 0
        consumes nothing, a count beyond its bound or a normal draw of 1 .. 15 values draws nothing OF THAT STREAM and sets
        _lib.MT_STATUS_* bits in its status word - `status` = (int32 device tensor, index of stream 0's word, elements between two
        streams' words), by default the streams' own B words, which counted_status() reads.  Always the sequential walk."""
        import ctypes as C
        items = self._counted_items(spec)
        if not 1 <= len(items) <= 8:
            raise _lib.MidasError("1 .. 8 draws a call")
        if len({it[3].shape[1] for it in items}) != 1:
            raise _lib.MidasError("the count tensors of one call share their row stride")
        if status is None:
            if getattr(self, "_status", None) is None:
                self._status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            status = (self._status, 0, 1)
        st_t, st_i, st_stride = status[0], int(status[1]), int(status[2])
        if (st_t.dtype != torch.int32 or not st_t.is_contiguous() or st_stride < 1 or st_i < 0
                or st_i + (self.B - 1) * st_stride >= st_t.numel()):
            raise _lib.MidasError(f"`status` wants {self.B} words of a contiguous int32 device tensor")
        outs = [None] * len(items) if outs is None else list(outs)
        arr = (_lib.MtCountedSegment * len(items))()
        need_tables = False
        for i, (a, (kind, mean, std, cnt, idx, per, bound)) in enumerate(zip(arr, items)):
            dt = torch.float64 if kind in _F64_KINDS else torch.float32
            if outs[i] is None:
                outs[i] = torch.empty((self.B, per * bound), dtype=dt, device=self.device)
                if self.side is not None:
                    outs[i].record_stream(self.side)
            elif outs[i].dtype != dt or outs[i].numel() != self.B * per * bound or not outs[i].is_contiguous() or outs[i].device != self.device:
                raise _lib.MidasError(f"draw {i}: `outs` wants a contiguous device tensor of {self.B} x {per * bound} values of the draw's type")
            need_tables |= kind == _lib.MT_SEGMENT_NORMAL32
            a.kind, a.per, a.count_dev, a.bound, a.mean, a.std = kind, per, cnt.data_ptr() + 4 * idx, bound, mean, std
            a.out_dev = outs[i].data_ptr()
        R, Ct, S = self._normal_tables() if need_tables else (None, None, None)
        self._enter()
        self._call("midas_mt19937_draws_counted_batch", self.B, _ptr(self.state), self.pending_skip, len(items), C.cast(arr, C.c_void_p),
                   int(items[0][3].shape[1]), _ptr(R), _ptr(Ct), _ptr(S), C.c_void_p(st_t.data_ptr() + 4 * st_i), st_stride)
        _, ev = self._drawn(0, None)  # (no history: the next call walks sequentially)
        return outs, ev

    def counted_status(self):
        """The _lib.MT_STATUS_* bits draws_counted_async calls have set in the streams' own status words: B ints (one read-back)."""
        st = getattr(self, "_status", None)
        return [0] * self.B if st is None else [int(v) for v in st.cpu()]
