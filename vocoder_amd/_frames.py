"""What the Python owners of a layered module's stream and pool share (csrc/frame_pool.h; ``fv_wnstream`` / ``fv_cnxstream``, ``fv_wnpool``
/ ``fv_cnxpool``): a module whose output frame needs the ``R`` input frames after it emits ``[E, max(E, N - R))`` per push and ``[E, N)`` at
the flush.  ``schedule`` is that rule for one utterance, ``FramePoolCounters`` per session; ``_FrameStream`` owns rows that advance in
lockstep, ``_FramePool`` sessions that advance independently.  A subclass names its library entries (``_prefix``) and itself (``_noun``), says
where its engine's handle and channel counts are (``_attach``) and, when a call takes more than one output tensor, how many (``_slots``,
``_count``) and what it returns for them (``_wrap``)."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._handle import _Handle, _pool_items, _pool_moved
from ._lib import check
from .sample_pool import SamplePoolCounters

_MSG_INFERENCE = "{} is inference-only: call .eval() first"
_MSG_DEVICE = ("{} needs a CUDA/HIP tensor (got {}); vocoder_amd has no CPU path — move the model and "
               "input to the GPU")


def schedule(chunks, R: int) -> list:
    """The frames a stream of reach ``R`` emits: ``(E, E')`` for every push of ``chunks`` (frame counts, zeros allowed) — the push emits the
    frames ``[E, E')``, ``E' = max(E, N - R)`` — and last ``(E, N)`` for the flush."""
    out, N, E = [], 0, 0
    for c in chunks:
        N += int(c)
        E2 = max(E, N - int(R))
        out.append((E, E2))
        E = E2
    out.append((E, N))
    return out


class FramePoolCounters(SamplePoolCounters):
    """The host counters of a layer pool and the plan of ``fv_wnpool_plan`` / ``fv_cnxpool_plan`` in plain Python: ``schedule``'s rule per
    session.  An item ``(session, frames, flush)`` takes its slot to ``N' = N + frames`` and ``E' = N' if flush else max(E, N' - R)`` and emits
    ``[E, E')``; ``plan(items)`` gives ``E' - E`` per item and refuses what the library refuses (``SamplePoolCounters``), counting frames."""
    _unit, _chunk_limit, _chunk_limit_name, _length_limit, _length_limit_name = "frames", 1 << 20, "2^20", 1 << 30, "2^30"

    def __init__(self, reach: int, sessions: int, max_chunk: int):
        super().__init__(sessions, max_chunk)
        self.R = int(reach)
        self.max_frames = self.max_chunk + self.R        # a flush with max_chunk frames after R pending ones

    def _emission(self, i: int, s: int, c: int, flush: bool, N2: int, E: int) -> int:
        return N2 if flush else max(E, N2 - self.R)

    def pending(self, session: int) -> int:
        return self.received[session] - self.emitted[session]


class _FrameHandle(_Handle):
    """The handle of a stream or pool (``_kind``) on its module's engine; it dies with that engine."""
    _prefix = ""                      # "fv_wnstream": the library's entries are _prefix + "_create", "_push", ...
    _noun = ""                        # "posterior stream": what the messages call it
    _kind = ""
    _entries: tuple = ()
    _slots = 1                        # output pointers in the library's call
    _out_names = ""                   # what the refusal of a pool's `out` calls more than one tensor

    def __init__(self, module, engine, rows: int, max_chunk_frames: int):
        self._lib, self._h = _lib.lib(), ctypes.c_void_p()
        self._module, self._engine = module, engine
        self._entry = {name: getattr(self._lib, f"{self._prefix}_{name}") for name in self._entries}
        handle, self.in_channels, self.out_channels = self._attach(module, engine)
        with torch.cuda.device(engine.device):
            check(getattr(self._lib, self._prefix + "_create")(handle, int(rows), int(max_chunk_frames), ctypes.byref(self._h)))
        engine._streams.add(self)
        self.max_chunk_frames = int(max_chunk_frames)
        self._last_stream = None

    @property
    def _destroy(self) -> str:
        return self._prefix + "_destroy"

    @property
    def _closed(self) -> str:
        return (f"this {self._noun} is closed (its engine was closed or rebuilt — e.g. load_state_dict or .to() on "
                f"the module): create a new {self._kind}")

    def _attach(self, module, engine) -> tuple:
        """(the engine's library handle, in_channels, out_channels)"""
        raise NotImplementedError

    def _count(self) -> int:
        """Output tensors one call takes."""
        return 1

    def _wrap(self, outs, mask_shape: tuple):
        """What a call returns for its output tensors (a stream's, or one item's views)."""
        return outs[0]

    def _enqueue(self, call, outs) -> None:
        """``call(output pointers, stream) -> fv_status`` on torch's current stream, ordered after the previous call."""
        dev = self._engine.device
        ptrs = [t.data_ptr() if t.numel() else None for t in outs] + [None] * (self._slots - len(outs))
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            if self._done is not None and self._last_stream != cur.cuda_stream:
                cur.wait_event(self._done)       # the rings are the handle's own: order after the previous call when it ran on another stream
            check(call(ptrs, int(cur.cuda_stream)))
            self._record_done(cur)
            self._last_stream = cur.cuda_stream


class _FrameStream(_FrameHandle):
    """A layered module chunk by chunk: ``push`` a ``(B, in_channels, c)`` chunk, ``c <= max_chunk_frames``, and get the frames that need no
    later input, possibly none; ``flush`` ends the utterance and returns the rest, then pushes raise until ``reset()``.  The ``batch`` rows
    advance in lockstep."""
    _kind = "stream"
    _entries = ("push", "flush", "reset", "pending", "lookahead")

    def __init__(self, module, engine, batch: int, max_chunk_frames: int):
        super().__init__(module, engine, batch, max_chunk_frames)
        self.batch = int(batch)
        self._R = int(self._entry["lookahead"](self._h))
        self._N = self._E = 0
        self._flushed = False

    # -- counters (host-side: reading them never synchronises) --
    @property
    def received_frames(self) -> int:
        return self._N

    @property
    def emitted_frames(self) -> int:
        return self._E

    @property
    def pending_frames(self) -> int:
        """Frames received and not yet emitted, as the library counts them (``*_pending``)."""
        self._check_open()
        return int(self._entry["pending"](self._h))

    @property
    def lookahead_frames(self) -> int:
        return self._R

    def schedule(self, chunks) -> list:
        return schedule(chunks, self._R)

    def plan(self, c: int, flush: bool = False) -> int:
        """Frames the next ``push`` of ``c`` frames (or the ``flush``) emits: host arithmetic, nothing moves."""
        return self._N - self._E if flush else max(self._E, self._N + int(c) - self._R) - self._E

    def push(self, x: torch.Tensor):
        self._check_open()
        what = f"{type(self).__name__}.push"
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError(_MSG_DEVICE.format(what, getattr(x, "device", type(x))))
        if x.dim() != 3 or x.shape[0] != self.batch or x.shape[1] != self.in_channels:
            raise ValueError(f"{what}: expected ({self.batch}, {self.in_channels}, c), got {tuple(x.shape)}")
        x = x.detach().to(torch.float32)
        c = int(x.shape[2])
        # a slice along T passes as it is (the strides of *_push)
        if c and not _strides_pass(x):
            x = x.contiguous()
        return self._call(x, c, flush=False)

    def flush(self):
        """The frames ``[E, N)`` against the utterance's end; pushes raise afterwards until ``reset()``."""
        self._check_open()
        return self._call(None, 0, flush=True)

    def _call(self, x, c: int, flush: bool):
        m, dev = self._module, self._engine.device
        if m.training:
            raise RuntimeError(_MSG_INFERENCE.format(type(m).__name__))
        if x is not None and x.device != dev:
            raise RuntimeError(f"{type(self).__name__}.push: the chunk is on {x.device}, the stream on {dev}")
        refused = self._flushed or c > self.max_chunk_frames      # a refused call emits nothing; the library says why
        k = 0 if refused else self.plan(c, flush)
        outs = [torch.empty((self.batch, self.out_channels, k), dtype=torch.float32, device=dev) for _ in range(self._count())]
        got = ctypes.c_int64(0)
        if flush:
            self._enqueue(lambda ptrs, run: self._entry["flush"](self._h, *ptrs, max(k, 1), ctypes.byref(got), run), outs)
        else:
            self._enqueue(lambda ptrs, run: self._entry["push"](self._h, x.data_ptr() if c else None, x.stride(0) if c else 0,
                                                                x.stride(1) if c else 0, c, *ptrs, max(k, 1), ctypes.byref(got), run), outs)
        if got.value != k:
            raise RuntimeError(f"{self._noun} emitted {got.value} frames where the rule says {k}")
        self._N += c
        self._E += k
        self._flushed = flush
        return self._wrap(outs, (self.batch, 1, k))

    def reset(self) -> None:
        """Start the next utterance: N = E = 0; the rings are kept (nothing they hold is read again)."""
        self._check_open()
        check(self._entry["reset"](self._h))
        self._N = self._E = 0
        self._flushed = False


def _strides_pass(x: torch.Tensor) -> bool:
    """Does ``(rows, channels, c)`` pass as it is: frames next to each other, channels at least a chunk apart, rows not backwards?"""
    return (x.shape[2] == 1 or x.stride(2) == 1) and x.stride(1) >= x.shape[2] and x.stride(0) >= 0


class _FramePool(_FrameHandle):
    """A layered module for sessions that advance independently: what ``_FrameStream`` is to rows in lockstep, for ``sessions`` slots with
    their own counters.  ``step(items)`` takes ``(session, x, flush)`` tuples — ``x``: ``(in_channels, n)`` with ``n <= max_chunk_frames``, or
    ``None`` for no frames; ``flush``: the utterance ends with these frames — and returns per item the frames that session emits in this
    step, possibly none.  A session appears at most once per step and refuses items after its flush until ``reset(session)``.  The whole
    step is checked before anything moves: a refused step leaves every session as it was.  Work is enqueued on torch's current stream and
    calls must be ordered."""
    _kind = "pool"
    _entries = ("step", "reset", "pending", "launches", "lookahead", "max_frames")

    def __init__(self, module, engine, sessions: int, max_chunk_frames: int):
        super().__init__(module, engine, sessions, max_chunk_frames)
        self.sessions = int(sessions)
        self.lookahead_frames = int(self._entry["lookahead"](self._h))
        self.max_frames = int(self._entry["max_frames"](self._h))
        self.counters = FramePoolCounters(self.lookahead_frames, self.sessions, self.max_chunk_frames)

    # -- counters (host-side: reading them never synchronises) --
    def received_frames(self, session: int) -> int:
        return self.counters.received[session]

    def emitted_frames(self, session: int) -> int:
        return self.counters.emitted[session]

    def pending_frames(self, session: int) -> int:
        """Frames one session has received and not yet emitted, as the library counts them (``*_pending``)."""
        self._check_open()
        return int(self._entry["pending"](self._h, int(session)))

    @property
    def last_step_launches(self) -> int:
        """The kernel launches the last accepted step enqueued (``*_launches``)."""
        self._check_open()
        return int(self._entry["launches"](self._h))

    def plan_frames(self, items) -> list:
        """Frames every ``(session, frames, flush)`` item would emit; refuses what ``step_padded`` would, and nothing moves."""
        return self.counters.plan(items)

    def step(self, items) -> list:
        """One step for ``items`` (see the class); returns each item's tensors, views of the step's output buffers."""
        self._check_open()
        what = f"{type(self).__name__}.step"
        meta, rows = [], []
        for it in map(tuple, items):
            s, x, flush = it[0], it[1], it[2] if len(it) > 2 else False
            if x is not None:
                if not isinstance(x, torch.Tensor) or not x.is_cuda:
                    raise RuntimeError(_MSG_DEVICE.format(what, getattr(x, "device", type(x))))
                if x.dim() != 2 or x.shape[0] != self.in_channels:
                    raise ValueError(f"{what}: expected ({self.in_channels}, n) or None, got {tuple(x.shape)}")
            rows.append(x)
            meta.append((int(s), 0 if x is None else int(x.shape[1]), bool(flush)))
        longest = max((c for _, c, _ in meta), default=0)
        chunks = None
        if longest:
            chunks = torch.zeros((len(meta), self.in_channels, longest), dtype=torch.float32, device=self._engine.device)
            for i, x in enumerate(rows):
                if x is not None and x.shape[1]:
                    chunks[i, :, :x.shape[1]] = x
        out, emit = self.step_padded(meta, chunks)
        outs = out if isinstance(out, tuple) else (out,)
        return [self._wrap([t[i, :, :k] for t in outs], (1, k)) for i, k in enumerate(emit)]

    def step_padded(self, items, chunks: "torch.Tensor | None", out=None) -> tuple:
        """The step on the caller's padded buffers, as ``*_step`` takes them: ``items``: ``(session, frames, flush)`` integers; ``chunks``:
        ``(count, in_channels, stride)`` with item i's frames first in row i (the rest, NaN included, is never read) — the output of
        ``WavPool.step_padded`` passes as it is — or ``None`` when no item has frames; ``out``: one contiguous ``(count, out_channels,
        out_cols)`` tensor per output of a call (a tuple where a call has several), sized from the Python plan when not given.  Returns
        ``(out, frames emitted per item)``: row i holds item i's frames first and zeros after them."""
        self._check_open()
        m, dev, what = self._module, self._engine.device, f"{type(self).__name__}.step_padded"
        if m.training:
            raise RuntimeError(_MSG_INFERENCE.format(type(m).__name__))
        items, arr, got = _pool_items(items)
        count, xptr, istride, rstride = len(items), None, 0, 0
        if chunks is not None:
            if not isinstance(chunks, torch.Tensor) or not chunks.is_cuda:
                raise RuntimeError(_MSG_DEVICE.format(what, getattr(chunks, "device", type(chunks))))
            if chunks.device != dev:
                raise RuntimeError(f"{what}: the chunks are on {chunks.device}, the pool on {dev}")
            if chunks.dim() != 3 or chunks.shape[0] != count or chunks.shape[1] != self.in_channels or chunks.dtype != torch.float32:
                raise ValueError(f"{what}: expected float32 chunks of shape ({count}, {self.in_channels}, stride), got {tuple(chunks.shape)}")
            if chunks.numel() and not _strides_pass(chunks):
                chunks = chunks.contiguous()
            if chunks.numel():
                xptr, istride, rstride = chunks.data_ptr(), int(chunks.stride(0)), int(chunks.stride(1))
        plan = self.counters.plan(items)                          # sizes the output before anything is launched; refuses what the library would
        n = self._count()
        if out is None:
            outs = tuple(torch.empty((count, self.out_channels, max(plan, default=0)), dtype=torch.float32, device=dev) for _ in range(n))
        else:
            outs = tuple(out) if n > 1 else (out,)
            ok = len(outs) == n and all(
                isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.dim() == 3 and t.shape[:2] == (count, self.out_channels)
                and t.shape == outs[0].shape and t.is_contiguous() for t in outs)
            if not ok:
                raise ValueError(f"{what}: expected out as {self._out_names + ', each ' if n > 1 else ''}a contiguous float32 tensor of shape "
                                 f"({count}, {self.out_channels}, out_cols) on {dev}")
        cols = int(outs[0].shape[2])
        self._enqueue(lambda ptrs, run: self._entry["step"](self._h, arr, count, xptr, istride, rstride, *ptrs, cols, got, run), outs)
        emit = _pool_moved(self.counters, items, plan, got, "the " + self._noun + " emitted {emit} frames where the rule says {plan}")
        return (outs if n > 1 else outs[0]), emit

    def reset(self, session: int) -> None:
        """Start the next utterance in one slot: its counters go to 0; its ring rows are kept (nothing they hold is read again)."""
        self._check_open()
        check(self._entry["reset"](self._h, int(session)))
        self.counters.reset(int(session))
