"""Sample-rate conversion on the GPU (include/fishvoc.h ``fv_resample_*``): the filter design and the streaming rule in plain Python, and the
drop-in module.

The reference resamples on the CPU in both of its audio front doors — ``librosa.load(..., sr=cfg.model.sampling_rate)`` (test.py:54) and
``torchaudio.functional.resample`` (data/transforms/hq_pitch_shift.py:33).  ``Resample`` takes the keyword arguments of
``torchaudio.transforms.Resample`` and computes the same polyphase windowed-sinc filter (restated; torchaudio is not a dependency)::

    g = gcd(orig_freq, new_freq);  o = orig_freq / g;  n = new_freq / g
    base = min(o, n) * rolloff;    width = ceil(lpw * o / base)
    t = clamp(((j - width) / o - p / n) * base, -lpw, +lpw)            phase p in [0, n), tap j in [0, 2 width + o)
    h[p][j] = (t == 0 ? 1 : sin(pi t) / (pi t)) * win(t) * base / o
    y[f n + p] = sum_j h[p][j] xp[f o + j]                             xp: x behind `width` zeros; ceil(n L / o) outputs are kept

Only the band ``|t| < lpw`` of a phase is not zero: phase ``p`` keeps the taps ``[first[p], first[p] + count[p])``, ``count[p] <= kp``.  Output
``m = f n + p`` therefore reads the input samples ``first_input(m) + i``, ``i < count[p]``, ``first_input(m) = f o + first[p] - width``.

Streaming rule (``ResampleStream``): after ``N`` input samples have arrived, every output whose band ends at or before ``N`` has been emitted —
``emit_count(N) = #{m : first_input(m) + count[p(m)] <= N}``; the flush emits the rest up to ``ceil(n N / o)`` against zeros.  The latency is
the band's half width (about ``lpw * o / base`` input samples), and the concatenated outputs are bit-identical to the whole-row forward.

Sessions that advance independently (``ResamplePool``, ``fv_respool_*``): the same rule per slot, push and flush folded into one item
``(session, samples, end)`` — ``N' = N + samples``, ``E' = output_length(N') if end else max(E, emit_count(N'))`` — stated in plain Python by
``ResamplePoolCounters``.
"""
from __future__ import annotations

import bisect
import ctypes
import math
from dataclasses import dataclass
from functools import cached_property

import numpy as np
import torch
from torch import nn

from . import _lib
from ._handle import _DeviceHandles, _Handle, _SamplePoolHandle, _emit, _require_value as _require_cuda
from ._lib import check
from .sample_pool import SamplePoolCounters

KAISER_BETA = 14.769656459379492


def _i0(x: np.ndarray) -> np.ndarray:
    """Modified Bessel function I0 by its power series (float64; the arguments stay below ~15)."""
    q = np.asarray(x, dtype=np.float64) ** 2 / 4
    term = np.ones_like(q)
    total = np.ones_like(q)
    for k in range(1, 500):
        term = term * q / (k * k)
        total = total + term
        if np.all(term < total * 1e-18):
            break
    return total


@dataclass(frozen=True)
class Design:
    """The filter of one rate pair: ``taps`` is ``(n, kp)`` float32 (float64 arithmetic, rounded once), zero past ``count[p]``."""
    orig_freq: int
    new_freq: int
    o: int
    n: int
    width: int
    kp: int
    first: tuple
    count: tuple
    taps: np.ndarray

    @cached_property
    def _end(self) -> list:
        """``first[p] + count[p]``: where every phase's band ends (non-decreasing)."""
        return [a + c for a, c in zip(self.first, self.count)]

    def output_length(self, L: int) -> int:
        return -((-self.n * int(L)) // self.o)

    def first_input(self, m: int) -> int:
        """Index of the first input sample that output ``m`` reads (negative near the row's start: zeros)."""
        f, p = divmod(int(m), self.n)
        return f * self.o + self.first[p] - self.width

    def emit_count(self, N: int) -> int:
        """Outputs emitted once ``N`` input samples have arrived: those whose band ends at or before ``N``."""
        end = self._end
        X = int(N) + self.width + 1                               # count the (f, p) with f o + end[p] < X
        if X <= end[0]:
            return 0
        full = -((end[-1] - X) // self.o) if X > end[-1] else 0   # frames whose every phase is below X
        total = full * self.n
        f = full
        while f * self.o + end[0] < X:
            total += bisect.bisect_left(end, X - f * self.o)
            f += 1
        return total

    def max_step_outputs(self, max_chunk: int) -> int:
        """The most one pool item emits in one step (``fv_respool_max_outputs``): a push of ``max_chunk`` samples that also flushes, from the
        state ``E = emit_count(N)`` with the most outputs pending.  ``g(N) = output_length(N + max_chunk) - emit_count(N)`` is largest just
        before ``emit_count`` jumps, and periodic in ``N`` with period ``o`` once every phase has emitted: the largest ``g`` just before the
        ``n`` jumps of frame 2."""
        c = int(max_chunk)
        return max(self.output_length(N + c) - self.emit_count(N) for N in (2 * self.o + e - self.width - 1 for e in self._end))


def design(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
           resampling_method: str = "sinc_interp_hann", beta: float | None = None) -> Design:
    """The filter design of ``fv_resample_design``, in numpy float64 (same expressions, so the same bands)."""
    orig_freq, new_freq, lpw = int(orig_freq), int(new_freq), int(lowpass_filter_width)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"orig_freq ({orig_freq}) and new_freq ({new_freq}) must be > 0")
    if lpw < 1:
        raise ValueError(f"lowpass_filter_width ({lpw}) must be >= 1")
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"rolloff ({rolloff}) must lie in (0, 1]")
    if resampling_method not in _lib.RESAMPLE_METHODS:
        raise ValueError(f"resampling_method {resampling_method!r} is not one of {sorted(_lib.RESAMPLE_METHODS)}")
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    base = min(o, n) * float(rolloff)
    width = int(math.ceil(lpw * o / base))
    half = lpw * o / base
    dense = 2 * width + o
    first, count, rows = [], [], []
    b = KAISER_BETA if beta is None or beta <= 0 else float(beta)
    for p in range(n):
        centre = width + p * o / n
        j = np.arange(max(0, math.floor(centre - half) - 2), min(dense - 1, math.ceil(centre + half) + 2) + 1, dtype=np.int64)
        t = ((j - width).astype(np.float64) / o - p / n) * base
        band = np.abs(t) < lpw
        j, t = j[band], np.clip(t[band], -lpw, lpw)
        if resampling_method == "sinc_interp_hann":
            win = np.cos(t * math.pi / lpw / 2) ** 2
        else:
            win = _i0(b * np.sqrt(np.maximum(0.0, 1 - (t / lpw) ** 2))) / _i0(np.float64(b))
        t = t * math.pi
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t))
        first.append(int(j[0]))
        count.append(len(j))
        rows.append((sinc * win * (base / o)).astype(np.float32))
    kp = max(count)
    taps = np.zeros((n, kp), dtype=np.float32)
    for p, r in enumerate(rows):
        taps[p, :len(r)] = r
    return Design(orig_freq, new_freq, o, n, width, kp, tuple(first), tuple(count), taps)


def native_design(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                  resampling_method: str | int = "sinc_interp_hann", beta: float | None = None) -> Design:
    """The same through ``fv_resample_design`` (pure host code in the library): what the kernel's table holds."""
    L = _lib.lib()
    cfg = _config(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
    o, n, width, kp = (ctypes.c_int32() for _ in range(4))
    check(L.fv_resample_design(ctypes.byref(cfg), ctypes.byref(o), ctypes.byref(n), ctypes.byref(width), ctypes.byref(kp), None, None, 0, None, 0))
    first = (ctypes.c_int32 * n.value)()
    count = (ctypes.c_int32 * n.value)()
    taps = np.zeros((n.value, kp.value), dtype=np.float32)
    check(L.fv_resample_design(ctypes.byref(cfg), ctypes.byref(o), ctypes.byref(n), ctypes.byref(width), ctypes.byref(kp), first, count, n.value,
                               taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), taps.size))
    return Design(int(orig_freq), int(new_freq), o.value, n.value, width.value, kp.value, tuple(first), tuple(count), taps)


def _config(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta) -> _lib.ResampleConfig:
    method = resampling_method if isinstance(resampling_method, int) else _lib.RESAMPLE_METHODS.get(resampling_method, -1)
    return _lib.ResampleConfig(int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff), int(method),
                               0.0 if beta is None else float(beta))


def _rows(x: torch.Tensor) -> torch.Tensor:
    """(..., L) -> a (rows, L) view whose samples are contiguous (a copy only when they are not)."""
    rows = 1
    for d in x.shape[:-1]:
        rows *= int(d)
    x2 = x.reshape(rows, x.shape[-1])      # (not -1: ambiguous for an empty chunk, (B, 0))
    if x2.shape[1] > 1 and x2.stride(1) != 1 or x2.shape[0] > 1 and x2.stride(0) < x2.shape[1]:
        x2 = x2.contiguous()
    return x2


class Resample(nn.Module):
    """Drop-in for ``torchaudio.transforms.Resample`` on the MI355X: ``forward(waveform (..., L)) -> (..., ceil(new_freq * L / orig_freq))``.

    ``lengths`` (a list or an int tensor, one entry per row of the flattened leading dimensions) makes the call ragged: row ``b`` holds
    ``lengths[b] <= L`` samples, its outputs are bit-identical to the row run alone and exact zeros follow them.  ``stream(batch, max_chunk)``
    gives the streaming form, ``pool(sessions, max_chunk)`` sessions that advance independently.  ``orig_freq == new_freq`` returns the
    input, as torchaudio does.

    ``table="lds"`` keeps the filter's table in LDS (``fv_resample_create``: rate pairs whose table fits, roughly ``n * kp <= 7000``);
    ``table="global"`` leaves it in global memory (``fv_global_resample_create``: any pair, e.g. 44101 -> 48000).  Where both exist their
    outputs agree bit for bit."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, resampling_method: str = "sinc_interp_hann",
                 lowpass_filter_width: int = 6, rolloff: float = 0.99, beta: float | None = None, table: str = "lds"):
        super().__init__()
        if table not in ("lds", "global"):
            raise ValueError(f"table {table!r} is neither 'lds' nor 'global'")
        self.table = table
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.resampling_method, self.lowpass_filter_width, self.rolloff, self.beta = resampling_method, int(lowpass_filter_width), rolloff, beta
        self.design = design(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
        self._handles = _DeviceHandles("fv_resample_destroy")     # fv_resample: the table lives on one device

    def output_length(self, L: int) -> int:
        return self.design.output_length(L)

    def emit_count(self, N: int) -> int:
        return self.design.emit_count(N)

    def first_input(self, m: int) -> int:
        return self.design.first_input(m)

    def _handle(self, device: torch.device) -> ctypes.c_void_p:
        def create(h) -> int:
            cfg = _config(self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff, self.resampling_method, self.beta)
            return getattr(_lib.lib(), "fv_global_resample_create" if self.table == "global" else "fv_resample_create")(ctypes.byref(cfg), h)
        return self._handles.get(device, create)

    def forward(self, waveform: torch.Tensor, lengths=None) -> torch.Tensor:
        _require_cuda(waveform, "Resample.forward")
        if waveform.dim() < 1:
            raise ValueError("Resample.forward: expected a waveform of shape (..., L)")
        if self.orig_freq == self.new_freq and lengths is None:
            return waveform
        L = int(waveform.shape[-1])
        x = _rows(waveform)
        B, M = int(x.shape[0]), self.output_length(L)
        lib = _lib.lib()
        h = self._handle(x.device)
        lptr = None
        if lengths is not None:
            if not (torch.is_tensor(lengths) and lengths.is_cuda):
                host = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
                if len(host) != B:
                    raise ValueError(f"Resample.forward: {len(host)} lengths for {B} rows")
                check(lib.fv_resample_check_lengths(h, (ctypes.c_int32 * B)(*host), B, L))
                lengths = torch.tensor(host, dtype=torch.int32, device=x.device)
            elif lengths.numel() != B:
                raise ValueError(f"Resample.forward: {lengths.numel()} lengths for {B} rows")
            lengths = lengths.to(device=x.device, dtype=torch.int32).contiguous()
            lptr = lengths.data_ptr()
        y = torch.empty((B, M), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            check(lib.fv_resample_forward(h, x.data_ptr(), x.stride(0) if B > 1 else max(L, 1), lptr, y.data_ptr(), max(M, 1), B, L,
                                          int(torch.cuda.current_stream().cuda_stream)))
        return y.reshape(*waveform.shape[:-1], M)

    def stream(self, batch: int, max_chunk: int) -> "ResampleStream":
        return ResampleStream(self, batch, max_chunk)

    def pool(self, sessions: int, max_chunk: int) -> "ResamplePool":
        return ResamplePool(self, sessions, max_chunk)

    def close(self) -> None:
        self._handles.close()

    def extra_repr(self) -> str:
        return (f"{self.orig_freq} -> {self.new_freq} Hz, {self.resampling_method}, lowpass_filter_width={self.lowpass_filter_width}, "
                f"rolloff={self.rolloff}, phases={self.design.n}, taps={self.design.kp}")


class ResampleStream(_Handle):
    """``batch`` rows resampled chunk by chunk, in lockstep (``fv_resample_stream``): ``push`` a ``(batch, c)`` chunk, ``c <= max_chunk``, and get
    the ``(batch, k)`` outputs whose bands have arrived (``k`` may be 0); ``flush`` emits the rest against zeros; ``reset`` starts the next
    utterance; ``close`` frees the stream (also a context manager).  Work is enqueued on torch's current stream; calls must be ordered."""
    _destroy = "fv_resample_stream_destroy"
    _closed = "this resample stream is closed: create a new one"

    def __init__(self, resample: Resample, batch: int, max_chunk: int, device=None):
        self._resample, self._lib = resample, _lib.lib()
        self.design = resample.design
        self.batch, self.max_chunk = int(batch), int(max_chunk)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(self._lib.fv_resample_stream_create(resample._handle(self.device), self.batch, self.max_chunk, ctypes.byref(self._h)))
        self._N = self._E = 0
        self._flushed = False

    # -- counters (host-side: reading them never synchronises) --
    @property
    def received_samples(self) -> int:
        return self._N

    @property
    def emitted_samples(self) -> int:
        return self._E

    @property
    def pending_samples(self) -> int:
        """``ceil(n N / o) - E`` as the library counts it (fv_resample_stream_pending): what a flush would emit now."""
        self._check_open()
        return int(self._lib.fv_resample_stream_pending(self._h))

    def push(self, chunk: torch.Tensor) -> torch.Tensor:
        self._check_open()
        _require_cuda(chunk, "ResampleStream.push")
        if chunk.dim() != 2 or chunk.shape[0] != self.batch:
            raise ValueError(f"expected a chunk of shape ({self.batch}, c), got {tuple(chunk.shape)}")
        return self._call(_rows(chunk), int(chunk.shape[1]), flush=False)

    def flush(self) -> torch.Tensor:
        self._check_open()
        return self._call(None, 0, flush=True)

    def _call(self, x, c: int, flush: bool) -> torch.Tensor:
        N2 = self._N + c
        ok = flush or c <= self.max_chunk                   # a refused push emits nothing; the library says why
        E2 = self.design.output_length(N2) if flush else max(self._E, self.design.emit_count(N2))
        k = E2 - self._E if ok and not self._flushed else 0

        def enqueue(optr, got) -> None:
            with torch.cuda.device(self.device):
                run = torch.cuda.current_stream()
                s = int(run.cuda_stream)
                check(self._lib.fv_resample_stream_flush(self._h, optr, max(k, 1), got, s) if flush else
                      self._lib.fv_resample_stream_push(self._h, x.data_ptr(), x.stride(0) if self.batch > 1 else max(c, 1), c, optr,
                                                        max(k, 1), got, s))
                self._record_done(run)      # the carried buffers are in use on the device until then
        out = _emit((self.batch, k), k, self.device, enqueue, "resample stream emitted {got} samples where the emission rule says {k}")
        self._N, self._E = N2, E2
        self._flushed = flush
        return out

    def reset(self) -> None:
        self._check_open()
        check(self._lib.fv_resample_stream_reset(self._h))
        self._N = self._E = 0
        self._flushed = False


class ResamplePoolCounters(SamplePoolCounters):
    """The host counters of a resample pool (``SamplePoolCounters``) and the plan of ``fv_respool_plan`` in plain Python over
    ``Design.emit_count`` / ``output_length``: ``E' = max(E, output_length(N') if flush else emit_count(N'))``."""

    def __init__(self, design: Design, sessions: int, max_chunk: int):
        super().__init__(sessions, max_chunk)
        self.design = design
        self.max_outputs = design.max_step_outputs(self.max_chunk)

    def _emission(self, i: int, s: int, c: int, flush: bool, N2: int, E: int) -> int:
        return max(E, self.design.output_length(N2) if flush else self.design.emit_count(N2))

    def pending(self, session: int) -> int:
        return self.design.output_length(self.received[session]) - self.emitted[session]


class ResamplePool(_SamplePoolHandle):
    """Resampler sessions that advance independently (``fv_respool``, include/fishvoc.h): what ``ResampleStream`` is to rows in lockstep, for
    ``sessions`` slots with their own counters.  ``step(items)`` takes ``(session, samples, end)`` tuples — ``samples``: a 1-D tensor of at
    most ``max_chunk`` samples, or ``None`` for none; ``end``: the utterance ends with them — and returns one 1-D tensor per item (possibly
    empty): the outputs whose bands have arrived, or with ``end`` all that remain, against zeros.  A session appears at most once per step and
    refuses items after its end until ``reset(session)``.  The whole step is checked before anything moves: a refused step leaves every
    session as it was.  A session's concatenated outputs are bit-identical to ``Resample.forward`` of its whole utterance.  One step is one
    FIR launch and one carry launch per 32 items; work is enqueued on torch's current stream, and calls must be ordered."""
    _destroy, _prefix = "fv_respool_destroy", "fv_respool"
    _closed = "this resample pool is closed: create a new one"
    _mismatch = "the resample pool emitted {emit} outputs where the emission rule says {plan}"

    def __init__(self, resample: Resample, sessions: int, max_chunk: int, device=None):
        super().__init__(resample, sessions, max_chunk, device)
        self.design = resample.design
        self.counters = ResamplePoolCounters(self.design, self.sessions, self.max_chunk)

    def step(self, items) -> list:
        """One step for ``items`` (see the class); returns each item's outputs, views of one output buffer."""
        out, emit = self.step_padded(*self._gather(items))
        return [out[i, :k] for i, k in enumerate(emit)]

    def step_padded(self, items, chunks: torch.Tensor | None, out: torch.Tensor | None = None) -> tuple:
        """The step on the caller's padded buffers, as ``fv_respool_step`` takes them: ``items``: ``(session, samples, end)`` integers;
        ``chunks``: ``(rows >= count, chunk_stride)`` with item i's samples first in row i (the rest, NaN included, is never read), ``None``
        when no item has samples; ``out``: ``(count, out_cols)``, sized from the Python plan when not given.  Returns ``(out, outputs per
        item)``: row i holds item i's outputs first and zeros after them."""
        items, arr, got, cptr, stride = self._padded(items, chunks)
        count = len(items)
        plan = self.counters.plan(items)                          # sizes the output before anything is launched; refuses what the library would
        out = self._out(out, (count,), max(plan, default=0), f"({count}, out_cols)")
        cols = int(out.shape[1])
        self._run(lambda stream: self._lib.fv_respool_step(self._h, arr, count, cptr, stride, out.data_ptr() if out.numel() else None,
                                                           max(cols, 1), cols, got, stream))
        return out, self._moved(items, plan, got)
