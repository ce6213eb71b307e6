"""Pitch shift on the GPU (include/fishvoc.h ``fv_pitch_shift_*``): the plan and the lengths in plain Python, and the drop-in module.

The reference's inference script shifts every file on the CPU between loading and the mel front-end —
``librosa.effects.pitch_shift(gt_y, sr=sr, n_steps=cfg.pitch_shift)`` (test.py:61-62).  librosa is not a dependency; its arithmetic is
restated: a phase-vocoder time stretch by ``rate = 2^(-n_steps / bins_per_octave)``, then a resample from ``sr / rate`` back to ``sr``, fixed
to the input length.  What differs from librosa is stated in integers::

    orig_freq = floor(sr * 2^(n_steps / bpo) + 0.5);  orig_freq -= orig_freq % freq_granularity      (hq_pitch_shift.py:30-31)
    g = gcd(orig_freq, sr);  o = orig_freq / g;  n = sr / g                                            the rate is exactly n / o
    T  = 1 + L / hop                                         analysis frames (centred, zero padding)
    T' = ceil(T o / n)                                       stretched frames: frame s sits at j = s n / o, alpha = (s n % o) / o
    Ls = (2 L o + n) / (2 n)                                 stretched samples, round(L o / n) with halves up
    M  = ceil(n Ls / o)                                      resampled samples, cut or zero-padded to L

The phase accumulator is an unsigned 32-bit count of turns / 2^32: it wraps where librosa's float grows, so a long file keeps its phase
(an fp32 accumulator is off by 0.12 of peak after 200 000 samples).  ``orig_freq == sr`` returns the input.

Streaming rule (``PitchShiftStream``, ``fv_pv_stream_*``), with ``F = n_fft``, ``h = hop_length`` and ``N`` samples received per row::

    A = 0 if N < F / 2 else (N - F / 2) / h + 1              analysis frames that read no sample at or after N
    S = 0 if A < 2 else ceil((A - 1) o / n)                  stretched frames whose columns j = s n / o and j + 1 are analysed
    Y = min(max(0, S h - F / 2), (2 N o + n) / (2 n))        stretched samples under which every covering frame exists
    E = min(emit_count(Y), N)                                the resampler's stream (orig_freq -> sr) after Y samples

The flush emits the rest, ``E = N``.  With ``batch_invariant=True`` the concatenated chunks are bit-identical to ``forward`` over whole rows.
``PitchShiftPool`` (``fv_pvpool_*``) applies the same rule per session: ``E' = N'`` with the flush, else ``max(E, E(N'))``.
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn

from . import _lib
from ._handle import _DeviceHandles, _Handle, _SamplePoolHandle, _emit
from ._lib import check
from .resample import KAISER_BETA, _require_cuda, _rows, design
from .sample_pool import SamplePoolCounters

MAX_UTTERANCE = 1 << 30                      # samples per utterance of a stream or a pool slot (the library's limit)

KAISER_BEST_ROLLOFF = 0.9475937167399596     # torchaudio's documented equivalent of librosa's kaiser_best, with width 64 and KAISER_BETA


def plan(sample_rate: int, n_steps: float, bins_per_octave: int = 12, freq_granularity: int = 100) -> tuple[int, int, int]:
    """``(orig_freq, o, n)`` as ``fv_pitch_shift_plan`` computes them."""
    sample_rate, bins_per_octave, freq_granularity = int(sample_rate), int(bins_per_octave), int(freq_granularity)
    if sample_rate <= 0:
        raise ValueError(f"sample_rate ({sample_rate}) must be > 0")
    if not math.isfinite(n_steps):
        raise ValueError(f"n_steps ({n_steps}) must be finite")
    if bins_per_octave < 1:
        raise ValueError(f"bins_per_octave ({bins_per_octave}) must be >= 1")
    if freq_granularity < 1:
        raise ValueError(f"freq_granularity ({freq_granularity}) must be >= 1")
    f = math.floor(sample_rate * 2.0 ** (float(n_steps) / bins_per_octave) + 0.5)
    if not 1 <= f <= 2 ** 31 - 1:
        raise ValueError(f"n_steps ({n_steps}) moves {sample_rate} Hz to {f} Hz, outside [1, 2^31)")
    orig_freq = f - f % freq_granularity
    if orig_freq < 1:
        raise ValueError(f"n_steps ({n_steps}) with freq_granularity ({freq_granularity}) leaves orig_freq = 0")
    g = math.gcd(orig_freq, sample_rate)
    return orig_freq, orig_freq // g, sample_rate // g


def lengths(L: int, o: int, n: int, hop_length: int) -> tuple[int, int, int, int]:
    """``(T, T', Ls, M)`` for ``L`` input samples, as ``fv_pitch_shift_lengths`` computes them."""
    L = int(L)
    T = 1 + L // hop_length
    Tout = -((-T * o) // n)
    Ls = (2 * L * o + n) // (2 * n)
    M = -((-n * Ls) // o)
    return T, Tout, Ls, M


def stream_ready(N: int, o: int, n: int, n_fft: int, hop_length: int) -> tuple[int, int, int]:
    """``(A, S, Y)`` once ``N`` samples have arrived, as ``fv_pv_stream_ready`` computes them."""
    N, F, h = int(N), int(n_fft), int(hop_length)
    A = 0 if N < F // 2 else (N - F // 2) // h + 1
    S = 0 if A < 2 else -((-(A - 1) * o) // n)
    Y = min(max(0, S * h - F // 2), (2 * N * o + n) // (2 * n))
    return A, S, Y


class PitchShift(nn.Module):
    """``librosa.effects.pitch_shift(y, sr=sample_rate, n_steps=n_steps)`` on the MI355X (test.py:61-62): ``forward(wave (..., L)) -> (..., L)``.
    Leading dimensions are flattened to rows (a stereo file is two rows, test.py:56-64).  ``time_stretch(wave)`` is the first stage alone,
    ``(..., Ls)``.  ``stream(batch, max_chunk)`` gives the streaming form.  ``batch_invariant=True`` runs the two DFT convs as fixed-order sums
    whatever the launch size (``fv_pv_set_batch_invariant``): the mode in which whole rows and any chunking of a stream agree bit for bit.
    No CPU fallback."""

    def __init__(self, sample_rate: int, n_steps: float, bins_per_octave: int = 12, n_fft: int = 2048, hop_length: int | None = None,
                 freq_granularity: int = 100, lowpass_filter_width: int = 64, rolloff: float = KAISER_BEST_ROLLOFF,
                 resampling_method: str = "sinc_interp_kaiser", beta: float | None = None, batch_invariant: bool = False):
        super().__init__()
        self.sample_rate, self.n_steps, self.bins_per_octave = int(sample_rate), float(n_steps), int(bins_per_octave)
        self.n_fft, self.hop_length = int(n_fft), int(n_fft) // 4 if hop_length is None else int(hop_length)
        self.freq_granularity, self.lowpass_filter_width, self.rolloff = int(freq_granularity), int(lowpass_filter_width), float(rolloff)
        self.resampling_method, self.beta, self.batch_invariant = resampling_method, beta, bool(batch_invariant)
        self._design = None
        self.orig_freq, self.o, self.n = plan(self.sample_rate, self.n_steps, self.bins_per_octave, self.freq_granularity)
        if self.n_fft < 2 or self.hop_length < 1 or self.n_fft % self.hop_length or self.n_fft % 2 or self.hop_length % 2:
            raise ValueError(f"n_fft ({self.n_fft}) must be a multiple of hop_length ({self.hop_length}) and both even")
        self._handles = _DeviceHandles("fv_pitch_shift_destroy")     # fv_pitch_shift: its tables live on one device

    def plan(self) -> tuple[int, int, int]:
        return self.orig_freq, self.o, self.n

    def lengths(self, L: int) -> tuple[int, int, int, int]:
        return lengths(L, self.o, self.n, self.hop_length)

    def config(self) -> _lib.PitchShiftConfig:
        method = self.resampling_method if isinstance(self.resampling_method, int) else _lib.RESAMPLE_METHODS.get(self.resampling_method, -1)
        return _lib.PitchShiftConfig(self.sample_rate, self.n_steps, self.bins_per_octave, self.n_fft, self.hop_length, self.freq_granularity,
                                     self.lowpass_filter_width, self.rolloff, int(method), KAISER_BETA if self.beta is None else float(self.beta))

    def _handle(self, device: torch.device) -> ctypes.c_void_p:
        def create(h) -> int:
            lib = _lib.lib()
            st = lib.fv_pitch_shift_create(ctypes.byref(self.config()), h)
            return st or lib.fv_pv_set_batch_invariant(h._obj, int(self.batch_invariant))
        return self._handles.get(device, create)

    def resample_design(self):
        """The filter of the second stage, ``orig_freq -> sample_rate`` (``vocoder_amd.resample.design``): the stream's emission rule counts with it."""
        if self._design is None:
            self._design = design(self.orig_freq, self.sample_rate, self.lowpass_filter_width, self.rolloff, self.resampling_method, self.beta)
        return self._design

    def stream_ready(self, N: int) -> tuple[int, int, int]:
        return stream_ready(N, self.o, self.n, self.n_fft, self.hop_length)

    def stream_emitted(self, N: int) -> int:
        """Outputs a stream has emitted once ``N`` samples have arrived (before the flush)."""
        if self.orig_freq == self.sample_rate:
            return int(N)
        return min(self.resample_design().emit_count(self.stream_ready(N)[2]), int(N))

    def stream(self, batch: int, max_chunk: int) -> "PitchShiftStream":
        return PitchShiftStream(self, batch, max_chunk)

    def pool(self, sessions: int, max_chunk: int) -> "PitchShiftPool":
        return PitchShiftPool(self, sessions, max_chunk)

    def _run(self, wave: torch.Tensor, whole: bool, what: str) -> torch.Tensor:
        _require_cuda(wave, what)
        if wave.dim() < 1:
            raise ValueError(f"{what}: expected a waveform of shape (..., L)")
        if self.orig_freq == self.sample_rate:
            return wave
        L = int(wave.shape[-1])
        x = _rows(wave)
        B = int(x.shape[0])
        out = L if whole else self.lengths(L)[2]
        lib = _lib.lib()
        h = self._handle(x.device)
        y = torch.empty((B, out), dtype=torch.float32, device=x.device)
        need = int(lib.fv_pitch_shift_workspace_bytes(h, B, L))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
        fn = lib.fv_pitch_shift_forward if whole else lib.fv_pitch_shift_stretch
        with torch.cuda.device(x.device):
            check(fn(h, x.data_ptr(), x.stride(0) if B > 1 else max(L, 1), y.data_ptr(), max(out, 1), B, L, ws.data_ptr(), need,
                     int(torch.cuda.current_stream().cuda_stream)))
        return y.reshape(*wave.shape[:-1], out)

    def forward(self, wave: torch.Tensor) -> torch.Tensor:
        return self._run(wave, True, "PitchShift.forward")

    def time_stretch(self, wave: torch.Tensor) -> torch.Tensor:
        return self._run(wave, False, "PitchShift.time_stretch")

    def close(self) -> None:
        self._handles.close()

    def extra_repr(self) -> str:
        return (f"{self.sample_rate} Hz, n_steps={self.n_steps}, orig_freq={self.orig_freq} (rate {self.n}/{self.o}), n_fft={self.n_fft}, "
                f"hop_length={self.hop_length}")


class PitchShiftStream(_Handle):
    """``batch`` rows shifted chunk by chunk, in lockstep (``fv_pv_stream``): ``push`` a ``(batch, c)`` chunk, ``c <= max_chunk``, and get the
    ``(batch, k)`` outputs that no later sample can change (``k`` may be 0); ``flush`` emits the rest, so that as many samples have come out as
    went in; ``reset`` starts the next utterance; ``close`` frees the stream (also a context manager).  Work is enqueued on torch's current
    stream; calls must be ordered."""
    _destroy = "fv_pv_stream_destroy"
    _closed = "this pitch-shift stream is closed: create a new one"

    def __init__(self, shift: PitchShift, batch: int, max_chunk: int, device=None):
        self._shift, self._lib = shift, _lib.lib()
        self.batch, self.max_chunk = int(batch), int(max_chunk)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(self._lib.fv_pv_stream_create(shift._handle(self.device), self.batch, self.max_chunk, ctypes.byref(self._h)))
            self._need = int(self._lib.fv_pv_stream_workspace_bytes(self._h))
            self._ws = torch.empty(max(self._need, 1), dtype=torch.uint8, device=self.device)
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
        """``N - E`` as the library counts it (fv_pv_stream_pending): what a flush would emit now."""
        self._check_open()
        return int(self._lib.fv_pv_stream_pending(self._h))

    def push(self, chunk: torch.Tensor) -> torch.Tensor:
        self._check_open()
        _require_cuda(chunk, "PitchShiftStream.push")
        if chunk.dim() != 2 or chunk.shape[0] != self.batch:
            raise ValueError(f"expected a chunk of shape ({self.batch}, c), got {tuple(chunk.shape)}")
        return self._call(_rows(chunk), int(chunk.shape[1]), flush=False)

    def flush(self) -> torch.Tensor:
        self._check_open()
        return self._call(None, 0, flush=True)

    def _call(self, x, c: int, flush: bool, workspace_bytes: int | None = None) -> torch.Tensor:
        N2 = self._N + c
        ok = flush or c <= self.max_chunk                   # a refused push emits nothing; the library says why
        E2 = N2 if flush else max(self._E, self._shift.stream_emitted(N2))
        k = E2 - self._E if ok and not self._flushed else 0
        need = self._need if workspace_bytes is None else int(workspace_bytes)

        def enqueue(optr, got) -> None:
            with torch.cuda.device(self.device):
                run = torch.cuda.current_stream()
                s = int(run.cuda_stream)
                check(self._lib.fv_pv_stream_flush(self._h, optr, max(k, 1), got, self._ws.data_ptr(), need, s) if flush else
                      self._lib.fv_pv_stream_push(self._h, x.data_ptr(), x.stride(0) if self.batch > 1 else max(c, 1), c, optr, max(k, 1), got,
                                                  self._ws.data_ptr(), need, s))
                self._record_done(run)      # the carried buffers and the workspace are in use on the device until then
        out = _emit((self.batch, k), k, self.device, enqueue, "pitch-shift stream emitted {got} samples where the emission rule says {k}")
        self._N, self._E = N2, E2
        self._flushed = flush
        return out

    def reset(self) -> None:
        self._check_open()
        check(self._lib.fv_pv_stream_reset(self._h))
        self._N = self._E = 0
        self._flushed = False


class PvPoolCounters(SamplePoolCounters):
    """The host counters of a pitch-shift pool (``SamplePoolCounters``) and the plan of ``fv_pvpool_plan`` in plain Python over
    ``PitchShift.stream_emitted``: ``E' = N'`` with the flush, else ``max(E, E(N'))``; the identity shift emits the item's own samples.  Beyond
    the shared refusals, ``ValueError`` past 2^30 samples in one utterance."""

    def __init__(self, shift: PitchShift, sessions: int, max_chunk: int):
        super().__init__(sessions, max_chunk)
        self.shift = shift
        self.max_outputs = self._max_outputs()

    def _max_outputs(self) -> int:
        """``fv_pvpool_max_outputs``: ``max_chunk`` plus the largest ``N - E(N)``, which stands just before a step of ``A(N)`` and has period
        ``n`` in the frame index past the start-up (the derivation: include/fishvoc.h)."""
        sh = self.shift
        if sh.orig_freq == sh.sample_rate:
            return self.max_chunk
        F, h, o, n = sh.n_fft, sh.hop_length, sh.o, sh.n
        need = 4 * o + 2 * sh.resample_design().kp
        a0 = (-((-(need + F) * n) // o) + 2 * F + 2 * h) // h + 2
        while sh.stream_ready(F // 2 + a0 * h - 1)[2] < need:
            a0 += n
        return self.max_chunk + max(N - sh.stream_emitted(N) for N in (F // 2 + a * h - 1 for a in range(a0, a0 + n)))

    def _emission(self, i: int, s: int, c: int, flush: bool, N2: int, E: int) -> int:
        if N2 > MAX_UTTERANCE:
            raise ValueError(f"item {i} takes session {s} past 2^30 samples in one utterance")
        if self.shift.orig_freq == self.shift.sample_rate:
            return E + c
        return N2 if flush else max(E, self.shift.stream_emitted(N2))

    def pending(self, session: int) -> int:
        return self.received[session] - self.emitted[session]


class PitchShiftPool(_SamplePoolHandle):
    """Pitch-shift sessions that advance independently (``fv_pvpool``, include/fishvoc.h): what ``PitchShiftStream`` is to rows in lockstep,
    for ``sessions`` slots with their own counters, all with the shifter's one ``n_steps``.  ``step(items)`` takes ``(session, samples, end)``
    tuples — ``samples``: a 1-D tensor of at most ``max_chunk`` samples, or ``None`` for none; ``end``: the utterance ends with them — and
    returns one 1-D tensor per item (possibly empty): the shifted samples that no later sample can change, or with ``end`` all that remain,
    so that as many samples have come out as went in.  A session appears at most once per step and refuses items after its end until
    ``reset(session)``.  The whole step is checked before anything moves: a refused step leaves every session as it was.  With
    ``batch_invariant=True`` on the shifter a session's concatenated outputs are bit-identical to ``PitchShift.forward`` of its whole
    utterance.  Work is enqueued on torch's current stream, and calls must be ordered."""
    _destroy, _prefix = "fv_pvpool_destroy", "fv_pvpool"
    _closed = "this pitch-shift pool is closed: create a new one"
    _mismatch = "the pitch-shift pool emitted {emit} outputs where the emission rule says {plan}"

    def __init__(self, shift: PitchShift, sessions: int, max_chunk: int, device=None):
        super().__init__(shift, sessions, max_chunk, device)
        with torch.cuda.device(self.device):
            self._need = int(self._lib.fv_pvpool_workspace_bytes(self._h))
            self._ws = torch.empty(max(self._need, 1), dtype=torch.uint8, device=self.device)
        self.counters = PvPoolCounters(shift, self.sessions, self.max_chunk)

    def step(self, items) -> list:
        """One step for ``items`` (see the class); returns each item's outputs, views of one output buffer."""
        out, emit = self.step_padded(*self._gather(items))
        return [out[i, :k] for i, k in enumerate(emit)]

    def step_padded(self, items, chunks: torch.Tensor | None, out: torch.Tensor | None = None, workspace_bytes: int | None = None) -> tuple:
        """The step on the caller's padded buffers, as ``fv_pvpool_step`` takes them: ``items``: ``(session, samples, end)`` integers;
        ``chunks``: ``(rows >= count, chunk_stride)`` with item i's samples first in row i (the rest, NaN included, is never read), ``None``
        when no item has samples; ``out``: ``(count, out_cols)``, sized from the Python plan when not given.  Returns ``(out, outputs per
        item)``: row i holds item i's outputs first and zeros after them."""
        items, arr, got, cptr, stride = self._padded(items, chunks)
        count = len(items)
        plan = self.counters.plan(items)                          # sizes the output before anything is launched; refuses what the library would
        out = self._out(out, (count,), max(plan, default=0), f"({count}, out_cols)")
        cols = int(out.shape[1])
        need = self._need if workspace_bytes is None else int(workspace_bytes)
        self._run(lambda stream: self._lib.fv_pvpool_step(self._h, arr, count, cptr, stride, out.data_ptr() if out.numel() else None,
                                                          max(cols, 1), cols, got, self._ws.data_ptr(), need, stream))
        return out, self._moved(items, plan, got)
