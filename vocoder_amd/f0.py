"""F0 tracking and pitch templates on the GPU (include/fishvoc.h ``fv_f0_*`` / ``fv_template_*``): the plan in plain Python and the drop-in
modules.

``RefineGANGenerator.forward(mel, template)`` (refinegan.py:287) and the ``use_template=True`` generators (hifigan.py:226) take a pitch
``template (B, 1, T * hop)`` next to the mel.  The reference does not make one; its users track F0 on the CPU (pyworld, parselmouth,
``librosa.yin``) and write their own oscillator.  Here both steps run on the device, on the samples the mel is made from::

    tau_max = sr // fmin;  tau_min = max(2, sr // fmax);  Wi = W - (tau_max + 1);  T = L // hop
    frame t: the W samples centred on t hop + hop // 2 (zeros outside the row)
    d(tau)  = sum_{j < Wi} (x[j] - x[j + tau])^2                   tau = 1 ... tau_max + 1, direct form
    d'(tau) = d(tau) tau / sum_{k <= tau} d(k)                     1 where the running sum is 0
    voiced: the smallest tau in [tau_min, tau_max] with d' < threshold, d'(tau) <= d'(tau - 1), d'(tau) < d'(tau + 1);
            f0 = sr / (tau + parabolic offset), aperiodicity = d'(tau); otherwise f0 = 0, aperiodicity = min d'
    F_t = rint(f0_t / sr * 2^32) as uint32;  inc[n] = (F_a (hop - k) + F_b k) // hop between the frame centres a, a + 1
    phi[n] = sum_{m <= n} inc[m] mod 2^32;  template = amplitude sin(2 pi phi / 2^32), exactly 0 in unvoiced frames

The phase is an unsigned 32-bit count of turns / 2^32, as the pitch shift's accumulator is (``pitch_shift.py``): it wraps where a float grows,
so a long file keeps its pitch.  No CPU fallback.

Streaming (``fv_yin_stream_*`` / ``fv_osc_stream_*``): ``YinF0.stream`` takes samples chunk by chunk and emits frame ``t`` once none of its
samples is at or after the ``N`` received, ``frames_ready(N)``; ``PitchTemplate.stream`` takes F0 frames and emits the ``hop`` samples of frame
``t`` once frame ``t + 1`` has arrived; ``TemplateStream`` is the first into the second.  Concatenated, every stream's output has the bits of
the whole-row call.

Pools (``fv_yinpool_*`` / ``fv_oscpool_*``): ``YinF0.pool``, ``PitchTemplate.pool`` and ``TemplatePool`` are the same three for sessions that
advance independently — any subset steps, each with its own chunk size, each ending at its own step — with every count planned on the host
(``YinPoolCounters``, ``OscPoolCounters``).  Per session the bits are again those of the whole-row call.
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn

from . import _lib
from ._handle import _DeviceHandles, _Handle, _SamplePoolHandle, _emit, _gather
from ._lib import check
from .resample import _require_cuda, _rows
from .sample_pool import SamplePoolCounters

MAX_FRAME_LENGTH = 4096      # one workgroup stages the frame in LDS (fv_f0_create)


def plan(sample_rate: int, frame_length: int = 2048, hop_length: int = 512, fmin: float = 40.0, fmax: float = 1100.0,
         threshold: float = 0.1) -> tuple[int, int, int]:
    """``(tau_min, tau_max, Wi)`` as ``fv_f0_plan`` computes them; ValueError says which knob to move."""
    sample_rate, frame_length, hop_length = int(sample_rate), int(frame_length), int(hop_length)
    fmin, fmax, threshold = float(fmin), float(fmax), float(threshold)
    if sample_rate <= 0:
        raise ValueError(f"sample_rate ({sample_rate}) must be > 0")
    if hop_length < 1:
        raise ValueError(f"hop_length ({hop_length}) must be >= 1")
    if frame_length < 2 or frame_length % 2:
        raise ValueError(f"frame_length ({frame_length}) must be even and >= 2")
    if not (0.0 < fmin < float("inf") and 0.0 < fmax < float("inf")):
        raise ValueError(f"fmin ({fmin}) and fmax ({fmax}) must be positive and finite")
    if not 0.0 < threshold <= 1.0:
        raise ValueError(f"threshold ({threshold}) must lie in (0, 1]")
    tau_max, tau_min = math.floor(sample_rate / fmin), max(2, math.floor(sample_rate / fmax))      # (floors of the double quotients, as in C)
    if tau_max > 1 << 24:
        raise ValueError(f"fmin ({fmin}) gives a longest lag of {tau_max} samples; raise fmin")
    Wi = frame_length - (tau_max + 1)
    if tau_min >= tau_max:
        raise ValueError(f"fmin ({fmin}) and fmax ({fmax}) at {sample_rate} Hz give lags [{tau_min}, {tau_max}]: no lag to search; lower fmin "
                         "or raise fmax")
    if 2 * Wi < tau_max:
        raise ValueError(f"frame_length ({frame_length}) leaves an integration window of {Wi} samples, less than half the longest lag "
                         f"({tau_max}, from fmin = {fmin}); raise frame_length or fmin")
    return tau_min, tau_max, Wi


def frames_ready(N: int, frame_length: int, hop_length: int) -> int:
    """Frames of the tracker that read no sample at or after ``N`` (``fv_yin_frames_ready``): frame ``t`` reads
    ``[t hop + hop // 2 - W // 2, ... + W)``; never above ``N // hop``."""
    N, W, hop = int(N), int(frame_length), int(hop_length)
    need = hop // 2 + W // 2
    return 0 if N < need else min(1 + (N - need) // hop, N // hop)


def _host_counts(counts, rows: int, what: str):
    host = [int(v) for v in (counts.tolist() if torch.is_tensor(counts) else counts)]
    if len(host) != rows:
        raise ValueError(f"{what}: {len(host)} entries for {rows} rows")
    return host, (ctypes.c_int32 * max(rows, 1))(*host)


class YinF0(nn.Module):
    """YIN on the MI355X: ``forward(wave (..., L)) -> (f0 (..., T), aperiodicity (..., T))`` with ``T = L // hop_length``, one value per mel
    frame; ``f0`` is 0 in unvoiced frames.  ``forward_ragged(wave (B, Lmax), lengths)``: row ``b`` holds ``lengths[b]`` samples (the rest is
    never loaded), its values are bit-identical to the row run alone and exact zeros follow them."""

    def __init__(self, sample_rate: int, hop_length: int, frame_length: int = 2048, fmin: float = 40.0, fmax: float = 1100.0,
                 threshold: float = 0.1):
        super().__init__()
        self.sample_rate, self.hop_length, self.frame_length = int(sample_rate), int(hop_length), int(frame_length)
        self.fmin, self.fmax, self.threshold = float(fmin), float(fmax), float(threshold)
        self.tau_min, self.tau_max, self.window = plan(self.sample_rate, self.frame_length, self.hop_length, self.fmin, self.fmax, self.threshold)
        if self.frame_length > MAX_FRAME_LENGTH:
            raise ValueError(f"frame_length ({self.frame_length}) is above {MAX_FRAME_LENGTH}, what one workgroup stages in LDS")
        self._handles = _DeviceHandles("fv_f0_destroy")

    def plan(self) -> tuple[int, int, int]:
        return self.tau_min, self.tau_max, self.window

    def frames(self, L: int) -> int:
        return int(L) // self.hop_length

    def config(self) -> _lib.F0Config:
        return _lib.F0Config(self.sample_rate, self.frame_length, self.hop_length, self.fmin, self.fmax, self.threshold)

    def _handle(self, device: torch.device) -> ctypes.c_void_p:
        return self._handles.get(device, lambda h: _lib.lib().fv_f0_create(ctypes.byref(self.config()), h))

    def _run(self, wave: torch.Tensor, lengths, what: str):
        _require_cuda(wave, what)
        if wave.dim() < 1:
            raise ValueError(f"{what}: expected a waveform of shape (..., L)")
        L = int(wave.shape[-1])
        x = _rows(wave)
        B, T = int(x.shape[0]), self.frames(L)
        lptr = None if lengths is None else _host_counts(lengths, B, what)[1]
        lib = _lib.lib()
        h = self._handle(x.device)
        out = torch.empty((2, B, T), dtype=torch.float32, device=x.device)
        need = int(lib.fv_f0_workspace_bytes(h, B, L))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            check(lib.fv_f0_forward(h, x.data_ptr(), x.stride(0) if B > 1 else max(L, 1), lptr, out[0].data_ptr(), out[1].data_ptr(), max(T, 1),
                                    B, L, ws.data_ptr(), need, int(torch.cuda.current_stream().cuda_stream)))
        return out[0].reshape(*wave.shape[:-1], T), out[1].reshape(*wave.shape[:-1], T)

    def forward(self, wave: torch.Tensor):
        return self._run(wave, None, "YinF0.forward")

    def forward_ragged(self, wave: torch.Tensor, lengths):
        if wave.dim() != 2:
            raise ValueError("YinF0.forward_ragged: expected a waveform of shape (B, Lmax)")
        return self._run(wave, lengths, "YinF0.forward_ragged")

    def stream(self, batch: int, max_chunk_samples: int) -> "YinF0Stream":
        return YinF0Stream(self, batch, max_chunk_samples)

    def pool(self, sessions: int, max_chunk_samples: int) -> "YinF0Pool":
        return YinF0Pool(self, sessions, max_chunk_samples)

    def close(self) -> None:
        self._handles.close()

    def extra_repr(self) -> str:
        return (f"{self.sample_rate} Hz, hop_length={self.hop_length}, frame_length={self.frame_length}, lags [{self.tau_min}, {self.tau_max}], "
                f"window={self.window}, threshold={self.threshold}")


class PitchTemplate(nn.Module):
    """The exact-phase oscillator: ``forward(f0 (..., T)) -> (..., 1, T * hop_length)``, what ``forward(mel, template)`` takes.  ``f0`` in Hz,
    0 (or negative, NaN, >= sample_rate) in unvoiced frames, where the template is exactly 0.  ``forward_ragged(f0 (B, Tmax), frames)``: row
    ``b`` holds ``frames[b]`` frames; its samples are bit-identical to the row run alone and exact zeros follow them."""

    def __init__(self, sample_rate: int, hop_length: int, kind: str = "sine", amplitude: float = 1.0):
        super().__init__()
        self.sample_rate, self.hop_length, self.kind, self.amplitude = int(sample_rate), int(hop_length), kind, float(amplitude)
        if kind not in _lib.TEMPLATE_KINDS:
            raise ValueError(f"kind ({kind!r}) must be one of {sorted(_lib.TEMPLATE_KINDS)}")
        if self.sample_rate <= 0 or not 1 <= self.hop_length <= 1 << 20:
            raise ValueError(f"sample_rate ({self.sample_rate}) must be > 0 and hop_length ({self.hop_length}) in [1, 2^20]")
        self._handles = _DeviceHandles("fv_template_destroy")

    def config(self) -> _lib.TemplateConfig:
        return _lib.TemplateConfig(self.sample_rate, self.hop_length, _lib.TEMPLATE_KINDS[self.kind], self.amplitude)

    def _handle(self, device: torch.device) -> ctypes.c_void_p:
        return self._handles.get(device, lambda h: _lib.lib().fv_template_create(ctypes.byref(self.config()), h))

    def _run(self, f0: torch.Tensor, frames, what: str) -> torch.Tensor:
        _require_cuda(f0, what)
        if f0.dim() < 1:
            raise ValueError(f"{what}: expected f0 of shape (..., T)")
        T = int(f0.shape[-1])
        x = _rows(f0)
        B, N = int(x.shape[0]), T * self.hop_length
        fptr = None if frames is None else _host_counts(frames, B, what)[1]
        lib = _lib.lib()
        h = self._handle(x.device)
        out = torch.empty((B, N), dtype=torch.float32, device=x.device)
        need = int(lib.fv_template_workspace_bytes(h, B, T))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            check(lib.fv_template_forward(h, x.data_ptr(), x.stride(0) if B > 1 else max(T, 1), fptr, out.data_ptr(), max(N, 1), B, T,
                                          ws.data_ptr(), need, int(torch.cuda.current_stream().cuda_stream)))
        return out.reshape(*f0.shape[:-1], 1, N)

    def forward(self, f0: torch.Tensor) -> torch.Tensor:
        return self._run(f0, None, "PitchTemplate.forward")

    def forward_ragged(self, f0: torch.Tensor, frames) -> torch.Tensor:
        if f0.dim() != 2:
            raise ValueError("PitchTemplate.forward_ragged: expected f0 of shape (B, Tmax)")
        return self._run(f0, frames, "PitchTemplate.forward_ragged")

    def stream(self, batch: int, max_chunk_frames: int) -> "PitchTemplateStream":
        return PitchTemplateStream(self, batch, max_chunk_frames)

    def pool(self, sessions: int, max_chunk_frames: int) -> "PitchTemplatePool":
        return PitchTemplatePool(self, sessions, max_chunk_frames)

    def close(self) -> None:
        self._handles.close()

    def extra_repr(self) -> str:
        return f"{self.sample_rate} Hz, hop_length={self.hop_length}, kind={self.kind!r}, amplitude={self.amplitude}"


def template_from_audio(wave: torch.Tensor, sample_rate: int, hop_length: int, frame_length: int = 2048, fmin: float = 40.0,
                        fmax: float = 1100.0, threshold: float = 0.1, kind: str = "sine", amplitude: float = 1.0) -> torch.Tensor:
    """``wave (..., L) -> template (..., 1, (L // hop_length) * hop_length)``: ``YinF0`` then ``PitchTemplate`` on the same samples the mel is
    made from."""
    f0, _ = YinF0(sample_rate, hop_length, frame_length, fmin, fmax, threshold)(wave)
    return PitchTemplate(sample_rate, hop_length, kind, amplitude)(f0)


class _F0Stream(_Handle):
    """What the two streams share: the handle's creation on one device, the chunk check, the host counters ``_N`` received / ``_E`` emitted."""
    _create = ""

    def __init__(self, parent, batch: int, max_chunk: int, device=None):
        self._parent, self._lib = parent, _lib.lib()
        self.batch, self.max_chunk = int(batch), int(max_chunk)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(getattr(self._lib, self._create)(parent._handle(self.device), self.batch, self.max_chunk, ctypes.byref(self._h)))
        self._N = self._E = 0
        self._flushed = False

    def _chunk(self, chunk: torch.Tensor, what: str) -> torch.Tensor:
        self._check_open()
        _require_cuda(chunk, what)
        if chunk.dim() != 2 or chunk.shape[0] != self.batch:
            raise ValueError(f"{what}: expected a chunk of shape ({self.batch}, c), got {tuple(chunk.shape)}")
        return _rows(chunk)

    def _moved(self, N2: int, E2: int, flush: bool) -> None:
        self._N, self._E = N2, E2
        self._flushed = self._flushed or flush


class YinF0Stream(_F0Stream):
    """``batch`` rows tracked chunk by chunk, in lockstep (``fv_yin_stream``): ``push`` a ``(batch, c)`` chunk of samples,
    ``c <= max_chunk_samples``, and get ``(f0 (batch, k), aperiodicity (batch, k))`` for the frames that read no later sample (``k`` may be 0);
    ``flush`` emits the rest against the rows' true end and then refuses pushes until ``reset``; ``close`` frees the stream (also a context
    manager).  A frame leaves ``W / 2 + hop / 2 - hop`` samples after its own hop has arrived.  The concatenated values have the bits of
    ``YinF0.forward`` on the whole rows.  Work is enqueued on torch's current stream; calls must be ordered."""
    _destroy, _create = "fv_yin_stream_destroy", "fv_yin_stream_create"
    _closed = "this F0 stream is closed: create a new one"

    def __init__(self, yin: YinF0, batch: int, max_chunk_samples: int, device=None):
        super().__init__(yin, batch, max_chunk_samples, device)
        self.frame_length, self.hop_length = yin.frame_length, yin.hop_length

    # -- counters (host-side: reading them never synchronises) --
    @property
    def received_samples(self) -> int:
        return self._N

    @property
    def emitted_frames(self) -> int:
        return self._E

    @property
    def pending_samples(self) -> int:
        """``N - max(0, E hop + hop // 2 - W // 2)`` as the library counts it (fv_yin_stream_pending_samples)."""
        self._check_open()
        return int(self._lib.fv_yin_stream_pending_samples(self._h))

    def push(self, chunk: torch.Tensor):
        return self._call(self._chunk(chunk, "YinF0Stream.push"), int(chunk.shape[1]), flush=False)

    def flush(self):
        self._check_open()
        return self._call(None, 0, flush=True)

    def _call(self, x, c: int, flush: bool):
        N2 = self._N + c
        ok = flush or c <= self.max_chunk                   # a refused push emits nothing; the library says why
        E2 = N2 // self.hop_length if flush else max(self._E, frames_ready(N2, self.frame_length, self.hop_length))
        k = E2 - self._E if ok and not self._flushed else 0

        def enqueue(optr, got) -> None:
            aptr = None if optr is None else optr + 4 * self.batch * k
            with torch.cuda.device(self.device):
                run = torch.cuda.current_stream()
                s = int(run.cuda_stream)
                check(self._lib.fv_yin_stream_flush(self._h, optr, aptr, max(k, 1), got, s) if flush else
                      self._lib.fv_yin_stream_push(self._h, x.data_ptr(), x.stride(0) if self.batch > 1 else max(c, 1), c, optr, aptr,
                                                   max(k, 1), got, s))
                self._record_done(run)      # the carried buffers are in use on the device until then
        out = _emit((2, self.batch, k), k, self.device, enqueue, "F0 stream emitted {got} frames where the emission rule says {k}")
        self._moved(N2, E2, flush)
        return out[0], out[1]

    def reset(self) -> None:
        self._check_open()
        check(self._lib.fv_yin_stream_reset(self._h))
        self._N = self._E = 0
        self._flushed = False


class PitchTemplateStream(_F0Stream):
    """``batch`` rows of the oscillator chunk by chunk, in lockstep (``fv_osc_stream``): ``push`` a ``(batch, c)`` chunk of F0 frames,
    ``c <= max_chunk_frames``, and get the ``(batch, 1, k hop)`` samples of the frames whose next frame has arrived (``k`` may be 0); ``flush``
    emits the last frame and then refuses pushes until ``reset``.  Latency: one F0 frame.  The concatenated samples have the bits of
    ``PitchTemplate.forward`` on the whole rows: the phase carried between calls is a wrapping integer."""
    _destroy, _create = "fv_osc_stream_destroy", "fv_osc_stream_create"
    _closed = "this pitch template stream is closed: create a new one"

    def __init__(self, template: PitchTemplate, batch: int, max_chunk_frames: int, device=None):
        super().__init__(template, batch, max_chunk_frames, device)
        self.hop_length = template.hop_length

    @property
    def received_frames(self) -> int:
        return self._N

    @property
    def emitted_frames(self) -> int:
        return self._E

    @property
    def pending_frames(self) -> int:
        """``Tn - E`` as the library counts it (fv_osc_stream_pending_frames)."""
        self._check_open()
        return int(self._lib.fv_osc_stream_pending_frames(self._h))

    def push(self, f0: torch.Tensor) -> torch.Tensor:
        return self._call(self._chunk(f0, "PitchTemplateStream.push"), int(f0.shape[1]), flush=False)

    def flush(self) -> torch.Tensor:
        self._check_open()
        return self._call(None, 0, flush=True)

    def _call(self, x, c: int, flush: bool) -> torch.Tensor:
        T2 = self._N + c
        ok = flush or c <= self.max_chunk
        E2 = T2 if flush else max(self._E, T2 - 1)
        k = (E2 - self._E) * self.hop_length if ok and not self._flushed else 0

        def enqueue(optr, got) -> None:
            with torch.cuda.device(self.device):
                run = torch.cuda.current_stream()
                s = int(run.cuda_stream)
                check(self._lib.fv_osc_stream_flush(self._h, optr, max(k, 1), got, s) if flush else
                      self._lib.fv_osc_stream_push(self._h, x.data_ptr(), x.stride(0) if self.batch > 1 else max(c, 1), c, optr, max(k, 1), got, s))
                self._record_done(run)
        out = _emit((self.batch, 1, k), k, self.device, enqueue, "pitch template stream emitted {got} samples where the emission rule says {k}")
        self._moved(T2, E2, flush)
        return out

    def reset(self) -> None:
        self._check_open()
        check(self._lib.fv_osc_stream_reset(self._h))
        self._N = self._E = 0
        self._flushed = False


class TemplateStream:
    """Audio in, template samples out: a ``YinF0Stream`` into a ``PitchTemplateStream``.  ``push((batch, c))``, ``c <= max_chunk_samples``,
    returns the ``(batch, 1, k hop)`` template samples that are final; ``flush()`` flushes both, tracker first; concatenated they have the
    bits of ``template_from_audio`` on the whole rows.  Latency: the tracker's ``W / 2 + hop / 2 - hop`` samples plus one frame."""

    def __init__(self, sample_rate: int, hop_length: int, batch: int, max_chunk_samples: int, frame_length: int = 2048, fmin: float = 40.0,
                 fmax: float = 1100.0, threshold: float = 0.1, kind: str = "sine", amplitude: float = 1.0):
        self.yin = YinF0(sample_rate, hop_length, frame_length, fmin, fmax, threshold)
        self.oscillator = PitchTemplate(sample_rate, hop_length, kind, amplitude)
        self.batch, self.max_chunk_samples, self.hop_length = int(batch), int(max_chunk_samples), int(hop_length)
        # the most frames the tracker emits at once: c // hop + 1 from a push, the frames still waiting for lookahead from the flush
        self.max_chunk_frames = max(self.max_chunk_samples, self.yin.frame_length // 2 + self.hop_length // 2) // self.hop_length + 1
        self.tracker = self.yin.stream(batch, max_chunk_samples)
        try:
            self.template = self.oscillator.stream(batch, self.max_chunk_frames)
        except Exception:
            self.tracker.close()
            raise

    @property
    def received_samples(self) -> int:
        return self.tracker.received_samples

    @property
    def emitted_samples(self) -> int:
        return self.template.emitted_frames * self.hop_length

    def push(self, chunk: torch.Tensor) -> torch.Tensor:
        return self.template.push(self.tracker.push(chunk)[0])

    def flush(self) -> torch.Tensor:
        head = self.template.push(self.tracker.flush()[0])
        return torch.cat([head, self.template.flush()], dim=-1)

    def reset(self) -> None:
        self.tracker.reset()
        self.template.reset()

    def close(self) -> None:
        self.tracker.close()
        self.template.close()
        self.yin.close()
        self.oscillator.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()


# ---------------------------------------------------------------------------------------------
# Pools: sessions that advance independently (fv_yinpool_* / fv_oscpool_*), what the streams above are to rows in lockstep
# ---------------------------------------------------------------------------------------------
class YinPoolCounters(SamplePoolCounters):
    """The tracker pool's rule: ``N' = N + samples``, ``E' = N' // hop`` with flush, else ``max(E, frames_ready(N'))``."""

    def __init__(self, frame_length: int, hop_length: int, sessions: int, max_chunk: int):
        super().__init__(sessions, max_chunk)
        self.frame_length, self.hop_length = int(frame_length), int(hop_length)
        W, hop = self.frame_length, self.hop_length
        # a push of max_chunk samples that also flushes, from E = frames_ready(N); periodic in N from hop // 2 + W // 2 on (fv_yinpool_max_frames)
        self.max_frames = max((N + self.max_chunk) // hop - frames_ready(N, W, hop) for N in range(hop // 2 + W // 2 + 2 * hop))

    def _emission(self, i: int, s: int, c: int, flush: bool, N2: int, E: int) -> int:
        return max(E, N2 // self.hop_length if flush else frames_ready(N2, self.frame_length, self.hop_length))

    def pending(self, session: int) -> int:
        N, E, W, hop = self.received[session], self.emitted[session], self.frame_length, self.hop_length
        return max(0, N - max(0, E * hop + hop // 2 - W // 2))


class OscPoolCounters(SamplePoolCounters):
    """The oscillator pool's rule, counted in F0 frames: ``Tn' = Tn + frames``, ``E' = Tn'`` with flush, else ``max(E, Tn' - 1)``."""

    def __init__(self, sessions: int, max_chunk_frames: int):
        super().__init__(sessions, max_chunk_frames)
        self.max_frames = self.max_chunk + 1      # a push of max_chunk frames that also flushes while one frame waits

    def _emission(self, i: int, s: int, c: int, flush: bool, T2: int, E: int) -> int:
        return max(E, T2 if flush else T2 - 1)

    def pending(self, session: int) -> int:
        return self.received[session] - self.emitted[session]


class YinF0Pool(_SamplePoolHandle):
    """Tracker sessions that advance independently (``fv_yinpool``, include/fishvoc.h): what ``YinF0Stream`` is to rows in lockstep, for
    ``sessions`` slots with their own counters.  ``step(items)`` takes ``(session, samples, end)`` tuples — ``samples``: a 1-D tensor of at
    most ``max_chunk_samples`` samples, or ``None`` for none; ``end``: the utterance ends with them — and returns one ``(f0 (k,),
    aperiodicity (k,))`` pair per item (``k`` may be 0): the frames that read no later sample, or with ``end`` all that remain, against the
    utterance's true end.  A session appears at most once per step and refuses items after its end until ``reset(session)``.  The whole step
    is checked before anything moves: a refused step leaves every session as it was.  A session's concatenated values have the bits of
    ``YinF0.forward`` on its whole utterance.  One step is one tracker launch and one carry launch per 32 items; work is enqueued on
    torch's current stream, and calls must be ordered."""
    _destroy, _prefix, _bound, _noun = "fv_yinpool_destroy", "fv_yinpool", "max_frames", "chunk"
    _closed = "this F0 pool is closed: create a new one"
    _mismatch = "the F0 pool emitted {emit} frames where the emission rule says {plan}"

    def __init__(self, yin: YinF0, sessions: int, max_chunk_samples: int, device=None):
        self.counters = YinPoolCounters(yin.frame_length, yin.hop_length, sessions, max_chunk_samples)
        super().__init__(yin, sessions, max_chunk_samples, device)
        self.frame_length, self.hop_length = yin.frame_length, yin.hop_length

    def step(self, items) -> list:
        f0, ap, emit = self.step_padded(*self._gather(items))
        return [(f0[i, :k], ap[i, :k]) for i, k in enumerate(emit)]

    def step_padded(self, items, chunks: torch.Tensor | None, out: torch.Tensor | None = None, aperiodicity: bool = True) -> tuple:
        """The step on the caller's padded buffers, as ``fv_yinpool_step`` takes them: ``items``: ``(session, samples, end)`` integers;
        ``chunks``: ``(rows >= count, chunk_stride)`` with item i's samples first in row i (the rest, NaN included, is never read), ``None``
        when no item has samples; ``out``: ``(2, count, out_cols)`` — ``(1, count, out_cols)`` with ``aperiodicity=False``, which is then
        not stored — sized from the Python plan when not given.  Returns ``(f0 (count, out_cols), aperiodicity or None, frames per item)``:
        row i holds item i's frames first and zeros after them."""
        items, arr, got, cptr, stride = self._padded(items, chunks)
        count, lead = len(items), 2 if aperiodicity else 1
        plan = self.counters.plan(items)                          # sizes the output before anything is launched; refuses what the library would
        out = self._out(out, (lead, count), max(plan, default=0), f"{(lead, count, 'out_cols')}")
        cols = int(out.shape[2])
        self._run(lambda stream: self._lib.fv_yinpool_step(self._h, arr, count, cptr, stride, out[0].data_ptr() if out[0].numel() else None,
                                                           out[1].data_ptr() if aperiodicity and out[1].numel() else None, max(cols, 1),
                                                           cols, got, stream))
        return out[0], (out[1] if aperiodicity else None), self._moved(items, plan, got)


class PitchTemplatePool(_SamplePoolHandle):
    """Oscillator sessions that advance independently (``fv_oscpool``): what ``PitchTemplateStream`` is to rows in lockstep.  ``step(items)``
    takes ``(session, f0, end)`` tuples — ``f0``: a 1-D tensor of at most ``max_chunk_frames`` F0 frames in Hz, or ``None`` — and returns one
    ``(1, k hop)`` tensor per item: the samples of the frames whose next frame has arrived, or with ``end`` of all that remain.  Sessions,
    refusals and ordering as ``YinF0Pool``.  A session's concatenated samples have the bits of ``PitchTemplate.forward`` on its whole track:
    the phase carried per slot is a wrapping integer.  One step is three launches and one carry launch per 32 items."""
    _destroy, _prefix, _bound, _noun = "fv_oscpool_destroy", "fv_oscpool", "max_frames", "chunk"
    _closed = "this pitch template pool is closed: create a new one"
    _mismatch = "the pitch template pool emitted {emit} frames where the emission rule says {plan}"

    def __init__(self, template: PitchTemplate, sessions: int, max_chunk_frames: int, device=None):
        self.counters = OscPoolCounters(sessions, max_chunk_frames)
        super().__init__(template, sessions, max_chunk_frames, device)
        self.hop_length = template.hop_length

    def step(self, items) -> list:
        out, emit = self.step_padded(*self._gather(items))
        return [out[i:i + 1, :k * self.hop_length] for i, k in enumerate(emit)]

    def step_padded(self, items, chunks: torch.Tensor | None, out: torch.Tensor | None = None) -> tuple:
        """The step on the caller's padded buffers, as ``fv_oscpool_step`` takes them: ``items``: ``(session, frames, end)`` integers;
        ``chunks``: ``(rows >= count, chunk_stride)`` F0 in Hz with item i's frames first in row i (the rest is never read) — a
        ``YinF0Pool.step_padded``'s f0 buffer serves as it is; ``out``: ``(count, out_cols)`` samples, sized from the Python plan when not
        given.  Returns ``(out, frames per item)``: row i holds the ``k hop`` samples of item i first and zeros after them."""
        items, arr, got, cptr, stride = self._padded(items, chunks)
        count = len(items)
        plan = self.counters.plan(items)
        out = self._out(out, (count,), max(plan, default=0) * self.hop_length, f"{(count, 'out_cols')}")
        cols = int(out.shape[1])
        self._run(lambda stream: self._lib.fv_oscpool_step(self._h, arr, count, cptr, stride, out.data_ptr() if out.numel() else None,
                                                           max(cols, 1), cols, got, stream))
        return out, self._moved(items, plan, got)


class TemplatePoolCounters:
    """The plan of a ``TemplatePool`` step on the host: the tracker's counters into the oscillator's.  ``plan(items)`` — ``(session, samples,
    end)`` — returns ``(tracker frames per item, template frames per item)`` and moves nothing; ``step`` moves both."""

    def __init__(self, tracker: YinPoolCounters, template: OscPoolCounters):
        self.tracker, self.template = tracker, template

    def plan(self, items) -> tuple:
        items = SamplePoolCounters._items(items)
        frames = self.tracker.plan(items)
        return frames, self.template.plan([(s, k, end) for (s, _, end), k in zip(items, frames)])

    def step(self, items) -> tuple:
        items = SamplePoolCounters._items(items)
        frames, emit = self.plan(items)
        self.tracker.commit(items, frames)
        self.template.commit([(s, k, end) for (s, _, end), k in zip(items, frames)], emit)
        return frames, emit

    def reset(self, session: int) -> None:
        self.tracker.reset(session)
        self.template.reset(session)


class TemplatePool:
    """Audio in, template samples out, per session: a ``YinF0Pool`` into a ``PitchTemplatePool``, what ``TemplateStream`` is to rows in
    lockstep.  ``step([(session, samples, end), ...])`` returns one ``(1, k hop)`` tensor per item: the template samples that are final.  The
    tracker pool's ``(count, out_cols)`` F0 buffer is the oscillator pool's chunk buffer as it stands, and the oscillator's items are
    ``(session, frames the tracker emitted, end)`` from the host counters: nothing is copied and nothing synchronises.  Both plans are
    checked before anything moves.  A session's concatenated samples have the bits of ``template_from_audio`` on its whole utterance."""

    def __init__(self, sample_rate: int, hop_length: int, sessions: int, max_chunk_samples: int, frame_length: int = 2048, fmin: float = 40.0,
                 fmax: float = 1100.0, threshold: float = 0.1, kind: str = "sine", amplitude: float = 1.0):
        self.yin = YinF0(sample_rate, hop_length, frame_length, fmin, fmax, threshold)
        self.oscillator = PitchTemplate(sample_rate, hop_length, kind, amplitude)
        self.sessions, self.max_chunk_samples, self.hop_length = int(sessions), int(max_chunk_samples), int(hop_length)
        self.tracker = self.template = None
        try:
            self.tracker = self.yin.pool(sessions, max_chunk_samples)
            self.template = self.oscillator.pool(sessions, max(self.tracker.max_frames, 1))
        except Exception:
            self.close()
            raise
        self.max_frames = self.template.max_frames      # the most template frames one item emits in one step
        self.counters = TemplatePoolCounters(self.tracker.counters, self.template.counters)
        self.device = self.tracker.device

    def received(self, session: int) -> int:
        """Samples of the session's utterance received so far."""
        return self.tracker.received(session)

    def emitted(self, session: int) -> int:
        """Frames of ``hop`` template samples emitted so far."""
        return self.template.emitted(session)

    def pending(self, session: int) -> int:
        """Frames an ``end`` would emit now: ``N // hop - E``."""
        return self.tracker.received(session) // self.hop_length - self.template.emitted(session)

    def step(self, items) -> list:
        self.tracker._check_open()
        out, emit = self.step_padded(*_gather(items, self.device, _require_cuda, "TemplatePool.step", "chunk"))
        return [out[i:i + 1, :k * self.hop_length] for i, k in enumerate(emit)]

    def step_padded(self, items, chunks: torch.Tensor | None, out: torch.Tensor | None = None) -> tuple:
        """``items``: ``(session, samples, end)`` integers; ``chunks`` as ``YinF0Pool.step_padded`` takes them; ``out``: ``(count, out_cols)``
        samples.  Returns ``(out, template frames per item)``."""
        self.tracker._check_open()
        self.template._check_open()
        items = SamplePoolCounters._items(items)
        self.counters.plan(items)                                 # both plans before anything moves
        f0, _, frames = self.tracker.step_padded(items, chunks, aperiodicity=False)
        return self.template.step_padded([(s, k, end) for (s, _, end), k in zip(items, frames)], f0 if f0.shape[1] else None, out)

    def reset(self, session: int) -> None:
        self.tracker.reset(session)
        self.template.reset(session)

    def close(self) -> None:
        for part in (self.tracker, self.template, self.yin, self.oscillator):
            if part is not None:
                part.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()
