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
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn

from . import _lib
from ._handle import _DeviceHandles
from ._lib import check
from .resample import KAISER_BETA, _require_cuda, _rows

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


class PitchShift(nn.Module):
    """``librosa.effects.pitch_shift(y, sr=sample_rate, n_steps=n_steps)`` on the MI355X (test.py:61-62): ``forward(wave (..., L)) -> (..., L)``.
    Leading dimensions are flattened to rows (a stereo file is two rows, test.py:56-64).  ``time_stretch(wave)`` is the first stage alone,
    ``(..., Ls)``.  No CPU fallback."""

    def __init__(self, sample_rate: int, n_steps: float, bins_per_octave: int = 12, n_fft: int = 2048, hop_length: int | None = None,
                 freq_granularity: int = 100, lowpass_filter_width: int = 64, rolloff: float = KAISER_BEST_ROLLOFF,
                 resampling_method: str = "sinc_interp_kaiser", beta: float | None = None):
        super().__init__()
        self.sample_rate, self.n_steps, self.bins_per_octave = int(sample_rate), float(n_steps), int(bins_per_octave)
        self.n_fft, self.hop_length = int(n_fft), int(n_fft) // 4 if hop_length is None else int(hop_length)
        self.freq_granularity, self.lowpass_filter_width, self.rolloff = int(freq_granularity), int(lowpass_filter_width), float(rolloff)
        self.resampling_method, self.beta = resampling_method, beta
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
        return self._handles.get(device, lambda h: _lib.lib().fv_pitch_shift_create(ctypes.byref(self.config()), h))

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
