"""The framing rule of the log-mel front-end in plain Python (include/fishvoc.h ``fv_logmel_frames`` / ``fv_logmel_frames_ready``).

``LinearSpectrogram`` (reference spectrogram.py:25-56) reflect-pads a row of ``L`` samples by ``pad_l = (win - hop) // 2`` on the left and
``pad_r = (win - hop + 1) // 2`` on the right and cuts ``n_fft``-sample frames every ``hop`` samples: frame ``f`` reads the wave indices
``[f hop - pad_l, f hop - pad_l + n_fft)``.

* ``frames(L)``: frames of a whole row, ``1 + (L + pad_l + pad_r - n_fft) // hop``, 0 if the padded row is shorter than one frame.
* ``frames_ready(N)``: frames that need no sample at or after ``N`` — what a stream can emit once ``N`` samples have arrived:
  ``1 + (N + pad_l - n_fft) // hop`` once ``N + pad_l >= n_fft``, else 0.  Never above ``frames(N)``.
* ``Counters`` replays a ``LogMelStream``'s host counters: a push sets ``N += c`` and emits ``[E, frames_ready(N))``, the flush emits
  ``[E, frames(N))`` against the row's true end.
"""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class Framing:
    n_fft: int
    win_length: int
    hop_length: int

    @property
    def pad_l(self) -> int:
        return (self.win_length - self.hop_length) // 2

    @property
    def pad_r(self) -> int:
        return (self.win_length - self.hop_length + 1) // 2

    def frames(self, L: int) -> int:
        span = int(L) + self.pad_l + self.pad_r - self.n_fft
        return 1 + span // self.hop_length if L >= 0 and span >= 0 else 0

    def frames_ready(self, N: int) -> int:
        span = int(N) + self.pad_l - self.n_fft
        return 1 + span // self.hop_length if N >= 0 and span >= 0 else 0

    def too_short(self, L: int) -> bool:
        """A row the front-end refuses: no frame, or not longer than the reflect padding."""
        return self.frames(L) < 1 or L <= max(self.pad_l, self.pad_r)

    def pending_samples(self, N: int, E: int) -> int:
        """Samples received that frames not yet emitted still read: ``[max(0, E hop - pad_l), N)``."""
        return int(N) - max(0, int(E) * self.hop_length - self.pad_l)


class Counters:
    """The host counters of one stream: ``N`` samples received, ``E`` frames emitted."""

    def __init__(self, framing: Framing):
        self.framing = framing
        self.N = self.E = 0
        self.flushed = False

    def emit_count(self, c: int) -> int:
        """Frames a push of ``c`` samples emits now."""
        return max(self.E, self.framing.frames_ready(self.N + int(c))) - self.E

    def flush_count(self) -> int:
        return max(self.E, self.framing.frames(self.N)) - self.E

    def push(self, c: int) -> range:
        k = self.emit_count(c)
        self.N += int(c)
        self.E += k
        return range(self.E - k, self.E)

    def flush(self) -> range:
        k = self.flush_count()
        self.E += k
        self.flushed = True
        return range(self.E - k, self.E)

    def reset(self) -> None:
        self.N = self.E = 0
        self.flushed = False
