"""The framing rule of the log-mel front-end in plain Python (include/fishvoc.h ``fv_logmel_frames`` / ``fv_logmel_frames_ready``).

``LinearSpectrogram`` (reference spectrogram.py:25-56) reflect-pads a row of ``L`` samples by ``pad_l = (win - hop) // 2`` on the left and
``pad_r = (win - hop + 1) // 2`` on the right and cuts ``n_fft``-sample frames every ``hop`` samples: frame ``f`` reads the wave indices
``[f hop - pad_l, f hop - pad_l + n_fft)``.

* ``frames(L)``: frames of a whole row, ``1 + (L + pad_l + pad_r - n_fft) // hop``, 0 if the padded row is shorter than one frame.
* ``frames_ready(N)``: frames that need no sample at or after ``N`` — what a stream can emit once ``N`` samples have arrived:
  ``1 + (N + pad_l - n_fft) // hop`` once ``N + pad_l >= n_fft``, else 0.  Never above ``frames(N)``.
* ``Counters`` replays a ``LogMelStream``'s host counters: a push sets ``N += c`` and emits ``[E, frames_ready(N))``, the flush emits
  ``[E, frames(N))`` against the row's true end.
* ``PoolCounters`` replays a ``WavPool``'s (include/fishvoc.h ``fv_wavpool_*``): ``S`` slots with their own ``N``, ``E`` and flushed flag.  A
  step is a list of items ``(session, samples, flush)``; per item ``N' = N + samples``, ``E' = max(E, frames(N') if flush else
  frames_ready(N'))``, and the item emits ``[E, E')``.  ``fv_wavpool_plan`` returns the same counts item for item.
"""
from __future__ import annotations

from dataclasses import dataclass

from .sample_pool import MAX_SAMPLES, SamplePoolCounters  # noqa: F401


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


class PoolCounters(SamplePoolCounters):
    """The host counters of a wav pool (``SamplePoolCounters``) with the framing rule: ``E' = max(E, frames(N') if flush else
    frames_ready(N'))``.  Beyond the shared refusals, ``ValueError`` for a flush that ends an utterance too short for the reflect padding or
    for one frame."""

    def __init__(self, framing: Framing, sessions: int, max_chunk: int):
        super().__init__(sessions, max_chunk)
        self.framing = framing

    def _emission(self, i: int, s: int, c: int, flush: bool, N2: int, E: int) -> int:
        fr = self.framing
        if flush and N2 > 0 and fr.too_short(N2):
            raise ValueError(f"session {s} (item {i}) ends after {N2} samples: too short for reflect padding {fr.pad_l}/{fr.pad_r} and one "
                             f"{fr.n_fft}-sample frame")
        return max(E, fr.frames(N2) if flush else fr.frames_ready(N2))

    def pending_samples(self, session: int) -> int:
        return self.framing.pending_samples(self.received[session], self.emitted[session])
