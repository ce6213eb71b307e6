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
from typing import Sequence

from .sessions import PoolStateError

MAX_SAMPLES = 1 << 40      # the longest utterance of a sample stream or pool (kSampleStreamMaxLen)


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


class PoolCounters:
    """The host counters of a wav pool: ``received[s]`` samples, ``emitted[s]`` frames and ``flushed[s]`` per slot.  ``plan(items)`` says what a
    step would emit per item and changes nothing; it refuses what ``fv_wavpool_step`` refuses of the items — ``ValueError`` for a session out
    of range, a duplicate session, samples outside ``[0, max_chunk]``, more than 2^40 samples and a flush that ends an utterance too short for
    the reflect padding or for one frame; ``PoolStateError`` for a flushed slot — checking the whole step before ``apply`` moves anything."""

    def __init__(self, framing: Framing, sessions: int, max_chunk: int):
        self.framing, self.S, self.max_chunk = framing, int(sessions), int(max_chunk)
        if not 1 <= self.S <= 65535 or not 1 <= self.max_chunk <= 1 << 28:
            raise ValueError(f"sessions ({self.S}) must lie in [1, 65535] and max_chunk ({self.max_chunk}) in [1, 2^28]")
        self.received = [0] * self.S
        self.emitted = [0] * self.S
        self.flushed = [False] * self.S

    @staticmethod
    def _items(items: Sequence) -> list:
        return [(int(it[0]), int(it[1]), bool(it[2]) if len(it) > 2 else False) for it in items]

    def plan(self, items: Sequence) -> list:
        """Frames every item of the step emits, in item order."""
        fr, seen, ends = self.framing, set(), []
        items = self._items(items)
        for i, (s, c, flush) in enumerate(items):
            if not 0 <= s < self.S:
                raise ValueError(f"item {i} names session {s}, outside [0, {self.S})")
            if s in seen:
                raise ValueError(f"duplicate session {s} (item {i}): a session appears at most once per step")
            seen.add(s)
            if not 0 <= c <= self.max_chunk:
                raise ValueError(f"item {i} (session {s}) has {c} samples, outside [0, max_chunk = {self.max_chunk}]")
            if self.flushed[s]:
                raise PoolStateError(f"session {s} was flushed (item {i}); reset it before the next utterance")
            if self.received[s] + c > MAX_SAMPLES:
                raise ValueError(f"item {i} takes session {s} past 2^40 samples in one utterance")
            ends.append(self.received[s] + c)
        for i, ((s, _, flush), N2) in enumerate(zip(items, ends)):
            if flush and N2 > 0 and fr.too_short(N2):
                raise ValueError(f"session {s} (item {i}) ends after {N2} samples: too short for reflect padding {fr.pad_l}/{fr.pad_r} and one "
                                 f"{fr.n_fft}-sample frame")
        return [max(self.emitted[s], fr.frames(N2) if flush else fr.frames_ready(N2)) - self.emitted[s] for (s, _, flush), N2 in zip(items, ends)]

    def apply(self, items: Sequence, plan: Sequence[int]) -> None:
        """Move the items' counters as a step that emitted ``plan`` does."""
        for (s, c, flush), k in zip(self._items(items), plan):
            self.received[s] += c
            self.emitted[s] += int(k)
            if flush:
                self.flushed[s] = True

    def step(self, items: Sequence) -> list:
        k = self.plan(items)
        self.apply(items, k)
        return k

    def pending_samples(self, session: int) -> int:
        return self.framing.pending_samples(self.received[session], self.emitted[session])

    def reset(self, session: int) -> None:
        if not 0 <= session < self.S:
            raise ValueError(f"no session {session}")
        self.received[session] = self.emitted[session] = 0
        self.flushed[session] = False
