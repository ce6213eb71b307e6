"""The host counters every per-session sample pool shares, in plain Python (csrc/sample_pool.h: admit and commit).  No torch.

A pool has ``S`` slots with their own ``received``, ``emitted`` and ``flushed``.  A step is a list of items ``(session, samples, flush)``.
``plan`` checks the whole step in two passes, as the library does: the refusals every pool shares over all items (``sample_pool_admit``),
which yield ``N' = N + samples`` per item, then the pool's own emission rule per item, which may refuse too.  Nothing moves before ``commit``.
A pool supplies its rule (``_emission``), its bound (``max_outputs`` / ``max_frames``) and its ``pending``.
"""
from __future__ import annotations

from typing import Sequence

from .sessions import PoolStateError

MAX_SAMPLES = 1 << 40      # the longest utterance of a sample stream or pool (kSampleStreamMaxLen)


class SamplePoolCounters:
    """``plan(items)`` says what a step would emit per item and changes nothing; it refuses what the library refuses of the items, in its
    order per item: ``ValueError`` for a session out of range, a duplicate session and samples outside ``[0, max_chunk]``,
    ``PoolStateError`` for a flushed slot, ``ValueError`` past 2^40 samples; then whatever the pool's own rule refuses.  ``commit`` moves the
    counters as a step that emitted the plan does; ``step`` is both.  A pool that counts something else names its unit and its limits
    (``_frames.FramePoolCounters``: frames, chunks up to 2^20, utterances up to 2^30)."""
    _unit, _chunk_limit, _chunk_limit_name, _length_limit, _length_limit_name = "samples", 1 << 28, "2^28", MAX_SAMPLES, "2^40"

    def __init__(self, sessions: int, max_chunk: int):
        self.S, self.max_chunk = int(sessions), int(max_chunk)
        if not 1 <= self.S <= 65535 or not 1 <= self.max_chunk <= self._chunk_limit:
            raise ValueError(f"sessions ({self.S}) must lie in [1, 65535] and max_chunk ({self.max_chunk}) in [1, {self._chunk_limit_name}]")
        self.received = [0] * self.S
        self.emitted = [0] * self.S
        self.flushed = [False] * self.S

    def _emission(self, i: int, s: int, c: int, flush: bool, N2: int, E: int) -> int:
        """``E'`` of item ``i``: session ``s`` with ``E`` emitted takes ``c`` samples up to ``N2``.  May refuse the step."""
        raise NotImplementedError

    @staticmethod
    def _items(items: Sequence) -> list:
        return [(int(it[0]), int(it[1]), bool(it[2]) if len(it) > 2 else False) for it in items]

    def plan(self, items: Sequence) -> list:
        """What every item of the step emits, in item order."""
        items, seen, ends = self._items(items), set(), []
        for i, (s, c, _) in enumerate(items):
            if not 0 <= s < self.S:
                raise ValueError(f"item {i} names session {s}, outside [0, {self.S})")
            if s in seen:
                raise ValueError(f"duplicate session {s} (item {i}): a session appears at most once per step")
            seen.add(s)
            if not 0 <= c <= self.max_chunk:
                raise ValueError(f"item {i} (session {s}) has {c} {self._unit}, outside [0, max_chunk = {self.max_chunk}]")
            if self.flushed[s]:
                raise PoolStateError(f"session {s} was flushed (item {i}); reset it before the next utterance")
            if self.received[s] + c > self._length_limit:
                raise ValueError(f"item {i} takes session {s} past {self._length_limit_name} {self._unit} in one utterance")
            ends.append(self.received[s] + c)
        emitted, rule = self.emitted, self._emission
        return [rule(i, s, c, flush, N2, emitted[s]) - emitted[s] for i, ((s, c, flush), N2) in enumerate(zip(items, ends))]

    def commit(self, items: Sequence, plan: Sequence[int]) -> None:
        """Move the items' counters as a step that emitted ``plan`` does."""
        for (s, c, flush), k in zip(self._items(items), plan):
            self.received[s] += c
            self.emitted[s] += int(k)
            if flush:
                self.flushed[s] = True

    def step(self, items: Sequence) -> list:
        k = self.plan(items)
        self.commit(items, k)
        return k

    def reset(self, session: int) -> None:
        if not 0 <= session < self.S:
            raise ValueError(f"no session {session}")
        self.received[session] = self.emitted[session] = 0
        self.flushed[session] = False
