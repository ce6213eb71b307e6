"""The plan of one step of a session pool (include/fishvoc.h ``fv_pool_*``, ``Engine.session_pool``) in plain Python: host only,
deterministic, and the tests' independent statement of what the library plans (``fv_pool_plan`` returns it row for row).

A pool holds ``S`` sessions.  Each has its own counters ``F`` (frames received) and ``E`` (frames emitted) and a ``flushed`` flag.  A step
is a list of items ``(session, n, flush)``: the session receives ``n >= 0`` frames and, with ``flush``, its utterance ends with them.  The
counters move as ``vocoder_amd.streaming.step`` moves a stream's: ``F' = F + n``; ``E' = F'`` on a flush, else ``max(E, F' - A)``;
``w = max(0, E - K)``.  An item with ``E' > E`` is a *row*: the model sees the frames ``[w, F')``, ``W = F' - w``, and the frames ``[E, E')``
come out.  A row owns its left edge iff ``w == 0`` and its right edge iff it flushes.

Rows of different lengths share one forward: ``Wg`` is the largest ``W``; group 0 is a ``(rows, C_in, Wg)`` tensor in which a row that owns
its left edge starts at column ``col0 = 0`` and any other row at ``col0 = Wg - W`` (right-aligned), every other column being zero.  The rule
is the one the time tiles, the streams and the ragged batches rest on: an emitted frame lies ``>= K`` (``A``) frames inside a left (right)
edge the row does not own, so with ``K, A >= reach`` what lies beyond that edge — the tensor edge, zeros, other data — does not matter.  The
only rows that cannot be placed are those that own BOTH edges and are shorter than ``Wg`` (whole short utterances): they form further groups
by exact ``W``, in descending ``W``, at ``col0 = 0``.  Rows keep item order within a group and are listed by group.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence

from . import streaming


class Item(NamedTuple):
    session: int
    frames: int
    flush: bool = False


class Row(NamedTuple):
    item: int       # index into the step's items
    group: int
    col0: int       # first column of the window inside the group's tensor
    frames: int     # W
    w: int          # the window is the utterance's frames [w, w + W)
    emit_lo: int    # the step emits the frames [emit_lo, emit_hi) = [E, E')
    emit_hi: int


class StepPlan(NamedTuple):
    rows: list          # of Row: by group, then by item
    groups: list        # of (rows, frames) per forward, in group order
    received: list      # F' per item
    emitted: list       # E' per item

    @property
    def emit_frames(self) -> list:
        """Frames every item emits, in item order (0 for an item without a row)."""
        out = [0] * len(self.received)
        for r in self.rows:
            out[r.item] = r.emit_hi - r.emit_lo
        return out


class PoolStateError(ValueError):
    """An item for a session that was flushed and not reset (``FV_ERR_STATE`` in the library)."""


def plan_step(K: int, A: int, max_chunk: int, received: Sequence[int], emitted: Sequence[int], flushed: Sequence[bool] | None,
              items: Sequence, in_frames: int | None = None, out_frames: int | None = None) -> StepPlan:
    """The plan of one step from the counters ``received[s]``, ``emitted[s]`` and flags ``flushed[s]`` of the ``S`` sessions; changes nothing.
    ``in_frames`` / ``out_frames``: the frames per row of the caller's chunk / output buffer, checked when given."""
    K, A, max_chunk = int(K), int(A), int(max_chunk)
    S = len(received)
    if S < 1 or max_chunk < 1 or K < 0 or A < 0 or len(emitted) != S:
        raise ValueError(f"sessions ({S}) and max_chunk_frames ({max_chunk}) must be >= 1, context_frames ({K}) and lookahead_frames ({A}) >= 0")
    items = [Item(int(it[0]), int(it[1]), bool(it[2]) if len(it) > 2 else False) for it in items]
    seen: set[int] = set()
    cand, F2, E2 = [], [], []
    for i, it in enumerate(items):
        if not 0 <= it.session < S:
            raise ValueError(f"item {i} names session {it.session}, outside [0, {S})")
        if it.session in seen:
            raise ValueError(f"duplicate session {it.session} (item {i}): a session appears at most once per step")
        seen.add(it.session)
        if not 0 <= it.frames <= max_chunk:
            raise ValueError(f"item {i} has {it.frames} frames, outside [0, max_chunk_frames = {max_chunk}]")
        F, E = int(received[it.session]), int(emitted[it.session])
        if flushed is not None and flushed[it.session]:
            raise PoolStateError(f"session {it.session} was flushed (item {i}); reset it before the next utterance")
        f2, w, e2 = streaming.step(F, E, it.frames, K, A)            # the push of the item's frames ...
        if it.flush:
            e2 = streaming.step(f2, E, 0, K, A, flush=True)[2]       # ... and, at the utterance's end, the flush over the same window
        F2.append(f2)
        E2.append(e2)
        if e2 > E:
            cand.append((i, f2 - w, w, E, e2, it.flush))
    max_n = max((it.frames for it in items), default=0)
    max_emit = max((e2 - int(emitted[it.session]) for it, e2 in zip(items, E2)), default=0)
    if in_frames is not None and 0 <= in_frames < max_n:
        raise ValueError(f"in_frames = {in_frames}, but an item of this step has {max_n} frames")
    if out_frames is not None and 0 <= out_frames < max_emit:
        raise ValueError(f"out_frames = {out_frames}, but an item of this step emits {max_emit} frames")
    if not cand:
        return StepPlan([], [], F2, E2)
    Wg = max(W for _, W, *_ in cand)
    whole_short = [c for c in cand if c[2] == 0 and c[5] and c[1] < Wg]
    rows = [Row(i, 0, 0 if w == 0 else Wg - W, W, w, lo, hi) for i, W, w, lo, hi, fl in cand if not (w == 0 and fl and W < Wg)]
    groups = [(len(rows), Wg)]
    for W in sorted({c[1] for c in whole_short}, reverse=True):
        same = [c for c in whole_short if c[1] == W]
        rows += [Row(i, len(groups), 0, W, 0, lo, hi) for i, _, _, lo, hi, _ in same]
        groups.append((len(same), W))
    return StepPlan(rows, groups, F2, E2)


class PoolState:
    """The host side of a pool: the counters of ``S`` sessions, advanced by ``step`` as ``fv_pool_step`` advances the library's."""

    def __init__(self, sessions: int, max_chunk: int, K: int, A: int):
        self.S, self.max_chunk, self.K, self.A = int(sessions), int(max_chunk), int(K), int(A)
        self.cap = self.K + self.A + self.max_chunk
        self.received = [0] * self.S
        self.emitted = [0] * self.S
        self.flushed = [False] * self.S

    def plan(self, items: Sequence, in_frames: int | None = None, out_frames: int | None = None) -> StepPlan:
        return plan_step(self.K, self.A, self.max_chunk, self.received, self.emitted, self.flushed, items, in_frames, out_frames)

    def apply(self, items: Sequence, plan: StepPlan) -> None:
        for it, f2, e2 in zip(items, plan.received, plan.emitted):
            s = int(it[0])
            self.received[s], self.emitted[s] = f2, e2
            if len(it) > 2 and it[2]:
                self.flushed[s] = True

    def step(self, items: Sequence, in_frames: int | None = None, out_frames: int | None = None) -> StepPlan:
        p = self.plan(items, in_frames, out_frames)
        self.apply(items, p)
        return p

    def reset(self, session: int) -> None:
        if not 0 <= session < self.S:
            raise ValueError(f"no session {session}")
        self.received[session] = self.emitted[session] = 0
        self.flushed[session] = False
