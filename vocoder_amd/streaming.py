"""The emission rule of a stream (include/fishvoc.h ``fv_stream_*``), in plain Python.

``Stream`` sizes its outputs with ``step`` before it launches anything; the tests build the expected windows with ``schedule``.

Counters: ``F`` frames received, ``E`` frames emitted; ``K`` frames of left context, ``A`` frames of lookahead.  A push of ``n`` frames sets
``F += n`` and ``E' = max(E, F - A)``; a flush sets ``E' = F``.  When ``E' > E`` the model runs once on the window of frames ``[w, F)``,
``w = max(0, E - K)``, and the call returns the frames ``[E, E')`` — the samples ``[(E - w) hop, (E' - w) hop)`` of that window's output.
"""
from __future__ import annotations

from typing import Iterable


def step(F: int, E: int, n: int, K: int, A: int, flush: bool = False) -> tuple[int, int, int]:
    """One push of ``n`` frames (``flush``: the flush, ``n`` ignored) from the counters ``(F, E)`` -> ``(F', w, E')``.  Frames ``[E, E')`` are
    emitted out of the window ``[w, F')``; ``E' == E`` means nothing is emitted (and nothing is run)."""
    if min(F, E, K, A) < 0 or E > F:
        raise ValueError(f"invalid stream state F={F}, E={E}, K={K}, A={A}")
    if not flush and n < 0:
        raise ValueError(f"negative push of {n} frames")
    F2 = F if flush else F + n
    E2 = F2 if flush else max(E, F2 - A)
    return F2, max(0, E - K), E2


def schedule(chunks: Iterable[int], K: int, A: int, flush: bool = True) -> list[tuple[int, int, int]]:
    """``(w, E, E')`` for every push of ``chunks`` frames in turn, then for the flush (``flush=True``).  The window of entry ``i`` is
    ``[w, F_i)``, ``F_i`` the frames received by then (the utterance's length for the flush)."""
    F = E = 0
    out = []
    for n in chunks:
        F, w, E2 = step(F, E, int(n), K, A)
        out.append((w, E, E2))
        E = E2
    if flush:
        F, w, E2 = step(F, E, 0, K, A, flush=True)
        out.append((w, E, E2))
    return out
