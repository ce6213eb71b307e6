"""The plan of a ragged batch (include/fishvoc.h ``fv_ragged_*``, ``Engine.forward_ragged``) in plain Python: host only, deterministic,
and the tests' independent statement of what the library plans (``fv_ragged_plan`` returns it window for window).

``lengths[b]`` frames of clip ``b`` are valid.  A *window* ``(clip, start, frames, keep_lo, keep_hi, group)`` says: the forward sees the frames
``[start, start + frames)`` of the clip (zeros from ``lengths[clip]`` on) and the output samples of the clip's frames ``[keep_lo, keep_hi)`` are
copied out.  Windows of one group have one length and run as ONE forward.  The rule is the one the time tiles and the streams rest on: a window
reproduces the clip's own samples at every frame that lies >= ``reach`` frames inside each window edge that is not the clip's own edge — and the
zero fill past the clip's end inside a longer window is NOT the clip's edge (every layer pads at the tensor edge), so such a window keeps only
the frames before ``T - reach``.

Per clip of ``T`` frames, ``R = reach`` (``Engine.reach_frames``):

* ``T == 0``: no window.
* ``1 <= T <= 2R`` (short): one window ``(b, 0, T, [0, T))``; short clips group by exact length.
* ``T > 2R`` (long): a body window ``(b, 0, Tg, [0, T - R))`` in a body group of ``Tg >= T`` frames and a tail window
  ``(b, T - 2R, 2R, [T - R, T))``; a clip with ``T == Tg`` is its group's own length: its body window keeps ``[0, T)`` and it has no tail.
  All tails, and the short clips of exactly ``2R`` frames, share the group of ``2R`` frames.

Body groups: the long clips sorted by ``(T, b)`` are cut into at most ``max_groups`` contiguous runs, never between two clips of one length,
minimising ``sum over runs (clips * Tg + 2R * #{T < Tg} + launch_frames)`` with ``Tg`` the run's longest clip.  Ties: the fewest runs, then
— from the last run backwards — the run that starts earliest.  Groups are numbered by descending length (bodies, then the ``2R`` group, then
the other short lengths); windows are listed by group, then by clip.  ``launch_frames`` is the fixed cost of one more forward in frames; it
moves speed only, never a sample.  A batch of equal lengths plans to one window per clip of ``n = T``: a plain forward.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence

# single-clip p50 / headline ms per frame of HiFiGAN-V1: 0.65 - 0.71 ms / (9.07 ms / 2752 frames) ~ 200 frames (README.md); overridable per plan
LAUNCH_FRAMES = 192
MAX_GROUPS = 8


class Window(NamedTuple):
    clip: int
    start: int
    frames: int
    keep_lo: int
    keep_hi: int
    group: int


def run_cost(L: Sequence[int], i: int, j: int, reach: int, launch_frames: int) -> int:
    """Cost of one body group made of the ascending long lengths ``L[i:j]``."""
    tg = L[j - 1]
    return (j - i) * tg + 2 * reach * sum(1 for t in L[i:j] if t < tg) + launch_frames


def body_runs(sorted_lengths: Sequence[int], reach: int, launch_frames: int = LAUNCH_FRAMES, max_groups: int = MAX_GROUPS) -> list[tuple[int, int]]:
    """The optimal cut of the ascending ``sorted_lengths`` (all > 2 * reach) into runs ``[(i, j), ...]`` (half-open), by dynamic programming
    (O(B^2 * max_groups) with B a few hundred at most)."""
    L = list(sorted_lengths)
    m = len(L)
    if m == 0:
        return []
    INF = 1 << 62
    K = min(max_groups, m)
    f = [[INF] * (m + 1) for _ in range(K + 1)]      # f[k][j]: the first j clips in exactly k runs
    arg = [[-1] * (m + 1) for _ in range(K + 1)]
    f[0][0] = 0
    for k in range(1, K + 1):
        for j in range(k, m + 1):
            if j < m and L[j] == L[j - 1]:
                continue                              # no cut between two clips of one length (merging them is never worse)
            for i in range(k - 1, j):
                if f[k - 1][i] >= INF:
                    continue
                c = f[k - 1][i] + run_cost(L, i, j, reach, launch_frames)
                if c < f[k][j]:                       # strict: the earliest start wins a tie
                    f[k][j], arg[k][j] = c, i
    best = min(range(1, K + 1), key=lambda k: (f[k][m], k))
    runs, j = [], m
    for k in range(best, 0, -1):
        i = arg[k][j]
        runs.append((i, j))
        j = i
    return runs[::-1]


def plan(lengths: Sequence[int], reach: int, launch_frames: int = LAUNCH_FRAMES, max_groups: int = MAX_GROUPS) -> list[Window]:
    lengths = [int(t) for t in lengths]
    reach = int(reach)
    if reach < 1:
        raise ValueError(f"reach must be >= 1, got {reach}")
    if not lengths:
        raise ValueError("empty batch: lengths has no entry")
    if any(t < 0 for t in lengths):
        raise ValueError(f"negative length in {lengths}")
    launch_frames = LAUNCH_FRAMES if launch_frames is None or launch_frames <= 0 else int(launch_frames)
    max_groups = MAX_GROUPS if max_groups is None or max_groups <= 0 else int(max_groups)
    R2 = 2 * reach
    long_ = sorted((t, b) for b, t in enumerate(lengths) if t > R2)
    items: list[tuple[int, int, int, int, int]] = []          # (frames, clip, start, keep_lo, keep_hi)
    for i, j in body_runs([t for t, _ in long_], reach, launch_frames, max_groups):
        tg = long_[j - 1][0]
        for t, b in long_[i:j]:
            if t == tg:
                items.append((tg, b, 0, 0, t))
            else:
                items.append((tg, b, 0, 0, t - reach))
                items.append((R2, b, t - R2, t - reach, t))
    for b, t in enumerate(lengths):
        if 1 <= t <= R2:
            items.append((t, b, 0, 0, t))
    items.sort(key=lambda it: (-it[0], it[1]))
    out, group, prev = [], -1, None
    for n, b, a, lo, hi in items:
        if n != prev:
            group, prev = group + 1, n
        out.append(Window(b, a, n, lo, hi, group))
    return out


def groups(windows: Sequence[Window]) -> list[tuple[int, int]]:
    """``(batch, frames)`` of every group's forward, in group order."""
    g: dict[int, list[int]] = {}
    for w in windows:
        g.setdefault(w.group, [0, w.frames])[0] += 1
    return [(g[k][0], g[k][1]) for k in sorted(g)]


def computed_frames(windows: Sequence[Window]) -> int:
    """Frames the forwards of the plan run over (the useful frames are ``sum(lengths)``)."""
    return sum(b * n for b, n in groups(windows))
