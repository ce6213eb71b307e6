"""CPU: the streaming API's C declarations and exports, the ctypes mirror of fv_stream_config, and the emission rule (vocoder_amd.streaming)."""
import ctypes
import os
import random
import re

import pytest

from vocoder_amd import _lib
from vocoder_amd.streaming import schedule, step

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
STREAM_API = ("fv_reach_frames", "fv_stream_create", "fv_stream_workspace_bytes", "fv_stream_pending_frames", "fv_stream_push",
              "fv_stream_flush", "fv_stream_reset", "fv_stream_destroy")


def test_stream_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in STREAM_API:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name


def test_stream_config_mirror_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    body = re.search(r"typedef struct fv_stream_config \{(.*?)\} fv_stream_config;", hdr, re.S).group(1)
    fields = re.findall(r"int32_t\s+(\w+);", body)
    assert fields == [f for f, _ in _lib.StreamConfig._fields_]
    assert ctypes.sizeof(_lib.StreamConfig) == 4 * len(fields) == 16


def _chunkings(seed, T, max_chunk):
    rng = random.Random(seed)
    out = []
    left = T
    while left > 0:
        n = min(left, rng.randint(1, max_chunk))
        out.append(n)
        left -= n
    return out


@pytest.mark.parametrize("seed", range(40))
def test_schedule_properties_over_random_chunkings(seed):
    rng = random.Random(1000 + seed)
    T = rng.choice([1, 2, 5, 17, 18, 60, 389, 1000])
    K, A = rng.randint(0, 40), rng.randint(0, 40)
    max_chunk = rng.randint(1, 70)
    chunks = _chunkings(seed, T, max_chunk)
    sched = schedule(chunks, K, A)
    assert len(sched) == len(chunks) + 1
    F = 0
    nxt = 0                                   # emitted ranges tile [0, T) in order: no gap, no overlap
    for i, (w, e0, e1) in enumerate(sched):
        flush = i == len(chunks)
        if not flush:
            F += chunks[i]
        assert e0 == nxt and e1 >= e0
        nxt = e1
        assert e1 <= F
        if e1 > e0:
            assert w == max(0, e0 - K)
            assert e0 - w >= min(K, e0)                # left context
            assert F - w <= K + A + max_chunk          # window length
            if not flush:
                assert F - e1 >= A                     # lookahead to the window's right edge
                assert e1 - e0 <= chunks[i]
        if flush:
            assert e1 - e0 <= A and e1 == F == T
        else:
            assert F - e1 <= A                         # F - E <= A after every push
    assert nxt == T


@pytest.mark.parametrize("T,A", [(1, 17), (17, 17), (5, 40), (3, 3)])
def test_short_utterance_is_a_single_window_at_flush(T, A):
    for chunks in ([1] * T, [T], _chunkings(T, T, 4)):
        sched = schedule(chunks, 17, A)
        assert all(e1 == e0 for _, e0, e1 in sched[:-1])
        assert sched[-1] == (0, 0, T)


def test_step_refuses_impossible_states():
    with pytest.raises(ValueError):
        step(3, 5, 1, 2, 2)
    with pytest.raises(ValueError):
        step(0, 0, -1, 2, 2)
    assert step(10, 7, 0, 2, 3) == (10, 5, 7)           # n = 0 after a push (F - E <= A): nothing to emit
    assert step(10, 7, 0, 2, 3, flush=True) == (10, 5, 10)
