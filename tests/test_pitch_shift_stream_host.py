"""Host (no GPU): the streaming pitch shift (include/fishvoc.h fv_pv_*) — the emission rule stated three times (C: fv_pv_stream_ready; Python:
vocoder_amd.pitch_shift.stream_ready; counting: pitch_shift_stream_reference), its relation to the whole-row lengths, the latency bound, the ABI
surface, and the refusals of the pure-host entry."""
import ctypes
import os
import re

import pytest

import pitch_shift_reference as pref
import pitch_shift_stream_reference as sref
from vocoder_amd import _lib
from vocoder_amd import pitch_shift as ps

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

PV_API = ("fv_pv_stream_ready", "fv_pv_set_batch_invariant", "fv_pv_stream_create", "fv_pv_stream_workspace_bytes", "fv_pv_stream_pending",
          "fv_pv_stream_push", "fv_pv_stream_flush", "fv_pv_stream_reset", "fv_pv_stream_destroy")
# two lengths beyond the grid at which, with hop == n_fft and n_steps = -4, Ls(N) is the smaller term of Y
EXTRA_N = (1888, 1889)


def _cfg(n_steps, n_fft, hop, sr=sref.SR):
    return _lib.PitchShiftConfig(sr, float(n_steps), 12, n_fft, hop, 100, 64, ps.KAISER_BEST_ROLLOFF, _lib.FV_RESAMPLE_SINC_KAISER, 0.0)


def _native_ready(c, N):
    out = [ctypes.c_int64() for _ in range(3)]
    _lib.check(_lib.lib().fv_pv_stream_ready(ctypes.byref(c), N, *[ctypes.byref(v) for v in out]))
    return tuple(v.value for v in out)


def test_entry_points_are_declared_listed_exported_and_the_abi_stays_5():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in PV_API:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert {d for d in declared if d.startswith("fv_pv_")} == set(PV_API)
    assert {n for n in _lib.EXPORTS if n.startswith("fv_pv_")} == set(PV_API)
    assert "#define FV_ABI_VERSION 5" in hdr and _lib.FV_ABI_VERSION == 5 and L.fv_abi_version() == 5
    # every entry names the reference code it stands in for
    for name in PV_API:
        at = re.search(r"FV_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr).start()
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "test.py:61-62" in comment, name
    assert "Not built: a streaming form" not in hdr


@pytest.mark.parametrize("n_fft,hop", sref.GRID_FRAMES)
def test_the_rule_agrees_between_c_python_and_counting(n_fft, hop):
    for n_steps in sref.GRID_STEPS:
        orig, o, n = pref.plan(sref.SR, n_steps)
        c = _cfg(n_steps, n_fft, hop)
        mod = ps.PitchShift(sref.SR, n_steps, n_fft=n_fft, hop_length=hop)
        filt = sref.resampler(sref.SR, n_steps)
        bound = sref.latency_bound(filt, n_fft, hop)
        last_y = last_e = 0
        worst = 0
        for N in sorted(sref.GRID_N + EXTRA_N):
            A, S, Y = sref.ready(N, o, n, n_fft, hop)
            assert _native_ready(c, N) == (A, S, Y) == ps.stream_ready(N, o, n, n_fft, hop) == mod.stream_ready(N), (n_steps, N)
            T, Tout, Ls = sref.whole_lengths(N, o, n, hop)
            assert (T, Tout, Ls) == mod.lengths(N)[:3]
            assert A <= T and S <= Tout and Y <= Ls, (n_steps, N)
            assert Y >= last_y, (n_steps, N)                      # monotone: a push never takes a stretched sample back
            E, raw = sref.emitted(filt, Y, N)
            assert raw <= N, (n_steps, N)                         # the cap at N does not bind
            assert E == mod.stream_emitted(N) and E >= last_e
            assert N - E <= bound, (n_steps, N, E, bound)
            worst = max(worst, N - E)
            last_y, last_e = Y, E
        print(f"n_fft {n_fft} hop {hop} n_steps {n_steps}: N - E <= {worst} on the grid, bound {bound}")


def test_ls_binds_only_where_the_hop_is_the_frame():
    """Y = min(max(0, S h - F/2), Ls(N)): the second term is the smaller one at n_fft = hop = 64, n_steps = -4, N = 1888 (1498 < 1504), which is
    why the stream carries n_fft / hop frames, one more than the overlap."""
    _, o, n = pref.plan(sref.SR, -4)
    A, S, Y = ps.stream_ready(1888, o, n, 64, 64)
    assert (A, S) == (30, 24) and Y == pref.stretched_length(1888, o, n) == 1498 < S * 64 - 32
    assert sref.ready(1888, o, n, 64, 64) == (A, S, Y)
    for n_fft, hop in ((64, 16), (64, 32), (2048, 512)):
        for n_steps in sref.GRID_STEPS:
            _, o, n = pref.plan(sref.SR, n_steps)
            for N in range(0, 6000, 7):
                A, S, Y = ps.stream_ready(N, o, n, n_fft, hop)
                assert Y == max(0, S * hop - n_fft // 2)


def test_identity_and_python_counts():
    mod = ps.PitchShift(sref.SR, 0)
    assert mod.plan() == (sref.SR, 1, 1)
    assert [mod.stream_emitted(N) for N in (0, 1, 777)] == [0, 1, 777]
    mod = ps.PitchShift(sref.SR, 3, batch_invariant=True)
    assert mod.batch_invariant and not ps.PitchShift(sref.SR, 3).batch_invariant
    assert mod.stream_emitted(0) == 0 and mod.stream_emitted(1023) == 0


def test_null_and_bad_arguments_of_the_pure_host_entry():
    L = _lib.lib()
    v = ctypes.c_int64(-7)
    assert L.fv_pv_stream_ready(None, 10, ctypes.byref(v), None, None) == _lib.FV_ERR_INVALID
    assert "fv_pv_stream_ready" in L.fv_last_error().decode() and v.value == -7
    for N in (-1, (1 << 30) + 1):
        assert L.fv_pv_stream_ready(ctypes.byref(_cfg(3, 2048, 512)), N, ctypes.byref(v), None, None) == _lib.FV_ERR_INVALID
        assert "fv_pv_stream_ready: N" in L.fv_last_error().decode() and v.value == -7
    assert L.fv_pv_stream_ready(ctypes.byref(_cfg(float("nan"), 2048, 512)), 10, None, None, None) == _lib.FV_ERR_INVALID
    assert "fv_pv_stream_ready" in L.fv_last_error().decode() and "n_steps" in L.fv_last_error().decode()
    assert L.fv_pv_stream_ready(ctypes.byref(_cfg(3, 2048, 500)), 10, None, None, None) == _lib.FV_ERR_UNSUPPORTED
    assert "fv_pv_stream_ready: n_fft = 2048 and hop_length = 500" in L.fv_last_error().decode()
    assert L.fv_pv_stream_ready(ctypes.byref(_cfg(3, 2048, 0)), 1 << 30, None, None, None) == _lib.FV_OK       # NULL outputs are skipped
    assert _native_ready(_cfg(3, 2048, 0), 20000) == ps.stream_ready(20000, 524, 441, 2048, 512)
    # the entries that take an object refuse NULL without touching a device
    h = ctypes.c_void_p()
    assert L.fv_pv_set_batch_invariant(None, 1) == _lib.FV_ERR_INVALID and "fv_pv_set_batch_invariant" in L.fv_last_error().decode()
    assert L.fv_pv_stream_create(None, 1, 16, ctypes.byref(h)) == _lib.FV_ERR_INVALID and "fv_pv_stream_create" in L.fv_last_error().decode()
    assert h.value is None
    got = ctypes.c_int64(5)
    assert L.fv_pv_stream_push(None, None, 0, 1, None, 0, ctypes.byref(got), None, 0, None) == _lib.FV_ERR_INVALID
    assert "fv_pv_stream_push" in L.fv_last_error().decode() and got.value == 0
    assert L.fv_pv_stream_flush(None, None, 0, ctypes.byref(got), None, 0, None) == _lib.FV_ERR_INVALID
    assert "fv_pv_stream_flush" in L.fv_last_error().decode()
    assert L.fv_pv_stream_reset(None) == _lib.FV_ERR_INVALID and "fv_pv_stream_reset" in L.fv_last_error().decode()
    assert L.fv_pv_stream_workspace_bytes(None) == 0 and L.fv_pv_stream_pending(None) == 0
    L.fv_pv_stream_destroy(None)
