"""Host (no GPU): the pitch shift (include/fishvoc.h fv_pitch_shift_*, fv_global_resample_create) — the ABI surface, the plan and the lengths
stated twice (C: fv_pitch_shift_plan / fv_pitch_shift_lengths; Python: vocoder_amd.pitch_shift) and a third time in the float64 restatement,
the two forms of the restatement's phase vocoder against each other, and the config errors."""
import ctypes
import os
import re

import numpy as np
import pytest

import pitch_shift_reference as pref
from vocoder_amd import _lib
from vocoder_amd import pitch_shift as ps
from vocoder_amd import resample as rs

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

PITCH_API = ("fv_pitch_shift_plan", "fv_pitch_shift_lengths", "fv_pitch_shift_create", "fv_pitch_shift_destroy",
             "fv_pitch_shift_workspace_bytes", "fv_pitch_shift_stretch", "fv_pitch_shift_forward")
STEPS = (-12, -4, -0.5, 0, 0.5, 1, 3, 7, 12)


def _cfg(sr=44100, n_steps=3.0, bpo=12, n_fft=2048, hop=0, gran=100, lpw=64, rolloff=ps.KAISER_BEST_ROLLOFF, method=_lib.FV_RESAMPLE_SINC_KAISER,
         beta=0.0):
    return _lib.PitchShiftConfig(sr, n_steps, bpo, n_fft, hop, gran, lpw, rolloff, method, beta)


def test_entry_points_are_declared_listed_exported_and_the_abi_stays_5():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in PITCH_API + ("fv_global_resample_create",):
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert {d for d in declared if d.startswith("fv_pitch_shift")} == set(PITCH_API)
    assert {n for n in _lib.EXPORTS if n.startswith("fv_pitch_shift")} == set(PITCH_API)
    assert "#define FV_ABI_VERSION 5" in hdr and _lib.FV_ABI_VERSION == 5 and L.fv_abi_version() == 5
    # every entry names the reference code it stands in for
    for name in PITCH_API + ("fv_global_resample_create",):
        at = re.search(r"FV_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr).start()
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "test.py:61-62" in comment, name


def test_config_mirror_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    body = re.search(r"typedef struct fv_pitch_shift_config \{(.*?)\} fv_pitch_shift_config;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+(\w+);", body, re.M)
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.PitchShiftConfig._fields_)
    # C layout of {i32, f64, i32 x 5, f64, i32, f64}: 4, pad to 8, 8, 20, pad to 40, 8, 4, pad to 56, 8
    assert ctypes.sizeof(_lib.PitchShiftConfig) == 64
    c = _lib.PitchShiftConfig
    assert (c.n_steps.offset, c.bins_per_octave.offset, c.rolloff.offset, c.method.offset, c.beta.offset) == (8, 16, 40, 48, 56)


@pytest.mark.parametrize("gran", [1, 100])
@pytest.mark.parametrize("sr", [24000, 44100, 48000])
def test_plan_and_lengths_agree_between_c_python_and_the_restatement(sr, gran):
    L = _lib.lib()
    for n_steps in STEPS:
        c = _cfg(sr=sr, n_steps=float(n_steps), gran=gran)
        of, o, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(L.fv_pitch_shift_plan(ctypes.byref(c), ctypes.byref(of), ctypes.byref(o), ctypes.byref(n)))
        got = (of.value, o.value, n.value)
        assert got == ps.plan(sr, n_steps, 12, gran) == pref.plan(sr, n_steps, 12, gran), n_steps
        assert got[0] % gran == 0 and got[0] * got[2] == sr * got[1] and np.gcd(got[1], got[2]) == 1
        assert abs(got[0] - sr * 2.0 ** (n_steps / 12)) < max(gran, 1)
        if n_steps == 0:
            assert got == (sr, 1, 1)
        mod = ps.PitchShift(sr, n_steps, freq_granularity=gran)
        assert mod.plan() == got
        for length in (0, 1, 511, 512, 513, 2047, 2048, 20000, 200000, 1 << 30):
            out = [ctypes.c_int64() for _ in range(4)]
            _lib.check(L.fv_pitch_shift_lengths(ctypes.byref(c), length, *[ctypes.byref(v) for v in out]))
            T, Tout, Ls, M = (v.value for v in out)
            assert (T, Tout, Ls, M) == mod.lengths(length), (n_steps, length)
            assert T == 1 + length // 512 and Tout == -((-T * got[1]) // got[2])
            assert Ls == pref.stretched_length(length, got[1], got[2]) and abs(Ls - length * got[1] / got[2]) <= 0.5
            assert abs(M - length) <= 1 + got[2] // got[1]          # the resample brings the row back to about L
            assert (Tout - 1) * got[2] // got[1] + 1 <= T           # the last stretched frame reads the columns j, j + 1 <= T


@pytest.mark.parametrize("n_fft,length", [(64, 1000), (2048, 20000)])
def test_the_literal_loop_and_the_telescoped_sum_agree(n_fft, length):
    """phi_advance and the wrap cancel out of exp(i Phi): forms (a) and (b) of the restatement, both float64, agree to 1e-7 of peak."""
    x = pref.broadband(length, 44100, seed=n_fft)
    for n_steps in (3, -4):
        _, o, n = pref.plan(44100, n_steps)
        a = pref.time_stretch(x, o, n, n_fft, form="literal")
        b = pref.time_stretch(x, o, n, n_fft, form="telescoped")
        assert a.shape == b.shape == (pref.stretched_length(length, o, n),)
        err = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"n_fft = {n_fft}, L = {length}, n_steps = {n_steps}: literal vs telescoped {err:.2e} of peak")
        assert err <= 1e-7


def test_the_restatement_shifts_a_sine_and_keeps_the_length():
    sr, L, k0 = 44100, 16384, 64
    f0 = k0 * sr / 2048
    x = np.sin(2 * np.pi * f0 * np.arange(L) / sr)
    y = pref.pitch_shift(x, sr, 3)
    orig, _, _ = pref.plan(sr, 3)
    assert y.shape == (L,)
    mid = y[L // 4:L // 4 + L // 2] * np.hanning(L // 2)
    peak = np.argmax(np.abs(np.fft.rfft(mid))) * sr / (L // 2)
    assert abs(peak - f0 * orig / sr) <= sr / (L // 2)
    assert np.array_equal(pref.pitch_shift(x, sr, 0), x)


@pytest.mark.parametrize("kwargs,field,status", [
    (dict(sr=0), "sample_rate", _lib.FV_ERR_INVALID), (dict(n_steps=float("nan")), "n_steps", _lib.FV_ERR_INVALID),
    (dict(n_steps=float("inf")), "n_steps", _lib.FV_ERR_INVALID), (dict(n_steps=400.0), "n_steps", _lib.FV_ERR_INVALID),
    (dict(bpo=0), "bins_per_octave", _lib.FV_ERR_INVALID), (dict(n_fft=1), "n_fft", _lib.FV_ERR_INVALID),
    (dict(hop=-1), "hop_length", _lib.FV_ERR_INVALID), (dict(gran=0), "freq_granularity", _lib.FV_ERR_INVALID),
    (dict(n_steps=-12.0, sr=100, gran=100), "freq_granularity", _lib.FV_ERR_INVALID),
    (dict(n_fft=2048, hop=500), "n_fft = 2048 and hop_length = 500", _lib.FV_ERR_UNSUPPORTED),
    (dict(n_fft=30, hop=15), "n_fft = 30 and hop_length = 15", _lib.FV_ERR_UNSUPPORTED),
    (dict(n_fft=6, hop=0), "n_fft = 6 and hop_length = 1", _lib.FV_ERR_UNSUPPORTED)])
def test_config_errors_name_the_field(kwargs, field, status):
    L = _lib.lib()
    c = _cfg(**kwargs)
    of = ctypes.c_int32()
    h = ctypes.c_void_p()
    for st in (L.fv_pitch_shift_plan(ctypes.byref(c), ctypes.byref(of), None, None),
               L.fv_pitch_shift_lengths(ctypes.byref(c), 100, None, None, None, None), L.fv_pitch_shift_create(ctypes.byref(c), ctypes.byref(h))):
        assert st == status and field in L.fv_last_error().decode(), L.fv_last_error().decode()
    assert h.value is None


@pytest.mark.parametrize("kwargs,field", [(dict(lpw=0), "lowpass_filter_width"), (dict(rolloff=0.0), "rolloff"), (dict(method=7), "method"),
                                          (dict(beta=float("nan")), "beta")])
def test_create_refuses_a_bad_filter_before_it_allocates(kwargs, field):
    L = _lib.lib()
    c = _cfg(**kwargs)
    h = ctypes.c_void_p()
    assert L.fv_pitch_shift_create(ctypes.byref(c), ctypes.byref(h)) == _lib.FV_ERR_INVALID
    assert field in L.fv_last_error().decode() and h.value is None


def test_null_arguments_and_lengths_out_of_range():
    L = _lib.lib()
    assert L.fv_pitch_shift_plan(None, None, None, None) == _lib.FV_ERR_INVALID
    assert L.fv_pitch_shift_create(ctypes.byref(_cfg()), None) == _lib.FV_ERR_INVALID
    assert L.fv_pitch_shift_lengths(ctypes.byref(_cfg()), -1, None, None, None, None) == _lib.FV_ERR_INVALID
    assert L.fv_pitch_shift_workspace_bytes(None, 1, 100) == 0
    assert L.fv_pitch_shift_forward(None, None, 0, None, 0, 1, 100, None, 0, None) == _lib.FV_ERR_INVALID
    L.fv_pitch_shift_destroy(None)
    with pytest.raises(ValueError, match="n_fft"):
        ps.PitchShift(44100, 3, n_fft=2048, hop_length=500)
    with pytest.raises(ValueError, match="n_steps"):
        ps.PitchShift(44100, float("nan"))


@pytest.mark.parametrize("kwargs,field", [(dict(orig_freq=0), "orig_freq"), (dict(lowpass_filter_width=0), "lowpass_filter_width"),
                                          (dict(rolloff=1.5), "rolloff"), (dict(method=7), "method")])
def test_the_global_resampler_takes_its_design_from_fv_resample_design(kwargs, field):
    """fv_global_resample_create runs the design of fv_resample_design (the same function, named in the message) before it touches the device:
    a config that the design refuses is refused in the same words.  That the uploaded table IS that design is checked on the GPU (impulses
    return the designed taps bit for bit, test_gpu_pitch_shift.py)."""
    L = _lib.lib()
    args = dict(orig_freq=44101, new_freq=48000, lowpass_filter_width=6, rolloff=0.99, method=0, beta=0.0)
    args.update(kwargs)
    c = _lib.ResampleConfig(*(args[k] for k in ("orig_freq", "new_freq", "lowpass_filter_width", "rolloff", "method", "beta")))
    h = ctypes.c_void_p()
    assert L.fv_global_resample_create(ctypes.byref(c), ctypes.byref(h)) == _lib.FV_ERR_INVALID
    msg = L.fv_last_error().decode()
    o, n, w, kp = (ctypes.c_int32() for _ in range(4))
    assert L.fv_resample_design(ctypes.byref(c), ctypes.byref(o), ctypes.byref(n), ctypes.byref(w), ctypes.byref(kp), None, None, 0, None,
                                0) == _lib.FV_ERR_INVALID
    assert field in msg and msg.replace("fv_global_resample_create", "fv_resample_design") == L.fv_last_error().decode()
    assert L.fv_global_resample_create(ctypes.byref(c), None) == _lib.FV_ERR_INVALID
    with pytest.raises(ValueError, match="table"):
        rs.Resample(44100, 48000, table="hbm")
    # the pair the LDS form refuses has a design: 48000 phases of 13 taps
    d = rs.native_design(44101, 48000)
    assert (d.o, d.n, d.kp) == (44101, 48000, 13) and d.n * d.kp > 7000


@pytest.mark.gpu   # (a handle holds device tables: the sizes are host arithmetic, but only a created shifter answers)
@pytest.mark.parametrize("n_fft,hop,B,L,max_chunk", [(64, 16, 3, 1000, 100), (2048, 512, 2, 20000, 4096)])
def test_workspace_sizes_are_the_closed_forms_of_the_one_layout(n_fft, hop, B, L, max_chunk):
    """One layout function serves the whole-row call and the stream (fv_pitch_shift::carve): parts [Yp (B, hop, nA + taps - 1) | Sp (B, 2 nb, nA) |
    Mg (B, nb, nA + 2) | Th (same) | S2 (B, 2 nb, nS) | Fr (B, N, nS) | St (B, nY) | Rs (B, nR)], each rounded up to 64 floats, the sum to 256
    bytes.  A whole-row call has (nA, nS, nY, nR) = (T, T', Ls, 0), a stream the most of one call as fv_pv_stream_create states them."""
    import torch
    lib = _lib.lib()
    shift = ps.PitchShift(44100, 3, n_fft=n_fft, hop_length=hop)
    _, o, n = shift.plan()
    nb, taps = n_fft // 2 + 1, n_fft // hop

    def up(v):
        return (v + 63) // 64 * 64

    def closed_form(nA, nS, nY, nR):
        elems = (up(B * hop * (nA + taps - 1)) + up(B * 2 * nb * nA) + 2 * up(B * nb * (nA + 2)) + up(B * 2 * nb * nS) + up(B * n_fft * nS)
                 + up(B * nY) + up(B * nR))
        return (elems * 4 + 255) // 256 * 256

    dev = torch.device("cuda", 0)
    T, Tout, Ls, _ = shift.lengths(L)
    assert int(lib.fv_pitch_shift_workspace_bytes(shift._handle(dev), B, L)) == closed_form(T, Tout, Ls, 0)
    kp = shift.resample_design().kp
    maxA = max(max_chunk // hop + 1, n_fft // (2 * hop) + 2)
    maxS = ((maxA + 1) * o + n - 1) // n + 2
    maxY = maxS * hop + n_fft
    maxR = ((maxY + 2 * kp + 2) * n + o - 1) // o + 8
    with shift.stream(B, max_chunk) as st:
        assert int(lib.fv_pv_stream_workspace_bytes(st._h)) == closed_form(maxA, maxS, maxY, maxR)
    shift.close()
