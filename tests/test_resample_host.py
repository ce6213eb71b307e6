"""CPU: the resampler's filter design (fv_resample_design, pure host code) against the float64 restatement, the restatement against scipy, the
streaming rule (vocoder_amd.resample), the C declarations / bindings / ABI, and the validation of the config and of the CLI's new options."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest

from resample_reference import Filter
from vocoder_amd import _lib
from vocoder_amd import resample as rs

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RESAMPLE_API = ("fv_resample_design", "fv_resample_input_tile", "fv_resample_create", "fv_resample_destroy", "fv_resample_output_length",
                "fv_resample_forward", "fv_resample_check_lengths", "fv_resample_stream_create", "fv_resample_stream_pending",
                "fv_resample_stream_push", "fv_resample_stream_flush", "fv_resample_stream_reset", "fv_resample_stream_destroy")
HANN, KAISER = "sinc_interp_hann", "sinc_interp_kaiser"
# the issue's table (rates, Kp), then three small coprime pairs and one kaiser case
TABLE = [(44100, 48000, 13), (24000, 44100, 13), (44100, 24000, 23), (44100, 16000, 34), (46700, 44100, 13), (48000, 8000, 73), (2, 1, 25)]
CASES = [(a, b, HANN) for a, b, _ in TABLE] + [(3, 2, HANN), (2, 3, HANN), (7, 5, HANN), (44100, 48000, KAISER)]


@pytest.mark.parametrize("orig,new,method", [(44100, 48000, HANN), (24000, 44100, HANN), (44100, 24000, HANN), (44100, 16000, HANN),
                                             (48000, 8000, HANN), (2, 1, HANN), (3, 2, HANN), (2, 3, HANN), (7, 5, HANN), (44100, 48000, KAISER)])
def test_restatement_matches_scipy_upfirdn_of_the_prototype(orig, new, method):
    """y[m] = sum_i G[m o - i n] x[i] with the prototype G[k] = g(k / (o n)): zero-stuff by n, filter with G, keep every o-th sample."""
    from scipy.signal import upfirdn
    ref = Filter(orig, new, resampling_method=method)
    o, n, lpw = ref.o, ref.n, ref.lpw
    N0 = int(math.ceil(lpw * o * n / ref.base / o)) * o + o                   # centre of the prototype: a multiple of o past its support
    k = np.arange(-N0, N0 + 1, dtype=np.float64)
    t_raw = k / (o * n) * ref.base
    t = np.clip(t_raw, -lpw, lpw)
    if method == HANN:
        win = np.cos(t * math.pi / lpw / 2) ** 2
    else:
        win = np.i0(14.769656459379492 * np.sqrt(1 - (t / lpw) ** 2)) / np.i0(14.769656459379492)
    tp = t * math.pi
    safe = np.where(tp == 0, 1.0, tp)
    G = np.where(tp == 0, 1.0, np.sin(safe) / safe) * win * (ref.base / o)
    x = np.random.default_rng(orig + new).uniform(-1, 1, size=3 * o + 5)
    full = upfirdn(G, x, up=n, down=1)
    want = full[N0::o][:ref.output_length(len(x))]
    got = ref(x)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    print(f"{orig} -> {new} {method}: restatement vs upfirdn max|d| = {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("orig,new,method", CASES)
def test_design_matches_the_restatement(orig, new, method):
    """o, n, width, Kp, first[] equal; every tap within 1 fp32 ulp of the rounded float64 value; the dense row is zero outside the band.

    Outside the band the hann window is cos^2(pi / 2) = 4e-33 in float64 and the tap rounds to 0.0f exactly.  The kaiser window at the clamp is
    1 / I0(beta) = 3e-7, not 0, so the dense tap there is sinc(lpw) / I0(beta) * base / o with sin(pi lpw) = 7e-16 in float64 — rounding noise
    of order 1e-22, which fp32 represents: there the check is |h| <= 2^-50 (2^-26 of an fp32 ulp of the largest tap, far below the parity
    bound), not == 0.0f."""
    ref = Filter(orig, new, resampling_method=method)
    d = rs.native_design(orig, new, resampling_method=method)
    assert (d.o, d.n, d.width, d.kp) == (ref.o, ref.n, ref.width, ref.kp)
    assert list(d.first) == ref.first.tolist() and list(d.count) == ref.count.tolist()
    h32 = ref.h.astype(np.float32)
    for p in range(ref.n):
        a, c = int(ref.first[p]), int(ref.count[p])
        want = h32[p, a:a + c]
        got = d.taps[p, :c]
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (p, int(ulps.max()))
        assert not d.taps[p, c:].any()
        outside = np.concatenate([ref.h[p, :a], ref.h[p, a + c:]])
        if method == HANN:
            assert not outside.astype(np.float32).any(), p
        else:
            assert np.abs(outside).max() <= 2.0 ** -50, p
    py = rs.design(orig, new, resampling_method=method)        # the plain-Python design: the same bands, the same taps within an ulp
    assert (py.o, py.n, py.width, py.kp, py.first, py.count) == (d.o, d.n, d.width, d.kp, d.first, d.count)
    assert np.abs(py.taps.view(np.int32).astype(np.int64) - d.taps.view(np.int32).astype(np.int64)).max() <= 1


@pytest.mark.parametrize("orig,new,kp", TABLE)
def test_band_lengths_of_the_documented_pairs(orig, new, kp):
    d = rs.native_design(orig, new)
    assert d.kp == kp
    assert 2 * d.n + d.n * (d.kp | 1) + _lib.resample_input_tile() + d.kp + 6 <= 64 * 1024 // 4      # every documented pair fits the LDS budget


@pytest.mark.parametrize("orig,new,method", CASES)
def test_emission_rule_against_brute_force(orig, new, method):
    ref = Filter(orig, new, resampling_method=method)
    d = rs.design(orig, new, resampling_method=method)
    o, n, width = d.o, d.n, d.width
    top = 3 * o + 2 * width
    ends = [ref.band_end(m) for m in range(n * (top // o + 2))]
    assert ends == sorted(ends)
    prev = 0
    for N in range(top + 1):
        want = sum(1 for e in ends if e <= N)
        got = d.emit_count(N)
        assert got == want, (N, got, want)
        assert prev <= got <= d.output_length(N)
        prev = got
    for m in (0, 1, n - 1, n, 2 * n + 1):
        f, p = divmod(m, n)
        assert d.first_input(m) == f * o + int(ref.first[p]) - width
        assert d.first_input(m) + d.count[p] == ref.band_end(m)
    rng = random.Random(orig * 7 + new)
    for L in (0, 1, o - 1, o, o + 1, 5 * o + 3):
        for chunk in (1, 7, o, o + 1, None):
            N = E = 0
            while N < L:
                c = min(L - N, chunk if chunk else rng.randint(1, 2 * o))
                N += c
                k = d.emit_count(N) - E
                assert k >= 0
                E += k
            tail = d.output_length(L) - E
            assert tail >= 0 and E + tail == -((-n * L) // o)


def test_entry_points_are_declared_listed_exported_and_the_abi_stays_5():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in RESAMPLE_API:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert {d for d in declared if d.startswith("fv_resample")} == set(RESAMPLE_API)
    assert "#define FV_ABI_VERSION 5" in hdr and _lib.FV_ABI_VERSION == 5 and L.fv_abi_version() == 5
    assert _lib.resample_input_tile() >= 64


def test_config_mirror_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    body = re.search(r"typedef struct fv_resample_config \{(.*?)\} fv_resample_config;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+(\w+);", body, re.M)
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.ResampleConfig._fields_)
    # C layout of {i32, i32, i32, f64, i32, f64}: 12 bytes, pad to 16, 8, 4, pad to 32, 8
    assert ctypes.sizeof(_lib.ResampleConfig) == 40
    assert _lib.ResampleConfig.rolloff.offset == 16 and _lib.ResampleConfig.method.offset == 24 and _lib.ResampleConfig.beta.offset == 32


@pytest.mark.parametrize("kwargs,field", [
    (dict(orig_freq=0), "orig_freq"), (dict(orig_freq=-5), "orig_freq"), (dict(new_freq=0), "new_freq"),
    (dict(lowpass_filter_width=0), "lowpass_filter_width"), (dict(rolloff=0.0), "rolloff"), (dict(rolloff=1.5), "rolloff"),
    (dict(rolloff=float("nan")), "rolloff"), (dict(resampling_method=7), "method")])
def test_config_validation_names_the_field(kwargs, field):
    args = dict(orig_freq=44100, new_freq=48000, lowpass_filter_width=6, rolloff=0.99, resampling_method=HANN, beta=None)
    args.update(kwargs)
    with pytest.raises(_lib.FishVocError) as ei:
        rs.native_design(**args)
    assert ei.value.status == _lib.FV_ERR_INVALID
    assert field in str(ei.value)
    rs.native_design(44100, 48000, rolloff=1.0)      # the closed end of (0, 1] is valid


def test_design_reports_short_buffers():
    L = _lib.lib()
    cfg = _lib.ResampleConfig(44100, 48000, 6, 0.99, 0, 0.0)
    o, n, w, kp = (ctypes.c_int32() for _ in range(4))
    first = (ctypes.c_int32 * 8)()
    assert L.fv_resample_design(ctypes.byref(cfg), ctypes.byref(o), ctypes.byref(n), ctypes.byref(w), ctypes.byref(kp), first, None, 8, None,
                                0) == _lib.FV_ERR_INVALID
    assert b"160 phases" in L.fv_last_error()
    assert (o.value, n.value, w.value, kp.value) == (147, 160, 7, 13)


@pytest.mark.parametrize("extra", [["--batch-size", "2"], ["--chunk-frames", "8", "--sessions", "2"]])
def test_cli_refuses_output_rate_with_batched_modes(extra, capsys):
    from vocoder_amd import inference
    with pytest.raises(SystemExit):
        inference.main(["--ckpt-path", "none.ckpt", "--input-path", "in", "--output-path", "out", "--output-rate", "48000"] + extra)
    assert "--output-rate" in capsys.readouterr().err


def test_cli_refuses_a_non_positive_output_rate(capsys):
    from vocoder_amd import inference
    with pytest.raises(SystemExit):
        inference.main(["--ckpt-path", "none.ckpt", "--input-path", "in", "--output-path", "out", "--output-rate", "0"])
    assert "--output-rate" in capsys.readouterr().err
