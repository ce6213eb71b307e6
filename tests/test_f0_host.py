"""Host (no GPU): the F0 tracker and the pitch template (include/fishvoc.h fv_f0_*, fv_template_*) — the ABI surface, the plan stated three
times (C: fv_f0_plan; Python: vocoder_amd.f0.plan; the float64 restatement f0_reference.py), the restatement against a signal of known F0 and
against a float64 phase, and the command line's refusals."""
import argparse
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import f0_reference as fref
from vocoder_amd import _lib
from vocoder_amd import f0 as f0mod

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

F0_API = ("fv_f0_plan", "fv_f0_create", "fv_f0_destroy", "fv_f0_workspace_bytes", "fv_f0_forward")
TEMPLATE_API = ("fv_template_create", "fv_template_destroy", "fv_template_workspace_bytes", "fv_template_forward")

# (sr, W, hop, fmin, fmax, L): the GPU test's configurations (test_gpu_f0_template.py)
CONFIGS = [(8000, 512, 128, 50.0, 500.0, 16000), (16000, 1024, 256, 60.0, 800.0, 16000), (44100, 2048, 512, 40.0, 1100.0, 11025)]


def test_entry_points_are_declared_listed_exported_and_the_abi_stays_5():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in F0_API + TEMPLATE_API:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert {d for d in declared if d.startswith("fv_f0_")} == set(F0_API)
    assert {d for d in declared if d.startswith("fv_template_")} == set(TEMPLATE_API)
    assert {n for n in _lib.EXPORTS if n.startswith(("fv_f0_", "fv_template_"))} == set(F0_API + TEMPLATE_API)
    assert "#define FV_ABI_VERSION 5" in hdr and _lib.FV_ABI_VERSION == 5 and L.fv_abi_version() == 5
    # every entry says what it replaces: the CPU tracker / oscillator in front of the template generators
    for name in F0_API + TEMPLATE_API:
        at = re.search(r"FV_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr).start()
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "refinegan.py:287" in comment and "hifigan.py:226" in comment, name
    import vocoder_amd
    assert vocoder_amd.YinF0 is f0mod.YinF0 and vocoder_amd.PitchTemplate is f0mod.PitchTemplate
    assert vocoder_amd.template_from_audio is f0mod.template_from_audio


def test_config_mirrors_match_the_header():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "float": ctypes.c_float}
    for cname, mirror in (("fv_f0_config", _lib.F0Config), ("fv_template_config", _lib.TemplateConfig)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        fields = re.findall(r"^\s*(int32_t|double|float)\s+(\w+);", body, re.M)
        assert [(n, ctype[t]) for t, n in fields] == list(mirror._fields_), cname
    assert ctypes.sizeof(_lib.F0Config) == 40 and _lib.F0Config.fmin.offset == 16      # {i32 x 3, pad, f64 x 3}
    assert ctypes.sizeof(_lib.TemplateConfig) == 16
    assert (_lib.FV_TEMPLATE_SINE, _lib.FV_TEMPLATE_SAWTOOTH) == (0, 1)
    assert "FV_TEMPLATE_SINE = 0, FV_TEMPLATE_SAWTOOTH = 1" in hdr


def _c_plan(sr, W, hop, fmin, fmax, thr, L=0):
    lib = _lib.lib()
    c = _lib.F0Config(sr, W, hop, fmin, fmax, thr)
    a, b, w, fr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    st = lib.fv_f0_plan(ctypes.byref(c), L, ctypes.byref(a), ctypes.byref(b), ctypes.byref(w), ctypes.byref(fr))
    return st, (a.value, b.value, w.value), fr.value, lib.fv_last_error().decode()


def test_plan_agrees_between_c_python_and_the_restatement_over_a_grid():
    """Every (sr, W, fmin, fmax) of the grid: either all three accept and agree, or all three refuse; the grid holds each rejected case."""
    accepted = refused = 0
    for sr in (8000, 16000, 22050, 24000, 44100, 48000):
        for W in (256, 512, 1024, 2048, 4096):
            for fmin in (30.0, 40.0, 50.0, 60.0, 110.5):
                for fmax in (45.0, 500.0, 800.0, 1100.0, 30000.0):
                    st, got, _, msg = _c_plan(sr, W, 256, fmin, fmax, 0.1)
                    try:
                        want = f0mod.plan(sr, W, 256, fmin, fmax, 0.1)
                    except ValueError:
                        want = None
                    try:
                        ref = fref.plan(sr, W, 256, fmin, fmax, 0.1)
                    except ValueError:
                        ref = None
                    if st == _lib.FV_OK:
                        assert got == want == ref, (sr, W, fmin, fmax)
                        tau_min, tau_max, Wi = got
                        assert tau_max == int(sr // fmin) and tau_min == max(2, int(sr // fmax)) and Wi == W - (tau_max + 1)
                        assert tau_min < tau_max and 2 * Wi >= tau_max
                        accepted += 1
                    else:
                        assert st == _lib.FV_ERR_INVALID and want is None and ref is None, (sr, W, fmin, fmax, msg)
                        refused += 1
    assert accepted > 100 and refused > 100
    # the production defaults, and the frames of a row
    assert _c_plan(44100, 2048, 512, 40.0, 1100.0, 0.1, L=11025)[1:3] == ((40, 1102, 945), 21)
    assert f0mod.YinF0(44100, 512).plan() == (40, 1102, 945) and f0mod.YinF0(44100, 512).frames(11025) == 21


@pytest.mark.parametrize("kwargs,words", [
    (dict(fmin=600.0, fmax=500.0), ("fmin", "fmax")),                   # tau_min >= tau_max
    (dict(W=1024), ("frame_length", "fmin")),                          # Wi < tau_max / 2 (Wi = -79)
    (dict(W=1500, fmin=44.0), ("frame_length", "fmin")),               # Wi = 497 < 1002 / 2
    (dict(W=2047), ("frame_length",)),                                  # odd
    (dict(hop=0), ("hop_length",)),
    (dict(thr=0.0), ("threshold",)), (dict(thr=1.5), ("threshold",)), (dict(thr=float("nan")), ("threshold",)),
    (dict(fmin=0.0), ("fmin",)), (dict(sr=0), ("sample_rate",))])
def test_rejected_configurations_say_which_knob_to_move(kwargs, words):
    args = dict(sr=44100, W=2048, hop=512, fmin=40.0, fmax=1100.0, thr=0.1)
    args.update(kwargs)
    order = ("sr", "W", "hop", "fmin", "fmax", "thr")
    st, _, _, msg = _c_plan(*(args[k] for k in order))
    assert st == _lib.FV_ERR_INVALID and all(w in msg for w in words), msg
    h = ctypes.c_void_p()
    c = _lib.F0Config(*(args[k] for k in order))
    assert _lib.lib().fv_f0_create(ctypes.byref(c), ctypes.byref(h)) == _lib.FV_ERR_INVALID and h.value is None
    with pytest.raises(ValueError) as ei:
        f0mod.plan(*(args[k] for k in order))
    assert all(w in str(ei.value) for w in words), str(ei.value)
    with pytest.raises(ValueError):
        fref.plan(*(args[k] for k in order))


def test_null_arguments_and_template_config_errors():
    L = _lib.lib()
    assert L.fv_f0_plan(None, 0, None, None, None, None) == _lib.FV_ERR_INVALID
    assert L.fv_f0_plan(ctypes.byref(_lib.F0Config(44100, 2048, 512, 40.0, 1100.0, 0.1)), -1, None, None, None, None) == _lib.FV_ERR_INVALID
    assert L.fv_f0_create(ctypes.byref(_lib.F0Config(44100, 2048, 512, 40.0, 1100.0, 0.1)), None) == _lib.FV_ERR_INVALID
    assert L.fv_f0_forward(None, None, 0, None, None, None, 0, 1, 100, None, 0, None) == _lib.FV_ERR_INVALID
    assert L.fv_template_forward(None, None, 0, None, None, 0, 1, 100, None, 0, None) == _lib.FV_ERR_INVALID
    assert L.fv_f0_workspace_bytes(None, 1, 100) == 0 and L.fv_template_workspace_bytes(None, 1, 100) == 0
    L.fv_f0_destroy(None)
    L.fv_template_destroy(None)
    h = ctypes.c_void_p()
    big = _lib.F0Config(44100, 8192, 512, 40.0, 1100.0, 0.1)      # a valid plan, but more than one workgroup stages
    assert L.fv_f0_create(ctypes.byref(big), ctypes.byref(h)) == _lib.FV_ERR_UNSUPPORTED and "frame_length" in L.fv_last_error().decode()
    for cfg, word in ((_lib.TemplateConfig(0, 512, 0, 1.0), "sample_rate"), (_lib.TemplateConfig(44100, 0, 0, 1.0), "hop_length"),
                      (_lib.TemplateConfig(44100, 512, 2, 1.0), "kind"), (_lib.TemplateConfig(44100, 512, 0, float("inf")), "amplitude")):
        assert L.fv_template_create(ctypes.byref(cfg), ctypes.byref(h)) == _lib.FV_ERR_INVALID and word in L.fv_last_error().decode()
        assert h.value is None
    assert L.fv_template_create(None, ctypes.byref(h)) == _lib.FV_ERR_INVALID
    # the handles hold no device state: they are made and sized without a GPU
    ok = _lib.TemplateConfig(44100, 512, 1, 0.5)
    _lib.check(L.fv_template_create(ctypes.byref(ok), ctypes.byref(h)))
    need = L.fv_template_workspace_bytes(h, 3, 100)
    assert need % 256 == 0 and need >= 4 * (3 * 100 + 3 * 25) and L.fv_template_workspace_bytes(h, 3, 1 << 30) == 0
    L.fv_template_destroy(h)
    with pytest.raises(ValueError, match="kind"):
        f0mod.PitchTemplate(44100, 512, kind="square")
    with pytest.raises(ValueError, match="frame_length"):
        f0mod.YinF0(44100, 512, frame_length=8192)
    with pytest.raises(ValueError, match="CUDA"):
        f0mod.YinF0(44100, 512)(torch.zeros(4096))
    with pytest.raises(ValueError, match="CUDA"):
        f0mod.PitchTemplate(44100, 512)(torch.zeros(8))


@pytest.mark.parametrize("sr,W,hop,fmin,fmax,L", CONFIGS)
def test_the_restatement_recovers_the_f0_of_a_harmonic_glide(sr, W, hop, fmin, fmax, L):
    """Within 1.5 % on every frame whose window lies inside a voiced stretch.  The known F0 is read where the frame measures it: the
    difference function compares x[j] with x[j + tau] for j < Wi, the samples [lo, lo + Wi + tau) of the frame that starts at lo, so the lag it
    finds is the period at the centre of that span, lo + (Wi + tau) / 2 — not at the frame's centre (the glide moves up to 14 % across one
    44.1 kHz frame).  The silent and the noise-only stretch come out unvoiced."""
    x, f_true, kind = fref.glide(L, sr, seed=1)
    r = fref.yin(x, sr, hop, W, fmin, fmax)
    _, _, Wi = fref.plan(sr, W, hop, fmin, fmax)
    worst, n = 0.0, 0
    for t in range(L // hop):
        lo = t * hop + hop // 2 - W // 2
        if lo >= 0 and lo + W <= L and (kind[lo:lo + W] == 0).all():
            assert r["lag"][t] > 0, t
            at = lo + (Wi + int(r["lag"][t])) // 2
            worst, n = max(worst, abs(r["f0"][t] / f_true[at] - 1.0)), n + 1
        if (kind[max(lo, 0):lo + W] != 0).all():
            assert r["lag"][t] == 0 and r["f0"][t] == 0.0 and np.isfinite(r["aperiodicity"][t]), t
    print(f"sr = {sr}: {n} voiced frames, worst relative F0 error {worst:.4f}")
    assert n >= 6 and worst <= 0.015
    assert r["stable"].all()          # no frame of these signals sits on the threshold


def test_the_integer_phase_is_a_float64_cumsum_and_the_hold_rule():
    sr, hop = 16000, 64
    f0 = np.array([0.0, 0.0, 220.0, 230.5, 0.0, 441.25, 440.0, 439.0, 0.0, 0.0, 100.0, -5.0, np.nan, 16000.0, 123.456])
    phi, inc, voiced = fref.phase(f0, sr, hop)
    turns = np.cumsum(inc.astype(np.float64) / 2.0 ** 32)
    d = np.abs((phi.astype(np.float64) / 2.0 ** 32 - turns + 0.5) % 1.0 - 0.5)
    print(f"integer phase vs float64 cumsum: {d.max():.2e} turns over {len(phi)} samples")
    assert d.max() <= 1e-9
    F = fref.increments(f0, sr)
    assert list(F != 0) == [False, False, True, True, False, True, True, True, False, False, True, False, False, False, True]
    assert F[2] == round(220.0 / sr * 2 ** 32)
    # exactly one neighbour unvoiced: the voiced one's value is held; both unvoiced: 0; both voiced: between the two, exact at the centres
    assert (inc[: hop + hop // 2] == 0).all()                                       # frames 0, 1 and the first half of the gap to frame 2
    assert (inc[hop + hop // 2: 2 * hop + hop // 2] == F[2]).all()                   # centre 1 (unvoiced) -> centre 2: held
    assert inc[2 * hop + hop // 2] == F[2] and inc[3 * hop + hop // 2] == F[3]
    mid = inc[2 * hop + hop // 2: 3 * hop + hop // 2].astype(np.int64)
    assert (np.diff(mid) >= 0).all() and mid[hop // 2] == (int(F[2]) * (hop // 2) + int(F[3]) * (hop // 2)) // hop
    assert (inc[3 * hop + hop // 2: 4 * hop + hop // 2] == F[3]).all() and (inc[4 * hop + hop // 2: 5 * hop + hop // 2] == F[5]).all()
    assert (inc[8 * hop + hop // 2: 9 * hop + hop // 2] == 0).all()                  # both unvoiced
    assert (inc[-(hop // 2):] == F[14]).all()                                       # past the last centre: the last frame's value
    assert list(voiced[::hop]) == list(F != 0)
    out = fref.template(f0, sr, hop)
    assert (out[~voiced] == 0.0).all() and np.abs(out[voiced]).max() > 0.9
    # a row's own frames: the rest of f0 is not read
    f0n = f0.copy()
    f0n[9:] = np.nan
    a, b = fref.template(f0, sr, hop, frames=9), fref.template(f0n, sr, hop, frames=9)
    assert np.array_equal(a, b) and np.array_equal(a[: 9 * hop], fref.template(f0[:9], sr, hop)) and not a[9 * hop:].any()


# ---- the command line ----

TINY = dict(hop_length=64, n_fft=256, win_length=256, num_mels=20, sampling_rate=16000)
TINY_GEN = dict(hop_length=64, num_mels=20, upsample_initial_channel=32, upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4],
                resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]], pre_conv_kernel_size=7, post_conv_kernel_size=7,
                use_template=True)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    import yaml
    from vocoder_amd import synthetic as syn
    root = tmp_path_factory.mktemp("tiny_template")
    (root / "cfg" / "model" / "resolution").mkdir(parents=True)
    (root / "cfg" / "model" / "generator").mkdir(parents=True)
    (root / "cfg" / "model" / "resolution" / "tiny.yaml").write_text(yaml.safe_dump(TINY))
    (root / "cfg" / "model" / "generator" / "hifigan.yaml").write_text(
        yaml.safe_dump(dict(TINY_GEN, _target_="vocoder_amd.modules.generators.hifigan.HiFiGANGenerator")))
    sd = syn.hifigan_state_dict(TINY_GEN, 5)
    torch.save({"state_dict": {f"generator.{k}": torch.from_numpy(v) for k, v in sd.items()}}, root / "g.ckpt")
    torch.save(torch.zeros(20, 12), root / "m.pt")
    return root, ["--generator", "hifigan", "--resolution", "tiny", "--config-root", str(root / "cfg"), "--ckpt-path", str(root / "g.ckpt")]


def test_cli_refuses_streaming_a_template_generator_before_it_touches_the_gpu(tiny):
    from vocoder_amd import inference
    root, base = tiny
    for extra in (["--chunk-frames", "8"], ["--chunk-frames", "8", "--sessions", "2"]):
        with pytest.raises(ValueError, match="no streaming form yet"):
            inference.main(base + ["--input-path", str(root / "m.pt"), "--output-path", str(root / "o")] + extra)
    assert not (root / "o").exists()
    with pytest.raises(SystemExit):      # the new flags are parsed: a kind that does not exist is argparse's error
        inference.main(base + ["--input-path", str(root / "m.pt"), "--output-path", str(root / "o"), "--template-kind", "square"])


def test_cli_sidecar_errors_name_the_file(tiny):
    from vocoder_amd import inference
    from vocoder_amd.modules.generators.hifigan import HiFiGANGenerator
    root, _ = tiny
    gen = HiFiGANGenerator(**TINY_GEN)
    assert inference.takes_template(gen) and not inference.takes_template(HiFiGANGenerator(**dict(TINY_GEN, use_template=False)))
    model = types.SimpleNamespace(generator=gen, sampling_rate=16000, hop_length=64, device=torch.device("cpu"))
    a = argparse.Namespace(template_kind="sine")
    mel = torch.zeros(1, 20, 12)
    with pytest.raises(ValueError) as ei:
        inference._sidecar_template(a, model, root / "m.pt", mel)
    assert str(root / "m.f0.npy") in str(ei.value) and "missing" in str(ei.value)
    np.save(root / "m.f0.npy", np.zeros(11, dtype=np.float32))
    with pytest.raises(ValueError) as ei:
        inference._sidecar_template(a, model, root / "m.pt", mel)
    assert str(root / "m.f0.npy") in str(ei.value) and "12 frames" in str(ei.value) and "(11,)" in str(ei.value)
    np.save(root / "m.f0.npy", np.zeros((2, 12), dtype=np.float32))      # two rows of F0 for a mel of one item
    with pytest.raises(ValueError, match="m.f0.npy"):
        inference._sidecar_template(a, model, root / "m.pt", mel)
