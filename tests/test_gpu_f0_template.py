"""GPU: the F0 tracker and the pitch template (vocoder_amd/csrc/f0_template.hip) through ``vocoder_amd.f0`` and the command line.

Parity is against the float64 restatement (f0_reference.py), computed once per configuration and shared.  The bars: |d| <= 1e-4 on the
aperiodicity and relative 1e-4 on the F0 of voiced frames — the project's parity bar; the direct form's own bound is Wi * 2^-24, about 5e-5 —
and 2e-6 on the template at amplitude 1 (the phase to fp32 costs 2 pi * 2^-25 = 1.9e-7 rad, plus a few ulp of the sine, times five).  A frame
is compared on F0 only if the restatement picks the same lag at threshold * (1 +- 1e-3) as at the threshold; at most 2 % may be left out.
Rows are strided views with NaN beside them: a NaN in the output means padding was read.  Each case prints what it measured.

Measured on an MI355X (profiles/LOG.md, the F0-template entry): see there."""
import functools

import numpy as np
import pytest
import torch

import f0_reference as fref
from vocoder_amd import f0 as f0mod

pytestmark = pytest.mark.gpu

BAR, TEMPLATE_BAR = 1e-4, 2e-6
# (sr, W, hop, fmin, fmax, L): tau_max + 1 and Wi are no multiples of 64 (161 / 351, 267 / 757); the production plan has 1103 lags
CONFIGS = [(8000, 512, 128, 50.0, 500.0, 16000), (16000, 1024, 256, 60.0, 800.0, 16000), (44100, 2048, 512, 40.0, 1100.0, 11025)]


def _strided(x: np.ndarray, extra: int = 5, fill: float = float("nan")) -> torch.Tensor:
    """(B, L) on the device as a view of a wider tensor (row stride L + extra); the columns beside it hold ``fill``."""
    B, L = x.shape
    big = torch.full((B, L + extra), fill, dtype=torch.float32, device="cuda")
    big[:, :L] = torch.from_numpy(x)
    return big[:, :L]


def _bits(a) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _case(i):
    """The signal of configuration i, its tracker and the restatement's result."""
    sr, W, hop, fmin, fmax, L = CONFIGS[i]
    x, _, kind = fref.glide(L, sr, seed=1)
    ref = fref.yin(x, sr, hop, W, fmin, fmax)
    return x, kind, ref, f0mod.YinF0(sr, hop, W, fmin, fmax)


@pytest.mark.parametrize("i", range(len(CONFIGS)))
def test_yin_parity_with_the_float64_restatement(i):
    sr, W, hop, fmin, fmax, L = CONFIGS[i]
    x, kind, ref, mod = _case(i)
    f0, ap = mod(_strided(x[None]))
    assert tuple(f0.shape) == tuple(ap.shape) == (1, L // hop)
    f0, ap = f0.cpu().numpy()[0].astype(np.float64), ap.cpu().numpy()[0].astype(np.float64)
    assert np.isfinite(f0).all() and np.isfinite(ap).all()
    T = L // hop
    d_ap = float(np.abs(ap - ref["aperiodicity"]).max())
    compared = ref["stable"]
    left_out = int((~compared).sum())
    voiced = ref["lag"] > 0
    both = compared & voiced
    d_f0 = float(np.abs(f0[both] / ref["f0"][both] - 1.0).max())
    print(f"sr = {sr}, W = {W}, hop = {hop}: {T} frames, {int(voiced.sum())} voiced, {left_out} left out; max|d aperiodicity| = {d_ap:.2e}, "
          f"max rel|d f0| = {d_f0:.2e}")
    assert left_out <= 0.02 * T
    assert np.array_equal(f0[compared] > 0, voiced[compared])          # the voiced / unvoiced pattern, frame for frame
    assert d_ap <= BAR and d_f0 <= BAR
    assert both.sum() >= 6
    # the silent stretch and the noise-only stretch: unvoiced and finite
    for t in range(T):
        lo = t * hop + hop // 2 - W // 2
        if (kind[max(lo, 0):lo + W] != 0).all():
            assert f0[t] == 0.0 and np.isfinite(ap[t]), t
        if (kind[max(lo, 0):lo + W] == 1).all():
            assert ap[t] == 1.0, t      # silence: the running sum is 0, d' = 1


@pytest.mark.parametrize("i", range(len(CONFIGS)))
def test_ragged_rows_equal_the_rows_alone_bit_for_bit(i):
    """Lengths {L, 9001, 130, 0} in one call: every row's F0, aperiodicity and template are the bits of the row run alone, exact zeros follow
    them, and NaN in every padded sample and every padded F0 frame changes nothing."""
    sr, W, hop, fmin, fmax, L = CONFIGS[i]
    x, _, _, mod = _case(i)
    lengths = [L, 9001, 130, 0]
    rows = np.stack([np.roll(x, 37 * b) for b in range(4)])
    clean, dirty = rows.copy(), rows.copy()
    for b, n in enumerate(lengths):
        clean[b, n:] = 0.25
        dirty[b, n:] = np.nan
    osc = f0mod.PitchTemplate(sr, hop)
    f0c, apc = mod.forward_ragged(_strided(clean), lengths)
    f0d, apd = mod.forward_ragged(_strided(dirty), lengths)
    assert np.array_equal(_bits(f0c), _bits(f0d)) and np.array_equal(_bits(apc), _bits(apd))
    frames = [n // hop for n in lengths]
    T = L // hop
    tc = osc.forward_ragged(f0c, frames)
    f0n = f0d.clone()
    for b, k in enumerate(frames):
        f0n[b, k:] = float("nan")
    tn = osc.forward_ragged(f0n, frames)
    assert tuple(tc.shape) == (4, 1, T * hop) and np.array_equal(_bits(tc), _bits(tn))
    for b, (n, k) in enumerate(zip(lengths, frames)):
        f0a, apa = mod(_strided(rows[b:b + 1, :n]))
        assert tuple(f0a.shape) == (1, k)
        assert np.array_equal(_bits(f0a[0]), _bits(f0d[b, :k])) and np.array_equal(_bits(apa[0]), _bits(apd[b, :k])), b
        assert not f0d[b, k:].cpu().numpy().any() and not apd[b, k:].cpu().numpy().any()
        assert _bits(f0d[b, k:]).sum() == 0 and _bits(apd[b, k:]).sum() == 0          # +0.0, not -0.0
        ta = osc(f0a)
        assert tuple(ta.shape) == (1, 1, k * hop)
        assert np.array_equal(_bits(ta[0, 0]), _bits(tn[b, 0, :k * hop])), b
        assert _bits(tn[b, 0, k * hop:]).sum() == 0
    assert frames[0] == T and (f0d[0] > 0).any() and tn[0].abs().max() > 0.9


WIDE_LENGTHS = {0: 16000, 1: 9001, 31: 4000, 32: 700, 33: 2613}      # the other rows of the 34: a few frames each


def test_thirty_four_ragged_rows_pass_one_launchs_lengths():
    """34 rows, more than the 32 lengths one launch carries, so rows 32 and 33 ride a second launch of every kernel; their lengths differ
    from those of rows 0 and 1.  Rows 31, 32 and 33 are the bits of the rows run alone and meet the float64 restatement within the file's bars."""
    sr, W, hop, fmin, fmax, L = CONFIGS[0]
    x, _, _, mod = _case(0)
    lengths = [WIDE_LENGTHS.get(b, (130, 0, 515, 1300, 127)[b % 5]) for b in range(34)]
    rows = np.stack([np.roll(x, 37 * b) for b in range(34)])
    dirty = rows.copy()
    for b, n in enumerate(lengths):
        dirty[b, n:] = np.nan
    frames = [n // hop for n in lengths]
    assert (frames[32], frames[33]) != (frames[0], frames[1]) and min(frames[31:]) >= 5 and 0 < max(frames[2:31]) <= 10
    osc = f0mod.PitchTemplate(sr, hop)
    f0, ap = mod.forward_ragged(_strided(dirty), lengths)
    f0n = f0.clone()
    for b, k in enumerate(frames):
        f0n[b, k:] = float("nan")
    tmpl = osc.forward_ragged(f0n, frames)
    assert tuple(f0.shape) == tuple(ap.shape) == (34, L // hop) and tuple(tmpl.shape) == (34, 1, L)
    total = left_out = voiced_frames = 0
    for b in (31, 32, 33):
        n, k = lengths[b], frames[b]
        f0a, apa = mod(_strided(rows[b:b + 1, :n]))
        ta = osc(f0a)
        assert np.array_equal(_bits(f0a[0]), _bits(f0[b, :k])) and np.array_equal(_bits(apa[0]), _bits(ap[b, :k])), b
        assert np.array_equal(_bits(ta[0, 0]), _bits(tmpl[b, 0, :k * hop])), b
        assert _bits(f0[b, k:]).sum() == 0 and _bits(ap[b, k:]).sum() == 0 and _bits(tmpl[b, 0, k * hop:]).sum() == 0
        ref = fref.yin(rows[b, :n], sr, hop, W, fmin, fmax)
        g0, g1 = f0[b, :k].cpu().numpy().astype(np.float64), ap[b, :k].cpu().numpy().astype(np.float64)
        compared, voiced = ref["stable"], ref["lag"] > 0
        both = compared & voiced
        d_ap = float(np.abs(g1 - ref["aperiodicity"]).max())
        d_f0 = float(np.abs(g0[both] / ref["f0"][both] - 1.0).max()) if both.any() else 0.0
        d_t = float(np.abs(tmpl[b, 0, :k * hop].cpu().numpy().astype(np.float64) - fref.template(g0.astype(np.float32), sr, hop, "sine", 1.0)).max())
        print(f"row {b} ({n} samples, {k} frames, {int(both.sum())} voiced and compared): max|d aperiodicity| = {d_ap:.2e}, "
              f"max rel|d f0| = {d_f0:.2e}, template max|d| = {d_t:.2e}")
        assert np.array_equal(g0[compared] > 0, voiced[compared]), b
        assert d_ap <= BAR and d_f0 <= BAR and d_t <= TEMPLATE_BAR, b
        total, left_out, voiced_frames = total + k, left_out + int((~compared).sum()), voiced_frames + int(both.sum())
    assert left_out <= 0.02 * total and voiced_frames >= 6


def _template_error(sr, hop, f0, kind, amplitude=1.0, tail=None):
    """max |GPU - oscillator on the restatement's exact integer phase|, and the GPU output."""
    y = f0mod.PitchTemplate(sr, hop, kind=kind, amplitude=amplitude)(_strided(f0[None].astype(np.float32)))
    assert tuple(y.shape) == (1, 1, len(f0) * hop)
    y = y.cpu().numpy()[0, 0]
    ref = fref.template(f0.astype(np.float32), sr, hop, kind, amplitude)
    sl = slice(None) if tail is None else slice(-tail, None)
    return float(np.abs(y.astype(np.float64) - ref)[sl].max()), y


@pytest.mark.parametrize("kind", ["sine", "sawtooth"])
def test_template_parity_with_the_exact_integer_phase(kind):
    """The restatement's own F0 track of the 8 kHz case: a glide with vibrato, the silent stretch, the noise stretch, and the boundaries
    between them, where the hold rule decides; then a hand-made track that flips voicing every frame or two."""
    sr, _, hop = CONFIGS[0][:3]
    track = _case(0)[2]["f0"]
    assert (track > 0).any() and (track == 0).any()
    err, y = _template_error(sr, hop, track, kind)
    _, _, voiced = fref.phase(track.astype(np.float32), sr, hop)
    print(f"{kind} template, {len(track)} frames of {hop}: max|d| = {err:.2e}")
    assert err <= TEMPLATE_BAR
    assert not y[~voiced].any() and np.abs(y[voiced]).max() > 0.99          # unvoiced samples are exactly 0
    flips = np.array([0, 200, 0, 0, 310.5, 320, 0, 150, 150, 0, -1, np.nan, 9000, 99.9, 0, 0, 440], dtype=np.float64)
    err2, y2 = _template_error(sr, hop, flips, kind, amplitude=0.5)
    _, inc, voiced2 = fref.phase(flips.astype(np.float32), sr, hop)
    print(f"{kind} template, voicing flips: max|d| = {err2:.2e}")
    assert err2 <= TEMPLATE_BAR * 0.5 + 1e-12 and not y2[~voiced2].any()
    assert (inc[hop // 2:hop + hop // 2] == inc[hop + hop // 2]).all() and inc[hop + hop // 2] != 0      # frame 0 unvoiced: frame 1's value is held


def test_no_drift_over_a_long_row():
    """2^20 samples at a constant 440.1 Hz: the last 1000 samples against the exact phase.  An fp32 accumulator of radians is off by
    about 1e-2 here; the integer phase is as close as at the row's start."""
    sr, hop, N = 44100, 512, 1 << 20
    f0 = np.full(N // hop, 440.1)
    err, _ = _template_error(sr, hop, f0, "sine", tail=1000)
    err_all, _ = _template_error(sr, hop, f0, "sawtooth")
    print(f"drift, 2^20 samples at 440.1 Hz: last 1000 samples max|d| = {err:.2e}; sawtooth over the whole row {err_all:.2e}")
    assert err <= TEMPLATE_BAR and err_all <= TEMPLATE_BAR


def test_template_from_audio_chains_the_two_and_errors_of_the_device_calls():
    import ctypes
    from vocoder_amd import _lib
    sr, W, hop, fmin, fmax, L = CONFIGS[0]
    x, _, _, mod = _case(0)
    xd = _strided(np.stack([x, x[::-1].copy()]))[:, None]                 # (2, 1, L): leading dimensions are rows
    t = f0mod.template_from_audio(xd, sr, hop, W, fmin, fmax)
    f0, _ = mod(xd)
    assert tuple(f0.shape) == (2, 1, L // hop) and tuple(t.shape) == (2, 1, 1, (L // hop) * hop)
    assert np.array_equal(_bits(t), _bits(f0mod.PitchTemplate(sr, hop)(f0)))
    lib = _lib.lib()
    h = mod._handle(xd.device)
    out = torch.zeros((2, 2, L // hop), dtype=torch.float32, device="cuda")
    flat = xd.reshape(2, L) if xd.is_contiguous() else xd[:, 0]
    args = (out[0].data_ptr(), out[1].data_ptr(), L // hop, 2, L, None, 0, None)
    bad = (ctypes.c_int32 * 2)(L, L + 1)
    assert lib.fv_f0_forward(h, flat.data_ptr(), flat.stride(0), bad, *args) == _lib.FV_ERR_INVALID and "row 1" in lib.fv_last_error().decode()
    assert lib.fv_f0_forward(h, flat.data_ptr(), L - 1, None, *args) == _lib.FV_ERR_INVALID and "stride" in lib.fv_last_error().decode()
    assert lib.fv_f0_forward(h, None, flat.stride(0), None, *args) == _lib.FV_ERR_INVALID
    assert lib.fv_f0_forward(h, flat.data_ptr(), flat.stride(0), None, out[0].data_ptr(), out[1].data_ptr(), L // hop, 0, L, None, 0, None) == 0
    osc = f0mod.PitchTemplate(sr, hop)
    ht = osc._handle(xd.device)
    f = torch.zeros((2, 10), dtype=torch.float32, device="cuda")
    y = torch.zeros((2, 10 * hop), dtype=torch.float32, device="cuda")
    need = lib.fv_template_workspace_bytes(ht, 2, 10)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert lib.fv_template_forward(ht, f.data_ptr(), 10, None, y.data_ptr(), 10 * hop, 2, 10, ws.data_ptr(), need - 256, None) == _lib.FV_ERR_INVALID
    assert "workspace" in lib.fv_last_error().decode()
    assert lib.fv_template_forward(ht, f.data_ptr(), 10, (ctypes.c_int32 * 2)(3, 11), y.data_ptr(), 10 * hop, 2, 10, ws.data_ptr(), need,
                                   None) == _lib.FV_ERR_INVALID and "row 1" in lib.fv_last_error().decode()
    with pytest.raises(ValueError, match="entries"):
        mod.forward_ragged(flat, [L])
    assert tuple(osc(torch.zeros((3, 0), dtype=torch.float32, device="cuda")).shape) == (3, 1, 0)
    e0, e1 = mod(torch.zeros((2, hop - 1), dtype=torch.float32, device="cuda"))      # shorter than a hop: no frame
    assert tuple(e0.shape) == tuple(e1.shape) == (2, 0)


# ---- end to end ----

TINY = dict(hop_length=64, n_fft=256, win_length=256, num_mels=20, sampling_rate=16000)
TINY_GEN = dict(hop_length=64, num_mels=20, upsample_initial_channel=32, upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4],
                resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]], pre_conv_kernel_size=7, post_conv_kernel_size=7,
                use_template=True)


def test_cli_feeds_a_template_generator_from_a_wav(tmp_path):
    """A tiny HiFiGANGenerator(use_template=True): the command line on a .wav writes the bytes of ``module.forward(mel,
    template_from_audio(wave))`` — the template is made from the samples the mel is made from.  Under --batch-size 2, with two files of
    different lengths, it writes the bytes of ``module.forward_list(mels, templates)`` with the same templates (the one ragged call the option
    makes), which are the whole-file wavs within 1 LSB, the bar every --batch-size run has.  A mel input takes its F0 from the sidecar."""
    import yaml
    from vocoder_amd import inference, synthetic as syn
    from vocoder_amd.data.transforms import LogMelSpectrogram
    from vocoder_amd.modules.generators.hifigan import HiFiGANGenerator
    (tmp_path / "cfg" / "model" / "resolution").mkdir(parents=True)
    (tmp_path / "cfg" / "model" / "generator").mkdir(parents=True)
    (tmp_path / "cfg" / "model" / "resolution" / "tiny.yaml").write_text(yaml.safe_dump(TINY))
    (tmp_path / "cfg" / "model" / "generator" / "hifigan.yaml").write_text(
        yaml.safe_dump(dict(TINY_GEN, _target_="vocoder_amd.modules.generators.hifigan.HiFiGANGenerator")))
    sd = syn.hifigan_state_dict(TINY_GEN, 5)
    torch.save({"state_dict": {f"generator.{k}": torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "g.ckpt")
    sr, hop = TINY["sampling_rate"], TINY["hop_length"]
    (tmp_path / "in").mkdir()
    for name, n, f in (("a", 64 * 150 + 17, 150.0), ("b", 64 * 101, 211.0)):      # steady five-harmonic tones, longer than a tracker frame
        ph = 2.0 * np.pi * f * np.arange(n) / sr
        inference.write_wav(tmp_path / "in" / f"{name}.wav", 0.3 * sum(np.sin(h * ph) / h for h in range(1, 6)), sr)
    base = ["--generator", "hifigan", "--resolution", "tiny", "--config-root", str(tmp_path / "cfg"), "--ckpt-path", str(tmp_path / "g.ckpt")]
    inference.main(base + ["--input-path", str(tmp_path / "in"), "--output-path", str(tmp_path / "whole")])
    inference.main(base + ["--input-path", str(tmp_path / "in"), "--output-path", str(tmp_path / "batch"), "--batch-size", "2"])

    gen = HiFiGANGenerator(**TINY_GEN).eval()
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    gen = gen.cuda()
    front = LogMelSpectrogram(sample_rate=sr, n_fft=256, win_length=256, hop_length=hop, n_mels=20, f_min=0, f_max=sr // 2).eval().cuda()
    mels, templates, waves = [], [], []
    for name in "ab":
        wave, _ = inference.read_wav(tmp_path / "in" / f"{name}.wav")
        wave = torch.from_numpy(wave).cuda()                                 # (1, L)
        mel, template = front(wave), f0mod.template_from_audio(wave, sr, hop)
        assert template.abs().max() > 0.9                                    # the tracker found the pitch: the template is not silence
        inference.write_wav(tmp_path / "want" / f"{name}.wav", gen(mel, template).squeeze(1).cpu().numpy().T, sr)
        assert (tmp_path / "whole" / f"{name}.wav").read_bytes() == (tmp_path / "want" / f"{name}.wav").read_bytes(), name
        mels.append(mel[0])
        templates.append(template[0])
        waves.append(wave[0])
    for name, w in zip("ab", gen.forward_list(front.forward_list(waves), templates)):      # (the rows' mels through the front-end's ragged call)
        inference.write_wav(tmp_path / "want_batch" / f"{name}.wav", w.cpu().numpy().T, sr)
        assert (tmp_path / "batch" / f"{name}.wav").read_bytes() == (tmp_path / "want_batch" / f"{name}.wav").read_bytes(), name
        a, _ = inference.read_wav(tmp_path / "batch" / f"{name}.wav")
        b, _ = inference.read_wav(tmp_path / "whole" / f"{name}.wav")
        assert a.shape == b.shape and np.abs(a - b).max() <= 1.0 / 32768, name
    # the template matters: a silent template gives another wav
    quiet = gen(mels[0][None], torch.zeros_like(templates[0])[None])
    assert (quiet - gen(mels[0][None], templates[0][None])).abs().max() > 1e-3
    # a mel input: F0 from <stem>.f0.npy
    torch.save(mels[1].cpu(), tmp_path / "m.pt")
    f0, _ = f0mod.YinF0(sr, hop)(torch.from_numpy(inference.read_wav(tmp_path / "in" / "b.wav")[0]).cuda())
    np.save(tmp_path / "m.f0.npy", f0[0].cpu().numpy())
    inference.main(base + ["--input-path", str(tmp_path / "m.pt"), "--output-path", str(tmp_path / "mel")])
    assert (tmp_path / "mel" / "m.wav").read_bytes() == (tmp_path / "want" / "b.wav").read_bytes()
    np.save(tmp_path / "m.f0.npy", f0[0, :-1].cpu().numpy())
    with pytest.raises(ValueError, match="m.f0.npy"):
        inference.main(base + ["--input-path", str(tmp_path / "m.pt"), "--output-path", str(tmp_path / "mel2")])
    assert not (tmp_path / "mel2").exists()


def test_refinegan_with_a_gpu_made_template_vs_the_oracle(golden):
    """RefineGANGenerator on refinegan_tiny's weights, the template from PitchTemplate on the device and explicit noise: the oracle fed the
    same template agrees within the existing bar (1e-4 of the expected waveform's own peak)."""
    from oracle import oracle as orc
    from vocoder_amd import synthetic as syn
    from vocoder_amd.modules.generators.refinegan import RefineGANGenerator
    g = golden("refinegan_tiny.npz")
    cfg = g["cfg"]
    sd = syn.refinegan_state_dict(cfg, g["seed"])
    B, _, T = g["mel"].shape
    hop, sr = cfg["hop_length"], cfg.get("sampling_rate", 44100)
    f0 = np.stack([np.where((np.arange(T) + b) % 5 == 3, 0.0, 180.0 * (b + 1) + 9.0 * np.arange(T)) for b in range(B)]).astype(np.float32)
    template = f0mod.PitchTemplate(sr, hop, amplitude=0.3)(torch.from_numpy(f0).cuda())
    assert tuple(template.shape) == (B, 1, T * hop) and template.abs().max() > 0.05
    noise = syn.refinegan_noise(cfg, B, T, seed=11)
    ref = orc.refinegan_forward(sd, cfg, g["mel"], template.cpu().numpy(), noise)
    gen = RefineGANGenerator(**cfg).eval()
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    gen = gen.cuda()
    y = gen(torch.from_numpy(g["mel"]).cuda(), template, torch.from_numpy(np.concatenate([n.reshape(-1) for n in noise])).cuda()).cpu().numpy()
    tol = min(1e-4, 1e-4 * float(np.abs(ref).max()))
    err = float(np.abs(y - ref).max())
    print(f"RefineGAN with a GPU-made template: max|d| = {err:.2e} (bar {tol:.1e}, peak {np.abs(ref).max():.3f})")
    assert err <= tol
