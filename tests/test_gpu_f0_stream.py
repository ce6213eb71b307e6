"""GPU: the streaming F0 tracker and pitch template (fv_yin_stream_*, fv_osc_stream_* in vocoder_amd/csrc/f0_template.hip) through
``vocoder_amd.f0`` and the wav -> wav chain of ``vocoder_amd.inference``.

Every comparison against the whole-row GPU result is on bits: a YIN frame's bits depend on the plan alone and the oscillator's phase is a
wrapping integer sum, so a stream has nothing to be approximately equal about.  Every pushed chunk is a strided view with NaN beside it: a NaN
in the output, or one changed bit, means a sample outside the chunk was read.  The chain's bar is the generator stream's own,
2e-5 * max(1, peak) (test_gpu_stream.py)."""
import functools

import numpy as np
import pytest
import torch

import f0_reference as fref
import f0_stream_reference as sref
from vocoder_amd import _lib
from vocoder_amd import f0 as f0mod

pytestmark = pytest.mark.gpu

# (sr, W, hop, fmin, fmax, L)
CONFIGS = [(8000, 512, 128, 50.0, 500.0, 3001), (16000, 1024, 256, 60.0, 800.0, 6001), (44100, 2048, 512, 40.0, 1100.0, 11025)]
WIDE_HOP = (8000, 512, 600, 50.0, 500.0, 3001)      # hop > W: frames do not overlap, and the stream carries more than W samples
B = 3


def _bits(a) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _strided(x: torch.Tensor, extra: int = 5) -> torch.Tensor:
    """A copy of x (B, c) as a view of a wider tensor whose other columns hold NaN."""
    big = torch.full((x.shape[0], x.shape[1] + extra), float("nan"), dtype=torch.float32, device="cuda")
    big[:, :x.shape[1]] = x
    return big[:, :x.shape[1]]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Configuration i: B rolled copies of the glide on the device, the tracker, and the whole-row GPU result (computed once, never changed)."""
    sr, W, hop, fmin, fmax, L = WIDE_HOP if i < 0 else CONFIGS[i]
    x = fref.glide(L, sr, seed=1)[0]
    rows = torch.from_numpy(np.stack([np.roll(x, 37 * b) for b in range(B)])).cuda()
    mod = f0mod.YinF0(sr, hop, W, fmin, fmax)
    f0, ap = mod(_strided(rows))
    assert tuple(f0.shape) == (B, L // hop) and int((f0[0] > 0).sum()) >= (6 if i >= 0 else 2)
    return rows, mod, _bits(f0), _bits(ap)


def _sizes(name, L, hop):
    if name == "random":
        return sref.chunk_sizes(L, np.random.default_rng(L), 3 * hop)
    c = {"one": L, "hop": hop, "37": 37, "1": 1}[name]
    return [c] * (L // c) + ([L % c] if L % c else [])


def _track(st, rows, sizes, W, hop):
    """Pushes rows in `sizes`, then flushes, checking every count against the rule; returns the concatenated (f0, ap)."""
    f0s, aps, at, E = [], [], 0, 0
    for c in sizes:
        f0, ap = st.push(_strided(rows[:, at:at + c]))
        at += c
        E2 = max(E, sref.frames_ready(at, W, hop))
        assert tuple(f0.shape) == tuple(ap.shape) == (rows.shape[0], E2 - E), (at, c)
        E = E2
        assert (st.received_samples, st.emitted_frames) == (at, E)
        assert st.pending_samples == sref.pending_samples(at, E, W, hop) < W // 2 + max(W // 2, (hop + 1) // 2)      # (W when hop <= W)
        f0s.append(f0), aps.append(ap)
    f0, ap = st.flush()
    assert tuple(f0.shape) == tuple(ap.shape) == (rows.shape[0], at // hop - E)
    assert st.emitted_frames == at // hop
    return torch.cat(f0s + [f0], dim=1), torch.cat(aps + [ap], dim=1)


@pytest.mark.parametrize("i,name", [(i, n) for i in range(len(CONFIGS)) for n in ("one", "hop", "37", "random")] + [(0, "1")])
def test_tracker_stream_equals_the_whole_row_forward_bit_for_bit(i, name):
    sr, W, hop, fmin, fmax, L = CONFIGS[i]
    rows, mod, f0_bits, ap_bits = _case(i)
    sizes = _sizes(name, L, hop)
    assert sum(sizes) == L and (name != "random" or 0 in sizes)
    with mod.stream(B, max(sizes)) as st:
        f0, ap = _track(st, rows, sizes, W, hop)
    assert np.array_equal(_bits(f0), f0_bits) and np.array_equal(_bits(ap), ap_bits)


@pytest.mark.parametrize("name", ["one", "37", "random"])
def test_tracker_stream_with_a_hop_above_the_frame_length(name):
    """hop = 600 > W = 512: a frame not yet emitted can start W / 2 + hop / 2 = 556 samples before N, more than W; the carry is that long."""
    sr, W, hop, fmin, fmax, L = WIDE_HOP
    rows, mod, f0_bits, ap_bits = _case(-1)
    sizes = _sizes(name, L, hop)
    with mod.stream(B, max(sizes)) as st:
        f0, ap = _track(st, rows, sizes, W, hop)
    assert tuple(f0.shape) == (B, 5) and np.array_equal(_bits(f0), f0_bits) and np.array_equal(_bits(ap), ap_bits)


def test_tracker_stream_ends_refusals_and_reset():
    sr, W, hop, fmin, fmax, L = CONFIGS[0]
    rows, mod, f0_bits, ap_bits = _case(0)
    with mod.stream(B, 4096) as st:
        f0, ap = st.flush()                                   # a flush at N = 0 emits nothing
        assert tuple(f0.shape) == tuple(ap.shape) == (B, 0)
        st.reset()
        f0, _ = st.push(_strided(rows[:, :hop - 28]))          # L < hop: no frame at all
        assert f0.shape[1] == 0 and st.flush()[0].shape[1] == 0
        st.reset()
        f0, _ = st.push(_strided(rows[:, :hop]))               # L = hop: one frame, which leaves only at the flush
        assert f0.shape[1] == 0 and st.pending_samples == hop
        f0, ap = st.flush()
        w0, w1 = mod(_strided(rows[:, :hop]))
        assert tuple(f0.shape) == (B, 1) and np.array_equal(_bits(f0), _bits(w0)) and np.array_equal(_bits(ap), _bits(w1))
        # a push after a flush is refused and changes nothing
        before = (st.received_samples, st.emitted_frames, st.pending_samples)
        with pytest.raises(_lib.FishVocError) as ei:
            st.push(_strided(rows[:, :hop]))
        assert ei.value.status == _lib.FV_ERR_STATE and "fv_yin_stream_reset" in str(ei.value)
        with pytest.raises(_lib.FishVocError) as ei:
            st.flush()
        assert ei.value.status == _lib.FV_ERR_STATE
        assert (st.received_samples, st.emitted_frames, st.pending_samples) == before
        with pytest.raises(_lib.FishVocError) as ei:          # a chunk above max_chunk_samples, on a fresh utterance
            st.reset()
            st.push(_strided(torch.zeros((B, 4097), device="cuda")))
        assert ei.value.status == _lib.FV_ERR_INVALID and st.received_samples == 0
        with pytest.raises(ValueError):
            st.push(rows[:2, :hop])
        # the first utterance fills both carry buffers with 1e3; after reset() the second equals its own whole-row bits
        st.reset()
        loud = torch.full((B, 700), 1e3, device="cuda")
        for _ in range(3):
            st.push(_strided(loud))
        st.flush()
        st.reset()
        f0, ap = _track(st, rows, _sizes("37", L, hop), W, hop)
        assert np.array_equal(_bits(f0), f0_bits) and np.array_equal(_bits(ap), ap_bits)
    with pytest.raises(_lib.FishVocError):                    # closed
        st.push(_strided(rows[:, :hop]))


OSC_T, OSC_SR, OSC_HOP = 600, 8000, 128


@functools.lru_cache(maxsize=None)
def _osc_f0():
    """(2, T): 80 - 1900 Hz with unvoiced runs and a NaN frame; row 0 starts and ends unvoiced, row 1 starts and ends voiced."""
    rng = np.random.default_rng(11)
    f0 = rng.uniform(80.0, 1900.0, (2, OSC_T)).astype(np.float32)
    for b in range(2):
        for at in rng.integers(5, OSC_T - 20, 12):
            f0[b, at:at + int(rng.integers(1, 9))] = 0.0
    f0[0, 0] = f0[0, 1] = f0[0, -1] = 0.0
    f0[0, 77] = np.nan
    f0[1, 300] = -5.0
    f0[1, 0], f0[1, -1] = 150.0, 1700.0
    return f0


@pytest.mark.parametrize("kind", ["sine", "sawtooth"])
@pytest.mark.parametrize("name", ["1", "3", "whole", "0-2-0-598"])
def test_oscillator_stream_equals_the_whole_row_forward_bit_for_bit(kind, name):
    f0 = _osc_f0()
    sizes = {"1": [1] * OSC_T, "3": [3] * (OSC_T // 3), "whole": [OSC_T], "0-2-0-598": [0, 2, 0, 598]}[name]
    assert sum(sizes) == OSC_T
    osc = f0mod.PitchTemplate(OSC_SR, OSC_HOP, kind=kind, amplitude=0.5)
    x = torch.from_numpy(f0).cuda()
    whole = osc(_strided(x))
    assert tuple(whole.shape) == (2, 1, OSC_T * OSC_HOP) and float(whole.abs().max()) > 0.49
    # the phase wraps thousands of times: the mean increment is about an eighth of a turn per sample
    assert float(np.nansum(np.where(f0 > 0, f0, 0.0)[0]) * OSC_HOP / OSC_SR) > 2000.0
    parts, at, E = [], 0, 0
    with osc.stream(2, max(max(sizes), OSC_T // 2)) as st:      # (the second utterance below goes in halves)
        for c in sizes:
            y = st.push(_strided(x[:, at:at + c]))
            at += c
            E2 = sref.osc_emitted(at, E)
            assert tuple(y.shape) == (2, 1, (E2 - E) * OSC_HOP), (at, c)
            E = E2
            assert (st.received_frames, st.emitted_frames, st.pending_frames) == (at, E, at - E)
            parts.append(y)
        parts.append(st.flush())
        assert tuple(parts[-1].shape) == (2, 1, OSC_HOP) and st.pending_frames == 0
        with pytest.raises(_lib.FishVocError) as ei:
            st.push(_strided(x[:, :1]))
        assert ei.value.status == _lib.FV_ERR_STATE
        # the next utterance starts from phase 0 by index, whatever the phase buffers hold
        st.reset()
        again = torch.cat([st.push(_strided(x[:, :OSC_T // 2])), st.push(_strided(x[:, OSC_T // 2:])), st.flush()], dim=-1)
    got = torch.cat(parts, dim=-1)
    assert np.array_equal(_bits(got), _bits(whole)) and np.array_equal(_bits(again), _bits(whole))
    unvoiced = np.repeat(~((f0 > 0) & (f0 < OSC_SR)), OSC_HOP, axis=1)
    assert unvoiced.any() and not _bits(got[:, 0])[unvoiced].any()          # +0.0, not -0.0


def test_streams_of_thirty_four_rows_pass_one_launchs_lengths():
    """Batch 34, more than the 32 lengths one launch carries, two pushes and a flush: rows 32 and 33 ride a second launch with the input of
    rows 0 and 1 and give their bits, in the tracker stream and in the oscillator stream; rows 0 ... 2 are the whole-row result of _case."""
    sr, W, hop, fmin, fmax, L = CONFIGS[0]
    rows3, mod, f0_bits, ap_bits = _case(0)
    x = rows3[0].cpu().numpy()
    wide = np.stack([np.roll(x, 37 * b) for b in list(range(32)) + [0, 1]])
    with mod.stream(34, 1501) as st:
        f0, ap = _track(st, torch.from_numpy(wide).cuda(), [1500, 1501], W, hop)
    f0b, apb = _bits(f0), _bits(ap)
    assert f0b.shape == (34, L // hop) and np.array_equal(f0b[:3], f0_bits) and np.array_equal(apb[:3], ap_bits)
    assert np.array_equal(f0b[32:], f0b[:2]) and np.array_equal(apb[32:], apb[:2])
    assert not np.array_equal(f0b[31], f0b[0]) and not np.array_equal(f0b[0], f0b[1])          # the rows differ

    T = 64
    track = _osc_f0()[:, :T]
    fw = np.stack([np.roll(track[b % 2], 5 * b) for b in list(range(32)) + [0, 1]])
    osc = f0mod.PitchTemplate(OSC_SR, OSC_HOP, amplitude=0.5)
    xw = torch.from_numpy(fw).cuda()
    with osc.stream(34, 34) as st:
        y = torch.cat([st.push(_strided(xw[:, :30])), st.push(_strided(xw[:, 30:])), st.flush()], dim=-1)
    yb = _bits(y[:, 0])
    assert yb.shape == (34, T * OSC_HOP) and np.array_equal(yb[:2], _bits(osc(_strided(xw[:2]))[:, 0]))
    assert np.array_equal(yb[32:], yb[:2]) and float(y[32:].abs().max()) > 0.49
    assert not np.array_equal(yb[31], yb[1]) and not np.array_equal(yb[0], yb[1])


def test_template_stream_equals_template_from_audio_bit_for_bit():
    sr, W, hop, fmin, fmax, L = CONFIGS[0]
    rows, _, _, _ = _case(0)
    kw = dict(frame_length=W, fmin=fmin, fmax=fmax, kind="sawtooth", amplitude=0.7)
    whole = f0mod.template_from_audio(_strided(rows), sr, hop, **kw)
    assert tuple(whole.shape) == (B, 1, (L // hop) * hop) and float(whole.abs().max()) > 0.6
    parts = []
    with f0mod.TemplateStream(sr, hop, B, 37, **kw) as st:
        for at in range(0, L, 37):
            parts.append(st.push(_strided(rows[:, at:at + 37])))
            assert parts[-1].shape[-1] % hop == 0
        assert st.received_samples == L
        parts.append(st.flush())
        assert st.emitted_samples == (L // hop) * hop
    assert np.array_equal(_bits(torch.cat(parts, dim=-1)), _bits(whole))


# ---- the chain, on the tiny use_template HiFiGAN of test_f0_host.py ----
TINY_GEN = dict(hop_length=64, num_mels=20, upsample_initial_channel=32, upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4],
                resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]], pre_conv_kernel_size=7, post_conv_kernel_size=7,
                use_template=True)
CHAIN_L, CHAIN_SR, CHAIN_HOP = 9617, 16000, 64
TRACKER = dict(frame_length=1024, fmin=60.0, fmax=800.0)


def test_the_wav_chain_with_a_template_matches_the_whole_file_forward(monkeypatch):
    from vocoder_amd import engine, inference, synthetic as syn
    from vocoder_amd.data.transforms import LogMelSpectrogram
    from vocoder_amd.modules.generators.hifigan import HiFiGANGenerator
    sr, hop, L = CHAIN_SR, CHAIN_HOP, CHAIN_L
    x = fref.glide(L, sr, seed=1)[0]
    ref = fref.yin(x, sr, hop, **TRACKER)
    assert len(ref["lag"]) == 150 and int((ref["lag"] > 0).sum()) == 104
    gen = HiFiGANGenerator(**TINY_GEN).eval()
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(TINY_GEN, 5).items()})
    front = LogMelSpectrogram(sample_rate=sr, n_fft=256, win_length=256, hop_length=hop, n_mels=20, f_min=0, f_max=sr // 2)
    model = inference.InferenceModel(gen, sr, 20, hop, mel_transform=front).eval().cuda()
    wave = torch.from_numpy(x)[None].cuda()
    mel = model.mel_transform(wave)
    template = f0mod.template_from_audio(wave, sr, hop, **TRACKER)
    assert tuple(mel.shape) == (1, 20, 150) and tuple(template.shape) == (1, 1, 150 * hop) and float(template.abs().max()) > 0.9
    whole = model(None, None, input_spec=mel, template=template)[0]
    peak = float(whole.abs().max())
    bar = 2e-5 * max(1.0, peak)
    assert float((whole - model(None, None, input_spec=mel, template=torch.zeros_like(template))[0]).abs().max()) > 1e-3      # the template matters

    pushed, push = [], engine.Stream.push

    def recording(self, m, t=None):
        pushed.append(None if t is None else t.clone())
        return push(self, m, t)
    monkeypatch.setattr(engine.Stream, "push", recording)
    chunks = [torch.from_numpy(x[at:at + 3 * hop])[None] for at in range(0, L, 3 * hop)]
    y, stats = inference.stream_wav_synthesis(model, iter(chunks), L, chunk_frames=3, template=dict(TRACKER))
    d = float((y - whole).abs().max())
    print(f"wav -> wav with a template, 3-frame chunks: max|d| = {d:.2e} (bar {bar:.1e}, peak {peak:.3f}); first audio after "
          f"{stats['reads_before_first_audio']} of {stats['reads']} reads")
    assert tuple(y.shape) == tuple(whole.shape) and d <= bar
    assert all(t is not None for t in pushed) and np.array_equal(_bits(torch.cat(pushed, dim=-1)), _bits(template))
    assert stats["reads"] == len(chunks) and stats["reads_before_first_audio"] < stats["reads"]

    pushed.clear()
    y2, _, lat = inference.stream_synthesis(model.generator, mel, 3, template=template)
    d2 = float((y2 - whole).abs().max())
    print(f"stream_synthesis with a template: max|d| = {d2:.2e}")
    assert tuple(y2.shape) == tuple(whole.shape) and d2 <= bar and len(lat) == 50
    assert np.array_equal(_bits(torch.cat(pushed, dim=-1)), _bits(template))
    with pytest.raises(ValueError, match="template"):
        inference.stream_synthesis(model.generator, mel, 3, template=template[..., :-1])
    # without a template nothing changed: the defaults leave the generator stream's call as it was
    pushed.clear()
    plain = HiFiGANGenerator(**dict(TINY_GEN, use_template=False)).eval()
    plain.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(dict(TINY_GEN, use_template=False), 5).items()})
    pm = inference.InferenceModel(plain, sr, 20, hop, mel_transform=front).eval().cuda()
    y3, _ = inference.stream_wav_synthesis(pm, iter(chunks), L, chunk_frames=3)
    assert pushed and all(t is None for t in pushed)
    assert float((y3 - pm(None, None, input_spec=mel)[0]).abs().max()) <= 2e-5 * max(1.0, float(y3.abs().max()))

