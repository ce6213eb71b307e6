"""GPU: the log-mel front-end on rows of different lengths (fv_logmel_ragged_forward) and on chunks of a stream (fv_logmel_stream_*), from the
modules down.  The checker is the CPU oracle on each row alone; the bar is the front-end's own, 2e-4 on the values
(test_logmel_frontend_module_and_wav_to_wav).  With batch_invariant every output column is one fixed-order sum, so a frame must not depend on
the call that produced it: ragged rows, whole rows and every chunking agree bit for bit."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc
from vocoder_amd import _lib, synthetic as syn
from vocoder_amd._lib import FishVocError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = 2e-4

# (n_fft, hop, n_mels): plain; hop does not divide n_fft (the last tap is partial, as 24000_2048_3072); win - hop odd (pad_l != pad_r);
# LinearSpectrogram; a stream carry (n_fft samples) wider than one 256-thread block of the carry kernel, with a partial last block
CONFIGS = [(256, 64, 20), (96, 64, 12), (256, 51, 20), (256, 64, 0), (320, 80, 16)]
_modules: dict = {}
_refs: dict = {}


def _module(cfg, invariant=True):
    """One front-end per (config, mode) for the whole file."""
    key = (cfg, invariant)
    if key not in _modules:
        from vocoder_amd.data.transforms import LogMelSpectrogram
        from vocoder_amd.data.transforms.spectrogram import LinearSpectrogram
        n_fft, hop, n_mels = cfg
        m = (LinearSpectrogram(n_fft, n_fft, hop) if n_mels == 0 else
             LogMelSpectrogram(sample_rate=24000, n_fft=n_fft, win_length=n_fft, hop_length=hop, n_mels=n_mels, f_min=0.0, f_max=12000))
        m = m.eval().cuda()
        m.batch_invariant = invariant
        _modules[key] = m
    return _modules[key]


def _wave(cfg, B, L):
    """The synthetic waves of the existing front-end tests: white noise at 0.2."""
    return (0.2 * np.random.default_rng(sum(cfg) + 7 * B + L).normal(size=(B, L))).astype(np.float32)


def _oracle(cfg, row):
    """The oracle on one row alone, computed once per (config, row)."""
    key = (cfg, row.tobytes())
    if key not in _refs:
        n_fft, hop, n_mels = cfg
        if n_mels == 0:
            ref = orc.linear_spectrogram(row[None], n_fft, n_fft, hop)
        else:
            ref = orc.logmel_forward(row[None], dict(sample_rate=24000, n_fft=n_fft, win_length=n_fft, hop_length=hop, n_mels=n_mels,
                                                     f_min=0.0, f_max=12000))
        _refs[key] = ref[0]
    return _refs[key]


def _ragged_cases(fr):
    """Two batches of four that cover: max(pad) + 1 rounded up to one frame, one frame exactly, a multiple of hop and that +- 1, L_max, 0."""
    hop, pad = fr.hop_length, max(fr.pad_l, fr.pad_r)
    shortest = max(pad + 1, hop)                   # the first length that is longer than the reflect padding and gives a frame
    one_frame = shortest                           # the last length with as few frames as the shortest row: exactly one where the padding allows it
    while fr.frames(one_frame + 1) == fr.frames(shortest):
        one_frame += 1
    assert fr.frames(shortest) >= 1 and not fr.too_short(shortest) and fr.too_short(shortest - 1)
    assert fr.frames(shortest) == 1 or shortest == pad + 1
    return [[shortest, 7 * hop, 9 * hop + 3, 0], [one_frame, 7 * hop - 1, 7 * hop + 1, 12 * hop]]


def _stream_all(m, wave, chunks, max_chunk):
    """``wave`` (B, L) through a stream in the given chunk sizes (cycled); checks every push's count; returns (B, C, frames(L))."""
    B, L = wave.shape
    x = torch.from_numpy(wave).cuda()
    outs, at, i = [], 0, 0
    with m.stream(batch=B, max_chunk_samples=max_chunk) as st:
        while at < L:
            c = min(chunks[i % len(chunks)], L - at)
            k = st.emit_count(c)
            y = st.push(x[:, at:at + c])
            assert tuple(y.shape) == (B, y.shape[1], k)
            at, i = at + c, i + 1
            assert st.received_samples == at and st.emitted_frames == m.frames_ready(at)
            assert 0 <= st.pending_samples == m._framing().pending_samples(at, st.emitted_frames) < m.n_fft
            outs.append(y)
        outs.append(st.flush())
        assert st.emitted_frames == m.frames(L)
    return torch.cat(outs, dim=-1)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("invariant", [False, True])
def test_ragged_rows_match_the_oracle_and_ignore_their_padding(cfg, invariant):
    m = _module(cfg, invariant)
    fr = m._framing()
    for lengths in _ragged_cases(fr):
        L_max = max(lengths)
        wave = _wave(cfg, len(lengths), L_max)
        x = torch.full((len(lengths), L_max), float("nan"), device="cuda")
        for b, n in enumerate(lengths):
            x[b, :n] = torch.from_numpy(wave[b, :n]).cuda()
        mel, fl = m.forward_ragged(x if invariant else x[:, None, :], lengths)
        assert fl == [fr.frames(n) for n in lengths] and mel.shape[0] == len(lengths) and mel.shape[2] == fr.frames(L_max)
        assert bool(torch.isfinite(mel).all())
        got = mel.cpu().numpy()
        for b, n in enumerate(lengths):
            assert not got[b, :, fl[b]:].any(), (lengths, b)          # exact zeros from column T_b on
            if n:
                ref = _oracle(cfg, wave[b, :n])
                err = float(np.abs(got[b, :, :fl[b]] - ref).max())
                print(f"cfg {cfg} L {n}: max|d| vs oracle {err:.2e}")
                assert ref.shape == got[b, :, :fl[b]].shape and err <= TOL, (lengths, b, err)
        lst = m.forward_list([x[b, :n] for b, n in enumerate(lengths)])
        assert all(torch.equal(lst[b], mel[b, :, :fl[b]]) for b in range(len(lengths)))


def test_ragged_rows_past_one_launchs_table():
    """33 rows: the per-row ends travel by value 32 at a time, so row 32 is served by a second launch of the window and zeroing kernels."""
    cfg = CONFIGS[1]
    m = _module(cfg)
    fr = m._framing()
    hop = fr.hop_length
    shortest = max(max(fr.pad_l, fr.pad_r) + 1, hop)
    lengths = [(shortest, 2 * hop + 1, 0, 3 * hop)[b % 4] for b in range(32)] + [2 * hop + 5]
    L_max = max(lengths)
    wave = _wave(cfg, len(lengths), L_max)
    x = torch.full((len(lengths), L_max), float("nan"), device="cuda")
    for b, n in enumerate(lengths):
        x[b, :n] = torch.from_numpy(wave[b, :n]).cuda()
    mel, fl = m.forward_ragged(x, lengths)
    assert fl == [fr.frames(n) for n in lengths] and fl[32] < fr.frames(L_max) and bool(torch.isfinite(mel).all())
    got = mel.cpu().numpy()
    for b in (0, 1, 2, 31, 32):
        assert not got[b, :, fl[b]:].any(), b
        if lengths[b]:
            err = float(np.abs(got[b, :, :fl[b]] - _oracle(cfg, wave[b, :lengths[b]])).max())
            print(f"cfg {cfg} row {b} of 33, L {lengths[b]}: max|d| vs oracle {err:.2e}")
            assert err <= TOL, (b, err)
    alone = m(x[32:33, :lengths[32]].contiguous())
    assert torch.equal(mel[32, :, :fl[32]], alone[0])                 # a ragged row and the same row run alone


@pytest.mark.parametrize("cfg", CONFIGS)
def test_ragged_refusals_name_the_row_and_enqueue_nothing(cfg):
    m = _module(cfg)
    fr = m._framing()
    pad, hop = max(fr.pad_l, fr.pad_r), fr.hop_length
    L_max = 8 * hop
    x = torch.zeros((3, L_max), device="cuda")
    with pytest.raises(FishVocError, match=r"lengths\[1\]") as ei:
        m.forward_ragged(x, [L_max, pad, 0])                          # not longer than the reflect padding
    assert ei.value.status == _lib.FV_ERR_INVALID
    for bad in (-1, L_max + 1):
        with pytest.raises(FishVocError, match=r"lengths\[2\]") as ei:
            m.forward_ragged(x, [L_max, 0, bad])
        assert ei.value.status == _lib.FV_ERR_INVALID
    eng = m.engine(x.device)
    out = torch.empty((3, eng.out_channels, fr.frames(L_max)), device="cuda")
    ws = torch.empty(eng.workspace_bytes(3, L_max) // 4 + 64, device="cuda")
    arr = (ctypes.c_int32 * 3)(L_max, 0, L_max)
    st = eng._lib.fv_logmel_ragged_forward(eng._h, x.data_ptr(), L_max, arr, 3, L_max, out.data_ptr(), ws.data_ptr(),
                                           eng.workspace_bytes(3, L_max) - 256, None)
    assert st == _lib.FV_ERR_INVALID and "workspace too small" in eng._lib.fv_last_error().decode()
    # engines that are not a front-end are refused by name
    from vocoder_amd.engine import Engine, upsampler_config
    gen = Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**TINY_GEN), state_dict=syn.hifigan_state_dict(TINY_GEN, 1))
    for call in (lambda: gen.logmel_ragged(x, [L_max, 0, 0]), lambda: gen.logmel_stream(1, 64)):
        with pytest.raises(FishVocError, match="log-mel"):
            call()
    gen.close()
    with pytest.raises(FishVocError, match="log-mel"):                # a pool is not built: the engine's own refusal, through the base's method
        m.session_pool(sessions=2, max_chunk_frames=4)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_stream_chunkings_match_the_counters_the_oracle_and_each_other(cfg):
    m = _module(cfg)
    fr = m._framing()
    n_fft, hop = fr.n_fft, fr.hop_length
    B, L = 2, 9 * hop + 5
    wave = _wave(cfg, B, L)
    whole = m(torch.from_numpy(wave).cuda())
    assert whole.shape[-1] == fr.frames(L)
    ref = np.stack([_oracle(cfg, wave[b]) for b in range(B)])
    assert float(np.abs(whole.cpu().numpy() - ref).max()) <= TOL
    first_short = max(1, fr.pad_l - 1)                                # a first push shorter than pad_l emits nothing
    assert fr.frames_ready(first_short) == 0
    chunkings = {"1": [1], "hop-1": [hop - 1], "hop": [hop], "hop+1": [hop + 1], "n_fft": [n_fft], "2n_fft+3": [2 * n_fft + 3],
                 "primes": [first_short, 2, 3, 5, 7, 11, 13, 61, 127, 251]}
    for name, chunks in chunkings.items():
        got = _stream_all(m, wave, chunks, max(2 * n_fft + 3, max(chunks)))   # (the prime mix's 251 is above 2 n_fft + 3 at n_fft = 96)
        assert got.shape == whole.shape, name                         # frames(L) columns
        err = float(np.abs(got.cpu().numpy() - ref).max())
        print(f"cfg {cfg} chunks {name}: max|d| vs oracle {err:.2e}, equal to forward: {torch.equal(got, whole)}")
        assert err <= TOL, (name, err)
        assert torch.equal(got, whole), name                          # two chunkings agree because each agrees with the whole row
    # a ragged row and the same row run alone
    lengths = [L, 7 * hop + 1, 0]
    x = torch.zeros((3, L), device="cuda")
    x[0] = torch.from_numpy(wave[0]).cuda()
    x[1, :lengths[1]] = torch.from_numpy(wave[1, :lengths[1]]).cuda()
    mel, fl = m.forward_ragged(x, lengths)
    assert torch.equal(mel[0], whole[0])
    alone = m(x[1:2, :lengths[1]].contiguous())
    assert torch.equal(mel[1, :, :fl[1]], alone[0])


@pytest.mark.parametrize("cfg", CONFIGS)
def test_stream_edges_refusals_and_reset(cfg):
    m = _module(cfg)
    fr = m._framing()
    n_fft, hop, pad = fr.n_fft, fr.hop_length, max(fr.pad_l, fr.pad_r)
    # an utterance that emerges from the flush alone: no frame is ready before its end
    L = n_fft - fr.pad_l - 1
    assert fr.frames_ready(L) == 0 and fr.frames(L) >= 1 and not fr.too_short(L)
    wave = _wave(cfg, 1, L)
    x = torch.from_numpy(wave).cuda()
    with m.stream(batch=1, max_chunk_samples=8 * hop) as st:
        assert st.push(x).shape[-1] == 0
        y = st.flush()
        assert y.shape[-1] == fr.frames(L) and torch.equal(y, m(x))
        assert float(np.abs(y[0].cpu().numpy() - _oracle(cfg, wave[0])).max()) <= TOL
        # a push after the flush: FV_ERR_STATE, counters unchanged
        with pytest.raises(FishVocError) as ei:
            st.push(x[:, :8])
        assert ei.value.status == _lib.FV_ERR_STATE and (st.received_samples, st.emitted_frames) == (L, fr.frames(L))
        # reset, then a second utterance: the same as a fresh stream
        st.reset()
        assert (st.received_samples, st.emitted_frames, st.pending_samples) == (0, 0, 0)
        L2 = 6 * hop + 3
        w2 = _wave(cfg, 1, L2)
        x2 = torch.from_numpy(w2).cuda()
        again = torch.cat([st.push(x2[:, :hop + 1]), st.push(x2[:, hop + 1:]), st.flush()], dim=-1)
    fresh = _stream_all(m, w2, [hop + 1, L2], 8 * hop)
    assert torch.equal(again, fresh) and torch.equal(fresh, m(x2))
    with m.stream(batch=1, max_chunk_samples=hop) as st:
        # an oversize chunk
        with pytest.raises(FishVocError) as ei:
            st.push(x[:, :hop + 1])
        assert ei.value.status == _lib.FV_ERR_INVALID and (st.received_samples, st.emitted_frames) == (0, 0)
        # a too-short flush: `pad` samples cannot be reflected
        at = 0
        while at < pad:
            st.push(x[:, at:min(at + hop, pad)])
            at = min(at + hop, pad)
        before = (st.received_samples, st.emitted_frames, st.pending_samples)
        with pytest.raises(FishVocError) as ei:
            st.flush()
        assert ei.value.status == _lib.FV_ERR_INVALID and (st.received_samples, st.emitted_frames, st.pending_samples) == before
        st.push(x[:, pad:pad + 1])                                    # the refused flush changed nothing: the stream goes on
        assert st.received_samples == pad + 1
    with m.stream(batch=2, max_chunk_samples=hop) as st:               # a flush at N = 0 emits nothing
        y = st.flush()
        assert tuple(y.shape) == (2, y.shape[1], 0) and st.emitted_frames == 0
        with pytest.raises(FishVocError) as ei:
            st.push(torch.zeros((2, 4), device="cuda"))
        assert ei.value.status == _lib.FV_ERR_STATE
    # the "make a new stream" error of the existing streams: a rebuilt engine closes its streams
    st = m.stream(batch=1, max_chunk_samples=hop)
    m.invalidate_engine()
    with pytest.raises(FishVocError, match="create a new stream"):
        st.push(x[:, :hop])


def test_forward_is_untouched_by_the_window_paths():
    """forward before and after a ragged call and a stream is bit-identical to itself, replayed graph included."""
    cfg = CONFIGS[0]
    m = _module(cfg)
    hop = cfg[1]
    wave = _wave(cfg, 2, 11 * hop)
    x = torch.from_numpy(wave).cuda()
    before = [m(x).clone() for _ in range(3)]                         # eager, captured, replayed
    assert all(torch.equal(b, before[0]) for b in before)
    m.forward_ragged(x, [11 * hop, 5 * hop])
    _stream_all(m, wave, [hop + 1], 2 * hop)
    after = [m(x).clone() for _ in range(3)]
    assert all(torch.equal(a, before[0]) for a in after)


# ---- CLI, on a tiny HiFiGAN ----
TINY = dict(hop_length=64, n_fft=256, win_length=256, num_mels=20, sampling_rate=16000)
TINY_GEN = dict(hop_length=64, num_mels=20, upsample_initial_channel=128, upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4],
                resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, pre_conv_kernel_size=7, post_conv_kernel_size=7,
                use_template=False)


LONG = 64 * 100 + 13


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    import yaml
    from vocoder_amd import inference
    root = tmp_path_factory.mktemp("tiny")
    (root / "cfg" / "model" / "resolution").mkdir(parents=True)
    (root / "cfg" / "model" / "generator").mkdir(parents=True)
    (root / "cfg" / "model" / "resolution" / "tiny.yaml").write_text(yaml.safe_dump(TINY))
    (root / "cfg" / "model" / "generator" / "hifigan.yaml").write_text(
        yaml.safe_dump(dict(TINY_GEN, _target_="vocoder_amd.modules.generators.hifigan.HiFiGANGenerator")))
    sd = syn.hifigan_state_dict(TINY_GEN, 5)
    torch.save({"state_dict": {f"generator.{k}": torch.from_numpy(v) for k, v in sd.items()}}, root / "g.ckpt")
    rng = np.random.default_rng(3)
    (root / "in").mkdir()
    for name, n in (("a", 64 * 21), ("b", 64 * 9 + 17), ("c", 64 * 30 - 1)):
        inference.write_wav(root / "in" / f"{name}.wav", (0.3 * rng.normal(size=(n, 1))).clip(-1, 1), 16000)
    (root / "long").mkdir()      # several times the generator's lookahead (30 frames), so that audio leaves long before the file ends
    inference.write_wav(root / "long" / "e.wav", (0.3 * rng.normal(size=(LONG, 1))).clip(-1, 1), 16000)
    (root / "in24").mkdir()      # 24-bit PCM, two channels: every width that the whole-file branch reads streams too
    pcm = (0.3 * rng.normal(size=(64 * 13 + 7, 2))).clip(-1, 1)
    v = np.round(pcm * 8388607.0).astype("<i4")
    import wave
    with wave.open(str(root / "in24" / "f.wav"), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(3)
        w.setframerate(16000)
        w.writeframes(v.view(np.uint8).reshape(-1, 4)[:, :3].tobytes())
    (root / "in8k").mkdir()
    inference.write_wav(root / "in8k" / "d.wav", (0.3 * rng.normal(size=(64 * 11 + 5, 1))).clip(-1, 1), 8000)
    base = ["--generator", "hifigan", "--resolution", "tiny", "--config-root", str(root / "cfg"), "--ckpt-path", str(root / "g.ckpt")]

    def run(inp, out, *extra):
        return inference.main(base + ["--input-path", str(root / inp), "--output-path", str(root / out), *extra])
    return root, run


def _pcm_close(a_path, b_path):
    from vocoder_amd import inference
    (a, ra), (b, rb) = inference.read_wav(a_path), inference.read_wav(b_path)
    assert ra == rb and a.shape == b.shape, (ra, rb, a.shape, b.shape)
    return float(np.abs(a - b).max()) * 32768.0


def test_cli_batches_wav_files_of_different_lengths(tiny):
    root, run = tiny
    run("in", "one_by_one")
    run("in", "batched", "--batch-size", "3")
    for name in "abc":
        assert _pcm_close(root / "one_by_one" / f"{name}.wav", root / "batched" / f"{name}.wav") <= 1.0, name


def test_cli_streams_a_wav_chunk_by_chunk(tiny, monkeypatch):
    from vocoder_amd import inference
    root, run = tiny
    stats, chain = [], inference.stream_wav_synthesis

    def recording(*a, **kw):
        out, st = chain(*a, **kw)
        stats.append(st)
        return out, st
    monkeypatch.setattr(inference, "stream_wav_synthesis", recording)
    assert run("long/e.wav", "whole") is None and not stats
    assert run("long/e.wav", "streamed", "--chunk-frames", "4") is None
    assert _pcm_close(root / "whole" / "e.wav", root / "streamed" / "e.wav") <= 1.0
    assert len(stats) == 1 and stats[0]["reads"] == -(-LONG // (4 * 64))
    assert stats[0]["reads_before_first_audio"] < stats[0]["reads"]   # the first audio was written before the last chunk was read


def test_cli_streams_a_24_bit_stereo_wav(tiny):
    from vocoder_amd import inference
    root, run = tiny
    run("in24/f.wav", "whole24")
    run("in24/f.wav", "streamed24", "--chunk-frames", "4")
    assert inference.read_wav(root / "whole24" / "f.wav")[0].shape[0] == 2     # channels are batch items: two rows through one chain
    assert _pcm_close(root / "whole24" / "f.wav", root / "streamed24" / "f.wav") <= 1.0


def test_cli_streams_a_wav_through_both_resamplers(tiny):
    root, run = tiny
    run("in8k/d.wav", "whole_rs", "--resample", "--output-rate", "24000")
    run("in8k/d.wav", "streamed_rs", "--resample", "--output-rate", "24000", "--chunk-frames", "4")
    assert _pcm_close(root / "whole_rs" / "d.wav", root / "streamed_rs" / "d.wav") <= 1.0
    with pytest.raises(ValueError, match="--sessions takes mel inputs"):
        run("in/a.wav", "sessions", "--chunk-frames", "4", "--sessions", "2")
