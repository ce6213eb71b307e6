"""Host (no GPU): the log-mel front-end on ragged rows and stream chunks (include/fishvoc.h fv_logmel_*) — the ABI surface, the framing rule
stated twice (C: fv_logmel_frames / fv_logmel_frames_ready; Python: vocoder_amd.framing) and against the oracle's frame count, and a replay
of a stream's host counters."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from oracle import oracle as orc
from vocoder_amd import _lib, framing

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

LOGMEL_API = ("fv_logmel_frames", "fv_logmel_frames_ready", "fv_logmel_ragged_forward", "fv_logmel_stream_create",
              "fv_logmel_stream_workspace_bytes", "fv_logmel_stream_pending_samples", "fv_logmel_stream_push", "fv_logmel_stream_flush",
              "fv_logmel_stream_reset", "fv_logmel_stream_destroy")
# (n_fft, hop, n_mels): plain; hop does not divide n_fft (the last tap is partial, as 24000_2048_3072); win - hop odd (pad_l != pad_r);
# LinearSpectrogram
CONFIGS = [(256, 64, 20), (96, 64, 12), (256, 51, 20), (256, 64, 0)]


def _cfg(n_fft, hop, n_mels):
    return _lib.LogMelConfig(24000, n_fft, n_fft, hop, n_mels, 0.0, 12000.0)


def test_entry_points_are_declared_listed_exported_and_the_abi_stays_5():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in LOGMEL_API:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert {d for d in declared if d.startswith("fv_logmel")} == set(LOGMEL_API)
    assert {n for n in _lib.EXPORTS if n.startswith("fv_logmel")} == set(LOGMEL_API)
    assert "#define FV_ABI_VERSION 5" in hdr and _lib.FV_ABI_VERSION == 5 and L.fv_abi_version() == 5
    assert ctypes.sizeof(_lib.LogMelConfig) == 28
    # every entry names the reference code it stands in for
    for name in LOGMEL_API:
        at = re.search(r"FV_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr).start()
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "spectrogram.py:25-" in comment and "test.py:64-71" in comment, name


@pytest.mark.parametrize("n_fft,hop,n_mels", CONFIGS)
def test_frames_and_frames_ready_equal_the_python_restatement(n_fft, hop, n_mels):
    L = _lib.lib()
    c, fr = _cfg(n_fft, hop, n_mels), framing.Framing(n_fft, n_fft, hop)
    assert fr.pad_l + fr.pad_r == n_fft - hop and 0 <= fr.pad_r - fr.pad_l <= 1
    for n in range(0, 3 * n_fft + 1):
        f, r = int(L.fv_logmel_frames(ctypes.byref(c), n)), int(L.fv_logmel_frames_ready(ctypes.byref(c), n))
        assert f == fr.frames(n) and r == fr.frames_ready(n), n
        assert 0 <= r <= f, n
        # the ready frames read nothing at or after n; the next frame does
        if r:
            assert (r - 1) * hop - fr.pad_l + n_fft <= n
        assert r * hop - fr.pad_l + n_fft > n
    assert L.fv_logmel_frames(None, 1000) == 0 and L.fv_logmel_frames(ctypes.byref(c), -1) == 0
    assert L.fv_logmel_frames_ready(ctypes.byref(c), -1) == 0


@pytest.mark.parametrize("n_fft,hop,n_mels", CONFIGS)
def test_frames_equal_the_oracles_frame_count(n_fft, hop, n_mels):
    L = _lib.lib()
    c, fr = _cfg(n_fft, hop, n_mels), framing.Framing(n_fft, n_fft, hop)
    ocfg = dict(sample_rate=24000, n_fft=n_fft, win_length=n_fft, hop_length=hop, n_mels=n_mels, f_min=0.0, f_max=12000)
    wave = np.random.default_rng(n_fft + hop).normal(size=(1, 3 * n_fft)).astype(np.float32)
    for n in range(0, 3 * n_fft + 1):
        if fr.too_short(n):      # the rows every entry refuses: no frame, or reflect padding as long as the row
            assert n <= max(fr.pad_l, fr.pad_r) or fr.frames(n) == 0
            continue
        ref = orc.linear_spectrogram(wave[:, :n], n_fft, n_fft, hop) if n_mels == 0 else orc.logmel_forward(wave[:, :n], ocfg)
        assert ref.shape[-1] == int(L.fv_logmel_frames(ctypes.byref(c), n)) == fr.frames(n), n


@pytest.mark.parametrize("n_fft,hop,n_mels", CONFIGS)
def test_counter_replay_covers_every_frame_once_and_in_order(n_fft, hop, n_mels):
    fr = framing.Framing(n_fft, n_fft, hop)
    rng = random.Random(n_fft * 1000 + hop)
    for trial in range(200):
        total = rng.randint(max(fr.pad_l, fr.pad_r, hop) + 1, 3 * n_fft)
        fixed = [0, 1, hop - 1, hop, hop + 1, n_fft, 2 * n_fft + 3][trial % 7]
        cn, seen, left = framing.Counters(fr), [], total
        while left:
            c = min(left, fixed if fixed else rng.choice([1, 2, 3, 5, 7, 11, 13, 17, 61, 127, 251]))
            k = cn.emit_count(c)
            got = cn.push(c)
            assert len(got) == k
            seen.extend(got)
            left -= c
            assert cn.N == total - left and cn.E == fr.frames_ready(cn.N) == len(seen)
            assert 0 <= fr.pending_samples(cn.N, cn.E) < n_fft      # what the carry must hold
        assert not fr.too_short(total)
        seen.extend(cn.flush())
        assert seen == list(range(fr.frames(total))) and cn.flushed
    cn = framing.Counters(fr)
    assert list(cn.flush()) == [] and cn.E == 0      # a flush at N = 0 emits nothing


def test_modules_offer_the_ragged_and_streaming_forms():
    from vocoder_amd.data.transforms import LogMelSpectrogram
    from vocoder_amd.data.transforms.spectrogram import LinearSpectrogram
    from vocoder_amd.engine import Engine, LogMelStream
    for m in (LogMelSpectrogram(sample_rate=24000, n_fft=256, win_length=256, hop_length=51, n_mels=20), LinearSpectrogram(96, 96, 64)):
        for name in ("forward_ragged", "forward_list", "stream", "frames", "frames_ready"):
            assert callable(getattr(m, name)), name
        fr = framing.Framing(m.n_fft, m.win_length, m.hop_length)
        assert [m.frames(n) for n in range(0, 600, 7)] == [fr.frames(n) for n in range(0, 600, 7)]
        assert [m.frames_ready(n) for n in range(0, 600, 7)] == [fr.frames_ready(n) for n in range(0, 600, 7)]
        with pytest.raises(RuntimeError, match="needs the module on a HIP device"):      # the base's session_pool: no override, no CPU path
            m.session_pool()
    assert callable(Engine.logmel_ragged) and callable(Engine.logmel_stream)
    for name in ("push", "flush", "reset", "close", "emit_count", "__enter__", "__exit__"):
        assert callable(getattr(LogMelStream, name)), name
    for name in ("received_samples", "emitted_frames", "pending_samples"):
        assert isinstance(getattr(LogMelStream, name), property), name


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_the_chunked_wav_reader_gives_read_wavs_samples_at_every_width(width, tmp_path):
    """--chunk-frames reads a .wav piece by piece: the pieces together are what read_wav decodes, for every width it takes."""
    import wave
    torch = pytest.importorskip("torch")
    from vocoder_amd import inference
    nch, n = 2, 1000
    raw = np.random.default_rng(width).integers(0, 256, size=n * nch * width, dtype=np.uint8).tobytes()      # every byte pattern is a sample
    path = tmp_path / f"w{width}.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(nch)
        w.setsampwidth(width)
        w.setframerate(16000)
        w.writeframes(raw)
    whole, sr = inference.read_wav(path)
    assert sr == 16000 and whole.shape == (nch, n) and whole.dtype == np.float32 and -1.0 <= whole.min() and whole.max() < 1.0
    for chunk in (1, 7, 256, n, n + 5):
        pieces = list(inference._wav_chunks(path, chunk))
        assert [int(p.shape[1]) for p in pieces] == [min(chunk, n - at) for at in range(0, n, chunk)]
        assert all(p.dtype == torch.float32 and p.shape[0] == nch for p in pieces)
        assert np.array_equal(torch.cat(pieces, dim=1).numpy(), whole), (width, chunk)


def test_the_wav_sink_closes_clean_when_nothing_was_written(tmp_path):
    import wave
    from vocoder_amd import inference
    sink = inference._WavSink(tmp_path / "out" / "empty.wav", 24000, 2)
    sink.close()
    with wave.open(str(tmp_path / "out" / "empty.wav"), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, 2, 24000, 0)
