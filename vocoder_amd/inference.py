"""Inference wrapper with the contract of the reference's task model + test CLI.

* ``InferenceModel.forward(audio, mask=None, input_spec=None) -> (fake_audio, 0)`` is what
  ``GANModel.forward`` promises ``test.py:89`` (reference models/gan.py:282-288).  With a ``mel_transform`` attached
  (the GPU log-mel front-end) the ``audio`` branch works too: ``input_spec = mel_transform(audio.squeeze(1))``
  (gan.py:284).
* ``load_generator_state_dict`` accepts a raw generator state dict or a Lightning checkpoint
  (``{"state_dict": {"generator.<key>": ...}}``, test.py:32-37).
* ``main`` mirrors test.py:50-99: ``.pt``/``.pth`` mels (add a batch dim to 2-D mels, transpose when the last dim is
  ``num_mels``) and ``.wav`` audio (channels become batch items, log-mel on the GPU), write ``(B, 1, T)`` -> wav.
  PCM wav only (librosa / soundfile are not available here): other inputs are refused, not guessed.  ``--resample`` converts a ``.wav`` at
  another rate to the model's on the GPU (test.py:54 ``librosa.load(sr=...)``; ``vocoder_amd.resample``), ``--output-rate HZ`` converts the
  generated audio before it is written.  ``--pitch-shift N_STEPS`` shifts a ``.wav`` after loading / resampling and before the mel front-end
  (test.py:61-62 ``librosa.effects.pitch_shift``; ``vocoder_amd.pitch_shift``); whole files and ``--batch-size`` only.
  ``--chunk-frames N`` streams each input N mel frames at a time (``stream_synthesis``) instead of one whole-utterance forward; a ``.wav`` is
  read, converted and written ``N * hop`` samples at a time through ``stream_wav_synthesis`` (resample stream, log-mel stream, generator
  stream, resample stream), so the first audio is out long before the file has been read.  ``--batch-size N`` takes ``.wav`` files too: their
  rows go through the front-end's ``forward_list`` and then the generator's.  A generator that takes a pitch template next to the mel
  (``RefineGANGenerator``, ``use_template=True``; refinegan.py:287, hifigan.py:226) gets one: for a ``.wav`` it is made on the GPU from the
  samples the mel is made from (``vocoder_amd.f0``: YIN, then an exact-phase oscillator; ``--f0-min`` / ``--f0-max`` / ``--f0-threshold`` /
  ``--template-kind``), for a mel from the sidecar ``<stem>.f0.npy`` (Hz per mel frame, 0 = unvoiced); whole files and ``--batch-size``.
  ``--noise-seed N`` (RefineGAN): the AdaIN noise (refinegan.py:125) is computed inside the kernels from the seed instead of drawn with
  ``torch.randn`` per call (``RefineGANGenerator.set_noise_seed``): the same file twice, no noise tensor, whole files of any length.
"""
from __future__ import annotations

import argparse
import time
import wave
from contextlib import ExitStack
from pathlib import Path

import numpy as np
import torch
from torch import nn

from . import config as fvconfig


class InferenceModel(nn.Module):
    def __init__(self, generator: nn.Module, sampling_rate: int = 44100, num_mels: int = 128, hop_length: int = 512,
                 mel_transform: nn.Module | None = None):
        super().__init__()
        self.generator = generator
        self.mel_transform = mel_transform   # mel_transforms.input of the reference's task model (gan.yaml:4,31)
        self.sampling_rate, self.num_mels, self.hop_length = sampling_rate, num_mels, hop_length

    @property
    def device(self):
        return next(self.generator.parameters()).device

    def forward(self, audio, mask=None, input_spec=None, template=None):
        if input_spec is None:
            if self.mel_transform is None or audio is None:
                raise NotImplementedError(
                    "wave -> mel (mel_transforms.input, gan.py:284) needs a mel_transform (build_model attaches one); "
                    "pass input_spec= otherwise")
            input_spec = self.mel_transform(audio.squeeze(1) if audio.dim() == 3 else audio)
        if template is not None:      # refinegan.py:287 / hifigan.py:226: forward(mel, template)
            return self.generator(input_spec, template), 0
        return self.generator(input_spec), 0


def load_generator_state_dict(ckpt, trust_checkpoint: bool = False) -> dict:
    """Raw state dict, or Lightning checkpoint with the ``generator.`` prefix (other prefixes — discriminators,
    mel_transforms — are dropped, they are not part of the generator).

    Files are read with ``torch.load(weights_only=True)``.  The reference (test.py:32) uses a plain ``torch.load``, and real
    Lightning ``.ckpt`` files usually carry non-tensor objects (hyper_parameters as a DictConfig, callbacks, optimizer
    state) that the weights-only unpickler rejects: pass ``trust_checkpoint=True`` (CLI ``--trust-checkpoint``) to fall
    back to a full unpickle for a file you trust, or export just the tensors once with
    ``torch.save({"state_dict": ckpt["state_dict"]}, "weights.pt")``."""
    if isinstance(ckpt, (str, Path)):
        path = ckpt
        import pickle
        try:
            ckpt = torch.load(path, map_location="cpu", weights_only=True)
        except OSError:
            raise          # missing / unreadable file: not a trust question, and no second (unsafe) attempt
        except (pickle.UnpicklingError, RuntimeError) as exc:   # the refusal itself, or a RuntimeError wrapping it (by torch version)
            refused = isinstance(exc, pickle.UnpicklingError) or any(
                m in str(exc) for m in ("weights_only", "Weights only", "Unsupported global", "unsupported global", "UnpicklingError"))
            if not refused:
                raise      # e.g. a corrupt zip archive: the full unpickler would fail the same way
            if not trust_checkpoint:
                raise RuntimeError(
                    f"{path}: the weights-only loader refused this checkpoint ({type(exc).__name__}: {str(exc)[:200]}). "
                    "Lightning checkpoints often hold non-tensor objects (hyper_parameters, callbacks). If you trust the "
                    "file, pass trust_checkpoint=True / --trust-checkpoint, or re-save only its 'state_dict'.") from exc
            ckpt = torch.load(path, map_location="cpu", weights_only=False)
    if "state_dict" in ckpt:
        ckpt = ckpt["state_dict"]
    if any(k.startswith("generator.") for k in ckpt):
        ckpt = {k[len("generator."):]: v for k, v in ckpt.items() if k.startswith("generator.")}
    return dict(ckpt)


def prepare_mel(mel: torch.Tensor, num_mels: int) -> torch.Tensor:
    """test.py:78-82: (T, M) or (M, T) or batched; returns (B, num_mels, T) float32."""
    mel = mel.to(torch.float32)
    if mel.dim() == 2:
        mel = mel[None]
    if mel.shape[-1] == num_mels:
        mel = mel.transpose(1, 2)
    return mel.contiguous()


def diffsinger_mel_to_ln(mel: torch.Tensor) -> torch.Tensor:
    """DiffSinger log10 mels -> the natural-log convention of the generators (scripts/convert_diffsinger_mel.py:9-17)."""
    return mel / 0.434294


def write_wav(path, audio: np.ndarray, sampling_rate: int) -> None:
    """audio: (T,) or (T, C) float in [-1, 1] -> 16-bit PCM (soundfile is not available here)."""
    a = np.asarray(audio, dtype=np.float32)
    if a.ndim == 1:
        a = a[:, None]
    pcm = (np.clip(a, -1.0, 1.0) * 32767.0).round().astype("<i2")
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(int(sampling_rate))
        w.writeframes(pcm.tobytes())


def _decode_pcm(raw: bytes, width: int, nch: int, path) -> np.ndarray:
    """Whole frames of PCM bytes (8 / 16 / 24 / 32 bit) -> (channels, T) float32 in [-1, 1)."""
    if width == 1:
        a = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0
    elif width == 2:
        a = np.frombuffer(raw, "<i2").astype(np.float32) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        a = (v - ((v & 0x800000) << 1)).astype(np.float32) / 8388608.0
    elif width == 4:
        a = np.frombuffer(raw, "<i4").astype(np.float32) / 2147483648.0
    else:
        raise ValueError(f"{path}: unsupported sample width {width}")
    return np.ascontiguousarray(a.reshape(-1, nch).T)


def read_wav(path) -> tuple[np.ndarray, int]:
    """PCM wav (8 / 16 / 24 / 32 bit) -> ((channels, T) float32 in [-1, 1), sampling rate), like
    ``librosa.load(path, sr=None, mono=False)`` for such files (test.py:51)."""
    with wave.open(str(path), "rb") as w:
        nch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    return _decode_pcm(raw, width, nch, path), int(sr)


def build_model(generator="hifigan", resolution="44100_512_2048", overrides=None, config_root=None,
                ckpt_path=None, device="cuda", trust_checkpoint=False) -> InferenceModel:
    from .data.transforms import LogMelSpectrogram
    gen, cfg = fvconfig.build_generator(generator, resolution, overrides, config_root)
    if ckpt_path is not None:
        gen.load_state_dict(load_generator_state_dict(ckpt_path, trust_checkpoint), strict=True)
    m = cfg["model"]
    # configs/model/spectrogram/mel.yaml:1-8 (mel_transforms.input)
    mel = LogMelSpectrogram(sample_rate=m["sampling_rate"], n_fft=m["n_fft"], win_length=m["win_length"],
                            hop_length=m["hop_length"], n_mels=m["num_mels"], f_min=0, f_max=m["sampling_rate"] // 2)
    model = InferenceModel(gen, m["sampling_rate"], m["num_mels"], m["hop_length"], mel_transform=mel)
    return model.eval().to(device)


def _feed(push, x: torch.Tensor, limit: int) -> torch.Tensor:
    """``x`` (..., n) through ``push`` in pieces of at most ``limit`` columns (a stage may emit more at once than the next one takes per push);
    the pieces' outputs concatenated.  An empty ``x`` is pushed once, so that the result has the stage's output shape."""
    outs = [push(x[..., i:i + limit]) for i in range(0, max(int(x.shape[-1]), 1), limit)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=-1)


class _Stage:
    """One stream of a cascade: its ``push`` and ``flush`` and the most columns one push takes.  ``audio``: the stream takes ``(B, c)`` and
    gives ``(B, k)`` where the cascade carries ``(B, 1, c)`` (a resample stream behind a generator)."""

    def __init__(self, stream, limit: int, audio: bool = False):
        self.limit = int(limit)
        self.push = (lambda y: stream.push(y[:, 0])[:, None]) if audio else stream.push
        self.flush = (lambda: stream.flush()[:, None]) if audio else stream.flush


class _Cascade:
    """Streams in a row: what a stage emits goes into the next one as it comes, and what the last one emits goes to ``sink``."""

    def __init__(self, stages: list, sink):
        self.stages, self.sink = stages, sink

    def feed(self, i: int, x: torch.Tensor) -> None:
        """``x`` into stage ``i`` (``_feed``'s rule) and its output on to stage ``i + 1``; past the last stage, to the sink."""
        if i == len(self.stages):
            return self.sink(x)
        self.feed(i + 1, _feed(self.stages[i].push, x, self.stages[i].limit))

    def finish(self, inject=None) -> None:
        """The flushes, first stage to last, each tail going through every later stage before that stage is flushed itself.
        ``inject = (stage, x)``: ``x`` is fed to that stage just before its own flush."""
        for i, st in enumerate(self.stages):
            if inject is not None and inject[0] is st:
                self.feed(i, inject[1])
            self.feed(i + 1, st.flush())


class _TemplateJoin:
    """The stage of a wav -> wav cascade in front of a generator that takes a pitch template: the model-rate samples go into the log-mel stream
    and into a ``TemplateStream``, whatever one branch has emitted ahead of the other waits here (the two latencies differ by a fixed number of
    samples, so the wait is bounded), and every ``n`` frames that both have emitted go into the generator stream with their ``n * hop``
    template samples.  ``push`` / ``flush`` return the generator's audio ``(B, 1, k)``."""

    def __init__(self, mel_stream, template_stream, gen_stream, chunk_frames: int, hop: int):
        self.mel_stream, self.template_stream, self.gen_stream = mel_stream, template_stream, gen_stream
        self.chunk_frames, self.hop = int(chunk_frames), int(hop)
        self.mel = self.template = None           # emitted by one branch, not yet pushed into the generator
        self.mel_frames = self.template_frames = 0      # emitted in all

    def _take(self, mel: torch.Tensor, template: torch.Tensor) -> None:
        self.mel_frames += int(mel.shape[-1])
        self.template_frames += int(template.shape[-1]) // self.hop
        self.mel = mel if self.mel is None else torch.cat([self.mel, mel], dim=-1)
        self.template = template if self.template is None else torch.cat([self.template, template], dim=-1)

    def _drain(self) -> list:
        n = min(int(self.mel.shape[-1]), int(self.template.shape[-1]) // self.hop)
        outs = []
        for i in range(0, n, self.chunk_frames):
            j = min(i + self.chunk_frames, n)
            outs.append(self.gen_stream.push(self.mel[..., i:j], self.template[..., i * self.hop:j * self.hop]))
        self.mel, self.template = self.mel[..., n:], self.template[..., n * self.hop:]
        return outs

    def push(self, x: torch.Tensor) -> torch.Tensor:
        self._take(self.mel_stream.push(x), self.template_stream.push(x))
        outs = self._drain()
        return torch.cat(outs, dim=-1) if outs else x.new_zeros((x.shape[0], 1, 0))

    def flush(self) -> torch.Tensor:
        self._take(self.mel_stream.flush(), self.template_stream.flush())
        if self.mel_frames != self.template_frames:
            raise ValueError(f"the log-mel front-end made {self.mel_frames} frames and the pitch template {self.template_frames} frames of "
                             f"{self.hop} samples: the generator takes one template frame per mel frame")
        return torch.cat(self._drain() + [self.gen_stream.flush()], dim=-1)


@torch.no_grad()
def stream_synthesis(generator: nn.Module, mel: torch.Tensor, chunk_frames: int, resample: nn.Module | None = None,
                     template: torch.Tensor | None = None):
    """Pushes ``mel`` (B, num_mels, T) through ``generator.stream()`` ``chunk_frames`` frames at a time, then flushes (exact mode: the lookahead
    and the left context are the generator's reach).  Returns (waveform (B, 1, T * hop), seconds to the first non-empty output, seconds per push).
    ``resample`` (a ``vocoder_amd.resample.Resample``): each push's audio goes through a resample stream on the device, and the waveform comes
    back at its ``new_freq``.  ``template`` ``(B, 1, T * hop)``: the whole pitch template of a ``use_template`` generator (``PitchTemplate`` on the
    F0 of the mel's frames), sliced per push."""
    if not hasattr(generator, "stream"):
        raise ValueError(f"--chunk-frames: {type(generator).__name__} has no stream(); HiFiGAN / BigVGAN generators stream")
    B, _, T = mel.shape
    outs, lat, first = [], [], None
    t0 = time.perf_counter()
    with ExitStack() as stack:
        st = stack.enter_context(generator.stream(batch=B, max_chunk_frames=chunk_frames))
        stages = [_Stage(st, chunk_frames)]
        if template is not None:
            if tuple(template.shape) != (B, 1, T * st.hop):
                raise ValueError(f"stream_synthesis: a template of shape {tuple(template.shape)} for a mel of {T} frames; expected "
                                 f"{(B, 1, T * st.hop)}")
            done = [0]

            def push_with_template(m: torch.Tensor) -> torch.Tensor:
                f, n = done[0], int(m.shape[-1])
                done[0] = f + n
                return st.push(m, template[:, :, f * st.hop:(f + n) * st.hop])
            stages[0].push = push_with_template
        if resample is not None:
            if st.out_channels != 1:
                raise ValueError(f"--output-rate: the generator emits {st.out_channels} channels; the resample stream takes waveforms (B, 1, T)")
            limit = max(chunk_frames, st.lookahead_frames) * st.hop      # a push emits at most chunk_frames frames, the flush at most the lookahead
            stages.append(_Stage(stack.enter_context(resample.stream(batch=B, max_chunk=limit)), limit, audio=True))
        cascade = _Cascade(stages, outs.append)
        for f in range(0, T, chunk_frames):
            t1 = time.perf_counter()
            cascade.feed(0, mel[:, :, f:f + chunk_frames])      # (one piece per stage: one output per push)
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t1)
            if first is None and outs[-1].shape[-1]:
                first = time.perf_counter() - t0
        cascade.finish()
        torch.cuda.synchronize()
        if first is None:
            first = time.perf_counter() - t0
    return torch.cat(outs, dim=-1), first, lat


def _pad_samples(hop: int, L: int) -> int:
    return hop - (hop % L) if L > 0 else 0      # test.py:64-68, as written upstream


@torch.no_grad()
def stream_wav_synthesis(model: InferenceModel, chunks, total_samples: int, chunk_frames: int, to_model: nn.Module | None = None,
                         to_out: nn.Module | None = None, sink=None, template: dict | None = None, pitch_shift: nn.Module | None = None):
    """wav -> wav chunk by chunk: [resample stream ->] [pitch-shift stream ->] log-mel stream -> generator stream [-> resample stream].
    ``chunks`` yields ``(B, c)``
    tensors of input samples (``c <= chunk_frames * hop``), ``total_samples`` is their sum (the zero padding of the whole-file branch,
    test.py:64-68, depends on it); ``to_model`` / ``to_out``: ``Resample`` modules into and out of the model's rate.  Every stage's output is
    pushed into the next one as it comes (its emit count sizes that push), and at the end the flushes cascade from the first stage to the
    last.  Each piece of finished audio ``(B, 1, k)`` goes to ``sink`` (default: collected).  Returns (the collected waveform or None, stats):
    ``first_audio_s``, ``push_s`` (seconds per input chunk), ``reads`` and ``reads_before_first_audio`` (input chunks consumed in all / when
    the first audio left).  ``template``: the keyword arguments of a ``vocoder_amd.f0.TemplateStream`` after its sizes (``frame_length``,
    ``fmin``, ``fmax``, ``threshold``, ``kind``, ``amplitude``) for a generator that takes a pitch template: the model-rate samples, the zero
    padding included, go into the log-mel stream and into the template stream, and the generator stream gets the frames both have emitted
    (``_TemplateJoin``); a ValueError names the two frame totals if they differ at the end.  ``pitch_shift``: a
    ``vocoder_amd.pitch_shift.PitchShift`` at the model's rate (test.py:61-62); its stream stands behind ``to_model``, gives back as many
    samples as it takes, and the log-mel front-end and the template are made from the shifted samples, as in the whole-file branch."""
    gen, front, hop = model.generator, model.mel_transform, model.hop_length
    if pitch_shift is not None and pitch_shift.sample_rate != model.sampling_rate:
        raise ValueError(f"pitch_shift runs at {pitch_shift.sample_rate} Hz, the model at {model.sampling_rate} Hz")
    if front is None or not hasattr(front, "stream"):
        raise ValueError("--chunk-frames on a .wav needs the GPU log-mel front-end (build_model attaches one)")
    if not hasattr(gen, "stream"):
        raise ValueError(f"--chunk-frames: {type(gen).__name__} has no stream(); HiFiGAN / BigVGAN generators stream")
    limit = chunk_frames * hop
    L_model = to_model.output_length(total_samples) if to_model is not None else total_samples
    pad = _pad_samples(hop, L_model)
    collected = [] if sink is None else None
    stats = dict(first_audio_s=None, push_s=[], reads=0, reads_before_first_audio=None)
    t0 = time.perf_counter()

    def emit(y):                                    # y: (B, 1, k) at the output rate
        if y.shape[-1] == 0:
            return
        if stats["first_audio_s"] is None:
            torch.cuda.synchronize()
            stats["first_audio_s"] = time.perf_counter() - t0
            stats["reads_before_first_audio"] = stats["reads"]
        (collected.append if sink is None else sink)(y)

    chunks = iter(chunks)
    first = next(chunks, None)      # (the first chunk tells the batch size)
    if first is None:
        raise ValueError("stream_wav_synthesis: no input samples")
    B = int(first.shape[0])
    with ExitStack() as stack:
        stages = []
        if to_model is not None:
            stages.append(_Stage(stack.enter_context(to_model.stream(batch=B, max_chunk=limit)), limit))
        if pitch_shift is not None:
            stages.append(_Stage(stack.enter_context(pitch_shift.stream(batch=B, max_chunk=limit)), limit))
        mel_stream = stack.enter_context(front.stream(batch=B, max_chunk_samples=limit))
        gst = stack.enter_context(gen.stream(batch=B, max_chunk_frames=chunk_frames))
        if gst.out_channels != 1:
            raise ValueError(f"the generator emits {gst.out_channels} channels; wav -> wav streaming takes waveforms (B, 1, T)")
        if template is None:
            mel_stage = _Stage(mel_stream, limit)
            stages += [mel_stage, _Stage(gst, chunk_frames)]
        else:
            from .f0 import TemplateStream
            tst = stack.enter_context(TemplateStream(model.sampling_rate, hop, B, limit, **template))
            mel_stage = _Stage(_TemplateJoin(mel_stream, tst, gst, chunk_frames, hop), limit)      # (the zero padding goes into both branches)
            stages.append(mel_stage)
        if to_out is not None:
            stages.append(_Stage(stack.enter_context(to_out.stream(batch=B, max_chunk=limit)), limit, audio=True))
        cascade = _Cascade(stages, emit)

        def one(x):
            t1 = time.perf_counter()
            stats["reads"] += 1
            cascade.feed(0, x.to(model.device, torch.float32))
            torch.cuda.synchronize()
            stats["push_s"].append(time.perf_counter() - t1)

        one(first)
        for x in chunks:
            one(x)
        # the zero padding of test.py:64-68 follows the input resampler's tail into the log-mel stream
        cascade.finish((mel_stage, torch.zeros((B, pad), dtype=torch.float32, device=model.device)) if pad else None)
        torch.cuda.synchronize()
    if stats["first_audio_s"] is None:
        stats["first_audio_s"] = time.perf_counter() - t0
        stats["reads_before_first_audio"] = stats["reads"]
    return (torch.cat(collected, dim=-1) if collected else None), stats


class WavSessionPool:
    """wav -> wav for live sources that advance independently: the front-end's ``WavPool`` (``vocoder_amd.engine``) feeding the generator's
    ``SessionPool`` on the device.  ``step([(session, samples, end), ...])`` — ``samples``: a 1-D tensor of at most ``max_chunk_samples``
    samples or ``None``; ``end``: the utterance ends with them — runs one ``WavPool.step_padded`` and hands its ``(count, n_mels, out_frames)``
    buffer and the per-item frame counts straight to ``SessionPool.step_padded``: the counts are known on the host (``framing.PoolCounters``),
    so nothing synchronises and nothing is copied.  Returns each item's audio ``(C_out, k * hop)``; a session's audio trails its samples by the
    front-end's ``pad_r`` samples plus the generator's lookahead.  All plans are checked before anything is launched: a refused step leaves
    every pool as it was.

    ``template`` (for a generator that takes a pitch template; such a generator is refused without it): the keyword arguments of a
    ``vocoder_amd.f0.TemplatePool`` after its sizes, the keys ``stream_wav_synthesis(template=...)`` takes (``frame_length``, ``fmin``, ``fmax``,
    ``threshold``, ``kind``, ``amplitude``).  A ``TemplatePool`` then stands beside the wav pool on the same model-rate samples.  Per session,
    what one branch has emitted ahead of the other waits on the device (what ``_TemplateJoin`` does for rows in lockstep), and the generator
    pool gets the ``n`` frames both have emitted with their ``n * hop`` template samples; ``n`` comes from the host counters.  With ``end``
    both branches flush in the same step, and a session whose two branches made different numbers of frames raises a ValueError that names it,
    before anything is launched.

    ``input_resample`` (a ``Resample`` from the client's rate to the model's) puts a ``ResamplePool`` in front: ``max_chunk_samples`` and the
    items' samples then count the client's samples.  ``output_resample`` (from the model's rate to the client's) puts one behind, a slot per
    session and output channel, and the audio comes back at its ``new_freq``: ``(C_out, k)`` with the ``k`` outputs whose bands have
    arrived.  ``end`` flushes every stage in the same step.

    ``pitch_shift`` (a ``vocoder_amd.pitch_shift.PitchShift`` at the front-end's rate; ``batch_invariant=True`` for bits that do not depend on
    the chunking) puts a ``PitchShiftPool`` behind ``input_resample``, if any, and in front of both the wav pool and the template pool — where
    ``stream_wav_synthesis`` puts its stream: the mel and the template are made from the shifted audio.  One ``n_steps`` serves every session.
    The shifter hands back as many samples as it takes, so utterance lengths and the join's frame check hold as without it."""

    _TEMPLATE_KEYS = ("frame_length", "fmin", "fmax", "threshold", "kind", "amplitude")

    def __init__(self, frontend: nn.Module, generator: nn.Module, sessions: int, max_chunk_samples: int, input_resample=None,
                 output_resample=None, template: dict | None = None, pitch_shift=None):
        if takes_template(generator) and template is None:
            raise ValueError(f"WavSessionPool: {type(generator).__name__} takes a pitch template next to the mel; the per-session F0 / template "
                             "pool it would need is not built (the template streams advance in lockstep) unless template= is passed: a dict "
                             "of the tracker's and the oscillator's keyword arguments, empty for the defaults")
        if template is not None:
            if not takes_template(generator):
                raise ValueError(f"WavSessionPool: template= was given, but {type(generator).__name__} takes no pitch template")
            unknown = sorted(set(template) - set(self._TEMPLATE_KEYS))
            if unknown:
                raise ValueError(f"WavSessionPool: template= has unknown keys {unknown}; it takes {list(self._TEMPLATE_KEYS)}")
        if not hasattr(frontend, "wav_pool") or not hasattr(generator, "session_pool"):
            raise ValueError(f"WavSessionPool needs a front-end with wav_pool() and a generator with session_pool(), got "
                             f"{type(frontend).__name__} and {type(generator).__name__}")
        self.in_pool = self.out_pool = self.wav_pool = self.gen_pool = self.template_pool = self.shift_pool = None
        wav_chunk = max_chunk_samples
        if input_resample is None and output_resample is None and pitch_shift is None:
            self.wav_pool = frontend.wav_pool(sessions, max_chunk_samples)
        else:
            sr = getattr(frontend, "sampling_rate", None) or getattr(frontend, "sample_rate", None)
            if pitch_shift is not None:
                if not hasattr(pitch_shift, "pool") or not hasattr(pitch_shift, "sample_rate"):
                    raise ValueError(f"WavSessionPool: pitch_shift must be a vocoder_amd.pitch_shift.PitchShift, got {type(pitch_shift).__name__}")
                if sr is not None and int(pitch_shift.sample_rate) != int(sr):
                    raise ValueError(f"WavSessionPool: pitch_shift has sample_rate = {pitch_shift.sample_rate} Hz, but it feeds a front-end that "
                                     f"runs at {sr} Hz")
            for name, r, end, what in (("input_resample", input_resample, "new_freq", "feeds"),
                                       ("output_resample", output_resample, "orig_freq", "takes the audio of")):
                if r is None:
                    continue
                if not hasattr(r, "pool") or not hasattr(r, end):
                    raise ValueError(f"WavSessionPool: {name} must be a vocoder_amd.resample.Resample, got {type(r).__name__}")
                if sr is not None and int(getattr(r, end)) != int(sr):
                    raise ValueError(f"WavSessionPool: {name} has {end} = {getattr(r, end)} Hz, but it {what} a front-end that runs at {sr} Hz")
            try:
                wav_chunk = max_chunk_samples
                if input_resample is not None:
                    self.in_pool = input_resample.pool(sessions, max_chunk_samples)
                    wav_chunk = max(self.in_pool.max_outputs, 1)
                if pitch_shift is not None:    # the wav and template pools are sized by what one shifter item can emit
                    self.shift_pool = pitch_shift.pool(sessions, wav_chunk)
                    wav_chunk = max(self.shift_pool.max_outputs, 1)
                self.wav_pool = frontend.wav_pool(sessions, wav_chunk)
            except Exception:
                self.close()
                raise
        try:
            release = self.wav_pool.max_frames
            if template is not None:
                from .f0 import TemplatePool
                sr = getattr(frontend, "sampling_rate", None) or getattr(frontend, "sample_rate", None)
                if sr is None:
                    raise ValueError("WavSessionPool: template= needs a front-end that declares its sample rate")
                self.template_pool = TemplatePool(int(sr), self.wav_pool.hop, sessions, wav_chunk, **template)
                # after a step one of a session's two waiting lists is empty, so the join releases at most what one branch emits in one step
                release = max(release, self.template_pool.max_frames)
            self.gen_pool = generator.session_pool(sessions, max_chunk_frames=release)
            if output_resample is not None:    # a flush emits at most the chunk's frames plus the lookahead the pool still held back
                gp = self.gen_pool
                self.out_pool = output_resample.pool(sessions * gp.out_channels, (gp.max_chunk_frames + gp.lookahead_frames) * gp.hop)
        except Exception:
            self.close()
            raise
        if self.gen_pool.in_channels != self.wav_pool.out_channels:
            self.close()
            raise ValueError(f"the front-end emits {self.wav_pool.out_channels} channels, the generator takes {self.gen_pool.in_channels}")
        self.sessions, self.max_chunk_samples, self.hop = int(sessions), int(max_chunk_samples), self.gen_pool.hop
        if self.template_pool is not None and self.wav_pool.hop != self.hop:
            self.close()
            raise ValueError(f"the front-end's hop is {self.wav_pool.hop} samples, the generator's {self.hop}")
        # per session: mel frames (C, r) / template samples (r * hop,) one branch has emitted ahead of the other; None: nothing waits
        self._mel_wait = [None] * self.sessions
        self._template_wait = [None] * self.sessions

    @torch.no_grad()
    def step(self, items) -> list:
        """One step for ``items`` (see the class); returns each item's audio, views of one output buffer."""
        wp, gp, tp = self.wav_pool, self.gen_pool, self.template_pool
        wp._check_open()
        gp._check_open()
        meta, rows = [], []
        for it in map(tuple, items):
            s, x, end = it[0], it[1], it[2] if len(it) > 2 else False
            if x is not None and x.dim() != 1:
                raise ValueError(f"expected a 1-D chunk of samples, got {tuple(x.shape)}")
            rows.append(x)
            meta.append((int(s), 0 if x is None else int(x.shape[0]), bool(end)))
        ip, sp, op, C = self.in_pool, self.shift_pool, self.out_pool, gp.out_channels
        for pool in (ip, sp, op) + ((tp.tracker, tp.template) if tp is not None else ()):
            if pool is not None:
                pool._check_open()
        # every stage's plan before anything moves (each refuses what its library would); the counts pass from stage to stage as host integers
        shift_items = meta if ip is None else [(s, k, end) for (s, _, end), k in zip(meta, ip.counters.plan(meta))]
        wav_items = shift_items if sp is None else [(s, k, end) for (s, _, end), k in zip(meta, sp.counters.plan(shift_items))]
        frames = wp.counters.plan(wav_items)
        release = frames if tp is None else self._plan_join(wav_items, frames, tp.counters.plan(wav_items)[1])
        gen_items = [(s, k, end) for (s, _, end), k in zip(meta, release)]
        emit = gp.state.plan(gen_items).emit_frames
        if op is not None:
            out_items = [(s * C + ch, k * self.hop, end) for (s, _, end), k in zip(meta, emit) for ch in range(C)]
            op.counters.plan(out_items)
        chunks = self._chunks(meta, rows)
        if ip is not None:
            chunks, _ = ip.step_padded(meta, chunks)
            chunks = chunks if chunks.shape[1] else None
        if sp is not None:
            chunks, _ = sp.step_padded(shift_items, chunks)
            chunks = chunks if chunks.shape[1] else None
        mel, _ = wp.step_padded(wav_items, chunks)
        if tp is None:
            audio, out_frames = gp.step_padded(gen_items, mel if mel.shape[2] else None)
        else:
            tmpl, tframes = tp.step_padded(wav_items, chunks)
            audio, out_frames = gp.step_padded(gen_items, *self._join(gen_items, mel, frames, tmpl, tframes))
        if op is None:
            return [audio[i, :, :k * self.hop] for i, k in enumerate(out_frames)]
        flat = audio.reshape(len(meta) * C, audio.shape[2])
        out, got = op.step_padded(out_items, flat if flat.shape[1] else None)
        return [out[i * C:(i + 1) * C, :got[i * C]] for i in range(len(meta))]

    def _waiting(self, s: int) -> tuple:
        """Frames of session ``s`` that wait in the mel branch and in the template branch (one of the two is 0)."""
        m, t = self._mel_wait[s], self._template_wait[s]
        return (0 if m is None else int(m.shape[1])), (0 if t is None else int(t.shape[0]) // self.hop)

    def _plan_join(self, items, mel_frames, template_frames) -> list:
        """Frames every item releases into the generator pool: what both branches have emitted, waiting frames included.  Host only."""
        release = []
        for i, ((s, _, end), fm, ft) in enumerate(zip(items, mel_frames, template_frames)):
            wm, wt = self._waiting(s)
            if end and wm + fm != wt + ft:
                raise ValueError(f"session {s} (item {i}) ends with {wm + fm} frames from the log-mel front-end and {wt + ft} from the pitch "
                                 f"template: the generator takes one template frame of {self.hop} samples per mel frame")
            release.append(min(wm + fm, wt + ft))
        return release

    def _join(self, gen_items, mel, mel_frames, tmpl, template_frames) -> tuple:
        """``(chunks, templates)`` for ``SessionPool.step_padded``: per item the waiting frames, then this step's, cut at what the item
        releases; the rest waits.  Device copies only; every count is a host integer."""
        hop, count = self.hop, len(gen_items)
        width = max((n for _, n, _ in gen_items), default=0)
        if not any(self._mel_wait[s] is not None or self._template_wait[s] is not None for s, _, _ in gen_items) \
                and all(n == fm == ft for (_, n, _), fm, ft in zip(gen_items, mel_frames, template_frames)) \
                and mel.shape[2] == width and tmpl.shape[1] == width * hop:
            return (mel, tmpl[:, None, :]) if width else (None, None)      # nothing waits and nothing will: the two buffers as they stand
        chunks = torch.zeros((count, mel.shape[1], width), dtype=torch.float32, device=mel.device) if width else None
        templates = torch.zeros((count, 1, width * hop), dtype=torch.float32, device=mel.device) if width else None
        for i, ((s, n, _), fm, ft) in enumerate(zip(gen_items, mel_frames, template_frames)):
            m, t = mel[i, :, :fm], tmpl[i, :ft * hop]
            if self._mel_wait[s] is not None:
                m = torch.cat([self._mel_wait[s], m], dim=1)
            if self._template_wait[s] is not None:
                t = torch.cat([self._template_wait[s], t])
            if n:
                chunks[i, :, :n] = m[:, :n]
                templates[i, 0, :n * hop] = t[:n * hop]
            self._mel_wait[s] = m[:, n:].clone() if m.shape[1] > n else None
            self._template_wait[s] = t[n * hop:].clone() if t.shape[0] > n * hop else None
        return chunks, templates

    def _chunks(self, meta, rows):
        """The items' samples as the padded ``(count, longest)`` buffer the first pool takes; ``None`` when no item has any."""
        longest = max((c for _, c, _ in meta), default=0)
        if not longest:
            return None
        chunks = torch.zeros((len(meta), longest), dtype=torch.float32, device=self.wav_pool._engine.device)
        for i, x in enumerate(rows):
            if x is not None and x.shape[0]:
                chunks[i, :x.shape[0]] = x
        return chunks

    def reset(self, session: int) -> None:
        """The next utterance of one slot, in every pool."""
        if self.in_pool is not None:
            self.in_pool.reset(session)
        if self.shift_pool is not None:
            self.shift_pool.reset(session)
        self.wav_pool.reset(session)
        self.gen_pool.reset(session)
        if self.template_pool is not None:
            self.template_pool.reset(session)
            self._mel_wait[int(session)] = self._template_wait[int(session)] = None
        if self.out_pool is not None:
            for ch in range(self.gen_pool.out_channels):
                self.out_pool.reset(int(session) * self.gen_pool.out_channels + ch)

    def close(self) -> None:
        for name in ("in_pool", "shift_pool", "wav_pool", "template_pool", "gen_pool", "out_pool"):
            if getattr(self, name, None) is not None:
                getattr(self, name).close()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()


def _wav_chunks(path, chunk: int):
    """A PCM wav (every width ``read_wav`` takes) ``chunk`` frames at a time: yields ``(channels, c)`` float32 tensors, read as the loop asks
    for them; together they are ``read_wav``'s samples."""
    with wave.open(str(path), "rb") as w:
        nch, width = w.getnchannels(), w.getsampwidth()
        while True:
            raw = w.readframes(chunk)      # whole frames: at most chunk * nch * width bytes
            if not raw:
                return
            yield torch.from_numpy(_decode_pcm(raw, width, nch, path))


class _WavSink:
    """16-bit PCM wav of ``channels`` channels written piece by piece: each ``(B, 1, k)`` tensor becomes ``k`` frames of ``B`` channels
    (``write_wav``'s rounding).  The header is complete from the start, so closing a sink that received nothing leaves an empty wav."""

    def __init__(self, path, sampling_rate: int, channels: int):
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        self._w, self.frames = wave.open(str(path), "wb"), 0
        self._w.setnchannels(int(channels))
        self._w.setsampwidth(2)
        self._w.setframerate(int(sampling_rate))

    def __call__(self, y: torch.Tensor) -> None:
        a = y[:, 0].cpu().numpy().T
        self._w.writeframes((np.clip(a, -1.0, 1.0) * 32767.0).round().astype("<i2").tobytes())
        self.frames += a.shape[0]

    def close(self) -> None:
        self._w.close()


def _main_wav_streamed(a, model, f, out, to_out, out_rate) -> None:
    """One .wav under --chunk-frames: read, converted and written ``chunk_frames * hop`` samples at a time."""
    with wave.open(str(f), "rb") as w:
        sr, total, nch = w.getframerate(), w.getnframes(), w.getnchannels()
    if total == 0:
        raise ValueError(f"{f}: the file holds no samples")
    to_model = None
    if sr != model.sampling_rate:
        if not a.resample:
            raise ValueError(f"{f}: {sr} Hz, the model runs at {model.sampling_rate} Hz and this tool does not resample")
        from .resample import Resample
        to_model = Resample(sr, model.sampling_rate)
    sink = _WavSink(out, out_rate, nch)
    t0 = time.time()
    try:
        _, stats = stream_wav_synthesis(model, _wav_chunks(f, a.chunk_frames * model.hop_length), total, a.chunk_frames, to_model, to_out, sink)
    finally:
        sink.close()
    print(f"{f}: {sink.frames / out_rate:.2f}s of audio in {time.time() - t0:.4f}s, wav -> wav streamed in {a.chunk_frames}-frame chunks: "
          f"first audio after {stats['first_audio_s'] * 1e3:.2f} ms ({stats['reads_before_first_audio']} of {stats['reads']} chunks read), "
          f"per-chunk p50 {np.percentile(stats['push_s'], 50) * 1e3:.2f} ms")


def _pitch_shifted(a, model, y: torch.Tensor) -> torch.Tensor:
    """test.py:61-62: ``librosa.effects.pitch_shift(gt_y, sr=sr, n_steps=cfg.pitch_shift)`` after loading / resampling, before the zero padding
    and the mel front-end; every row of ``y`` (..., L) on its own, on the GPU.  ``--pitch-shift 0`` (the default) returns ``y``."""
    if not a.pitch_shift:
        return y
    from .pitch_shift import PitchShift
    return PitchShift(model.sampling_rate, a.pitch_shift)(y)


def takes_template(generator: nn.Module) -> bool:
    """Does ``generator.forward`` take a pitch template next to the mel (refinegan.py:287; hifigan.py:226 / bigvgan.py with use_template)?"""
    from .modules.generators.refinegan import RefineGANGenerator
    return isinstance(generator, RefineGANGenerator) or bool(getattr(generator, "use_template", False))


def _wav_template(a, model, y: torch.Tensor) -> torch.Tensor:
    """The template of the rows ``y`` (..., L) — the samples the mel is made from: after loading, --resample, --pitch-shift and the zero
    padding — ``(..., 1, (L // hop) * hop)``, on the GPU."""
    from .f0 import template_from_audio
    return template_from_audio(y, model.sampling_rate, model.hop_length, fmin=a.f0_min, fmax=a.f0_max, threshold=a.f0_threshold,
                               kind=a.template_kind)


def _sidecar_template(a, model, f, mel: torch.Tensor) -> torch.Tensor:
    """The template of a mel input ``(B, num_mels, T)`` from ``<stem>.f0.npy``: Hz per mel frame, 0 in unvoiced frames, ``(T,)`` or
    ``(B, T)``; ``(B, 1, T * hop)``."""
    from .f0 import PitchTemplate
    side = f.with_suffix(".f0.npy")
    if not side.is_file():
        raise ValueError(f"{f}: {type(model.generator).__name__} takes a pitch template and a mel input carries no audio to track; {side} "
                         "(frame-level F0 in Hz, 0 = unvoiced) is missing")
    f0 = np.load(side, allow_pickle=False)
    B, T = int(mel.shape[0]), int(mel.shape[-1])
    if f0.ndim == 1:
        f0 = f0[None]
    if f0.ndim != 2 or f0.shape[1] != T or f0.shape[0] not in (1, B):
        raise ValueError(f"{side}: F0 of shape {tuple(np.load(side, allow_pickle=False).shape)}, the mel {f} has {T} frames"
                         + (f" in {B} items" if B > 1 else ""))
    f0 = torch.from_numpy(np.array(np.broadcast_to(f0, (B, T)), dtype=np.float32)).to(model.device)      # (a writable copy)
    return PitchTemplate(model.sampling_rate, model.hop_length, kind=a.template_kind)(f0)


def _wav_rows(a, model, f) -> torch.Tensor:
    """A .wav as the whole-file branch prepares it (test.py:50-68): channels -> rows at the model's rate, pitch shift, zero padding;
    ``(channels, L)``."""
    y, sr = read_wav(f)
    if sr != model.sampling_rate and not a.resample:
        raise ValueError(f"{f}: {sr} Hz, the model runs at {model.sampling_rate} Hz and this tool does not resample")
    y = torch.from_numpy(y).to(model.device)
    if sr != model.sampling_rate:      # test.py:54: librosa.load(..., sr=cfg.model.sampling_rate), file by file
        from .resample import Resample
        y = Resample(sr, model.sampling_rate)(y)
    y = _pitch_shifted(a, model, y)    # each file on its own, before the ragged call
    return torch.nn.functional.pad(y, (0, _pad_samples(model.hop_length, y.shape[-1])))


def _main_batched(a, model, files, base) -> None:
    """--batch-size N: the mel files N at a time, each batch (every mel of a file one utterance) through one ``forward_list`` call."""
    if not hasattr(model.generator, "forward_list"):
        raise ValueError(f"--batch-size: {type(model.generator).__name__} has no forward_list()")
    for i in range(0, len(files), a.batch_size):
        chunk = files[i:i + a.batch_size]
        mels, owner = [], []
        templates = [] if takes_template(model.generator) else None
        for f in chunk:
            if f.suffix == ".wav":     # the rows of every .wav of the batch go through the front-end together, below
                rows = _wav_rows(a, model, f)
                mels.extend(rows[b] for b in range(rows.shape[0]))
                owner.extend([f] * rows.shape[0])
                if templates is not None:
                    templates.extend(_wav_template(a, model, rows))
                continue
            mel = torch.load(f, map_location="cpu", weights_only=True)
            if a.diffsinger:
                mel = diffsinger_mel_to_ln(mel)
            mel = prepare_mel(mel, model.num_mels).to(model.device)
            mels.extend(mel[b] for b in range(mel.shape[0]))
            owner.extend([f] * mel.shape[0])
            if templates is not None:
                templates.extend(_sidecar_template(a, model, f, mel))
        wav_at = [j for j, o in enumerate(owner) if o.suffix == ".wav"]
        if wav_at:
            for j, m in zip(wav_at, model.mel_transform.forward_list([mels[j] for j in wav_at])):
                mels[j] = m
        t0 = time.time()
        waves = model.generator.forward_list(mels) if templates is None else model.generator.forward_list(mels, templates)
        torch.cuda.synchronize()
        secs = sum(w.shape[-1] for w in waves) / model.sampling_rate
        print(f"{len(chunk)} files ({chunk[0]} ...): {secs:.2f}s of audio in {time.time() - t0:.4f}s, one ragged forward")
        for f in chunk:
            fake = torch.stack([w for w, o in zip(waves, owner) if o is f])      # (B, 1, T): the items of one file share a length
            write_wav(Path(a.output_path) / f.relative_to(base).with_suffix(".wav"), fake.squeeze(1).cpu().numpy().T, model.sampling_rate)


def _main_sessions(a, model, files, base) -> None:
    """--chunk-frames n --sessions N: N mel files in flight through one session pool (``generator.session_pool``).  Every step gives each live
    session its next n frames (the last chunk flushes it); a file ends at its own length and its slot takes the next file."""
    if any(f.suffix == ".wav" for f in files):
        raise ValueError("--sessions takes mel inputs (.pt / .pth); run .wav inputs without it")
    if not hasattr(model.generator, "session_pool"):
        raise ValueError(f"--sessions: {type(model.generator).__name__} has no session_pool()")
    n, queue, steps = a.chunk_frames, list(files), 0
    slots: list = [None] * min(a.sessions, max(len(files), 1))      # per slot: [file, mel (num_mels, T), frames pushed, outputs]
    t0 = time.time()
    secs = 0.0
    with model.generator.session_pool(sessions=len(slots), max_chunk_frames=n) as pool:
        while queue or any(s is not None for s in slots):
            for i, s in enumerate(slots):
                if s is None and queue:
                    f = queue.pop(0)
                    mel = torch.load(f, map_location="cpu", weights_only=True)
                    if a.diffsinger:
                        mel = diffsinger_mel_to_ln(mel)
                    mel = prepare_mel(mel, model.num_mels).to(model.device)
                    if mel.shape[0] != 1:
                        raise ValueError(f"{f}: --sessions takes one utterance per file, got a batch of {mel.shape[0]}")
                    slots[i] = [f, mel[0], 0, []]
            live = [i for i, s in enumerate(slots) if s is not None]
            items = []
            for i in live:
                _, mel, done, _ = slots[i]
                items.append((i, mel[:, done:done + n], done + n >= mel.shape[1]))
            outs = pool.step(items)
            steps += 1
            for i, (_, chunk, last), y in zip(live, items, outs):
                s = slots[i]
                s[2] += chunk.shape[1]
                s[3].append(y.clone())      # (the views share one buffer per step)
                if last:
                    fake = torch.cat(s[3], dim=-1)
                    secs += fake.shape[-1] / model.sampling_rate
                    write_wav(Path(a.output_path) / s[0].relative_to(base).with_suffix(".wav"), fake.cpu().numpy().T, model.sampling_rate)
                    pool.reset(i)
                    slots[i] = None
        torch.cuda.synchronize()
    print(f"{len(files)} files: {secs:.2f}s of audio in {time.time() - t0:.4f}s, {len(slots)} sessions in one pool, {steps} steps of "
          f"{n}-frame chunks")


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser(description="mel (.pt) or audio (.wav) -> wav on the MI355X engine (mirrors fish_vocoder/test.py)")
    ap.add_argument("--generator", default="hifigan")
    ap.add_argument("--resolution", default="44100_512_2048")
    ap.add_argument("--config-root", default=None, help="use another configs/ tree (e.g. the reference's)")
    ap.add_argument("--ckpt-path", required=True)
    ap.add_argument("--input-path", required=True)
    ap.add_argument("--output-path", required=True)
    ap.add_argument("--num-mels", type=int, default=None)
    ap.add_argument("--diffsinger", action="store_true", help="inputs are log10 mels")
    ap.add_argument("--trust-checkpoint", action="store_true",
                    help="fall back to a full unpickle (like the reference's plain torch.load) when the weights-only loader "
                         "refuses a Lightning checkpoint that holds non-tensor objects")
    ap.add_argument("--chunk-frames", type=int, default=None,
                    help="push each input through a stream, N mel frames at a time (same wav as the whole-utterance run, within 1 LSB); a "
                         ".wav (any PCM width the whole-file run reads) is read, converted and written N * hop samples at a time (log-mel "
                         "stream -> generator stream); prints the "
                         "time to first audio and the per-chunk p50 latency")
    ap.add_argument("--batch-size", type=int, default=None,
                    help="take the inputs N files at a time and run each batch of utterances, whatever their lengths, through ONE ragged "
                         "forward (generator.forward_list; .wav inputs through the front-end's forward_list first); same wavs as the "
                         "one-by-one run, within 1 LSB")
    ap.add_argument("--sessions", type=int, default=None,
                    help="with --chunk-frames: keep N mel (.pt / .pth) files in flight through ONE session pool (generator.session_pool); each "
                         "file ends at its own length and its slot takes the next file; same wavs as the one-by-one run, within 1 LSB")
    ap.add_argument("--resample", action="store_true",
                    help="convert a .wav whose sampling rate is not the model's to the model's rate on the GPU (the reference's "
                         "librosa.load(sr=...)); without it such a file is refused")
    ap.add_argument("--output-rate", type=int, default=None, metavar="HZ",
                    help="convert the generated audio to HZ on the GPU before it is written (with --chunk-frames: chunk by chunk through a "
                         "resample stream); not with --batch-size / --sessions")
    ap.add_argument("--pitch-shift", type=float, default=0.0, metavar="N_STEPS",
                    help="shift every .wav input by N_STEPS semitones on the GPU after loading and --resample, before the mel front-end (the "
                         "reference's librosa.effects.pitch_shift, test.py:61-62); whole files and --batch-size, not mel inputs, "
                         "--chunk-frames or --sessions")
    ap.add_argument("--f0-min", type=float, default=40.0, metavar="HZ",
                    help="lowest F0 the tracker searches, for a generator that takes a pitch template (RefineGAN, use_template=True)")
    ap.add_argument("--f0-max", type=float, default=1100.0, metavar="HZ", help="highest F0 the tracker searches")
    ap.add_argument("--f0-threshold", type=float, default=0.1, help="YIN's voicing threshold on the normalised difference function, in (0, 1]")
    ap.add_argument("--template-kind", choices=("sine", "sawtooth"), default="sine", help="waveform of the pitch template")
    ap.add_argument("--noise-seed", type=int, default=None, metavar="N",
                    help="RefineGAN: AdaIN's noise (refinegan.py:125) is computed inside the kernels from this seed instead of drawn with "
                         "torch.randn per call: reproducible output, no noise tensor, whole files of any length")
    a = ap.parse_args(argv)
    if a.noise_seed is not None and not 0 <= a.noise_seed < 1 << 64:
        ap.error("--noise-seed is an unsigned 64-bit integer")
    if a.pitch_shift and (a.chunk_frames is not None or a.sessions is not None):
        raise ValueError("--pitch-shift is not available with --chunk-frames / --sessions on the command line: run the files whole or under "
                         "--batch-size, or call stream_wav_synthesis(pitch_shift=PitchShift(...)), which shifts chunk by chunk")
    if a.output_rate is not None and a.output_rate < 1:
        ap.error("--output-rate must be >= 1 Hz")
    if a.output_rate is not None and (a.batch_size is not None or a.sessions is not None):
        ap.error("--output-rate is not available with --batch-size / --sessions yet: run those at the model's rate, or the files one by one")
    if a.chunk_frames is not None and a.chunk_frames < 1:
        ap.error("--chunk-frames must be >= 1")
    if a.sessions is not None and (a.sessions < 1 or a.chunk_frames is None or a.batch_size is not None):
        ap.error("--sessions must be >= 1, needs --chunk-frames and cannot be combined with --batch-size")
    if a.batch_size is not None and (a.batch_size < 1 or a.chunk_frames is not None):
        ap.error("--batch-size must be >= 1 and cannot be combined with --chunk-frames")
    model = build_model(a.generator, a.resolution, {"num_mels": a.num_mels} if a.num_mels else None, a.config_root,
                        a.ckpt_path, device="cpu", trust_checkpoint=a.trust_checkpoint)      # (on the host first: the refusal below needs no GPU)
    if a.noise_seed is not None:
        if not hasattr(model.generator, "set_noise_seed"):
            raise ValueError(f"--noise-seed: {type(model.generator).__name__} draws no noise (RefineGAN's AdaIN layers do)")
        model.generator.set_noise_seed(a.noise_seed)
    with_template = takes_template(model.generator)
    if with_template and (a.chunk_frames is not None or a.sessions is not None):
        raise ValueError(f"{type(model.generator).__name__} takes a pitch template, and the template has no streaming form yet (it would carry "
                         "the oscillator's phase and half a tracker frame of lookahead): run without --chunk-frames / --sessions, whole files "
                         "or --batch-size")
    model = model.to("cuda")
    inp = Path(a.input_path)
    files = [inp] if inp.is_file() else sorted(p for p in inp.rglob("*") if p.suffix in (".pt", ".pth", ".wav"))
    base = inp.parent if inp.is_file() else inp
    out_rate = a.output_rate if a.output_rate is not None else model.sampling_rate
    to_out = None
    if out_rate != model.sampling_rate:
        from .resample import Resample
        to_out = Resample(model.sampling_rate, out_rate)
    if a.pitch_shift and any(f.suffix != ".wav" for f in files):
        raise ValueError(f"--pitch-shift takes .wav inputs ({next(f for f in files if f.suffix != '.wav')} is a mel): the shift is applied to the "
                         "waveform in front of the mel front-end")
    if a.batch_size:
        return _main_batched(a, model, files, base)
    if a.sessions:
        return _main_sessions(a, model, files, base)
    for f in files:
        if f.suffix == ".wav" and a.chunk_frames:
            _main_wav_streamed(a, model, f, Path(a.output_path) / f.relative_to(base).with_suffix(".wav"), to_out, out_rate)
            continue
        if f.suffix == ".wav":   # test.py:50-71: channels -> batch items, zero padding, mel_transforms.input
            y, sr = read_wav(f)
            if sr != model.sampling_rate and not a.resample:
                raise ValueError(f"{f}: {sr} Hz, the model runs at {model.sampling_rate} Hz and this tool does not resample")
            y = torch.from_numpy(y)[:, None]
            if sr != model.sampling_rate:      # test.py:54: librosa.load(..., sr=cfg.model.sampling_rate)
                from .resample import Resample
                y = Resample(sr, model.sampling_rate)(y.to(model.device))
            y = _pitch_shifted(a, model, y.to(model.device))      # test.py:61-62
            y = torch.nn.functional.pad(y, (0, model.hop_length - (model.hop_length % y.shape[-1])))   # as written upstream
            mel = model.mel_transform(y.to(model.device).squeeze(1))
            template = _wav_template(a, model, y.squeeze(1)) if with_template else None
        else:
            mel = torch.load(f, map_location="cpu", weights_only=True)
            if a.diffsinger:
                mel = diffsinger_mel_to_ln(mel)
            mel = prepare_mel(mel, model.num_mels).to(model.device)
            template = _sidecar_template(a, model, f, mel) if with_template else None
        t0 = time.time()
        if a.chunk_frames:
            fake, first, lat = stream_synthesis(model.generator, mel, a.chunk_frames, resample=to_out)
            print(f"{f}: {fake.shape[-1] / out_rate:.2f}s of audio in {time.time() - t0:.4f}s, streamed in {a.chunk_frames}-frame "
                  f"chunks: first audio after {first * 1e3:.2f} ms, per-chunk p50 {np.percentile(lat, 50) * 1e3:.2f} ms")
        else:
            fake = model(None, None, input_spec=mel, template=template)[0]
            if to_out is not None:
                fake = to_out(fake)
            torch.cuda.synchronize()
            print(f"{f}: {fake.shape[-1] / out_rate:.2f}s of audio in {time.time() - t0:.4f}s")
        out = Path(a.output_path) / f.relative_to(base).with_suffix(".wav")
        write_wav(out, fake.squeeze(1).cpu().numpy().T, out_rate)


if __name__ == "__main__":
    main()
