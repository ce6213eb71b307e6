"""Drop-in for ``fish_vocoder.data.transforms.spectrogram.LogMelSpectrogram`` (reference spectrogram.py:59-104) —
SURVEY §8 "next" row f1: the step immediately before the generator in test.py:71, so that wav -> mel -> wav stays on
the GPU.  Same ctor kwargs and buffer names (``spectrogram.window``, ``mel_scale.fb``); ``forward(wave (B, L) or
(B, 1, L)) -> (B, n_mels, frames)`` natural-log mel with floor ln(1e-5).

Engine side (FV_MODEL_LOGMEL): reflect padding + polyphase re-layout (hop channels x n_fft/hop taps) turns the STFT into a
stride-1 conv on the fp32 MFMA kernel against a window-folded real-DFT basis; magnitude; slaney filterbank as a pointwise
conv with log(clamp) fused into its epilogue.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from ...modules import _base
from ... import _lib
from ...engine import Engine, logmel_config


def melscale_fbanks_slaney(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> torch.Tensor:
    """Triangular slaney-scale, slaney-normalised filterbank (n_freqs, n_mels) — what torchaudio's
    ``MelScale(norm="slaney", mel_scale="slaney")`` registers as its ``fb`` buffer (third-party; restated)."""
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def hz_to_mel(f: float) -> float:
        return min_log_mel + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp

    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_pts = torch.linspace(hz_to_mel(f_min), hz_to_mel(f_max), n_mels + 2, dtype=torch.float64)
    f_pts = torch.where(m_pts >= min_log_mel, min_log_hz * torch.exp(logstep * (m_pts - min_log_mel)), f_sp * m_pts)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    fb = torch.clamp(torch.min(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]), min=0.0)
    return (fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])).unsqueeze(0)).to(torch.float32)


class _FrontEnd(_base.EngineModule):
    """What both transforms add to the whole-tensor ``forward``: rows of different lengths and chunks of a stream (include/fishvoc.h
    ``fv_logmel_*``; the framing rule: ``vocoder_amd.framing``).  They replace the frame-windowed ``forward_ragged`` / ``forward_list`` /
    ``stream`` of the generators, which a front-end cannot have: it windows samples, not frames.  Its pool of independent sessions is
    ``wav_pool`` (``fv_wavpool_*``); ``session_pool`` is the base's, and the engine refuses it."""

    def frames(self, L: int) -> int:
        """Frames of a whole row of ``L`` samples."""
        return self._framing().frames(L)

    def frames_ready(self, N: int) -> int:
        """Frames that need no sample at or after ``N``."""
        return self._framing().frames_ready(N)

    def _framing(self):
        from ...framing import Framing
        return Framing(int(self.n_fft), int(self.win_length), int(self.hop_length))

    def _ragged_engine(self, what: str):
        b = next(self.buffers(), None)      # a front-end has buffers only (the window, the filterbank)
        if b is None or not b.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.{what} needs the module on a HIP device (.to('cuda')); vocoder_amd has no CPU path")
        if self.training:
            raise RuntimeError(f"{type(self).__name__} is inference-only: call .eval() first")
        return self.engine(b.device)

    def forward_ragged(self, waves: torch.Tensor, lengths):
        """``waves`` ``(B, L_max)`` or ``(B, 1, L_max)`` with ``lengths[b]`` valid samples per row -> ``(mel (B, C, frames(L_max)),
        frame_lengths)``: row ``b`` holds its own result in ``[0, frame_lengths[b])`` and zeros after it; the padding of ``waves`` is never read."""
        with torch.no_grad():
            eng = self._ragged_engine("forward_ragged")
            lengths = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
            mel = eng.logmel_ragged(waves.to(torch.float32), lengths)
            return mel, [eng.framing.frames(n) for n in lengths]

    def forward_list(self, waves) -> list:
        """A list of ``(L_i,)`` or ``(1, L_i)`` waveforms -> a list of ``(C, frames(L_i))`` views of one ``forward_ragged`` result."""
        waves = [w.reshape(-1) for w in waves]
        if not waves:
            return []
        lengths = [int(w.shape[0]) for w in waves]
        x = torch.zeros((len(waves), max(max(lengths), 1)), dtype=torch.float32, device=waves[0].device)
        for b, w in enumerate(waves):
            x[b, :lengths[b]] = w
        mel, fl = self.forward_ragged(x, lengths)
        return [mel[b, :, :fl[b]] for b in range(len(waves))]

    def stream(self, batch: int = 1, max_chunk_samples: int = 4096):
        """The front-end chunk by chunk (``vocoder_amd.engine.LogMelStream``): ``push`` at most ``max_chunk_samples`` samples per row, ``flush``
        at the utterance's end.  Reloading the weights or moving the module rebuilds the engine and closes its streams: create a new one then."""
        return self._ragged_engine("stream").logmel_stream(batch, max_chunk_samples)


    def wav_pool(self, sessions: int = 1, max_chunk_samples: int = 4096):
        """The front-end as a pool of sessions that advance independently (``vocoder_amd.engine.WavPool``): every ``step`` serves any subset of
        the ``sessions`` slots, each with its own chunk of at most ``max_chunk_samples`` samples, each ending at its own length.  Lives and
        dies with the engine like ``stream()``."""
        return self._ragged_engine("wav_pool").wav_pool(sessions, max_chunk_samples)


class LinearSpectrogram(_FrontEnd):
    """Reference spectrogram.py:8-56: reflect-padded ``torch.stft(center=False)`` magnitude ``sqrt(re^2 + im^2 + 1e-6)``,
    ``forward(y (B, L) or (B, 1, L)) -> (B, n_fft/2+1, frames)``.  Same buffer name (``window``); runs on the log-mel
    engine with the filterbank stage switched off (``n_mels = 0``).  Inside LogMelSpectrogram it only holds the window."""

    def __init__(self, n_fft=2048, win_length=2048, hop_length=512, center=False, mode="pow2_sqrt"):
        super().__init__()
        if mode != "pow2_sqrt":
            raise NotImplementedError("only mode='pow2_sqrt' (the reference default) is built")
        self.n_fft, self.win_length, self.hop_length, self.center, self.mode = n_fft, win_length, hop_length, center, mode
        self.register_buffer("window", torch.hann_window(win_length))
        self._cfg = dict(sample_rate=2, n_fft=n_fft, win_length=win_length, hop_length=hop_length, n_mels=0, center=center)
        logmel_config(**self._cfg)   # validates center=False

    def _make_engine(self, state_dict):
        sd = {"spectrogram.window": v for k, v in state_dict.items() if k == "window"}
        return Engine(_lib.FV_MODEL_LOGMEL, mel=logmel_config(**self._cfg), state_dict=sd, precision=self.precision)

    def forward(self, y: torch.Tensor) -> torch.Tensor:
        if y.ndim == 2:
            y = y[:, None, :]
        return self._run(y)


class _MelScaleBuffers(nn.Module):
    def __init__(self, fb):
        super().__init__()
        self.register_buffer("fb", fb)


class LogMelSpectrogram(_FrontEnd):
    def __init__(self, sample_rate=44100, n_fft=2048, win_length=2048, hop_length=512, n_mels=128, center=False,
                 f_min=0.0, f_max=None):
        super().__init__()
        self.sample_rate, self.n_fft, self.win_length, self.hop_length = sample_rate, n_fft, win_length, hop_length
        self.center, self.n_mels, self.f_min, self.f_max = center, n_mels, f_min, f_max or sample_rate // 2
        self._cfg = dict(sample_rate=sample_rate, n_fft=n_fft, win_length=win_length, hop_length=hop_length,
                         n_mels=n_mels, center=center, f_min=f_min, f_max=self.f_max)
        logmel_config(**self._cfg)   # validates center=False
        self.spectrogram = LinearSpectrogram(n_fft, win_length, hop_length, center)
        self.mel_scale = _MelScaleBuffers(melscale_fbanks_slaney(n_fft // 2 + 1, f_min, self.f_max, n_mels, sample_rate))

    def _make_engine(self, state_dict):
        return Engine(_lib.FV_MODEL_LOGMEL, mel=logmel_config(**self._cfg), state_dict=state_dict, precision=self.precision)

    def compress(self, x: torch.Tensor) -> torch.Tensor:
        return torch.log(torch.clamp(x, min=1e-5))

    def decompress(self, x: torch.Tensor) -> torch.Tensor:
        return torch.exp(x)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim == 2:
            x = x[:, None, :]
        return self._run(x)
