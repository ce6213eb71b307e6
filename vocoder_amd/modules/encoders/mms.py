"""Drop-in for the reference's ``MMSEncoder`` (fish_vocoder/modules/encoders/mms.py): resample to 16 kHz, HF's processor normalisation,
``Wav2Vec2Model`` of ``facebook/mms-300m`` (the stable-layer-norm graph of w2v.hip), then nearest-frame interpolation to ``L // hop_length``
frames, channel major.  The whole chain stays on the device::

    Resample(sampling_rate, 16000, table="global") -> fv_mms_normalize -> fv_w2v_forward (post_channels = 0) -> fv_mms_interpolate

(include/fishvoc.h, vocoder_amd/csrc/mms_front.hip); the reference moves every row through numpy between the first two steps.  With
``sampling_rate == 16000`` the resampler is skipped, as ``torchaudio.functional.resample`` returns its input there.  The output sits on the
vocoder's own frame grid, ``(B, hidden, L // hop_length)``, so the module fits the ``generator.encoder`` slot of a codec (``takes_audio``:
``VQVAECodec`` hands it the audio, vae.py:81).

The state-dict keys are the reference module's: ``model.`` + ``Wav2Vec2Model``'s keys in its order, nothing for the processor.  The legacy
``...conv.weight_g`` / ``weight_v`` names load as in ``HubertEncoder``, and ``model.masked_spec_embed`` may be absent.  It never downloads
anything: the architecture comes from ``config`` (a dict or an object with HF's field names) or from the ``config.json`` of a local directory,
the weights from ``load_state_dict``.  ``transformers`` is not imported.

Ragged rows (``forward(x, lengths=...)``, ``forward_list``): every stage takes the row's own sample count, resampled count and frame counts;
a row has the bits of the row run alone, and the output holds exact zeros past its ``lengths[b] // hop_length`` frames.  On a padded batch
this differs from the reference on purpose, as ``HubertEncoder`` does ("Encoders"): the reference normalises and attends
over the padding, this module equals the reference on the row run alone.  Not built: the group-norm / post-LN family, adapters, gradients,
f16x3.  No CPU fallback.
"""
from __future__ import annotations

import ctypes

import torch

from ... import _lib
from ..._lib import check
from ...resample import Resample
from .hubert import _BackboneModule

MODEL_RATE = 16000      # the backbone's sample rate (mms.py:21)


class MMSEncoder(_BackboneModule):
    takes_audio = True      # VQVAECodec: the encoder slot receives the audio, not the front-end's spectrogram

    def __init__(self, sampling_rate: int = 44100, hop_length: int = 512, model_name: str = "facebook/mms-300m", config=None):
        super().__init__()
        self.sample_rate, self.hop_length, self.model_name = int(sampling_rate), int(hop_length), model_name
        if self.sample_rate < 1 or self.hop_length < 1:
            raise ValueError(f"MMSEncoder: sampling_rate = {sampling_rate} and hop_length = {hop_length} must be >= 1")
        get = config.get if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
        if config is not None and get("add_adapter", False):
            raise ValueError("MMSEncoder: add_adapter = True is not supported: only the stable-layer-norm family without an adapter has kernels")
        self._init_backbone(config, model_name)
        self.resample = None if self.sample_rate == MODEL_RATE else Resample(self.sample_rate, MODEL_RATE, table="global")

    # -- frame counts -------------------------------------------------------------------------------
    def frames(self, samples: int) -> int:
        """Output frames of ``samples`` input samples: ``samples // hop_length`` (mms.py:18)."""
        return int(samples) // self.hop_length

    def resampled(self, samples: int) -> int:
        """Samples at 16 kHz: ``ceil(16000 samples / sampling_rate)``, torchaudio's count."""
        return int(samples) if self.resample is None else self.resample.output_length(int(samples))

    def backbone_frames(self, samples: int) -> int:
        """Frames the backbone yields for ``samples`` input samples: the resampler's count, then HF's ``_get_feat_extract_output_lengths``."""
        return self.conv_frames(self.resampled(samples))

    def min_samples(self) -> int:
        """The shortest input that yields one backbone frame."""
        field = 1
        for k, s in zip(reversed(self.hf_config["conv_kernel"]), reversed(self.hf_config["conv_stride"])):
            field = (field - 1) * s + k
        if self.resample is None:
            return field
        o, n = self.resample.design.o, self.resample.design.n
        return (field - 1) * o // n + 1         # the smallest L with ceil(n L / o) >= field

    # -- calls ---------------------------------------------------------------------------------
    def _run(self, x: torch.Tensor, lengths, what: str) -> torch.Tensor:
        if self.training:
            raise RuntimeError(f"{type(self).__name__} is inference-only: call .eval() first")
        B, T = (int(v) for v in x.shape)
        if lengths is not None:
            lengths = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
            if len(lengths) != B:
                raise ValueError(f"{what}: {len(lengths)} lengths for {B} rows")
            for b, v in enumerate(lengths):
                if not 0 <= v <= T:
                    raise ValueError(f"{what}: the length of row {b}, {v}, lies outside [0, T = {T}]")
        rows = [T] * B if lengths is None else lengths
        n_out, f_in = [self.frames(v) for v in rows], [self.backbone_frames(v) for v in rows]
        for b, v in enumerate(rows):
            if n_out[b] > 0 and f_in[b] == 0:
                raise ValueError(f"{what}: row {b} holds {v} samples, which give {n_out[b]} output frames but no backbone frame to take them "
                                 f"from; a row needs at least {self.min_samples()} samples")
        if not x.is_cuda:
            raise RuntimeError(
                f"{what} needs a CUDA/HIP tensor (got {x.device}); vocoder_amd has no CPU path — move the model and input to the GPU")
        x = x.detach().to(torch.float32).contiguous()
        H, N = int(self.hf_config["hidden_size"]), self.frames(T)
        out = torch.empty((B, H, N), dtype=torch.float32, device=x.device)
        if B == 0 or N == 0:
            return out
        L = _lib.lib()
        i32 = ctypes.c_int32 * B
        with torch.cuda.device(x.device):
            stream = int(torch.cuda.current_stream().cuda_stream)
            wave = x if self.resample is None else self.resample(x, lengths=lengths)
            M = int(wave.shape[1])
            mptr = None if lengths is None else i32(*(self.resampled(v) for v in lengths))
            need = int(L.fv_mms_normalize_workspace_bytes(B, M))
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
            values = torch.empty_like(wave)
            check(L.fv_mms_normalize(wave.data_ptr(), M, mptr, B, values.data_ptr(), ws.data_ptr(), need, stream))
            F = self.backbone_frames(T)
            hidden = torch.empty((B, F, H), dtype=torch.float32, device=x.device)
            if F:
                eng = self.engine(x.device)
                need = int(L.fv_w2v_workspace_bytes(eng.handle, B, M))
                ws = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
                check(L.fv_w2v_forward(eng.handle, values.data_ptr(), M, mptr, B, hidden.data_ptr(), None, ws.data_ptr(), need, stream))
            check(L.fv_mms_interpolate(hidden.data_ptr() if F else None, F, H, None if lengths is None else i32(*f_in),
                                       None if lengths is None else i32(*n_out), B, out.data_ptr(), N, stream))
        return out

    def forward(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """mms.py:17-33.  ``x``: (B, L) or (B, 1, L); ``lengths``: samples per row (a list or an int tensor), making the call ragged.
        Returns (B, hidden, L // hop_length), exact zeros past a row's ``lengths[b] // hop_length`` frames."""
        what = f"{type(self).__name__}.forward"
        if isinstance(x, torch.Tensor) and x.dim() == 3:
            if x.shape[1] != 1:
                raise ValueError(f"{what}: a 3-d input must be (B, 1, L), got {tuple(x.shape)}")
            x = x[:, 0]
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise ValueError(f"{what}: expected (B, L) or (B, 1, L), got {tuple(getattr(x, 'shape', ()))}")
        return self._run(x, lengths, what)

    def forward_list(self, waves) -> list:
        """A list of 1-d waves -> a list of (hidden, L_i // hop_length) through one padded call."""
        waves = list(waves)
        if not waves:
            return []
        what = f"{type(self).__name__}.forward_list"
        for x in waves:
            if not isinstance(x, torch.Tensor) or x.dim() != 1:
                raise ValueError(f"{what}: expected 1-d tensors, got {tuple(getattr(x, 'shape', ()))}")
        lengths = [int(x.shape[0]) for x in waves]
        padded = torch.zeros((len(waves), max(lengths)), dtype=torch.float32, device=waves[0].device)
        for b, x in enumerate(waves):
            padded[b, : lengths[b]] = x
        out = self._run(padded, lengths, what)
        return [out[b, :, : self.frames(n)] for b, n in enumerate(lengths)]

    def extra_repr(self) -> str:
        c = self.hf_config
        return (f"sampling_rate={self.sample_rate}, hop_length={self.hop_length}, hidden_size={c['hidden_size']}, "
                f"layers={c['num_hidden_layers']}, heads={c['num_attention_heads']}, backend=libfishvoc_hip (gfx950)")
