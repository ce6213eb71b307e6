"""Drop-in for ``fish_vocoder.modules.generators.unify.UnifyGenerator`` (reference unify.py:5-60):
``head(backbone(x), template=template)``, channel dim added for 2-D heads.  With ``vq`` (a ``modules.quantizers`` quantiser) the backbone's
output is quantised on the way (unify.py:21-23), ``forward`` returns ``(audio, vq_result)`` (unify.py:30-31), ``encode`` gives the codes and
``decode`` turns codes into audio (unify.py:35-53)."""
from __future__ import annotations

import torch
from torch import nn


class UnifyGenerator(nn.Module):
    def __init__(self, backbone: nn.Module, head: nn.Module, vq: nn.Module | None = None):
        super().__init__()
        self.backbone, self.head, self.vq = backbone, head, vq

    def forward(self, x: torch.Tensor, template=None):
        x = self.backbone(x)
        if self.vq is not None:
            vq_result = self.vq(x)
            x = vq_result.z
        x = self.head(x, template=template)
        x = x[:, None, :] if x.ndim == 2 else x
        return (x, vq_result) if self.vq is not None else x

    def encode(self, x):
        if self.vq is None:
            raise ValueError("VQ module is not present in the model.")  # unify.py:36-37
        return self.vq(self.backbone(x)).codes

    def decode(self, codes, template=None):
        if self.vq is None:
            raise ValueError("VQ module is not present in the model.")  # unify.py:44-45
        x = self.head(self.vq.from_codes(codes)[0], template=template)
        return x[:, None, :] if x.ndim == 2 else x

    def decode_stream(self, batch: int = 1, max_chunk_frames: int = 64, backbone: str = "window"):
        """``decode`` chunk by chunk (``vocoder_amd.codec.CodecDecodeStream`` on the head alone, as ``decode`` runs the head alone): codes in,
        audio out after the head's lookahead; the ring keeps the codes.  ``backbone`` is ``CodecDecodeStream``'s option: ``"layers"`` asks
        for a ConvNeXt backbone stage in front of the head, which this ``decode`` does not run, and is refused by name."""
        from ...codec import CodecDecodeStream
        if self.vq is None:
            raise ValueError("VQ module is not present in the model.")
        return CodecDecodeStream(self.head, self.vq, batch, max_chunk_frames, backbone)

    def decode_pool(self, sessions: int, max_chunk_frames: int = 64, backbone: str = "window"):
        """``decode`` for ``sessions`` clients that advance independently (``vocoder_amd.codec.CodecDecodePool`` on the head alone).
        ``backbone`` is ``CodecDecodePool``'s option: ``"layers"`` asks for a ConvNeXt backbone stage in front of the head, which this
        ``decode`` does not run, and is refused by name."""
        from ...codec import CodecDecodePool
        if self.vq is None:
            raise ValueError("VQ module is not present in the model.")
        return CodecDecodePool(self.head, self.vq, sessions, max_chunk_frames, backbone)

    def remove_parametrizations(self):
        for m in (self.backbone, self.head):
            if hasattr(m, "remove_parametrizations"):
                m.remove_parametrizations()
