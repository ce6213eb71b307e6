"""Drop-in for ``fish_vocoder.modules.encoders.convnext.ConvNeXtEncoder`` (reference convnext.py:146-214).

Keys: ``downsample_layers.{i}.{0,1}``, ``stages.{i}.{j}.{dwconv,norm,pwconv1,pwconv2}.{weight,bias}``,
``stages.{i}.{j}.gamma``, ``norm.{weight,bias}``.  Eval-mode semantics only (DropPath is identity).  Engine side:
depthwise conv + LayerNorm fused in one kernel, the two pointwise Linear layers run as 1x1 convs on the fp32 MFMA
kernel with GELU / layer-scale + residual fused into their epilogues.

``stream()`` is the windowed engine stream (every push recomputes a window; 2e-5 of the whole row).  ``layer_stream(batch,
max_chunk_frames)`` is the encoder layer by layer (``ConvNeXtStream``, ``fv_cnxstream_*``): every block keeps the last 6 columns of its
input in a ring and a push runs each layer over its new columns only; the concatenated frames have the bits of ``forward`` with
``batch_invariant = True``, ``3 * (1 + sum(depths))`` frames behind the input.  Where ``input_channels == dims[0]`` the stem is a C -> C
conv with a Winograd form, whose bits depend on the launch's alignment: the stream runs it as direct sums, and the bits are those of
``forward`` with ``conv_algorithm = "direct"`` as well (``stem_has_winograd_form``).  ``layer_pool(sessions, max_chunk_frames)`` is the
same for sessions that advance independently (``ConvNeXtPool``, ``fv_cnxpool_*``): per-slot rings and packed per-frame work.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import _base
from ... import _lib
from ..._frames import _MSG_DEVICE, _MSG_INFERENCE, FramePoolCounters, _FramePool, _FrameStream, schedule      # noqa: F401  (schedule: re-exported)
from ...engine import Engine, convnext_config

ConvNeXtPoolCounters = FramePoolCounters
_PAD = 3        # (7 - 1) / 2: the layer stream serves kernel_size 7


def lookahead(depths) -> int:
    """R of the layer stream: the stem and every block reach 3 frames ahead."""
    return _PAD * (1 + sum(int(d) for d in depths))


def front(N: int, level: int, flush: bool = False) -> int:
    """Where level ``level``'s output ends after ``N`` frames (level 0: the stem, 1 .. L: the blocks); csrc/cnx_stream_plan.h ``cnx_front``."""
    return N if flush else max(0, N - _PAD * (level + 1))


def ring_cap(max_chunk: int, levels: int) -> int:
    """Slots of a block's ring: the power of two >= 6 + max(max_chunk, R) (``cnx_ring_cap``)."""
    cap = 1
    while cap < 2 * _PAD + max(int(max_chunk), _PAD * (levels + 1)):
        cap <<= 1
    return cap


def pool_ring_cap(max_chunk: int, levels: int) -> int:
    """Slots of a ring of the layer pool: the power of two >= 6 + max_chunk + R — an item may flush together with its last frames, and a
    level's frontier then moves by up to ``max_chunk + R`` frames in one step (``cnx_ring_cap(cnx_pool_step(...))``)."""
    cap = 1
    while cap < 2 * _PAD + int(max_chunk) + _PAD * (levels + 1):
        cap <<= 1
    return cap


def level_plan(N0: int, N1: int, flush: bool, level: int) -> dict:
    """One block's launch of a call that takes the stream from ``N0`` to ``N1`` frames (``cnx_level_plan``): the chunk ``[in0, in1)`` from the
    level below (the ring serves ``[in0 - 6, in0)``), the output columns ``[out0, out1)`` and the workgroups per row; workgroup ``j`` owns
    the columns ``[out0 + 32 j, + 32)``, stages the frames 3 below to 3 above them and files the chunk frames from ``file_from(j)`` on."""
    in0, in1 = front(N0, level - 1), front(N1, level - 1, flush)
    out0, out1 = front(N0, level), front(N1, level, flush)
    span = max(out1 - out0, in1 - _PAD - out0)
    if in1 > in0:
        span = max(span, 1)
    tiles = (span + 31) // 32 if span > 0 else 0
    return dict(in0=in0, in1=in1, out0=out0, out1=out1, tiles=tiles,
                file_from=lambda j: in0 if j == 0 else out0 + 32 * j + _PAD)


class _LayerHandle:
    """What the layer stream and the layer pool say of themselves: one output tensor per call, and the device memory they hold."""
    hop = 1

    def _attach(self, module, engine: Engine) -> tuple:
        return engine._h, engine.in_channels, engine.out_channels

    @property
    def state_bytes(self) -> int:
        """Device memory the handle holds: the rings and one call's scratch (``fv_cnxstream_state_bytes`` / ``fv_cnxpool_state_bytes``)."""
        self._check_open()
        return int(self._entry["state_bytes"](self._h))


class ConvNeXtStream(_LayerHandle, _FrameStream):
    """``ConvNeXtEncoder`` layer by layer and chunk by chunk (``fv_cnxstream_*``, include/fishvoc.h): ``push`` a ``(B, input_channels, c)``
    chunk, ``c <= max_chunk_frames``, and get the frames that need no later input — ``[E, max(E, N - R))``, ``R = lookahead_frames``,
    possibly none; ``flush`` ends the utterance at ``N`` and returns the rest, then pushes raise until ``reset()``.  The concatenation has
    the bits of ``forward`` over the whole utterance with ``batch_invariant = True``, under any chunking (``schedule`` gives the counts).
    The ``batch`` rows advance in lockstep.  A stream dies with the module's engine: ``load_state_dict`` or ``.to()`` closes it."""
    _prefix, _noun = "fv_cnxstream", "ConvNeXt layer stream"
    _entries = _FrameStream._entries + ("state_bytes",)


class ConvNeXtPool(_LayerHandle, _FramePool):
    """``ConvNeXtEncoder`` layer by layer for sessions that advance independently (``fv_cnxpool_*``, include/fishvoc.h): what
    ``ConvNeXtStream`` is to rows in lockstep, for ``sessions`` slots with their own counters and their own row of every ring.
    ``step(items)`` takes ``(session, x, flush)`` tuples — ``x``: ``(in_channels, n)`` with ``n <= max_chunk_frames``, or ``None`` for no
    frames; ``flush``: the utterance ends with these frames — and returns per item the ``(out_channels, k)`` frames that session emits in
    this step, ``k`` possibly 0.  A session appears at most once per step and refuses items after its flush until ``reset(session)``.  The
    whole step is checked before anything moves: a refused step leaves every session as it was.  A session's concatenated frames have the
    bits of ``forward`` over its whole utterance with ``batch_invariant = True`` (and ``conv_algorithm = "direct"`` where the stem has a
    Winograd form), whatever the other sessions do and in any item order.  Work is enqueued on torch's current stream and calls must be
    ordered; the pool dies with the module's engine, as a ``ConvNeXtStream`` does."""
    _prefix, _noun = "fv_cnxpool", "ConvNeXt layer pool"
    _entries = _FramePool._entries + ("state_bytes",)


class LayerNorm(nn.Module):
    """weight/bias holder for both data formats of the reference LayerNorm (convnext.py:47-74)."""

    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        if data_format not in ("channels_last", "channels_first"):
            raise NotImplementedError
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps, self.data_format = eps, data_format


class ConvNeXtBlockParams(nn.Module):
    def __init__(self, dim, layer_scale_init_value=1e-6, mlp_ratio=4.0, kernel_size=7):
        super().__init__()
        self.dwconv = nn.Conv1d(dim, dim, kernel_size, padding=(kernel_size - 1) // 2, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, int(mlp_ratio * dim))
        self.pwconv2 = nn.Linear(int(mlp_ratio * dim), dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim)) if layer_scale_init_value > 0 else None


class ConvNeXtEncoder(_base.EngineModule):
    def __init__(self, input_channels: int = 3, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768),
                 drop_path_rate: float = 0.0, layer_scale_init_value: float = 1e-6, kernel_size: int = 7):
        super().__init__()
        assert len(depths) == len(dims)
        self._cfg = dict(input_channels=input_channels, depths=list(depths), dims=list(dims), kernel_size=kernel_size)
        self.drop_path_rate = drop_path_rate  # identity in eval (convnext.py:20-21); recorded only
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(nn.Sequential(
            nn.Conv1d(input_channels, dims[0], kernel_size, padding=kernel_size // 2),
            LayerNorm(dims[0], eps=1e-6, data_format="channels_first")))
        for i in range(len(depths) - 1):
            self.downsample_layers.append(nn.Sequential(
                LayerNorm(dims[i], eps=1e-6, data_format="channels_first"), nn.Conv1d(dims[i], dims[i + 1], 1)))
        self.stages = nn.ModuleList(
            nn.Sequential(*[ConvNeXtBlockParams(dims[i], layer_scale_init_value, kernel_size=kernel_size)
                            for _ in range(depths[i])]) for i in range(len(depths)))
        self.norm = LayerNorm(dims[-1], eps=1e-6, data_format="channels_first")
        for m in self.modules():  # trunc_normal(0.02) / zero bias, as upstream (convnext.py:201-204)
            if isinstance(m, (nn.Conv1d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.constant_(m.bias, 0)

    def _make_engine(self, state_dict):
        return Engine(_lib.FV_MODEL_CONVNEXT, backbone=convnext_config(**self._cfg), state_dict=state_dict, precision=self.precision)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._run(x)

    @property
    def stem_has_winograd_form(self) -> bool:
        """The stem is a C -> C conv (``input_channels == dims[0]``, at least 16): ``layer_stream`` then has the bits of ``forward`` with
        ``conv_algorithm = "direct"`` and ``batch_invariant = True``; otherwise ``batch_invariant`` alone decides them."""
        return self._cfg["input_channels"] == self._cfg["dims"][0] >= 16 and self._cfg["kernel_size"] in (3, 7, 11)

    @property
    def stream_is_bit_exact(self) -> bool:
        """Does a stream of this encoder have ``forward``'s bits?  ``layer_stream`` has the bits of the batch-invariant forward (with direct
        sums in a stem that has a Winograd form), so only in that mode — in which ``forward``'s own bits do not depend on the launch — is
        that a true sentence."""
        return self.batch_invariant and (not self.stem_has_winograd_form or self.conv_algorithm == "direct")

    @property
    def lookahead_frames(self) -> int:
        """R of ``layer_stream``: ``3 * (1 + sum(depths))``."""
        return lookahead(self._cfg["depths"])

    def layer_stream(self, batch: int = 1, max_chunk_frames: int = 64) -> ConvNeXtStream:
        """The encoder layer by layer and chunk by chunk (``ConvNeXtStream``): rings of 6 columns per block instead of a recomputed
        window, the bits of the batch-invariant ``forward``, ``lookahead_frames`` behind the input.  ``kernel_size`` 7, widths up to 1024,
        precision f32.  Reloading the weights or moving the module rebuilds the engine and closes its streams: create a new one then."""
        p = next(self.parameters(), None)
        if p is None or not p.is_cuda:
            raise RuntimeError(_MSG_DEVICE.format(f"{type(self).__name__}.layer_stream", getattr(p, "device", None)))
        if self.training:
            raise RuntimeError(_MSG_INFERENCE.format(type(self).__name__))
        return ConvNeXtStream(self, self.engine(p.device), batch, max_chunk_frames)

    def layer_pool(self, sessions: int, max_chunk_frames: int = 64) -> ConvNeXtPool:
        """``layer_stream`` for ``sessions`` clients that advance independently (``ConvNeXtPool``): per-slot rings, one step serves any
        subset of the sessions, and a session's frames have the bits of the batch-invariant ``forward`` of its utterance alone.  The same
        limits as ``layer_stream``; the pool is closed with the engine, as a stream is."""
        p = next(self.parameters(), None)
        if p is None or not p.is_cuda:
            raise RuntimeError(_MSG_DEVICE.format(f"{type(self).__name__}.layer_pool", getattr(p, "device", None)))
        if self.training:
            raise RuntimeError(_MSG_INFERENCE.format(type(self).__name__))
        return ConvNeXtPool(self, self.engine(p.device), sessions, max_chunk_frames)
