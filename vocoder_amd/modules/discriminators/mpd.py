"""Drop-ins for the reference's ``DiscriminatorP`` and ``MultiPeriodDiscriminator`` (fish_vocoder/modules/discriminators/mpd.py): the
forward in eval mode on the ``fv_disc_*`` kernels (include/fishvoc.h, vocoder_amd/csrc/disc.hip).

The modules hold ordinary torch parameters under exactly the reference's keys — ``discriminators.{i}.convs.{l}.bias`` and
``.parametrizations.weight.original0 / original1``, then ``conv_post`` — so a checkpoint loads strictly; the holders are never called.  The
legacy ``weight_g`` / ``weight_v`` names are taken too.  A row has the same bits alone, in any batch and padded to any T; on a padded batch
(``forward(x, lengths=)``, ``forward_list``) every row is the reference run on the row alone.  Not built: spectral norm, gradients, f16x3.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch
from torch import nn

from ... import _lib
from ._critic import Critic, normed_conv, refuse_spectral_norm


def _period_config(periods, channels, kernel_size: int, stride: int) -> "_lib.DiscConfig":
    if not 1 <= len(periods) <= _lib.DISC_MAX_SUB:
        raise ValueError(f"periods: {len(periods)} sub-discriminators; the library takes 1 to {_lib.DISC_MAX_SUB}")
    if not 2 <= len(channels) <= _lib.DISC_MAX_CHANNELS:
        raise ValueError(f"channels: {len(channels)} entries; the library takes 2 to {_lib.DISC_MAX_CHANNELS}")
    cfg = _lib.DiscConfig()
    cfg.kind, cfg.n_sub, cfg.n_channels, cfg.kernel_size, cfg.stride = _lib.FV_DISC_PERIOD, len(periods), len(channels), kernel_size, stride
    for i, p in enumerate(periods):
        cfg.period[i] = int(p)
    for i, c in enumerate(channels):
        cfg.channels[i] = int(c)
    return cfg


def period_extents(L: int, period: int, n_convs: int, kernel_size: int = 5, stride: int = 3) -> list:
    """(H, W) after every conv of a ``DiscriminatorP`` and after ``conv_post`` for ``L`` samples: mpd.py:47-59."""
    h = -(-L // period)
    out = []
    for _ in range(n_convs):
        h = (h + 2 * (kernel_size // 2) - kernel_size) // stride + 1
        out.append((h, period))
    return out + [(h, period)]


class DiscriminatorP(Critic):
    _multi = False

    def __init__(self, *, period: int, kernel_size: int = 5, stride: int = 3, use_spectral_norm: bool = False,
                 channels: Optional[list] = None) -> None:
        super().__init__()
        refuse_spectral_norm("DiscriminatorP", use_spectral_norm)
        self.period, self.kernel_size, self.stride = int(period), int(kernel_size), int(stride)
        self.channels = [1, 64, 128, 256, 512, 1024] if channels is None else [int(c) for c in channels]
        self._disc_config(validate=True)        # before any parameter is allocated
        self.convs = nn.ModuleList(normed_conv(cin, cout, (self.kernel_size, 1), (self.stride, 1), (self.kernel_size // 2, 0))
                                   for cin, cout in zip(self.channels[:-1], self.channels[1:]))
        self.conv_post = normed_conv(self.channels[-1], 1, (3, 1), 1, (1, 0))
        self._init_critic()

    def _disc_config(self, validate: bool = False) -> "_lib.DiscConfig":
        return self._validated(_period_config([self.period], self.channels, self.kernel_size, self.stride), validate)

    def _sub_extents(self, i: int, L: int) -> list:
        return period_extents(L, self.period, len(self.channels) - 1, self.kernel_size, self.stride)

    def extra_repr(self) -> str:
        return f"period={self.period}, channels={self.channels}, backend=libfishvoc_hip (gfx950)"


class MultiPeriodDiscriminator(Critic):
    def __init__(self, periods: Optional[list] = None):
        super().__init__()
        self.periods = [2, 3, 5, 7, 11] if periods is None else [int(p) for p in periods]
        self._disc_config(validate=True)
        self.discriminators = nn.ModuleList(DiscriminatorP(period=p) for p in self.periods)
        self._init_critic()

    def _disc_config(self, validate: bool = False) -> "_lib.DiscConfig":
        subs = self.__dict__.get("_modules", {}).get("discriminators")
        first = subs[0] if subs is not None and len(subs) else None
        channels = first.channels if first is not None else [1, 64, 128, 256, 512, 1024]
        kernel_size, stride = (first.kernel_size, first.stride) if first is not None else (5, 3)
        if subs is not None:
            for d in subs:
                if (d.channels, d.kernel_size, d.stride) != (channels, kernel_size, stride):
                    raise ValueError("MultiPeriodDiscriminator: every DiscriminatorP must share channels, kernel_size and stride "
                                     "(fv_disc_config holds one of each)")
        return self._validated(_period_config(self.periods, channels, kernel_size, stride), validate)

    def _sub_extents(self, i: int, L: int) -> list:
        return self.discriminators[i]._sub_extents(0, L)
