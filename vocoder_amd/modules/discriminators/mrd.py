"""Drop-ins for the reference's ``DiscriminatorR`` and ``MultiResolutionDiscriminator`` (fish_vocoder/modules/discriminators/mrd.py): the
rectangular-window STFT magnitude and the 2-D conv stack in eval mode on the ``fv_disc_*`` kernels (include/fishvoc.h,
vocoder_amd/csrc/disc.hip).

Parameters live under exactly the reference's keys, so a checkpoint loads strictly; the holders are never called.  A row has the same bits
alone, in any batch and padded to any T: its reflect padding is taken at its own ends.  A row must be longer than the padding
``(n_fft - hop + 1) // 2`` and hold one hop.  Not built: spectral norm, gradients, f16x3.
"""
from __future__ import annotations

import torch
from torch import nn

from ... import _lib
from ._critic import Critic, normed_conv, refuse_spectral_norm


def _resolution_config(resolutions) -> "_lib.DiscConfig":
    if not 1 <= len(resolutions) <= _lib.DISC_MAX_SUB:
        raise ValueError(f"resolutions: {len(resolutions)} sub-discriminators; the library takes 1 to {_lib.DISC_MAX_SUB}")
    cfg = _lib.DiscConfig()
    cfg.kind, cfg.n_sub = _lib.FV_DISC_RESOLUTION, len(resolutions)
    for i, (n_fft, hop, win) in enumerate(resolutions):
        cfg.n_fft[i], cfg.hop_length[i], cfg.win_length[i] = int(n_fft), int(hop), int(win)
    return cfg


def resolution_extents(L: int, n_fft: int, hop_length: int) -> list:
    """(H, W) after every conv of a ``DiscriminatorR`` and after ``conv_post`` for ``L`` samples: mrd.py:24-33 on ``L // hop`` frames."""
    h, w = n_fft // 2 + 1, L // hop_length
    out = [(h, w)]
    for _ in range(3):
        w = (w - 1) // 2 + 1 if w > 0 else 0
        out.append((h, w))
    return out + [(h, w), (h, w)]


class DiscriminatorR(Critic):
    _multi = False

    def __init__(self, *, n_fft: int = 1024, hop_length: int = 120, win_length: int = 600, use_spectral_norm: bool = False):
        super().__init__()
        refuse_spectral_norm("DiscriminatorR", use_spectral_norm)
        self.n_fft, self.hop_length, self.win_length = int(n_fft), int(hop_length), int(win_length)
        self._disc_config(validate=True)
        self.convs = nn.ModuleList([
            normed_conv(1, 32, (3, 9), padding=(1, 4)),
            normed_conv(32, 32, (3, 9), stride=(1, 2), padding=(1, 4)),
            normed_conv(32, 32, (3, 9), stride=(1, 2), padding=(1, 4)),
            normed_conv(32, 32, (3, 9), stride=(1, 2), padding=(1, 4)),
            normed_conv(32, 32, (3, 3), padding=(1, 1)),
        ])
        self.conv_post = normed_conv(32, 1, (3, 3), padding=(1, 1))
        self._init_critic()

    def _disc_config(self, validate: bool = False) -> "_lib.DiscConfig":
        return self._validated(_resolution_config([(self.n_fft, self.hop_length, self.win_length)]), validate)

    def _sub_extents(self, i: int, L: int) -> list:
        return resolution_extents(L, self.n_fft, self.hop_length)

    def min_length(self) -> int:
        """The shortest row the spectrogram takes: longer than the reflect padding, and one hop."""
        return max(self.hop_length, (self.n_fft - self.hop_length + 1) // 2 + 1)

    def extra_repr(self) -> str:
        return f"n_fft={self.n_fft}, hop_length={self.hop_length}, win_length={self.win_length}, backend=libfishvoc_hip (gfx950)"


class MultiResolutionDiscriminator(Critic):
    def __init__(self, resolutions: list):
        super().__init__()
        self.resolutions = [tuple(int(v) for v in r) for r in resolutions]
        for r in self.resolutions:
            if len(r) != 3:
                raise ValueError(f"MultiResolutionDiscriminator: a resolution is (n_fft, hop_length, win_length), got {r}")
        self._disc_config(validate=True)
        self.discriminators = nn.ModuleList(DiscriminatorR(n_fft=n, hop_length=h, win_length=w) for n, h, w in self.resolutions)
        self._init_critic()

    def _disc_config(self, validate: bool = False) -> "_lib.DiscConfig":
        return self._validated(_resolution_config(self.resolutions), validate)

    def _sub_extents(self, i: int, L: int) -> list:
        return self.discriminators[i]._sub_extents(0, L)

    def min_length(self) -> int:
        return max(d.min_length() for d in self.discriminators)

    def forward(self, x: torch.Tensor, lengths=None):
        """mrd.py:89-102: the scores of every resolution concatenated, (B, sum n)."""
        scores, fmaps = super().forward(x, lengths)
        return torch.cat(scores, dim=1), fmaps

    def forward_list(self, waves) -> list:
        return [(torch.cat(scores, dim=1), fmaps) for scores, fmaps in super().forward_list(waves)]
