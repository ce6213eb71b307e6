"""The critics restated in numpy (fish_vocoder/modules/discriminators/mpd.py, mrd.py in eval mode, and the sums behind
models/gan.py:149 / 155 / 204), float64 by default with a ``dtype=`` switch, one row at a time: what the ``fv_disc_*`` kernels are tested
against.  Feature maps are (C, H, W), the reference's layout without the batch axis."""
from __future__ import annotations

import numpy as np

DEFAULT_CHANNELS = (1, 64, 128, 256, 512, 1024)


# -- extents ---------------------------------------------------------------------------------------
def conv_extent(n: int, k: int, s: int, pad: int) -> int:
    return (n + 2 * pad - k) // s + 1


def period_extents(L: int, period: int, n_convs: int = 5, kernel_size: int = 5, stride: int = 3) -> list:
    """(H, W) after every conv and after conv_post of a DiscriminatorP (mpd.py:47-59)."""
    h = -(-L // period)
    out = []
    for _ in range(n_convs):
        h = conv_extent(h, kernel_size, stride, kernel_size // 2)
        out.append((h, period))
    return out + [(conv_extent(h, 3, 1, 1), period)]


def resolution_extents(L: int, n_fft: int, hop: int) -> list:
    """(H, W) after every conv and after conv_post of a DiscriminatorR (mrd.py:24-33, :52-73)."""
    h, w = n_fft // 2 + 1, L // hop
    out = []
    for kw, sw, pw in ((9, 1, 4), (9, 2, 4), (9, 2, 4), (9, 2, 4), (3, 1, 1), (3, 1, 1)):
        w = conv_extent(w, kw, sw, pw)
        out.append((h, w))
    return out


def brute_force_extent(n: int, k: int, s: int, pad: int) -> int:
    """Output positions whose window starts inside the padded extent and ends inside it: the rule the closed form restates."""
    return sum(1 for o in range(n + 2 * pad) if o * s + k <= n + 2 * pad)


# -- layers ----------------------------------------------------------------------------------------
def fold_weight(g: np.ndarray, v: np.ndarray, dtype=np.float64) -> np.ndarray:
    """weight_norm with dim = 0: g v / |v|, the norm over dims 1-3, in float64, rounded once to float32 (as the library folds it)."""
    g64, v64 = g.astype(np.float64), v.astype(np.float64)
    norm = np.sqrt((v64 ** 2).sum((1, 2, 3), keepdims=True))
    return (g64 * v64 / norm).astype(np.float32).astype(dtype)


def folded_layers(sd: dict, i: int, n_convs: int, dtype=np.float64) -> list:
    """[(w (N, C, KH, KW), b (N,))] of sub-discriminator ``i``: its convs, then conv_post."""
    out = []
    for name in [f"convs.{l}" for l in range(n_convs)] + ["conv_post"]:
        p = f"discriminators.{i}.{name}."
        out.append((fold_weight(np.asarray(sd[p + "parametrizations.weight.original0"]), np.asarray(sd[p + "parametrizations.weight.original1"]), dtype),
                    np.asarray(sd[p + "bias"]).astype(dtype)))
    return out


def conv2d(x: np.ndarray, w: np.ndarray, b: np.ndarray, stride, pad) -> np.ndarray:
    """x (C, H, W), w (N, C, KH, KW) -> (N, H', W'), zero padding."""
    C, H, W = x.shape
    N, _, KH, KW = w.shape
    (sh, sw), (ph, pw) = stride, pad
    Ho, Wo = conv_extent(H, KH, sh, ph), conv_extent(W, KW, sw, pw)
    xp = np.zeros((C, H + 2 * ph, W + 2 * pw), dtype=x.dtype)
    xp[:, ph: ph + H, pw: pw + W] = x
    y = np.zeros((N, Ho, Wo), dtype=x.dtype)
    for kh in range(KH):
        for kw in range(KW):
            win = xp[:, kh: kh + sh * (Ho - 1) + 1: sh, kw: kw + sw * (Wo - 1) + 1: sw]
            y += np.einsum("nc,chw->nhw", w[:, :, kh, kw], win, optimize=True)
    return y + b[:, None, None]


def silu(x: np.ndarray) -> np.ndarray:
    return x / (1 + np.exp(-x))


def run_stack(x: np.ndarray, layers: list, strides: list, pads: list, truncated: bool = False) -> list:
    """Every conv + SiLU, then the last layer (conv_post) without it: the fmap list.  ``truncated``: ``layers`` holds the first convs only."""
    fmap = []
    for l, ((w, b), s, p) in enumerate(zip(layers, strides, pads)):
        x = conv2d(x, w, b, s, p)
        if truncated or l < len(layers) - 1:
            x = silu(x)
        fmap.append(x)
    return fmap


# -- MPD -------------------------------------------------------------------------------------------
def period_fold(wave: np.ndarray, period: int, dtype=np.float64) -> np.ndarray:
    L = len(wave)
    h = -(-L // period)
    x = np.zeros(h * period, dtype=dtype)
    x[:L] = wave
    return x.reshape(1, h, period)


def period_forward(wave, period: int, layers: list, kernel_size: int = 5, stride: int = 3, dtype=np.float64, extent: int = None,
                   truncated: bool = False) -> list:
    """mpd.py:43-63 on one row; ``layers`` from ``folded_layers``.  ``extent``: run the row zero-padded to that many samples (what a
    batch-extent run would compute), for the tests that show the row's own padding matters."""
    wave = np.asarray(wave, dtype=dtype)
    if extent is not None:
        wave = np.concatenate([wave, np.zeros(extent - len(wave), dtype=dtype)])
    n = len(layers) - (0 if truncated else 1)
    return run_stack(period_fold(wave, period, dtype), layers, [(stride, 1)] * n + [(1, 1)], [(kernel_size // 2, 0)] * n + [(1, 0)], truncated)


# -- MRD -------------------------------------------------------------------------------------------
def spectrogram(wave, n_fft: int, hop: int, win: int, dtype=np.float64) -> np.ndarray:
    """mrd.py:52-73: reflect padding, frames at hop, a window of ones of ``win`` centred in ``n_fft``, |DFT| -> (bins, frames)."""
    x = np.asarray(wave, dtype=dtype)
    x = np.pad(x, ((n_fft - hop) // 2, (n_fft - hop + 1) // 2), mode="reflect")
    frames = 1 + (len(x) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(frames)[:, None]
    window = np.zeros(n_fft, dtype=dtype)
    left = (n_fft - win) // 2
    window[left: left + win] = 1
    k = np.arange(n_fft // 2 + 1)
    ang = 2 * np.pi * ((k[:, None] * np.arange(n_fft)[None, :]) % n_fft) / n_fft
    fr = x[idx] * window
    re, im = fr @ np.cos(ang).astype(dtype).T, fr @ (-np.sin(ang)).astype(dtype).T
    return np.sqrt(re * re + im * im).T.astype(dtype)


RES_STRIDES = [(1, 1), (1, 2), (1, 2), (1, 2), (1, 1), (1, 1)]
RES_PADS = [(1, 4), (1, 4), (1, 4), (1, 4), (1, 1), (1, 1)]


def resolution_forward(wave, n_fft: int, hop: int, win: int, layers: list, dtype=np.float64, extent: int = None, truncated: bool = False) -> list:
    """mrd.py:35-50 on one row.  ``extent``: the magnitudes zero-padded to ``extent // hop`` frames before the convs."""
    mag = spectrogram(wave, n_fft, hop, win, dtype)
    if extent is not None:
        mag = np.concatenate([mag, np.zeros((mag.shape[0], extent // hop - mag.shape[1]), dtype=dtype)], axis=1)
    return run_stack(mag[None], layers, RES_STRIDES, RES_PADS, truncated)


# -- sums ------------------------------------------------------------------------------------------
def distance_sums(real_fmaps: list, fake_fmaps: list) -> np.ndarray:
    """(layers, 5) float64: sum |r - f|, sum (1 - f)^2, sum f^2, sum (r - 1)^2, count — fv_disc_distance's columns."""
    out = np.zeros((len(real_fmaps), 5))
    for l, (r, f) in enumerate(zip(real_fmaps, fake_fmaps)):
        r, f = r.astype(np.float64), f.astype(np.float64)
        out[l] = [np.abs(r - f).sum(), ((1 - f) ** 2).sum(), (f ** 2).sum(), ((r - 1) ** 2).sum(), r.size]
    return out
