"""The seeded AdaIN noise of RefineGAN (include/fishvoc.h ``fv_refinegan_set_noise_seed``), in plain numpy.

The reference's AdaIN adds ``torch.randn_like(x) * weight`` on every call (refinegan.py:125).  With a seed set, the engine computes that
standard-normal sample inside its AdaIN kernel as a pure function of (seed, noise row, AdaIN layer, channel, absolute sample position), so a
window of an utterance regenerates exactly the samples the whole utterance has at those positions.  The rule:

  ``q = p >> 2``, ``lane = p & 3``;
  ``(x0, x1, x2, x3) = Philox4x32-10(counter = (q & 0xffffffff, q >> 32, (r * C + c) & 0xffffffff, l), key = (s & 0xffffffff, s >> 32))``;
  Box-Muller per pair: ``u1 = ((xa >> 8) + 1) * 2**-24`` in (0, 1], ``u2 = (xb >> 8) * 2**-24`` in [0, 1), ``rad = sqrt(-2 ln u1)``;
  lanes 0 / 1 are ``rad cos(2 pi u2)`` / ``rad sin(2 pi u2)`` of (x0, x1), lanes 2 / 3 the same of (x2, x3).

``l`` counts the AdaIN layers in the order the forward meets them (up-sampling stage, branch k = 3 / 7 / 11, first / second AdaIN); ``p`` is
counted from the utterance's first sample at that layer's rate; ``r = first_row + b`` for batch row ``b``.  Everything here is float64 until the
final cast: the kernels' fp32 ``logf`` / ``sqrtf`` / ``sincospif`` agree to a few ulp (tests/test_gpu_refinegan_noise.py states the bound).
"""
from __future__ import annotations

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Random123's Philox4x32 with ten rounds.  ``counter``: four, ``key``: two arrays (or scalars) of 32-bit words, broadcast against each
    other -> four uint32 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & _M32 for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & _M32 for w in key]
    c = list(np.broadcast_arrays(*c))
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    s32 = np.uint64(32)
    for rnd in range(10):
        if rnd:
            k = [(k[0] + np.uint64(PHILOX_W0)) & _M32, (k[1] + np.uint64(PHILOX_W1)) & _M32]
        p0, p1 = m0 * c[0], m1 * c[2]          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & _M32, (p0 >> s32) ^ c[3] ^ k[1], p0 & _M32]
    return tuple(w.astype(np.uint32) for w in c)


def _box_muller(seed: int, row: int, layer: int, channel: int, C: int, p0: int, n: int):
    """(z, rad) at the absolute positions ``[p0, p0 + n)``, both float64: the samples and the ``sqrt(-2 ln u1)`` behind each."""
    seed, p0, n = int(seed), int(p0), int(n)
    if p0 < 0 or n < 0:
        raise ValueError(f"positions are counted from the utterance's first sample: p0 = {p0}, n = {n}")
    q0, q1 = p0 >> 2, (p0 + max(n, 1) - 1) >> 2
    q = np.arange(q0, q1 + 1, dtype=np.uint64)
    x = philox4x32_10((q & _M32, q >> np.uint64(32), (int(row) * int(C) + int(channel)) & 0xFFFFFFFF, int(layer)),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    z, r = np.empty((q.size, 4), dtype=np.float64), np.empty((q.size, 4), dtype=np.float64)
    for h in (0, 1):
        u1 = ((x[2 * h] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (x[2 * h + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r[:, 2 * h] = r[:, 2 * h + 1] = rad = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * h] = rad * np.cos(2.0 * np.pi * u2)
        z[:, 2 * h + 1] = rad * np.sin(2.0 * np.pi * u2)
    a = p0 - 4 * q0
    return z.reshape(-1)[a:a + n], r.reshape(-1)[a:a + n]


def normal(seed: int, row: int, layer: int, channel: int, C: int, p0: int, n: int) -> np.ndarray:
    """The ``n`` samples at the absolute positions ``[p0, p0 + n)`` of (seed, noise row, AdaIN layer, channel of ``C``) -> float32."""
    return _box_muller(seed, row, layer, channel, C, p0, n)[0].astype(np.float32)


def radius(seed: int, row: int, layer: int, channel: int, C: int, p0: int, n: int) -> np.ndarray:
    """``rad = sqrt(-2 ln u1)`` behind each of ``normal``'s samples (float64): what the fp32 error of a sample scales with."""
    return _box_muller(seed, row, layer, channel, C, p0, n)[1]


def layers(cfg) -> list[tuple[int, int]]:
    """(channels, samples per frame) of the 6 S AdaIN layers, in the order the forward meets them."""
    ups = list(cfg["upsample_rates"])
    ch = int(cfg["start_channels"]) * 2 ** len(ups) * 2
    out, spf = [], 1
    for r in ups:
        ch //= 2
        spf *= int(r)
        out += [(ch, spf)] * 6
    return out


def noise_for_forward(cfg, seed: int, first_row: int, batch: int, frames: int, origin_frame: int = 0, fn=normal) -> list[np.ndarray]:
    """The draws of one forward of ``batch`` x ``frames`` frames that starts at frame ``origin_frame`` of its utterance: the list of
    ``(batch, C, frames * samples_per_frame)`` arrays that ``oracle.refinegan_forward`` takes as ``noise`` (flattened and concatenated: the
    explicit-noise layout of ``fv_forward_refinegan``)."""
    out = []
    for l, (C, spf) in enumerate(layers(cfg)):
        a = np.empty((batch, C, frames * spf), dtype=np.float64 if fn is radius else np.float32)
        for b in range(batch):
            for c in range(C):
                a[b, c] = fn(seed, first_row + b, l, c, C, origin_frame * spf, frames * spf)
        out.append(a)
    return out


def refinegan_reach(cfg) -> int:
    """The one-sided reach of RefineGAN in input frames (what ``fv_reach_frames`` returns for a seeded engine; the C walk restated): an upper
    bound on how far, in frames, an output sample's inputs (mel and template) lie from it.  Walked backwards from the output, in samples at each
    layer's own rate: a conv of kernel k and dilation d adds (k - 1) / 2 * d; a ResBlock's six convs 2 * (k - 1) / 2 * (1 + 3 + 5); an
    up-sampling interpolation by u divides by u (rounded up) and adds its two taps; a down-sampling one by d multiplies by d and adds d + 1."""
    downs, ups = [int(r) for r in cfg["downsample_rates"]], [int(r) for r in cfg["upsample_rates"]]
    S, hop = len(ups), int(cfg["hop_length"])
    R = 3                                        # output_conv (k = 7)
    at_skip = [0] * S                            # what up stage i needs of the skip tensor it concatenates (skip[S - 1 - i], at its own rate)
    for i in range(S - 1, -1, -1):
        R += 2 * 5 * 9 + 3                       # the widest branch (k = 11) and input_conv (k = 7); AdaIN is pointwise
        at_skip[S - 1 - i] = R
        R = (R + ups[i] - 1) // ups[i] + 2       # nn.Upsample(scale_factor=u, mode="linear"): two taps
    mel = R + 3                                  # mel_conv (k = 7), at the frame rate
    need = R                                     # of the down path's last tensor, at the frame rate
    for k in range(S - 1, -1, -1):               # down block k: interpolation by 1 / d, then a k = 7 ResBlock at the lower rate
        need = max(at_skip[k], (need + 2 * 3 * 9) * downs[k] + downs[k] + 1)
    tmpl = need + 3                              # template_conv (k = 7), in samples
    return max(mel, (tmpl + hop - 1) // hop + 1) + 2
