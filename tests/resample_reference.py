"""Float64 numpy restatement of the polyphase windowed-sinc resampler (the checker of the resample tests, like conv_reference.py for the convs).

The dense form, exactly as the formula reads — every tap j in [0, 2 width + o) of every phase, no band, no fp32 anywhere::

    g = gcd(orig_freq, new_freq);  o = orig_freq / g;  n = new_freq / g
    base = min(o, n) * rolloff;    width = ceil(lpw * o / base)
    t = clamp(((j - width) / o - p / n) * base, -lpw, +lpw)
    win = cos(t pi / lpw / 2)^2  |  I0(beta sqrt(1 - (t / lpw)^2)) / I0(beta)
    h[p][j] = (t == 0 ? 1 : sin(pi t) / (pi t)) * win * base / o
    xp = x behind `width` zeros, `width + o` zeros after;  y[f n + p] = sum_j h[p][j] xp[f o + j];  the first ceil(n L / o) outputs are kept
"""
import math

import numpy as np

KAISER_BETA = 14.769656459379492


class Filter:
    def __init__(self, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
        g = math.gcd(int(orig_freq), int(new_freq))
        self.o, self.n, self.lpw = int(orig_freq) // g, int(new_freq) // g, int(lowpass_filter_width)
        o, n, lpw = self.o, self.n, self.lpw
        self.base = base = min(o, n) * rolloff
        self.width = width = int(math.ceil(lpw * o / base))
        j = np.arange(2 * width + o, dtype=np.float64)[None, :]
        p = np.arange(n, dtype=np.float64)[:, None]
        self.t_raw = ((j - width) / o - p / n) * base                  # (n, 2 width + o), before the clamp
        t = np.clip(self.t_raw, -lpw, lpw)
        if resampling_method == "sinc_interp_hann":
            win = np.cos(t * math.pi / lpw / 2) ** 2
        elif resampling_method == "sinc_interp_kaiser":
            b = KAISER_BETA if beta is None else float(beta)
            win = np.i0(b * np.sqrt(1 - (t / lpw) ** 2)) / np.i0(b)
        else:
            raise ValueError(resampling_method)
        t = t * math.pi
        safe = np.where(t == 0, 1.0, t)
        self.h = np.where(t == 0, 1.0, np.sin(safe) / safe) * win * (base / o)     # float64 (n, 2 width + o)
        # the band, analytically: |t| < lpw (the computed window at the edge is ~4e-33, not 0)
        inside = np.abs(self.t_raw) < lpw
        self.first = inside.argmax(axis=1)
        self.count = inside.sum(axis=1)
        assert all(inside[q, self.first[q]:self.first[q] + self.count[q]].all() for q in range(n))    # one contiguous band per phase
        self.kp = int(self.count.max())

    def output_length(self, L):
        return -((-self.n * int(L)) // self.o)

    def band_end(self, m):
        """One past the last input sample output m reads."""
        f, p = divmod(int(m), self.n)
        return f * self.o + int(self.first[p]) + int(self.count[p]) - self.width

    def bound(self, xmax=1.0):
        """|y32 - y64| <= (Kp + 2) 2^-24 max_p sum_j |h[p][j]| max|x|: the rounding of a Kp-term fp32 dot product, in any order, plus that of
        the taps."""
        return (self.kp + 2) * 2.0 ** -24 * float(np.abs(self.h).sum(axis=1).max()) * xmax

    def outputs(self, x, m0, m1, start=0, total=None):
        """Outputs [m0, m1) of the row whose samples [start, start + len(x)) are ``x`` (float64) and whose length is ``total`` (default: the end of
        ``x``); every sample those outputs read inside [0, total) must lie in ``x``."""
        x = np.asarray(x, dtype=np.float64)
        o, n, width = self.o, self.n, self.width
        total = start + len(x) if total is None else total
        f0, f1 = m0 // n, (m1 - 1) // n + 1
        lo = f0 * o - width                                          # global index of xp[f0 o]
        hi = (f1 - 1) * o + width + o                                # one past the last sample read
        a, b = max(lo, 0), min(hi, total)
        assert a >= b or (start <= a and b <= start + len(x)), "the slice does not cover what these outputs read"
        xp = np.zeros(hi - lo, dtype=np.float64)
        if b > a:
            xp[a - lo:b - lo] = x[a - start:b - start]
        win = np.lib.stride_tricks.as_strided(xp, shape=(f1 - f0, 2 * width + o), strides=(o * xp.strides[0], xp.strides[0]))
        y = (win @ self.h.T).reshape(-1)                             # (frames, n) -> m = f n + p
        return y[m0 - f0 * n:m1 - f0 * n]

    def __call__(self, x):
        """(..., L) -> (..., ceil(n L / o)) in float64."""
        x = np.asarray(x, dtype=np.float64)
        L = x.shape[-1]
        M = self.output_length(L)
        rows = x.reshape(-1, L)
        out = np.zeros((rows.shape[0], M))
        if M:
            for b in range(rows.shape[0]):
                out[b] = self.outputs(rows[b], 0, M)
        return out.reshape(*x.shape[:-1], M)
