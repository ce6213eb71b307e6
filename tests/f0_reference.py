"""float64 NumPy restatement of the F0 tracker and the pitch template (include/fishvoc.h, the "pitch template" section): the plan, YIN in its
direct form, the integer phase and the oscillator.  A plain module, like resample_reference.py; the tests share its results."""
import math

import numpy as np


def plan(sample_rate, frame_length=2048, hop_length=512, fmin=40.0, fmax=1100.0, threshold=0.1):
    """(tau_min, tau_max, Wi); ValueError for a rejected configuration."""
    if sample_rate <= 0 or hop_length < 1 or frame_length < 2 or frame_length % 2:
        raise ValueError("sample_rate, hop_length or frame_length")
    if not (0.0 < fmin < math.inf and 0.0 < fmax < math.inf) or not 0.0 < threshold <= 1.0:
        raise ValueError("fmin, fmax or threshold")
    tau_max, tau_min = math.floor(sample_rate / float(fmin)), max(2, math.floor(sample_rate / float(fmax)))
    Wi = frame_length - (tau_max + 1)
    if tau_max > 1 << 24 or tau_min >= tau_max or 2 * Wi < tau_max:
        raise ValueError("lags")
    return tau_min, tau_max, Wi


def frame(x, t, W, hop):
    """The W samples centred on t hop + hop // 2, zeros outside the row."""
    lo = t * hop + hop // 2 - W // 2
    idx = lo + np.arange(W)
    ok = (idx >= 0) & (idx < len(x))
    out = np.zeros(W)
    out[ok] = np.asarray(x, dtype=np.float64)[idx[ok]]
    return out


def cmnd(xf, tau_max, Wi):
    """d'(tau) for tau = 0 ... tau_max + 1 (entry 0 is unused and set to 1)."""
    lagged = np.lib.stride_tricks.sliding_window_view(xf, Wi)[1:tau_max + 2]        # row tau - 1: x[tau ... tau + Wi)
    d = ((xf[None, :Wi] - lagged) ** 2).sum(axis=1)
    run = np.cumsum(d)
    tau = np.arange(1, tau_max + 2)
    dp = np.where(run == 0.0, 1.0, d * tau / np.where(run == 0.0, 1.0, run))
    return np.concatenate([[1.0], dp])


def decide(dp, tau_min, tau_max, threshold, sample_rate):
    """(lag or 0, f0, aperiodicity) of one frame's d'."""
    tau = np.arange(tau_min, tau_max + 1)
    ok = (dp[tau] < threshold) & (dp[tau] <= dp[tau - 1]) & (dp[tau] < dp[tau + 1])
    if not ok.any():
        return 0, 0.0, float(dp[tau].min())
    best = int(tau[np.argmax(ok)])
    a, b, c = dp[best - 1], dp[best], dp[best + 1]
    den = a - 2.0 * b + c
    delta = 0.5 * (a - c) / den if den > 0.0 else 0.0
    return best, sample_rate / (best + delta), float(b)


def yin(x, sample_rate, hop_length, frame_length=2048, fmin=40.0, fmax=1100.0, threshold=0.1, length=None, slack=1e-3):
    """One row: dict of f0 (T,), aperiodicity (T,), lag (T,) (0: unvoiced) and stable (T,): the frame's lag is the same at
    threshold * (1 - slack), threshold and threshold * (1 + slack).  ``length``: the row's own samples (the rest is not read); frames at or
    past length // hop are zeros."""
    tau_min, tau_max, Wi = plan(sample_rate, frame_length, hop_length, fmin, fmax, threshold)
    x = np.asarray(x, dtype=np.float64)
    T = len(x) // hop_length
    own = x if length is None else x[:length]
    f0, ap, lag, stable = np.zeros(T), np.zeros(T), np.zeros(T, dtype=np.int64), np.ones(T, dtype=bool)
    for t in range(len(own) // hop_length):
        dp = cmnd(frame(own, t, frame_length, hop_length), tau_max, Wi)
        lag[t], f0[t], ap[t] = decide(dp, tau_min, tau_max, threshold, sample_rate)
        stable[t] = all(decide(dp, tau_min, tau_max, threshold * s, sample_rate)[0] == lag[t] for s in (1.0 - slack, 1.0 + slack))
    return dict(f0=f0, aperiodicity=ap, lag=lag, stable=stable)


def increments(f0, sample_rate):
    """F_t = rint(f0_t / sr * 2^32) as integers; 0 unless 0 < f0_t < sr."""
    f = np.asarray(f0, dtype=np.float64)
    ok = (f > 0.0) & (f < sample_rate)
    return np.where(ok, np.rint(np.where(ok, f, 0.0) / sample_rate * 2.0 ** 32), 0.0).astype(np.uint64)


def phase(f0, sample_rate, hop_length, frames=None):
    """(phi (T hop,) uint64 in [0, 2^32), inc (T hop,) uint64, voiced (T hop,) bool) of one row; ``frames``: the row's own frames (the rest of
    f0 is not read, its samples get inc = 0 and voiced = False)."""
    T = len(f0)
    Ti = T if frames is None else int(frames)
    N, hop = T * hop_length, hop_length
    inc, voiced = np.zeros(N, dtype=np.uint64), np.zeros(N, dtype=bool)
    if Ti > 0:
        F = increments(np.asarray(f0)[:Ti], sample_rate)
        n = np.arange(Ti * hop)
        m = n - hop // 2
        a = np.floor_divide(m, hop)
        k = (m - a * hop).astype(np.uint64)
        Fa, Fb = F[np.clip(a, 0, Ti - 1)], F[np.clip(a + 1, 0, Ti - 1)]
        Fa, Fb = np.where(Fa == 0, Fb, Fa), np.where(Fb == 0, Fa, Fb)
        inc[:Ti * hop] = (Fa * (np.uint64(hop) - k) + Fb * k) // np.uint64(hop)
        voiced[:Ti * hop] = F[n // hop] != 0
    phi = np.cumsum(inc, dtype=np.uint64) % np.uint64(2 ** 32)
    return phi, inc, voiced


def template(f0, sample_rate, hop_length, kind="sine", amplitude=1.0, frames=None):
    """(T hop,) float64: the oscillator on the exact integer phase, 0 in unvoiced frames and past the row's own frames."""
    phi, _, voiced = phase(f0, sample_rate, hop_length, frames)
    turns = phi.astype(np.float64) / 2.0 ** 32
    wave = np.sin(2.0 * np.pi * turns) if kind == "sine" else 2.0 * turns - 1.0
    return np.where(voiced, amplitude * wave, 0.0)


def glide(L, sample_rate, seed=0, f_lo=110.0, f_hi=220.0):
    """The test signal: a five-harmonic glide f_lo -> f_hi over the row with 3 % vibrato at 5.5 Hz, harmonic amplitudes 1 / h, noise at 1e-3, an
    all-zero segment at 40 - 50 % and a noise-only segment at 70 - 80 % of the row.  Returns (x float32 (L,), the instantaneous F0 (L,),
    kind (L,): 0 voiced, 1 silent, 2 noise only)."""
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    f = f_lo * (f_hi / f_lo) ** (n / max(L, 1)) * (1.0 + 0.03 * np.sin(2.0 * np.pi * 5.5 * n / sample_rate))
    ph = 2.0 * np.pi * np.cumsum(f) / sample_rate
    tone = 0.3 * sum(np.sin(h * ph) / h for h in range(1, 6))
    noise = 1e-3 * rng.standard_normal(L)
    kind = np.zeros(L, dtype=np.int64)
    kind[int(0.4 * L):int(0.5 * L)] = 1
    kind[int(0.7 * L):int(0.8 * L)] = 2
    x = np.where(kind == 0, tone + noise, np.where(kind == 2, noise, 0.0))
    return x.astype(np.float32), f, kind
