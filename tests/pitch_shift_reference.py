"""Float64 numpy restatement of librosa 0.9's ``effects.pitch_shift`` (the checker of the pitch-shift tests, as resample_reference.py is for the
resampler): ``time_stretch(rate = n / o)`` — stft, phase_vocoder, istft — then a resample from ``orig_freq`` to ``sr``, fixed to the input length.

The phase vocoder is stated twice:

(a) ``phase_vocoder_literal``: librosa's loop as written — ``phi_advance = linspace(0, pi hop, nb)``, the accumulator starts at ``angle(D[:, 0])``
    and grows by ``phi_advance + wrap(angle(D[:, j + 1]) - angle(D[:, j]) - phi_advance)`` after every output frame;
(b) ``phase_vocoder_telescoped``: ``Phi[s] = angle(D[:, 0]) + sum_{u < s} (angle(D[:, j_u + 1]) - angle(D[:, j_u]))`` — ``phi_advance`` and the wrap
    cancel out of ``exp(i Phi)``, the wrap being a multiple of 2 pi.

Both take the exact time axis ``s n / o`` (``j_s = s n // o``, ``alpha_s = (s n % o) / o``) for ``T' = ceil(T o / n)`` output frames.
"""
import math

import numpy as np

from resample_reference import KAISER_BETA, Filter

KAISER_BEST_ROLLOFF = 0.9475937167399596


def plan(sr, n_steps, bins_per_octave=12, freq_granularity=100):
    f = math.floor(sr * 2.0 ** (n_steps / bins_per_octave) + 0.5)
    orig = f - f % freq_granularity
    g = math.gcd(orig, sr)
    return orig, orig // g, sr // g


def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)      # periodic


def stft(x, n_fft, hop):
    """(L,) -> (nb, T + 2) complex128: T = 1 + L // hop centred frames over zero padding, then the two zero columns the vocoder reads."""
    x = np.asarray(x, dtype=np.float64)
    L, T = len(x), 1 + len(x) // hop
    xp = np.concatenate([np.zeros(n_fft // 2), x, np.zeros(n_fft // 2 + hop)])
    frames = np.lib.stride_tricks.as_strided(xp, shape=(T, n_fft), strides=(hop * xp.strides[0], xp.strides[0]))
    D = np.fft.rfft(frames * hann(n_fft)[None, :], axis=1).T
    return np.concatenate([D, np.zeros((D.shape[0], 2), dtype=D.dtype)], axis=1)


def _frames_out(T, o, n):
    return -((-T * o) // n)


def phase_vocoder_literal(D, o, n, hop):
    nb, T = D.shape[0], D.shape[1] - 2
    Tout = _frames_out(T, o, n)
    out = np.zeros((nb, Tout), dtype=np.complex128)
    phi_advance = np.linspace(0, np.pi * hop, nb)
    phase_acc = np.angle(D[:, 0])
    for s in range(Tout):
        step = (s * n) / o
        j, alpha = int(step), np.mod(step, 1.0)
        c0, c1 = D[:, j], D[:, j + 1]
        mag = (1.0 - alpha) * np.abs(c0) + alpha * np.abs(c1)
        out[:, s] = mag * np.exp(1.0j * phase_acc)
        dphase = np.angle(c1) - np.angle(c0) - phi_advance
        dphase = dphase - 2.0 * np.pi * np.round(dphase / (2.0 * np.pi))
        phase_acc = phase_acc + phi_advance + dphase
    return out


def phase_vocoder_telescoped(D, o, n, hop=None):
    T = D.shape[1] - 2
    Tout = _frames_out(T, o, n)
    q = np.arange(Tout, dtype=np.int64) * n
    j, alpha = q // o, (q % o) / o
    mag = (1.0 - alpha)[None, :] * np.abs(D[:, j]) + alpha[None, :] * np.abs(D[:, j + 1])
    ang = np.angle(D)
    d = ang[:, j + 1] - ang[:, j]
    phi = ang[:, :1] + np.cumsum(d, axis=1) - d            # exclusive
    return mag * np.exp(1.0j * phi)


def istft(S, n_fft, hop, length):
    """irfft times the window, overlap-add, divide by the overlap-added window^2 where it is positive, crop n_fft / 2, cut or pad to ``length``."""
    Tout = S.shape[1]
    w = hann(n_fft)
    frames = np.fft.irfft(S, n=n_fft, axis=0) * w[:, None]
    total = n_fft + hop * (Tout - 1)
    y, env = np.zeros(max(total, 0)), np.zeros(max(total, 0))
    for s in range(Tout):
        y[s * hop:s * hop + n_fft] += frames[:, s]
        env[s * hop:s * hop + n_fft] += w * w
    y = np.where(env > 0, y / np.where(env > 0, env, 1.0), 0.0)[n_fft // 2:]
    out = np.zeros(length)
    k = min(length, len(y))
    out[:k] = y[:k]
    return out


def stretched_length(L, o, n):
    return (2 * L * o + n) // (2 * n)


def time_stretch(x, o, n, n_fft=2048, hop=None, form="telescoped"):
    """(L,) -> (Ls,) float64."""
    hop = n_fft // 4 if hop is None else hop
    D = stft(x, n_fft, hop)
    S = (phase_vocoder_telescoped if form == "telescoped" else phase_vocoder_literal)(D, o, n, hop)
    return istft(S, n_fft, hop, stretched_length(len(x), o, n))


def pitch_shift(x, sr, n_steps, bins_per_octave=12, n_fft=2048, hop=None, freq_granularity=100, lowpass_filter_width=64,
                rolloff=KAISER_BEST_ROLLOFF, resampling_method="sinc_interp_kaiser", beta=KAISER_BETA):
    """(L,) -> (L,) float64: the whole of librosa.effects.pitch_shift, phase vocoder in form (b)."""
    x = np.asarray(x, dtype=np.float64)
    orig, o, n = plan(sr, n_steps, bins_per_octave, freq_granularity)
    if orig == sr:
        return x.copy()
    st = time_stretch(x, o, n, n_fft, hop)
    y = Filter(orig, sr, lowpass_filter_width, rolloff, resampling_method, beta)(st)
    out = np.zeros(len(x))
    k = min(len(x), len(y))
    out[:k] = y[:k]
    return out


def broadband(L, sr, seed):
    """uniform(-1, 1) plus 0.5 sin at 440 Hz: every bin excited (the phase of an empty bin is ill-conditioned in any precision)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, L) + 0.5 * np.sin(2.0 * np.pi * 440.0 * np.arange(L) / sr)
