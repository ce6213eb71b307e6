"""The emission rule of the streaming pitch shift (include/fishvoc.h, fv_pv_stream_*) a third time, by counting: no closed form is shared with
the library or with vocoder_amd.pitch_shift.stream_ready.  With F = n_fft, h = hop, the rate n / o and N samples received per row:

    A  analysis frames f whose window [f h - F/2, f h + F/2) holds no sample at or after N
    S  stretched frames s whose two columns j = floor(s n / o) and j + 1 are among those A
    Y  stretched samples i < Ls(N) under which every frame that covers i (t h <= i + F/2 < t h + F) is among those S
    E  outputs m of the resampler orig_freq -> sr whose band ends at or before Y, and never more than N

and the bound on the latency N - E that the header states."""
import numpy as np

import pitch_shift_reference as pref
from f0_stream_reference import chunk_sizes  # noqa: F401  (the GPU test's random chunkings)
from resample_reference import Filter


def frames_ready(N, n_fft, hop):
    f = 0
    while f * hop - n_fft // 2 + n_fft <= N:
        f += 1
    return f


def stretched_frames_ready(A, o, n):
    s = 0
    while (s * n) // o + 1 <= A - 1:
        s += 1
    return s


def stretched_samples_ready(S, N, o, n, n_fft, hop):
    limit = pref.stretched_length(N, o, n)
    i = np.arange(limit, dtype=np.int64)
    last = (i + n_fft // 2) // hop                     # the last frame that covers sample i; the earlier ones lie below it
    bad = np.nonzero(last >= S)[0]
    return int(bad[0]) if len(bad) else int(limit)


def ready(N, o, n, n_fft, hop):
    A = frames_ready(N, n_fft, hop)
    S = stretched_frames_ready(A, o, n)
    return A, S, stretched_samples_ready(S, N, o, n, n_fft, hop)


def resampler(sr, n_steps, lowpass_filter_width=64, rolloff=pref.KAISER_BEST_ROLLOFF, method="sinc_interp_kaiser"):
    orig, _, _ = pref.plan(sr, n_steps)
    return Filter(orig, sr, lowpass_filter_width, rolloff, method)


def band_ends(filt, count):
    """band_end(m) for m < count, non-decreasing in m."""
    m = np.arange(count, dtype=np.int64)
    f, p = m // filt.n, m % filt.n
    return f * filt.o + filt.first[p] + filt.count[p] - filt.width


def resampled_ready(filt, Y, count):
    """Outputs m < count whose band has ended once Y stretched samples exist."""
    return int(np.count_nonzero(band_ends(filt, count) <= Y))


def emitted(filt, Y, N):
    """What the stream has emitted: the resampler's own count, capped at N.  Returns (E, uncapped)."""
    raw = resampled_ready(filt, Y, N + filt.n + 1)
    return min(raw, N), raw


def latency_bound(filt, n_fft, hop):
    """N - E <= F/2 + h + ceil((F/2 + D) n / o), D = max_p (band_end(p) - p o / n).

    (A - 1) h >= N - F/2 - h + 1 and S >= (A - 1) o / n give Y >= (N - F/2 - h + 1) o / n - F/2 (or Ls(N) >= N o / n - 1/2, which is larger);
    every m with m o / n + D <= Y is out, so E >= floor((Y - D) n / o) + 1."""
    o, n = filt.o, filt.n
    p = np.arange(n, dtype=np.int64)
    Dn = int(((filt.first + filt.count - filt.width) * n - p * o).max())        # D n
    return n_fft // 2 + hop + -((-(n_fft // 2 * n + max(Dn, 0))) // o)


def whole_lengths(L, o, n, hop):
    T = 1 + L // hop
    return T, -((-T * o) // n), pref.stretched_length(L, o, n)


GRID_FRAMES = ((64, 16), (2048, 512), (64, 64), (64, 32))
GRID_STEPS = (3, -4, 12, -12, 0.5)
GRID_N = tuple(range(400)) + (1000, 20000, 20001)
SR = 44100
