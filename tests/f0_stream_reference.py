"""NumPy restatement of the two pitch-template streams (include/fishvoc.h, fv_yin_stream_* / fv_osc_stream_*): the emission rules as host
arithmetic, and each stream holding no more than the library carries — the tracker the samples that frames not yet emitted still read, the
oscillator the increments of the frames [E - 1, Tn) and the phase at the start of frame E.  The per-frame arithmetic is f0_reference's."""
import numpy as np

import f0_reference as fref


def frames_ready(N, W, hop):
    """Frames that read no sample at or after N: frame t reads [t hop + hop // 2 - W // 2, ... + W)."""
    need = hop // 2 + W // 2
    return 0 if N < need else min(1 + (N - need) // hop, N // hop)


def pending_samples(N, E, W, hop):
    return max(0, N - max(0, E * hop + hop // 2 - W // 2))


def osc_emitted(Tn, E, flush=False):
    """Frames emitted once Tn frames have arrived: frame t needs the centre t + 1, the flush clamps it to Tn - 1."""
    return Tn if flush else max(E, Tn - 1)


class YinStream:
    """One row.  push(chunk) / flush() -> dict of f0, aperiodicity, lag for the frames emitted by the call."""

    def __init__(self, sample_rate, hop_length, frame_length=2048, fmin=40.0, fmax=1100.0, threshold=0.1):
        self.sr, self.hop, self.W, self.threshold = sample_rate, hop_length, frame_length, threshold
        self.tau_min, self.tau_max, self.Wi = fref.plan(sample_rate, frame_length, hop_length, fmin, fmax, threshold)
        self.reset()

    def reset(self):
        self.N = self.E = 0
        self.origin, self.kept = 0, np.zeros(0)          # kept[i] is sample origin + i
        self.flushed = False
        self.max_pending = 0

    def _frame(self, t, limit):
        idx = t * self.hop + self.hop // 2 - self.W // 2 + np.arange(self.W)
        ok = (idx >= 0) & (idx < limit)
        assert (idx[ok] >= self.origin).all(), "a frame reads a sample the stream no longer carries"
        out = np.zeros(self.W)
        out[ok] = self.kept[idx[ok] - self.origin]
        return out

    def _emit(self, E2):
        f0, ap, lag = [], [], []
        for t in range(self.E, E2):
            dp = fref.cmnd(self._frame(t, self.N), self.tau_max, self.Wi)
            l, f, a = fref.decide(dp, self.tau_min, self.tau_max, self.threshold, self.sr)
            f0.append(f), ap.append(a), lag.append(l)
        self.E = max(self.E, E2)
        keep = self.N - pending_samples(self.N, self.E, self.W, self.hop)
        self.kept, self.origin = self.kept[keep - self.origin:], keep
        self.max_pending = max(self.max_pending, len(self.kept))
        return dict(f0=np.array(f0), aperiodicity=np.array(ap), lag=np.array(lag, dtype=np.int64))

    def push(self, chunk):
        assert not self.flushed
        self.kept = np.concatenate([self.kept, np.asarray(chunk, dtype=np.float64)])
        self.N += len(chunk)
        return self._emit(frames_ready(self.N, self.W, self.hop))

    def flush(self):
        assert not self.flushed
        out = self._emit(self.N // self.hop)
        self.flushed = True
        return out


class OscStream:
    """One row.  push(f0 frames) / flush() -> (phi, inc, voiced) of the samples emitted by the call, as f0_reference.phase gives them."""

    def __init__(self, sample_rate, hop_length):
        self.sr, self.hop = sample_rate, hop_length
        self.reset()

    def reset(self):
        self.Tn = self.E = 0
        self.first, self.F = 0, np.zeros(0, dtype=np.uint64)        # F[i] is frame first + i
        self.phi = np.uint64(0)                                     # the phase before the first sample of frame E
        self.flushed = False

    def _emit(self, E2):
        hop = self.hop
        n = np.arange(self.E * hop, E2 * hop)
        m = n - hop // 2
        a = np.floor_divide(m, hop)
        k = (m - a * hop).astype(np.uint64)
        ia, ib = np.clip(a, 0, self.Tn - 1), np.clip(a + 1, 0, self.Tn - 1)
        if len(n):
            assert ia.min() >= self.first and ib.max() < self.first + len(self.F)
        Fa, Fb = self.F[ia - self.first], self.F[ib - self.first]
        Fa, Fb = np.where(Fa == 0, Fb, Fa), np.where(Fb == 0, Fa, Fb)
        inc = (Fa * (np.uint64(hop) - k) + Fb * k) // np.uint64(hop)
        voiced = self.F[n // hop - self.first] != 0
        phi = (self.phi + np.cumsum(inc, dtype=np.uint64)) % np.uint64(2 ** 32)
        if len(n):
            self.phi = phi[-1]
        self.E = E2
        keep = max(0, self.E - 1)
        self.F, self.first = self.F[keep - self.first:], keep
        return phi, inc, voiced

    def push(self, f0):
        assert not self.flushed
        self.F = np.concatenate([self.F, fref.increments(np.asarray(f0, dtype=np.float64), self.sr)]).astype(np.uint64)
        self.Tn += len(f0)
        return self._emit(osc_emitted(self.Tn, self.E))

    def flush(self):
        assert not self.flushed
        out = self._emit(osc_emitted(self.Tn, self.E, flush=True))
        self.flushed = True
        return out


def chunk_sizes(total, rng, largest, zeros=True):
    """Seeded random push sizes that add up to `total`, zero-length pushes among them."""
    sizes = []
    while total > 0:
        c = 0 if zeros and rng.random() < 0.2 else int(rng.integers(1, largest + 1))
        c = min(c, total)
        sizes.append(c)
        total -= c
    return sizes
