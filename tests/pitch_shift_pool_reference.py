"""The emission of a pitch-shift pool (include/fishvoc.h, fv_pvpool_*) per session, by counting: every slot is a stream of its own, and what it
has emitted after N samples is pitch_shift_stream_reference's count (ready, emitted) — frames, stretched frames, stretched samples and
resampler bands counted one by one.  No closed form is shared with the library or with vocoder_amd.pitch_shift.PvPoolCounters.

    a step's item (session, samples, flush):  N' = N + samples;  E' = N' with flush, else max(E, counted(N'));  the item emits E' - E

and per item the frames, stretched frames and stretched samples the step makes ready, with the whole utterance's lengths at the flush."""
import pitch_shift_reference as pref
import pitch_shift_stream_reference as sref


class Rule:
    """One shifter: the rate n / o, the frame, and the float64 filter of its resampler (None for the identity shift)."""

    def __init__(self, sr, n_steps, n_fft, hop):
        self.sr, self.n_steps, self.n_fft, self.hop = sr, n_steps, n_fft, hop
        self.orig_freq, self.o, self.n = pref.plan(sr, n_steps)
        self.filt = sref.resampler(sr, n_steps) if self.orig_freq != sr else None
        self._seen = {}

    def ready(self, N):
        if N not in self._seen:
            self._seen[N] = sref.ready(N, self.o, self.n, self.n_fft, self.hop)
        return self._seen[N]

    def emitted(self, N):
        """Outputs a session has emitted once N samples have arrived, before its flush."""
        if self.filt is None:
            return N
        return sref.emitted(self.filt, self.ready(N)[2], N)[0]

    def made_ready(self, N, N2, flush):
        """(dA, dS, dY) of a step that takes a session from N to N2 samples."""
        a = self.ready(N)
        b = sref.whole_lengths(N2, self.o, self.n, self.hop) if flush else self.ready(N2)
        return tuple(y - x for x, y in zip(a, b))


class Sessions:
    """The counters of `sessions` slots under Rule: step(items) -> outputs per item."""

    def __init__(self, rule, sessions):
        self.rule = rule
        self.N = [0] * sessions
        self.E = [0] * sessions
        self.flushed = [False] * sessions

    def step(self, items):
        out = []
        for s, c, flush in items:
            assert not self.flushed[s]
            N2 = self.N[s] + c
            E2 = N2 if flush else max(self.E[s], self.rule.emitted(N2))
            out.append(E2 - self.E[s])
            self.N[s], self.E[s] = N2, E2
            self.flushed[s] = bool(flush)
        return out

    def reset(self, s):
        self.N[s] = self.E[s] = 0
        self.flushed[s] = False
