"""Plain-Python restatement of the two pitch-template pools (include/fishvoc.h, fv_yinpool_* / fv_oscpool_*): the two emission rules and a
planner of one step over per-slot counters.  Host arithmetic only; nothing here imports the package."""

MAX_SAMPLES = 1 << 40


def yin_ready(N, W, hop):
    """Frames that read no sample at or after N: frame t reads [t hop + hop // 2 - W // 2, ... + W); never above N // hop."""
    need = hop // 2 + W // 2
    return 0 if N < need else min(1 + (N - need) // hop, N // hop)


def yin_emitted(N2, E, W, hop, flush):
    """E' of a tracker slot once N2 samples have arrived."""
    return max(E, N2 // hop if flush else yin_ready(N2, W, hop))


def osc_emitted(T2, E, flush):
    """E' of an oscillator slot once T2 F0 frames have arrived: frame t needs the centre t + 1, the flush clamps it to T2 - 1."""
    return max(E, T2 if flush else T2 - 1)


class Refused(Exception):
    """A step the pools refuse: ``kind`` is "invalid" or "state", with the item and the session it names."""

    def __init__(self, kind, item, session):
        super().__init__(f"{kind}: item {item}, session {session}")
        self.kind, self.item, self.session = kind, item, session


class Slots:
    """S slots with their own received / emitted / flushed; ``rule(N2, E, flush) -> E'``."""

    def __init__(self, sessions, max_chunk, rule):
        self.S, self.max_chunk, self.rule = sessions, max_chunk, rule
        self.received, self.emitted, self.flushed = [0] * sessions, [0] * sessions, [False] * sessions

    def plan(self, items):
        """Frames per item; raises Refused in the order of the library's admit; changes nothing."""
        seen, out = set(), []
        for i, (s, c, flush) in enumerate(items):
            if not 0 <= s < self.S:
                raise Refused("invalid", i, s)
            if s in seen:
                raise Refused("invalid", i, s)
            seen.add(s)
            if not 0 <= c <= self.max_chunk:
                raise Refused("invalid", i, s)
            if self.flushed[s]:
                raise Refused("state", i, s)
            if self.received[s] + c > MAX_SAMPLES:
                raise Refused("invalid", i, s)
            out.append(self.rule(self.received[s] + c, self.emitted[s], flush) - self.emitted[s])
        return out

    def step(self, items):
        out = self.plan(items)
        for (s, c, flush), k in zip(items, out):
            self.received[s] += c
            self.emitted[s] += k
            self.flushed[s] = self.flushed[s] or flush
        return out

    def reset(self, s):
        self.received[s] = self.emitted[s] = 0
        self.flushed[s] = False


def yin_slots(sessions, max_chunk, W, hop):
    return Slots(sessions, max_chunk, lambda N2, E, flush: yin_emitted(N2, E, W, hop, flush))


def osc_slots(sessions, max_chunk):
    return Slots(sessions, max_chunk, osc_emitted)


def yin_max_frames(max_chunk, W, hop):
    """The most one item emits, by brute force: a push of max_chunk samples that also flushes, from every state (N, E = ready(N))."""
    return max((N + max_chunk) // hop - yin_ready(N, W, hop) for N in range(hop // 2 + W // 2 + 2 * hop))
