"""Host (no GPU): the pitch-shift pool (include/fishvoc.h fv_pvpool_*) — the ABI surface, the plan of a step stated three times (C:
fv_pvpool_plan; Python: vocoder_amd.pitch_shift.PvPoolCounters; by counting: pitch_shift_pool_reference) over seeded random schedules, the
bound on one item's emission and the pool's internal per-step sizes by brute force over every state below 400 samples, and every refusal
of a step by status and by the name in its message."""
import ctypes
import os
import random
import re

import pytest

import pitch_shift_pool_reference as pool_ref
import pitch_shift_stream_reference as sref
from vocoder_amd import _lib
from vocoder_amd import pitch_shift as ps
from vocoder_amd.sessions import PoolStateError

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PVPOOL_API = ("fv_pvpool_create", "fv_pvpool_workspace_bytes", "fv_pvpool_max_outputs", "fv_pvpool_received", "fv_pvpool_emitted",
              "fv_pvpool_pending", "fv_pvpool_bounds", "fv_pvpool_plan", "fv_pvpool_step", "fv_pvpool_reset", "fv_pvpool_destroy")
SR = sref.SR
i64, i32 = ctypes.c_int64, ctypes.c_int32
_rules: dict = {}


def _rule(n_steps, frame):
    """The counting rule and the module (no device handle is made) of one configuration, once."""
    key = (n_steps, frame)
    if key not in _rules:
        _rules[key] = (pool_ref.Rule(SR, n_steps, *frame), ps.PitchShift(SR, n_steps, n_fft=frame[0], hop_length=frame[1]))
    return _rules[key]


def _c_plan(mod, pc, items, flushed=True):
    """fv_pvpool_plan over the counters of ``pc`` -> (result, outputs per item, message)."""
    L = _lib.lib()
    S, n = pc.S, len(items)
    arr = (_lib.WavPoolItem * max(n, 1))(*[_lib.WavPoolItem(int(s), int(c), int(f)) for s, c, f in items])
    out = (i64 * max(n, 1))()
    r = L.fv_pvpool_plan(ctypes.byref(mod.config()), S, pc.max_chunk, (i64 * S)(*pc.received), (i64 * S)(*pc.emitted),
                         (i32 * S)(*[int(f) for f in pc.flushed]) if flushed else None, arr, n, out)
    return int(r), [int(out[i]) for i in range(n)], L.fv_last_error().decode()


def _c_bounds(mod, max_chunk):
    out = (i64 * 5)()
    assert _lib.lib().fv_pvpool_bounds(ctypes.byref(mod.config()), max_chunk, out) == 0, _lib.lib().fv_last_error()
    return [int(v) for v in out]


def test_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in PVPOOL_API:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert {d for d in declared if d.startswith("fv_pvpool_")} == set(PVPOOL_API)
    assert {n for n in _lib.EXPORTS if n.startswith("fv_pvpool_")} == set(PVPOOL_API)
    assert "#define FV_ABI_VERSION 5" in hdr and L.fv_abi_version() == 5      # the ABI version stays
    for name in PVPOOL_API:       # every entry names the reference code it stands beside, as the fv_pv_stream_* entries do
        at = re.search(r"FV_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr).start()
        assert "test.py:61-62" in hdr[hdr.rindex("/*", 0, at):at], name
    for name in ("step", "step_padded", "reset", "close", "received", "emitted", "pending"):
        assert callable(getattr(ps.PitchShiftPool, name)), name
    assert callable(ps.PitchShift.pool)


@pytest.mark.parametrize("frame", sref.GRID_FRAMES)
@pytest.mark.parametrize("n_steps", sref.GRID_STEPS)
def test_c_plan_python_plan_and_the_counting_rule_agree_over_random_schedules(n_steps, frame):
    """Subsets of the slots, chunk sizes including 0 and 1, flushes at any step including at N' = 0; a session's emissions sum to its
    length."""
    rule, mod = _rule(n_steps, frame)
    F, hop = frame
    rng = random.Random(int(n_steps * 10) * 131 + F + hop)
    S, max_chunk = 5, 3 * hop + 5
    pc = ps.PvPoolCounters(mod, S, max_chunk)
    ref = pool_ref.Sessions(rule, S)
    assert pc.plan([(4, 0, True)]) == [0] and _c_plan(mod, pc, [(4, 0, True)])[:2] == (0, [0]) == (0, ref.step([(4, 0, True)]))
    pc.step([(4, 0, True)])                                                          # a flush at N' = 0 emits nothing
    assert pc.flushed[4] and pc.received[4] == pc.emitted[4] == 0
    total = [0] * S
    utterances = zero_items = flushes = emitting = 0
    for t in range(60 if F > 64 else 160):
        live = [s for s in range(S) if not pc.flushed[s]]
        items = []
        for s in rng.sample(live, rng.randint(0, len(live))):
            c = rng.choice([0, 1, rng.randint(0, max_chunk), rng.randint(0, hop), max_chunk])
            items.append((s, c, rng.random() < 0.1))
            zero_items += c == 0
        r, got, msg = _c_plan(mod, pc, items)
        want, counted = pc.plan(items), ref.step(items)
        assert r == max(counted, default=0) and got == want == counted, (items, r, got, want, counted, msg)
        pc.commit(items, want)
        assert pc.max_outputs >= max(want, default=0)
        for (s, _, flush), k in zip(items, want):
            total[s] += k
            emitting += k > 0
            assert (pc.received[s], pc.emitted[s]) == (ref.N[s], ref.E[s]) and pc.pending(s) == ref.N[s] - ref.E[s] >= 0
            if flush:
                assert total[s] == pc.received[s] == pc.emitted[s]                   # as many samples out as went in
                flushes += 1
        for s in range(S):
            if pc.flushed[s] and rng.random() < 0.5:
                pc.reset(s), ref.reset(s)
                total[s] = 0
                utterances += 1
    assert zero_items > 5 and flushes > 5 and utterances > 2 and emitting > 10


@pytest.mark.parametrize("frame", [(64, 16), (64, 32)])
@pytest.mark.parametrize("n_steps", sref.GRID_STEPS)
@pytest.mark.parametrize("max_chunk", [1, 16, 100])
def test_a_max_chunk_push_that_flushes_stays_inside_every_bound_from_every_state(n_steps, frame, max_chunk):
    """Every state N < 400 (E = the counted emission): the step (max_chunk samples, flush) emits at most max_outputs — the C bound and the
    Python one, which agree — and makes ready at most the frames, stretched frames, stretched samples and resampled outputs the pool is sized
    for (fv_pvpool_bounds).  The plan refuses a step past its own bounds as an internal error, so its result says the same."""
    rule, mod = _rule(n_steps, frame)
    states = list(range(400))
    maxA, maxS, maxY, maxR, max_out = _c_bounds(mod, max_chunk)
    pc = ps.PvPoolCounters(mod, len(states), max_chunk)
    assert pc.max_outputs == max_out >= max_chunk
    pc.received = list(states)
    pc.emitted = [rule.emitted(N) for N in states]
    assert pc.emitted == [mod.stream_emitted(N) for N in states]
    items = [(N, max_chunk, True) for N in states]
    r, got, msg = _c_plan(mod, pc, items)
    want = [N + max_chunk - rule.emitted(N) for N in states]
    assert r == max(want) and got == want == pc.plan(items), msg
    assert max(want) <= max_out
    for N in states:
        dA, dS, dY = rule.made_ready(N, N + max_chunk, True)
        assert 0 <= dA <= maxA and 0 <= dS <= maxS and 0 <= dY <= maxY, (N, dA, dS, dY, maxA, maxS, maxY)
        Y, Y2 = rule.ready(N)[2], sref.whole_lengths(N + max_chunk, rule.o, rule.n, rule.hop)[2]
        out_len = -((-rule.filt.n * Y2) // rule.filt.o)
        inner = out_len - sref.resampled_ready(rule.filt, Y, out_len + rule.filt.n + 1)
        assert inner <= maxR, (N, inner, maxR)
    # the same push without the flush emits no more
    r2, got2, _ = _c_plan(mod, pc, [(N, max_chunk, False) for N in states])
    assert r2 >= 0 and all(a <= b for a, b in zip(got2, got))


@pytest.mark.parametrize("frame", [(64, 16), (64, 32)])
@pytest.mark.parametrize("n_steps", sref.GRID_STEPS)
def test_max_outputs_is_attained_over_two_periods(n_steps, frame):
    """max_outputs - max_chunk is the largest N - E(N) over every N of two periods of n hop samples past the start-up: the bound is exact."""
    _, mod = _rule(n_steps, frame)
    span = 2 * mod.n * frame[1] + 8 * frame[0] + 20000
    worst = max(N - mod.stream_emitted(N) for N in range(span))
    for max_chunk in (1, 100):
        assert _c_bounds(mod, max_chunk)[4] == ps.PvPoolCounters(mod, 1, max_chunk).max_outputs == max_chunk + worst


def test_every_refusal_by_status_and_by_name():
    rule, mod = _rule(3, (64, 16))
    S, max_chunk = 4, 300
    pc = ps.PvPoolCounters(mod, S, max_chunk)
    pc.step([(0, 200, False), (1, 300, True), (2, 5, False)])
    state = (list(pc.received), list(pc.emitted), list(pc.flushed))
    cases = [      # in sample_pool_admit's order per item
        ([(0, 1, False), (4, 1, False)], _lib.FV_ERR_INVALID, ValueError, r"item 1 names session 4"),
        ([(0, 1, False), (-1, 1, False)], _lib.FV_ERR_INVALID, ValueError, r"item 1 names session -1"),
        ([(3, 1, False), (0, 1, False), (3, 2, False)], _lib.FV_ERR_INVALID, ValueError, r"duplicate session 3 \(item 2\)"),
        ([(0, max_chunk + 1, False)], _lib.FV_ERR_INVALID, ValueError, r"item 0 \(session 0\) has %d samples" % (max_chunk + 1)),
        ([(3, 0, False), (0, -1, False)], _lib.FV_ERR_INVALID, ValueError, r"item 1 \(session 0\) has -1 samples"),
        ([(0, 1, False), (1, 0, False)], _lib.FV_ERR_STATE, PoolStateError, r"session 1 was flushed \(item 1\)"),
        ([(1, max_chunk + 1, False)], _lib.FV_ERR_INVALID, ValueError, r"item 0 \(session 1\) has %d samples" % (max_chunk + 1)),   # the size first
    ]
    for items, status, exc, pattern in cases:
        r, _, msg = _c_plan(mod, pc, items)
        assert r == status and msg.startswith("fv_pvpool_plan:") and re.search(pattern, msg), (items, r, msg)
        with pytest.raises(exc, match=pattern):
            pc.plan(items)
        with pytest.raises(exc, match=pattern):
            pc.step(items)
        assert (pc.received, pc.emitted, pc.flushed) == state, items      # a refused plan leaves the counters as they were
    # the pool's own, after the core's: more than 2^30 samples in one utterance
    far = ps.PvPoolCounters(mod, S, max_chunk)
    far.received[2] = (1 << 30) - 3
    far.emitted[2] = mod.stream_emitted(far.received[2])
    r, got, msg = _c_plan(mod, far, [(2, 3, False)])
    assert r >= 0 and got == far.plan([(2, 3, False)]), msg              # exactly 2^30 is taken
    r, _, msg = _c_plan(mod, far, [(0, 1, False), (2, 4, False)])
    assert r == _lib.FV_ERR_INVALID and re.search(r"item 1 takes session 2 past 2\^30 samples", msg), msg
    with pytest.raises(ValueError, match=r"item 1 takes session 2 past 2\^30 samples"):
        far.plan([(0, 1, False), (2, 4, False)])
    r, _, msg = _c_plan(mod, far, [(2, 4, False), (1, max_chunk + 1, False)])          # the core's refusal of a later item comes first
    assert r == _lib.FV_ERR_INVALID and re.search(r"item 1 \(session 1\) has %d samples" % (max_chunk + 1), msg), msg
    with pytest.raises(ValueError, match=r"item 1 \(session 1\) has %d samples" % (max_chunk + 1)):
        far.plan([(2, 4, False), (1, max_chunk + 1, False)])
    # flushed = NULL: no slot is flushed
    r, got, _ = _c_plan(mod, pc, [(3, 0, True)], flushed=False)
    assert r == 0 and got == [0]
    # the plan's own arguments
    L = _lib.lib()
    one, out = (_lib.WavPoolItem * 1)(_lib.WavPoolItem(0, 1, 0)), (i64 * 1)()
    z = (i64 * S)()
    cfg = mod.config()
    bad = ps.PitchShift(SR, 3).config()
    bad.sample_rate = 0
    for args, pattern in (((None, S, max_chunk), "null config"), ((ctypes.byref(bad), S, max_chunk), r"sample_rate = 0"),
                          ((ctypes.byref(cfg), 0, max_chunk), r"sessions \(0\)"), ((ctypes.byref(cfg), 65536, max_chunk), r"sessions \(65536\)"),
                          ((ctypes.byref(cfg), S, 0), r"max_chunk \(0\)")):
        assert L.fv_pvpool_plan(*args, z, z, None, one, 1, out) == _lib.FV_ERR_INVALID
        assert re.search(pattern, L.fv_last_error().decode()), L.fv_last_error()
    for sessions in (0, 65536):
        with pytest.raises(ValueError, match=r"sessions \(%d\)" % sessions):
            ps.PvPoolCounters(mod, sessions, max_chunk)
    # the identity shift: every item emits its own samples
    ident = ps.PitchShift(SR, 0, n_fft=64)
    ic = ps.PvPoolCounters(ident, 2, 50)
    assert ic.max_outputs == 50 == _c_bounds(ident, 50)[4]
    assert _c_plan(ident, ic, [(0, 50, False), (1, 7, True)])[:2] == (50, [50, 7]) and ic.step([(0, 50, False), (1, 7, True)]) == [50, 7]
    # the handle's entries on NULL: nothing to count, nothing to step, nothing to free
    assert L.fv_pvpool_max_outputs(None) == 0 and L.fv_pvpool_workspace_bytes(None) == 0
    assert L.fv_pvpool_received(None, 0) == L.fv_pvpool_emitted(None, 0) == L.fv_pvpool_pending(None, 0) == 0
    assert L.fv_pvpool_step(None, one, 1, None, 0, None, 0, 0, out, None, 0, None) == _lib.FV_ERR_INVALID
    assert L.fv_pvpool_reset(None, 0) == _lib.FV_ERR_INVALID
    assert L.fv_pvpool_bounds(ctypes.byref(cfg), 16, None) == _lib.FV_ERR_INVALID
    h = ctypes.c_void_p()
    assert L.fv_pvpool_create(None, 2, 64, ctypes.byref(h)) == _lib.FV_ERR_INVALID and not h.value
    L.fv_pvpool_destroy(None)
