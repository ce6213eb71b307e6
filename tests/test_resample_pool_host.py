"""Host (no GPU): the resample pool (include/fishvoc.h fv_respool_*) — the ABI surface, the plan of a step stated twice (C: fv_respool_plan;
Python: vocoder_amd.resample.ResamplePoolCounters) over seeded random schedules against Design.emit_count / output_length, the bound on one
item's emission by brute force, every refusal of a step by status and by the name in its message, and the keyword refusals of
inference.WavSessionPool."""
import ctypes
import os
import random
import re

import pytest

from vocoder_amd import _lib
from vocoder_amd import resample as rs
from vocoder_amd.sessions import PoolStateError

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RESPOOL_API = ("fv_respool_create", "fv_respool_max_outputs", "fv_respool_received", "fv_respool_emitted", "fv_respool_pending",
               "fv_respool_plan", "fv_respool_step", "fv_respool_reset", "fv_respool_destroy")
PAIRS = [(44100, 48000), (48000, 8000), (2, 3), (3, 2)]
i64, i32 = ctypes.c_int64, ctypes.c_int32
_designs: dict = {}


def _design(pair):
    if pair not in _designs:
        _designs[pair] = rs.design(*pair)
    return _designs[pair]


def _cfg(pair):
    return _lib.ResampleConfig(pair[0], pair[1], 6, 0.99, _lib.FV_RESAMPLE_SINC_HANN, 0.0)


def _c_plan(cfg, pc, items, flushed=True):
    """fv_respool_plan over the counters of ``pc`` -> (result, outputs per item, message)."""
    L = _lib.lib()
    S, n = pc.S, len(items)
    arr = (_lib.WavPoolItem * max(n, 1))(*[_lib.WavPoolItem(int(s), int(c), int(f)) for s, c, f in items])
    out = (i64 * max(n, 1))()
    r = L.fv_respool_plan(ctypes.byref(cfg), S, pc.max_chunk, (i64 * S)(*pc.received), (i64 * S)(*pc.emitted),
                          (i32 * S)(*[int(f) for f in pc.flushed]) if flushed else None, arr, n, out)
    return int(r), [int(out[i]) for i in range(n)], L.fv_last_error().decode()


def test_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in RESPOOL_API:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert {d for d in declared if d.startswith("fv_respool_")} == set(RESPOOL_API)
    assert {n for n in _lib.EXPORTS if n.startswith("fv_respool_")} == set(RESPOOL_API)
    assert "#define FV_ABI_VERSION 5" in hdr and L.fv_abi_version() == 5
    for name in RESPOOL_API:      # every entry names the reference code it stands beside, as the fv_resample_* entries do
        at = re.search(r"FV_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr).start()
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "test.py:54" in comment and "hq_pitch_shift.py:33" in comment, name
    for name in ("step", "step_padded", "reset", "close", "received", "emitted", "pending"):
        assert callable(getattr(rs.ResamplePool, name)), name
    assert callable(rs.Resample.pool)


@pytest.mark.parametrize("pair", PAIRS)
def test_c_plan_and_python_plan_agree_over_random_schedules(pair):
    """Between flushes a session's emitted total is emit_count(N), after its flush output_length(N); zero-sample items and a flush at
    N' = 0 are part of the schedule."""
    cfg, d = _cfg(pair), _design(pair)
    rng = random.Random(pair[0] * 7 + pair[1])
    S, max_chunk = 5, 3 * d.o + 11
    pc = rs.ResamplePoolCounters(d, S, max_chunk)
    assert pc.plan([(4, 0, True)]) == [0] and _c_plan(cfg, pc, [(4, 0, True)])[:2] == (0, [0])      # a flush at N' = 0 emits nothing
    pc.step([(4, 0, True)])
    assert pc.flushed[4] and pc.received[4] == pc.emitted[4] == 0
    utterances, zero_items, flushes = 0, 0, 0
    for t in range(400):
        live = [s for s in range(S) if not pc.flushed[s]]
        items = []
        for s in rng.sample(live, rng.randint(0, len(live))):
            c = rng.choice([0, 1, rng.randint(0, max_chunk), rng.randint(0, d.o), max_chunk])
            items.append((s, c, rng.random() < 0.08))
            zero_items += c == 0
        r, got, msg = _c_plan(cfg, pc, items)
        want = pc.plan(items)
        assert r == max(want, default=0) and got == want, (items, r, got, want, msg)
        pc.commit(items, want)
        for s, _, flush in items:
            N = pc.received[s]
            assert pc.emitted[s] == (d.output_length(N) if flush else d.emit_count(N)), (s, N, flush)
            assert pc.pending(s) == d.output_length(N) - pc.emitted[s] >= 0
            flushes += flush
        for s in range(S):
            if pc.flushed[s] and rng.random() < 0.5:
                pc.reset(s)
                utterances += 1
    assert zero_items > 20 and flushes > 10 and utterances > 5


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("max_chunk", [1, 7, 4096])
def test_max_outputs_bounds_every_step_and_is_attained(pair, max_chunk):
    """E' - E of a step from the state (N, E = emit_count(N)), for every N over a few periods of o from 0 on and every chunk size up to
    min(max_chunk, 64), with and without flush: never above max_outputs.  Where the sweep reaches c = max_chunk (1 and 7) some state attains
    the bound; at 4096 the bound is the sweep's flush maximum moved from c = 64 to c = 4096 by whole outputs: within one of
    n (4096 - 64) / o above it."""
    d = _design(pair)
    bound = rs.ResamplePoolCounters(d, 1, max_chunk).max_outputs
    top = min(max_chunk, 64)
    worst = 0
    for N in range(0, 4 * d.o + 2 * d.width + 1):
        E = d.emit_count(N)
        for c in range(0, top + 1):
            push, flush = max(E, d.emit_count(N + c)) - E, d.output_length(N + c) - E
            assert 0 <= push <= flush <= bound, (N, c, push, flush, bound)
            worst = max(worst, flush)
    if top == max_chunk:
        assert worst == bound, (worst, bound)
    else:
        shift = d.n * (max_chunk - top) / d.o
        assert worst + shift - 1 < bound < worst + shift + 1, (worst, bound, shift)


@pytest.mark.parametrize("pair", PAIRS[:2])
def test_every_refusal_by_status_and_by_name(pair):
    cfg, d = _cfg(pair), _design(pair)
    S, max_chunk = 4, 300
    pc = rs.ResamplePoolCounters(d, S, max_chunk)
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
        r, _, msg = _c_plan(cfg, pc, items)
        assert r == status and msg.startswith("fv_respool_plan:") and re.search(pattern, msg), (items, r, msg)
        with pytest.raises(exc, match=pattern):
            pc.plan(items)
        with pytest.raises(exc, match=pattern):
            pc.step(items)
        assert (pc.received, pc.emitted, pc.flushed) == state, items      # a refused plan leaves the counters as they were
    # more than 2^40 samples in one utterance
    far = rs.ResamplePoolCounters(d, S, max_chunk)
    far.received[2] = (1 << 40) - 3
    far.emitted[2] = d.emit_count(far.received[2])
    assert _c_plan(cfg, far, [(2, 3, False)])[1] == far.plan([(2, 3, False)])      # exactly 2^40 is taken
    r, _, msg = _c_plan(cfg, far, [(0, 1, False), (2, 4, False)])
    assert r == _lib.FV_ERR_INVALID and re.search(r"item 1 takes session 2 past 2\^40 samples", msg), msg
    with pytest.raises(ValueError, match=r"item 1 takes session 2 past 2\^40 samples"):
        far.plan([(0, 1, False), (2, 4, False)])
    # flushed = NULL: no slot is flushed
    r, got, _ = _c_plan(cfg, pc, [(1, 0, False), (3, 0, True)], flushed=False)
    assert r == 0 and got == [0, 0]
    # the plan's own arguments
    L = _lib.lib()
    one, out = (_lib.WavPoolItem * 1)(_lib.WavPoolItem(0, 1, 0)), (i64 * 1)()
    z = (i64 * S)()
    bad = _lib.ResampleConfig(pair[0], 0, 6, 0.99, 0, 0.0)
    for args, pattern in (((None, S, max_chunk), "null config"), ((ctypes.byref(bad), S, max_chunk), r"new_freq = 0"),
                          ((ctypes.byref(cfg), 0, max_chunk), r"sessions \(0\)"), ((ctypes.byref(cfg), 65536, max_chunk), r"sessions \(65536\)"),
                          ((ctypes.byref(cfg), S, 0), r"max_chunk \(0\)")):
        assert L.fv_respool_plan(*args, z, z, None, one, 1, out) == _lib.FV_ERR_INVALID
        assert re.search(pattern, L.fv_last_error().decode()), L.fv_last_error()
    for sessions in (0, 65536):
        with pytest.raises(ValueError, match=r"sessions \(%d\)" % sessions):
            rs.ResamplePoolCounters(d, sessions, max_chunk)
    # the handle's entries on NULL: nothing to count, nothing to step, nothing to free
    assert L.fv_respool_max_outputs(None) == 0
    assert L.fv_respool_received(None, 0) == L.fv_respool_emitted(None, 0) == L.fv_respool_pending(None, 0) == 0
    assert L.fv_respool_step(None, one, 1, None, 0, None, 0, 0, out, None) == _lib.FV_ERR_INVALID
    assert L.fv_respool_reset(None, 0) == _lib.FV_ERR_INVALID
    h = ctypes.c_void_p()
    assert L.fv_respool_create(None, 2, 64, ctypes.byref(h)) == _lib.FV_ERR_INVALID and not h.value
    L.fv_respool_destroy(None)


class _Front:
    """What WavSessionPool's constructor reads of a front-end before it touches the device."""
    sampling_rate = 24000

    def wav_pool(self, sessions, max_chunk_samples):
        raise AssertionError("the keyword refusals come before any pool is made")


class _Gen:
    use_template = False

    def session_pool(self, sessions, max_chunk_frames):
        raise AssertionError("the keyword refusals come before any pool is made")


def test_wav_session_pool_refuses_its_keywords_by_name_before_any_device_work():
    from vocoder_amd import inference
    front, gen = _Front(), _Gen()
    to_model, to_client = rs.Resample(48000, 24000), rs.Resample(24000, 48000)
    with pytest.raises(ValueError, match=r"input_resample has new_freq = 48000 Hz.*24000 Hz"):
        inference.WavSessionPool(front, gen, 2, 256, input_resample=to_client)
    with pytest.raises(ValueError, match=r"output_resample has orig_freq = 48000 Hz.*24000 Hz"):
        inference.WavSessionPool(front, gen, 2, 256, output_resample=to_model)
    with pytest.raises(ValueError, match=r"output_resample has orig_freq = 48000 Hz"):      # the good one of the two does not hide the other
        inference.WavSessionPool(front, gen, 2, 256, input_resample=to_model, output_resample=to_model)
    with pytest.raises(ValueError, match=r"input_resample must be a vocoder_amd.resample.Resample, got int"):
        inference.WavSessionPool(front, gen, 2, 256, input_resample=48000)
    with pytest.raises(ValueError, match=r"output_resample must be a vocoder_amd.resample.Resample, got str"):
        inference.WavSessionPool(front, gen, 2, 256, output_resample="48000")
    # matching rates pass the keyword checks and reach the pools (here: the stub's own assertion; no device)
    with pytest.raises(AssertionError, match="before any pool is made"):
        inference.WavSessionPool(front, gen, 2, 256, output_resample=to_client)
    # LogMelSpectrogram declares its rate as sample_rate
    from vocoder_amd.data.transforms import LogMelSpectrogram
    mel = LogMelSpectrogram(sample_rate=16000, n_fft=256, win_length=256, hop_length=64, n_mels=20)
    with pytest.raises(ValueError, match=r"input_resample has new_freq = 24000 Hz.*16000 Hz"):
        inference.WavSessionPool(mel, gen, 2, 256, input_resample=to_model)
