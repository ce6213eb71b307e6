"""Host (no GPU): the tracker pool and the oscillator pool (include/fishvoc.h fv_yinpool_*, fv_oscpool_*) — the ABI surface, the plan of a step
stated three times (C: fv_yinpool_plan / fv_oscpool_plan; Python: vocoder_amd.f0.YinPoolCounters / OscPoolCounters; the restatement
f0_pool_reference.py) over seeded random step lists, every refusal by status, item and session, the bound on one item's emission by brute
force, a session alone against the streams' rule, and the template= refusals of inference.WavSessionPool."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import f0_pool_reference as pref
import f0_stream_reference as sref
from vocoder_amd import _lib
from vocoder_amd import f0 as f0mod
from vocoder_amd.sessions import PoolStateError

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
YINPOOL_API = ("fv_yinpool_create", "fv_yinpool_max_frames", "fv_yinpool_received", "fv_yinpool_emitted", "fv_yinpool_pending",
               "fv_yinpool_plan", "fv_yinpool_step", "fv_yinpool_reset", "fv_yinpool_destroy")
OSCPOOL_API = tuple(n.replace("fv_yinpool", "fv_oscpool") for n in YINPOOL_API)
# (sr, W, hop, fmin, fmax): the stream tests' configurations, hop > W among them
CONFIGS = [(8000, 512, 128, 50.0, 500.0), (16000, 1024, 256, 60.0, 800.0), (8000, 512, 600, 50.0, 500.0), (44100, 2048, 512, 40.0, 1100.0)]
i64, i32 = ctypes.c_int64, ctypes.c_int32


def _c_plan(fn, cfg, pc, items, flushed=True):
    """fv_*pool_plan over the counters of ``pc`` -> (result, frames per item, message)."""
    L = _lib.lib()
    S, n = pc.S, len(items)
    arr = (_lib.WavPoolItem * max(n, 1))(*[_lib.WavPoolItem(int(s), int(c), int(f)) for s, c, f in items])
    out = (i64 * max(n, 1))()
    r = getattr(L, fn)(ctypes.byref(cfg), S, pc.max_chunk, (i64 * S)(*pc.received), (i64 * S)(*pc.emitted),
                       (i32 * S)(*[int(f) for f in pc.flushed]) if flushed else None, arr, n, out)
    return int(r), [int(out[i]) for i in range(n)], L.fv_last_error().decode()


def _pools(cfg, S, max_chunk):
    """(plan entry, config struct, Python counters, reference slots) of both pools for one configuration."""
    sr, W, hop, fmin, fmax = cfg
    return [("fv_yinpool_plan", _lib.F0Config(sr, W, hop, fmin, fmax, 0.1), f0mod.YinPoolCounters(W, hop, S, max_chunk),
             pref.yin_slots(S, max_chunk, W, hop)),
            ("fv_oscpool_plan", _lib.TemplateConfig(sr, hop, 0, 1.0), f0mod.OscPoolCounters(S, max_chunk), pref.osc_slots(S, max_chunk))]


def test_entry_points_are_declared_listed_exported_and_the_abi_stays_5():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in YINPOOL_API + OSCPOOL_API:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
        at = re.search(r"FV_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr).start()
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "refinegan.py:287" in comment and "hifigan.py:226" in comment, name
    assert {d for d in declared if d.startswith("fv_yinpool_")} == set(YINPOOL_API)
    assert {d for d in declared if d.startswith("fv_oscpool_")} == set(OSCPOOL_API)
    assert {n for n in _lib.EXPORTS if n.startswith(("fv_yinpool_", "fv_oscpool_"))} == set(YINPOOL_API + OSCPOOL_API)
    assert "#define FV_ABI_VERSION 5" in hdr and _lib.FV_ABI_VERSION == 5 and L.fv_abi_version() == 5
    assert "Not built: per-session" not in hdr
    import vocoder_amd
    for name in ("YinF0Pool", "PitchTemplatePool", "TemplatePool"):
        assert getattr(vocoder_amd, name) is getattr(f0mod, name), name
    assert callable(f0mod.YinF0.pool) and callable(f0mod.PitchTemplate.pool)
    for cls in (f0mod.YinF0Pool, f0mod.PitchTemplatePool, f0mod.TemplatePool):
        for m in ("step", "step_padded", "reset", "close", "received", "emitted", "pending", "__enter__", "__exit__"):
            assert callable(getattr(cls, m)), (cls, m)
    for cls in (f0mod.YinPoolCounters, f0mod.OscPoolCounters, f0mod.TemplatePoolCounters):
        assert callable(cls.plan) and callable(cls.step), cls


@pytest.mark.parametrize("cfg", CONFIGS)
def test_c_plan_python_plan_and_the_restatement_agree_over_random_step_lists(cfg):
    """Subsets of the slots, chunk sizes from 0 to max_chunk, flushes (one at N' = 0 first) and resets; plan() moves nothing."""
    sr, W, hop = cfg[:3]
    rng = random.Random(sr + W + hop)
    S = 5
    for max_chunk in (1, W // 3 + 7, 2 * W + hop):
        for fn, ccfg, pc, ref in _pools(cfg, S, max_chunk):
            assert pc.plan([(4, 0, True)]) == ref.plan([(4, 0, True)]) == [0] and _c_plan(fn, ccfg, pc, [(4, 0, True)])[:2] == (0, [0])
            pc.step([(4, 0, True)]), ref.step([(4, 0, True)])
            assert pc.flushed[4] and pc.received[4] == pc.emitted[4] == 0
            zero_items = flushes = utterances = emitted = 0
            for _ in range(250):
                live = [s for s in range(S) if not pc.flushed[s]]
                items = []
                for s in rng.sample(live, rng.randint(0, len(live))):
                    c = rng.choice([0, 1, rng.randint(0, max_chunk), rng.randint(0, min(max_chunk, hop)), max_chunk])
                    items.append((s, c, rng.random() < 0.08))
                    zero_items += c == 0
                before = (list(pc.received), list(pc.emitted), list(pc.flushed))
                want = ref.plan(items)
                r, got, msg = _c_plan(fn, ccfg, pc, items)
                assert pc.plan(items) == want and got == want and r == max(want, default=0), (fn, items, r, got, want, msg)
                assert (pc.received, pc.emitted, pc.flushed) == before                    # plan() moves nothing
                assert pc.step(items) == ref.step(items) == want
                assert (pc.received, pc.emitted, pc.flushed) == (ref.received, ref.emitted, ref.flushed)
                assert max(want, default=0) <= pc.max_frames
                emitted += sum(want)
                flushes += sum(f for _, _, f in items)
                for s in range(S):
                    if pc.flushed[s] and rng.random() < 0.5:
                        pc.reset(s), ref.reset(s)
                        utterances += 1
            assert zero_items > 10 and flushes > 5 and utterances > 3 and (emitted > 0 or max_chunk == 1), (fn, max_chunk)


@pytest.mark.parametrize("which", [0, 1])
def test_every_refusal_by_status_item_and_session(which):
    cfg = CONFIGS[0]
    S, max_chunk = 4, 300
    fn, ccfg, pc, ref = _pools(cfg, S, max_chunk)[which]
    first = [(0, 200, False), (1, 300, True), (2, 5, False)]
    pc.step(first), ref.step(first)
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
        r, _, msg = _c_plan(fn, ccfg, pc, items)
        assert r == status and msg.startswith(fn + ":") and re.search(pattern, msg), (items, r, msg)
        with pytest.raises(exc, match=pattern):
            pc.plan(items)
        with pytest.raises(exc, match=pattern):
            pc.step(items)
        with pytest.raises(pref.Refused) as ei:
            ref.plan(items)
        named = re.search(r"item (\d+)", msg), re.search(r"session (-?\d+)", msg)
        assert (ei.value.kind == "state") == (status == _lib.FV_ERR_STATE)
        assert (int(named[0].group(1)), int(named[1].group(1))) == (ei.value.item, ei.value.session), (msg, ei.value)
        assert (pc.received, pc.emitted, pc.flushed) == state, items      # a refused plan leaves the counters as they were
    # more than 2^40 samples in one utterance
    far = _pools(cfg, S, max_chunk)[which][2]
    far.received[2] = (1 << 40) - 3
    far.emitted[2] = far.received[2] - 1 if which else sref.frames_ready(far.received[2], cfg[1], cfg[2])
    assert _c_plan(fn, ccfg, far, [(2, 3, False)])[1] == far.plan([(2, 3, False)])      # exactly 2^40 is taken
    r, _, msg = _c_plan(fn, ccfg, far, [(0, 1, False), (2, 4, False)])
    assert r == _lib.FV_ERR_INVALID and re.search(r"item 1 takes session 2 past 2\^40 samples", msg), msg
    with pytest.raises(ValueError, match=r"item 1 takes session 2 past 2\^40 samples"):
        far.plan([(0, 1, False), (2, 4, False)])
    # flushed = NULL: no slot is flushed
    r, got, _ = _c_plan(fn, ccfg, pc, [(1, 0, False), (3, 0, True)], flushed=False)
    assert r == 0 and got == [0, 0]
    # the plan's own arguments
    L = _lib.lib()
    one, out, z = (_lib.WavPoolItem * 1)(_lib.WavPoolItem(0, 1, 0)), (i64 * 1)(), (i64 * S)()
    plan = getattr(L, fn)
    for args, pattern in (((None, S, max_chunk), "null config"), ((ctypes.byref(ccfg), 0, max_chunk), r"sessions \(0\)"),
                          ((ctypes.byref(ccfg), 65536, max_chunk), r"sessions \(65536\)"), ((ctypes.byref(ccfg), S, 0), r"max_chunk \(0\)")):
        assert plan(*args, z, z, None, one, 1, out) == _lib.FV_ERR_INVALID
        assert re.search(pattern, L.fv_last_error().decode()), L.fv_last_error()
    bad = _lib.TemplateConfig(8000, 0, 0, 1.0) if which else _lib.F0Config(8000, 511, 128, 50.0, 500.0, 0.1)
    assert plan(ctypes.byref(bad), S, max_chunk, z, z, None, one, 1, out) == _lib.FV_ERR_INVALID
    assert re.search("hop_length" if which else "frame_length", L.fv_last_error().decode())
    for sessions in (0, 65536):
        with pytest.raises(ValueError, match=r"sessions \(%d\)" % sessions):
            type(pc)(*((sessions, max_chunk) if which else (cfg[1], cfg[2], sessions, max_chunk)))
    # the handle's entries on NULL: nothing to count, nothing to step, nothing to free
    pre = "fv_oscpool" if which else "fv_yinpool"
    assert getattr(L, pre + "_max_frames")(None) == 0
    assert getattr(L, pre + "_received")(None, 0) == getattr(L, pre + "_emitted")(None, 0) == getattr(L, pre + "_pending")(None, 0) == 0
    if which:
        assert L.fv_oscpool_step(None, one, 1, None, 0, None, 0, 0, out, None) == _lib.FV_ERR_INVALID
    else:
        assert L.fv_yinpool_step(None, one, 1, None, 0, None, None, 0, 0, out, None) == _lib.FV_ERR_INVALID
    assert getattr(L, pre + "_reset")(None, 0) == _lib.FV_ERR_INVALID
    h = ctypes.c_void_p()
    assert getattr(L, pre + "_create")(None, 2, 64, ctypes.byref(h)) == _lib.FV_ERR_INVALID and not h.value
    getattr(L, pre + "_destroy")(None)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("max_chunk", [1, 37, 4096])
def test_max_frames_is_the_brute_force_maximum_and_a_state_attains_it(cfg, max_chunk):
    sr, W, hop, fmin, fmax = cfg
    pc = f0mod.YinPoolCounters(W, hop, 1, max_chunk)
    states = range(hop // 2 + W // 2 + 2 * hop)
    brute = max((N + max_chunk) // hop - sref.frames_ready(N, W, hop) for N in states)
    assert pc.max_frames == brute == pref.yin_max_frames(max_chunk, W, hop)
    # the period: a sweep three hops longer finds nothing larger
    assert max((N + max_chunk) // hop - sref.frames_ready(N, W, hop) for N in range(states[-1] + 1, states[-1] + 1 + 3 * hop)) <= brute
    ccfg = _lib.F0Config(sr, W, hop, fmin, fmax, 0.1)
    attained = False
    for N in states:
        pc.received[0], pc.emitted[0] = N, sref.frames_ready(N, W, hop)
        for flush in (False, True):
            k = pc.plan([(0, max_chunk, flush)])[0]
            assert 0 <= k <= brute
            if k == brute:
                attained = attained or _c_plan("fv_yinpool_plan", ccfg, pc, [(0, max_chunk, flush)])[:2] == (brute, [brute])
    assert attained
    assert f0mod.OscPoolCounters(1, max_chunk).max_frames == max_chunk + 1      # Tn - E = 1, then max_chunk frames and the flush


@pytest.mark.parametrize("cfg", CONFIGS)
def test_a_session_alone_emits_the_counts_of_the_streams_rule(cfg):
    sr, W, hop = cfg[:3]
    rng = np.random.default_rng(W + hop)
    for L in (0, 1, hop, 3 * W + 17, int(rng.integers(1, 9 * max(W, hop)))):
        sizes = sref.chunk_sizes(L, rng, 2 * max(W, hop))
        yc, oc = f0mod.YinPoolCounters(W, hop, 3, 2 * max(W, hop)), f0mod.OscPoolCounters(3, 2 * max(W, hop) // hop + 2)
        N = E = Tn = Eo = 0
        for c in sizes:
            N += c
            E2 = max(E, sref.frames_ready(N, W, hop))
            assert yc.step([(1, c, False)]) == [E2 - E]
            Tn += E2 - E
            Eo2 = sref.osc_emitted(Tn, Eo)
            assert oc.step([(1, E2 - E, False)]) == [Eo2 - Eo]
            E, Eo = E2, Eo2
            assert yc.pending(1) == sref.pending_samples(N, E, W, hop) and oc.pending(1) == Tn - Eo
        assert yc.step([(1, 0, True)]) == [N // hop - E]
        Tn += N // hop - E
        assert oc.step([(1, N // hop - E, True)]) == [Tn - Eo]
        assert yc.received[1] == L and yc.emitted[1] == oc.received[1] == oc.emitted[1] == L // hop
        assert yc.received[0] == yc.emitted[0] == oc.received[2] == 0


def test_the_template_pool_counters_chain_the_two_plans():
    W, hop, S = 512, 128, 3
    tc = f0mod.TemplatePoolCounters(f0mod.YinPoolCounters(W, hop, S, 700), f0mod.OscPoolCounters(S, 9))
    before = list(tc.tracker.received), list(tc.template.received)
    frames, emit = tc.plan([(2, 700, False), (0, 100, True)])
    assert frames == [sref.frames_ready(700, W, hop), 0] and emit == [frames[0] - 1, 0]
    assert (tc.tracker.received, tc.template.received) == tuple(before)
    assert tc.step([(2, 700, False), (0, 100, True)]) == (frames, emit)
    assert tc.step([(2, 0, True)]) == ([700 // hop - frames[0]], [700 // hop - emit[0]])
    with pytest.raises(PoolStateError, match=r"session 0 was flushed"):
        tc.plan([(0, 1, False)])
    tc.reset(0)
    assert tc.plan([(0, 1, False)]) == ([0], [0])


class _Front:
    sampling_rate = 24000

    def wav_pool(self, sessions, max_chunk_samples):
        raise AssertionError("the keyword refusals come before any pool is made")


class _Gen:
    use_template = False

    def session_pool(self, sessions, max_chunk_frames):
        raise AssertionError("the keyword refusals come before any pool is made")


class _TemplateGen(_Gen):
    use_template = True


def test_wav_session_pool_refuses_template_keywords_before_any_device_work():
    from vocoder_amd import inference
    with pytest.raises(ValueError, match=r"template= was given, but _Gen takes no pitch template"):
        inference.WavSessionPool(_Front(), _Gen(), 2, 256, template={})
    with pytest.raises(ValueError, match=r"_TemplateGen takes a pitch template.*template="):
        inference.WavSessionPool(_Front(), _TemplateGen(), 2, 256)
    with pytest.raises(ValueError, match=r"unknown keys \['hop_length'\]"):
        inference.WavSessionPool(_Front(), _TemplateGen(), 2, 256, template=dict(hop_length=64))
    with pytest.raises(AssertionError, match="before any pool is made"):      # a good dict passes the keyword checks and reaches the pools
        inference.WavSessionPool(_Front(), _TemplateGen(), 2, 256, template=dict(frame_length=1024, fmin=60.0))
