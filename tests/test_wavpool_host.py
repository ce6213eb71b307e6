"""Host (no GPU): the wav pool (include/fishvoc.h fv_wavpool_*) — the ABI surface, the plan of a step stated twice (C: fv_wavpool_plan;
Python: vocoder_amd.framing.PoolCounters) over seeded random schedules, against one stream's counters per session, and every refusal of a
step by status and by the name in its message."""
import ctypes
import os
import random
import re

import pytest

from vocoder_amd import _lib, framing
from vocoder_amd.sessions import PoolStateError

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

WAVPOOL_API = ("fv_wavpool_create", "fv_wavpool_workspace_bytes", "fv_wavpool_max_frames", "fv_wavpool_received_samples",
               "fv_wavpool_emitted_frames", "fv_wavpool_pending_samples", "fv_wavpool_plan", "fv_wavpool_step", "fv_wavpool_reset",
               "fv_wavpool_destroy")
# (n_fft, hop): plain; hop does not divide n_fft; win - hop odd (pad_l != pad_r); a carry wider than one 256-thread block
FRAMINGS = [(256, 64), (96, 64), (256, 51), (320, 80)]
i64, i32 = ctypes.c_int64, ctypes.c_int32


def _cfg(n_fft, hop):
    return _lib.LogMelConfig(24000, n_fft, n_fft, hop, 20, 0.0, 12000.0)


def _c_plan(cfg, pc, items, flushed=True):
    """fv_wavpool_plan over the counters of ``pc`` -> (result, frames per item, message)."""
    L = _lib.lib()
    S, n = pc.S, len(items)
    arr = (_lib.WavPoolItem * max(n, 1))(*[_lib.WavPoolItem(int(s), int(c), int(f)) for s, c, f in items])
    out = (i64 * max(n, 1))()
    r = L.fv_wavpool_plan(ctypes.byref(cfg), S, pc.max_chunk, (i64 * S)(*pc.received), (i64 * S)(*pc.emitted),
                          (i32 * S)(*[int(f) for f in pc.flushed]) if flushed else None, arr, n, out)
    return int(r), [int(out[i]) for i in range(n)], L.fv_last_error().decode()


def test_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in WAVPOOL_API:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert {d for d in declared if d.startswith("fv_wavpool_")} == set(WAVPOOL_API)
    assert {n for n in _lib.EXPORTS if n.startswith("fv_wavpool_")} == set(WAVPOOL_API)
    assert ctypes.sizeof(_lib.WavPoolItem) == 12
    assert "#define FV_ABI_VERSION 5" in hdr and L.fv_abi_version() == 5
    for name in WAVPOOL_API:      # every entry names the reference code it stands beside, as the fv_logmel_* entries do
        at = re.search(r"FV_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr).start()
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "spectrogram.py:25-" in comment and "test.py:64-71" in comment, name


@pytest.mark.parametrize("n_fft,hop", FRAMINGS)
def test_c_plan_and_python_plan_agree_over_random_schedules(n_fft, hop):
    cfg, fr = _cfg(n_fft, hop), framing.Framing(n_fft, n_fft, hop)
    rng = random.Random(n_fft * 1000 + hop)
    S, max_chunk = 5, 2 * n_fft + 3
    pc = framing.PoolCounters(fr, S, max_chunk)
    lone = [framing.Counters(fr) for _ in range(S)]       # every session advanced alone through one stream's counters
    sizes = [0, 1, hop - 1, hop, hop + 1, n_fft, max_chunk]
    emitted_total = flushes = resets = idle = empty = 0
    for step in range(300):
        items = []
        for s in rng.sample(range(S), rng.randint(0, S)):
            if pc.flushed[s]:
                if rng.random() < 0.7:
                    pc.reset(s)
                    lone[s].reset()
                    resets += 1
                continue
            c = rng.choice(sizes) if rng.random() < 0.6 else rng.randint(0, max_chunk)
            flush = rng.random() < 0.15
            if flush and pc.received[s] + c > 0 and fr.too_short(pc.received[s] + c):
                flush = False                             # (the too-short flush has its own test)
            items.append((s, c, flush))
            empty += c == 0
        idle += len(items) < S
        r, got, msg = _c_plan(cfg, pc, items)
        want = pc.plan(items)
        assert r == max(want, default=0) and got == want, (step, items, got, want, msg)
        before = (list(pc.received), list(pc.emitted))
        pc.commit(items, want)
        for (s, c, flush), k in zip(items, want):
            lo = before[1][s]
            rng_frames = list(lone[s].push(c)) + (list(lone[s].flush()) if flush else [])
            assert rng_frames == list(range(lo, lo + k)), (step, s)
            assert (pc.received[s], pc.emitted[s], pc.flushed[s]) == (lone[s].N, lone[s].E, lone[s].flushed)
            assert 0 <= pc.pending_samples(s) < n_fft or flush
            assert k <= (n_fft + max_chunk) // hop + 2    # fv_wavpool_max_frames
            emitted_total += k
            flushes += flush
        untouched = set(range(S)) - {s for s, _, _ in items}
        assert all((pc.received[s], pc.emitted[s]) == (before[0][s], before[1][s]) for s in untouched)
    assert emitted_total > 100 and flushes > 10 and resets > 5 and idle > 50 and empty > 10      # the schedule did mix them


@pytest.mark.parametrize("n_fft,hop", FRAMINGS)
def test_every_refusal_by_status_and_by_name(n_fft, hop):
    cfg, fr = _cfg(n_fft, hop), framing.Framing(n_fft, n_fft, hop)
    S, max_chunk = 4, 3 * n_fft
    pc = framing.PoolCounters(fr, S, max_chunk)
    pc.step([(0, n_fft, False), (1, 2 * n_fft, True), (2, 5, False)])
    state = (list(pc.received), list(pc.emitted), list(pc.flushed))
    pad = max(fr.pad_l, fr.pad_r)
    assert fr.too_short(pad) and pc.received[2] + 1 <= pad
    cases = [
        ([(0, 1, False), (4, 1, False)], _lib.FV_ERR_INVALID, ValueError, r"item 1 names session 4"),
        ([(0, 1, False), (-1, 1, False)], _lib.FV_ERR_INVALID, ValueError, r"item 1 names session -1"),
        ([(3, 1, False), (0, 1, False), (3, 2, False)], _lib.FV_ERR_INVALID, ValueError, r"duplicate session 3 \(item 2\)"),
        ([(0, max_chunk + 1, False)], _lib.FV_ERR_INVALID, ValueError, r"item 0 \(session 0\) has %d samples" % (max_chunk + 1)),
        ([(3, 0, False), (0, -1, False)], _lib.FV_ERR_INVALID, ValueError, r"item 1 \(session 0\) has -1 samples"),
        ([(0, 1, False), (1, 0, False)], _lib.FV_ERR_STATE, PoolStateError, r"session 1 was flushed \(item 1\)"),
        ([(0, 1, False), (2, 1, True)], _lib.FV_ERR_INVALID, ValueError, r"session 2 \(item 1\) ends after 6 samples"),
        ([(3, pad, True)], _lib.FV_ERR_INVALID, ValueError, r"session 3 \(item 0\) ends after %d samples" % pad),
    ]
    for items, status, exc, pattern in cases:
        r, _, msg = _c_plan(cfg, pc, items)
        assert r == status and re.search(pattern, msg), (items, r, msg)
        with pytest.raises(exc, match=pattern):
            pc.plan(items)
        with pytest.raises(exc, match=pattern):
            pc.step(items)
        assert (pc.received, pc.emitted, pc.flushed) == state, items      # a refused plan leaves the counters as they were
    # more than 2^40 samples in one utterance
    far = framing.PoolCounters(fr, S, max_chunk)
    far.received[2] = framing.MAX_SAMPLES - 3
    far.emitted[2] = fr.frames_ready(far.received[2])
    assert _c_plan(cfg, far, [(2, 3, False)])[1] == far.plan([(2, 3, False)])      # exactly 2^40 is taken
    r, _, msg = _c_plan(cfg, far, [(0, 1, False), (2, 4, False)])
    assert r == _lib.FV_ERR_INVALID and re.search(r"item 1 takes session 2 past 2\^40 samples", msg), msg
    with pytest.raises(ValueError, match=r"item 1 takes session 2 past 2\^40 samples"):
        far.plan([(0, 1, False), (2, 4, False)])
    # flushed = NULL: no slot is flushed; a flush at N' = 0 emits nothing and is no refusal
    r, got, _ = _c_plan(cfg, pc, [(1, 0, False), (3, 0, True)], flushed=False)
    assert r == 0 and got == [0, 0]
    assert pc.plan([(3, 0, True)]) == [0]
    # the plan's own arguments
    L = _lib.lib()
    one, out = (_lib.WavPoolItem * 1)(_lib.WavPoolItem(0, 1, 0)), (i64 * 1)()
    z = (i64 * S)()
    for args, pattern in (((None, S, max_chunk), "unusable config"), ((ctypes.byref(cfg), 0, max_chunk), r"sessions \(0\)"),
                          ((ctypes.byref(cfg), 65536, max_chunk), r"sessions \(65536\)"), ((ctypes.byref(cfg), S, 0), r"max_chunk \(0\)")):
        assert L.fv_wavpool_plan(*args, z, z, None, one, 1, out) == _lib.FV_ERR_INVALID
        assert re.search(pattern, L.fv_last_error().decode()), L.fv_last_error()
    for sessions in (0, 65536):
        with pytest.raises(ValueError, match=r"sessions \(%d\)" % sessions):
            framing.PoolCounters(fr, sessions, max_chunk)
    # the handle's entries on NULL: nothing to count, nothing to step, nothing to free
    assert L.fv_wavpool_workspace_bytes(None) == 0 and L.fv_wavpool_max_frames(None) == 0
    assert L.fv_wavpool_received_samples(None, 0) == L.fv_wavpool_emitted_frames(None, 0) == L.fv_wavpool_pending_samples(None, 0) == 0
    assert L.fv_wavpool_step(None, one, 1, None, 0, None, 0, out, None, 0, None) == _lib.FV_ERR_INVALID
    assert L.fv_wavpool_reset(None, 0) == _lib.FV_ERR_INVALID
    h = ctypes.c_void_p()
    assert L.fv_wavpool_create(None, 2, 64, ctypes.byref(h)) == _lib.FV_ERR_INVALID and not h.value
    L.fv_wavpool_destroy(None)


def test_modules_and_classes_offer_the_pool():
    from vocoder_amd import inference
    from vocoder_amd.data.transforms import LogMelSpectrogram
    from vocoder_amd.data.transforms.spectrogram import LinearSpectrogram
    from vocoder_amd.engine import Engine, WavPool
    from vocoder_amd.modules.generators import HiFiGANGenerator
    for m in (LogMelSpectrogram(sample_rate=24000, n_fft=256, win_length=256, hop_length=51, n_mels=20), LinearSpectrogram(96, 96, 64)):
        with pytest.raises(RuntimeError, match="needs the module on a HIP device"):      # no CPU path
            m.wav_pool(2, 64)
    assert callable(Engine.wav_pool)
    for name in ("step", "step_padded", "reset", "close", "received_samples", "emitted_frames", "pending_samples"):
        assert callable(getattr(WavPool, name)), name
    # a generator that takes a pitch template is refused by name, before any device work
    tiny = dict(hop_length=64, num_mels=20, upsample_initial_channel=32, upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4],
                resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]], pre_conv_kernel_size=7, post_conv_kernel_size=7)
    front = LogMelSpectrogram(sample_rate=16000, n_fft=256, win_length=256, hop_length=64, n_mels=20)
    with pytest.raises(ValueError, match="HiFiGANGenerator takes a pitch template"):
        inference.WavSessionPool(front, HiFiGANGenerator(**tiny, use_template=True), 2, 256)
