"""GPU: the tracker pool and the oscillator pool (fv_yinpool_*, fv_oscpool_*; yin_pool_kernel and the osc_pool kernels in
vocoder_amd/csrc/f0_template.hip) through ``vocoder_amd.f0``, and ``inference.WavSessionPool(template=...)``.

Every comparison of the pools is on bits against the whole-row GPU result of the session's own utterance: a YIN frame's bits depend on the plan
alone and the oscillator's phase is a wrapping integer sum, so there is no tolerance to choose.  Every chunk buffer is a strided view with NaN
beside and below the items' samples, and every output buffer starts as NaN: a NaN or a changed bit means something outside an item's samples
was read, a surviving NaN that a column was not written.  The chain's bar is the generator pool's own, 2e-5 * max(1, peak)
(tests/test_gpu_pool.py, tests/test_gpu_stream.py)."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

import f0_pool_reference as pref
import f0_reference as fref
from vocoder_amd import _lib
from vocoder_amd import f0 as f0mod
from vocoder_amd import synthetic as syn
from vocoder_amd._lib import FishVocError
from vocoder_amd.sessions import PoolStateError

pytestmark = pytest.mark.gpu

# (sr, W, hop, fmin, fmax, L): the three smallest of tests/test_gpu_f0_stream.py
CONFIGS = [(8000, 512, 128, 50.0, 500.0, 3001), (16000, 1024, 256, 60.0, 800.0, 6001)]
WIDE_HOP = (8000, 512, 600, 50.0, 500.0, 3001)      # hop > W: the carry is longer than a frame
S = 4


def _bits(a) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _cfg(i):
    return WIDE_HOP if i < 0 else CONFIGS[i]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Configuration i: S rolled glides of different lengths on the device, the tracker, and YinF0.forward of every utterance alone (computed
    once, never changed)."""
    sr, W, hop, fmin, fmax, L = _cfg(i)
    x = fref.glide(L, sr, seed=1)[0]
    lengths = (L, L - 517, 2 * hop + 3, L // 2 + 11)
    xs = tuple(torch.from_numpy(np.roll(x, 37 * s)[:n].copy()).cuda() for s, n in enumerate(lengths))
    mod = f0mod.YinF0(sr, hop, W, fmin, fmax)
    whole = tuple(tuple(_bits(v[0]) for v in mod(u[None])) for u in xs)
    assert all(w[0].shape == (n // hop,) for w, n in zip(whole, lengths)) and int((whole[0][0] != 0).sum()) >= 2
    return xs, mod, whole


def _schedule(seed, lengths, max_chunk, hop):
    """Seeded steps of ``(session, samples, end)``: random subsets (some empty) in shuffled order, sizes 0, 1, hop, max_chunk and random ones;
    even sessions end on their last chunk, odd ones on an item without samples."""
    rng = random.Random(seed)
    n = len(lengths)
    at, done, steps = [0] * n, [False] * n, []
    while not all(done):
        live = [s for s in range(n) if not done[s]]
        chosen = live if not steps else rng.sample(live, rng.randint(0 if rng.random() < 0.15 else 1, len(live)))
        items = []
        for s in chosen:
            left = lengths[s] - at[s]
            c = min(rng.choice([0, 1, hop, max_chunk, rng.randint(0, max_chunk), rng.randint(0, max_chunk)]), left)
            end = c == left and (s % 2 == 0 or c == 0) and bool(steps)
            items.append((s, c, end))
            at[s] += c
            done[s] = end
        rng.shuffle(items)
        steps.append(items)
    return steps


def _chunks(items, xs, at, extra=5):
    """The items' samples as a strided view: one row more than items and `extra` columns more than the longest chunk, NaN wherever no sample
    lies.  None when no item has samples."""
    longest = max((c for _, c, _ in items), default=0)
    if not longest:
        return None
    big = torch.full((len(items) + 1, longest + extra), float("nan"), dtype=torch.float32, device="cuda")
    for i, (s, c, _) in enumerate(items):
        if c:
            big[i, :c] = xs[s][at[s]:at[s] + c]
    return big[:, :longest]


def _run_yin(pool, xs, steps, at=None, got=None, ref=None):
    """Steps on NaN-filled buffers three columns wider than the plan: counts against the host plan and the restatement, exact zeros behind
    every item's frames.  Returns per session the list of (f0, ap) pieces."""
    n = len(xs)
    at = [0] * n if at is None else at
    got = [[] for _ in range(n)] if got is None else got
    for items in steps:
        plan = pool.counters.plan(items)
        if ref is not None:
            assert ref.step(items) == plan, items
        out = torch.full((2, len(items), max(plan, default=0) + 3), float("nan"), device="cuda")
        f0, ap, emit = pool.step_padded(items, _chunks(items, xs, at), out)
        assert emit == plan and f0.data_ptr() == out.data_ptr()
        assert bool(torch.isfinite(out).all()), items                                     # every column was written, no NaN was read
        for i, ((s, c, _), k) in enumerate(zip(items, emit)):
            assert not _bits(out[:, i, k:]).any(), (items, i)                             # +0.0 behind the frames
            at[s] += c
            got[s].append((f0[i, :k].clone(), ap[i, :k].clone()))
            assert (pool.received(s), pool.emitted(s)) == (at[s], pool.counters.emitted[s])
    return got


def _cat(pieces, j):
    return _bits(torch.cat([p[j] for p in pieces])) if pieces else np.zeros(0, np.int32)


@pytest.mark.parametrize("i", [0, 1, -1])
def test_tracker_sessions_equal_each_utterance_alone_and_a_stream_fed_the_same_chunks(i):
    sr, W, hop, fmin, fmax, L = _cfg(i)
    xs, mod, whole = _case(i)
    lengths = tuple(int(x.shape[0]) for x in xs)
    max_chunk = 3 * hop + 1
    steps = _schedule(W + hop, lengths, max_chunk, hop)
    flat = [it for items in steps for it in items]
    assert any(c == 0 and not f for _, c, f in flat) and any(c == 1 for _, c, _ in flat) and any(c == max_chunk for _, c, _ in flat)
    assert any([s for s, _, _ in items] != sorted(s for s, _, _ in items) for items in steps)           # item order is not slot order
    assert len({t for t, items in enumerate(steps) for _, _, f in items if f}) > 1                      # the sessions end at different steps
    with mod.pool(S, max_chunk) as pool:
        assert pool.max_frames == pool.counters.max_frames == pref.yin_max_frames(max_chunk, W, hop)
        got = _run_yin(pool, xs, steps, ref=pref.yin_slots(S, max_chunk, W, hop))
        for s in range(S):
            assert (pool.received(s), pool.emitted(s), pool.pending(s)) == (lengths[s], lengths[s] // hop, pool.counters.pending(s))
    for s in range(S):
        assert np.array_equal(_cat(got[s], 0), whole[s][0]) and np.array_equal(_cat(got[s], 1), whole[s][1]), s
    # the same chunks through a lockstep stream of one row: the same bits, piece by piece
    for s in range(S):
        at, k = 0, 0
        with mod.stream(1, max_chunk) as st:
            for items in steps:
                for a, c, end in items:
                    if a != s:
                        continue
                    f0, ap = st.push(xs[s][None, at:at + c])
                    if end:
                        f1, a1 = st.flush()
                        f0, ap = torch.cat([f0, f1], dim=1), torch.cat([ap, a1], dim=1)
                    at += c
                    assert np.array_equal(_bits(f0[0]), _bits(got[s][k][0])) and np.array_equal(_bits(ap[0]), _bits(got[s][k][1])), (s, k)
                    k += 1


def test_the_carry_of_slots_a_step_does_not_touch_survives():
    sr, W, hop, fmin, fmax, L = _cfg(0)
    xs, mod, whole = _case(0)
    with mod.pool(S, 700) as pool:
        got = _run_yin(pool, xs, [[(0, 700, False), (3, 650, False)]])
        # sessions 1 and 2 step four times (their bits flip back and forth, session 2 ends); 0 and 3 are not named
        others = [[(2, 100, False), (1, 300, False)], [(1, 1, False)], [(1, 699, False), (2, 2 * hop + 3 - 100, True)], [(1, 250, False)]]
        at = [700, 0, 0, 650]
        _run_yin(pool, xs, others, at, got)
        rest = [[(3, 700, False), (0, 600, False)], [(0, 700, False)], [(0, 700, False), (3, xs[3].shape[0] - 1350, True)],
                [(0, L - 2700, True), (1, 700, False)], [(1, L - 517 - 1950, True)]]
        _run_yin(pool, xs, rest, at, got)
    for s in range(S):
        assert np.array_equal(_cat(got[s], 0), whole[s][0]) and np.array_equal(_cat(got[s], 1), whole[s][1]), s


def test_tracker_edge_cases():
    sr, W, hop, fmin, fmax, L = _cfg(0)
    xs, mod, whole = _case(0)
    short = xs[2]                                             # 2 hop + 3 samples: both frames wait for the flush
    with mod.pool(3, 4096) as pool:
        # a flush at N' = 0 and an item that emits no frame: rows of exact zeros; aperiodicity not stored when not asked for
        out = torch.full((1, 2, 3), float("nan"), device="cuda")
        items = [(0, 0, True), (1, int(short.shape[0]), False)]
        f0, ap, emit = pool.step_padded(items, _chunks(items, [None, short], [0, 0]), out, aperiodicity=False)
        assert emit == [0, 0] and ap is None and not _bits(out).any()
        assert pool.counters.flushed[0] and pool.received(0) == 0 and pool.pending(1) == short.shape[0]
        # a flush with no samples: both frames come from the carry alone
        f0, ap, emit = pool.step_padded([(1, 0, True)], None)
        assert emit == [2] and np.array_equal(_bits(f0[0]), whole[2][0]) and np.array_equal(_bits(ap[0]), whole[2][1])
        # a reset slot reused while its carry holds the first utterance: 1e3 everywhere, then utterance 3
        loud = torch.full((8192,), 1e3, device="cuda")
        _run_yin(pool, [None, None, loud], [[(2, 4096, False)], [(2, 4096, False)], [(2, 0, True)]])
        pool.reset(2)
        assert pool.received(2) == pool.emitted(2) == pool.pending(2) == 0
        n = int(xs[3].shape[0])
        got = _run_yin(pool, [None, None, xs[3]], [[(2, 3, False)], [(2, 1000, False)], [(2, n - 1003, True)]])
        assert np.array_equal(_cat(got[2], 0), whole[3][0]) and np.array_equal(_cat(got[2], 1), whole[3][1])
        with pytest.raises(FishVocError, match=r"session 7 lies outside \[0, 3\)"):
            pool.reset(7)
    with pytest.raises(FishVocError):                         # closed
        pool.step([(1, None, False)])


def test_thirty_four_sessions_in_one_step_equal_the_same_sessions_stepped_32_and_2():
    sr, W, hop, fmin, fmax, L = _cfg(0)
    xs3, mod, whole = _case(0)
    n = 1200
    base = xs3[0].cpu().numpy()
    xs = [torch.from_numpy(np.roll(base, 53 * s)[:n].copy()).cuda() for s in range(34)]
    order = list(range(33, -1, -1))
    steps = [[(s, 700, False) for s in order], [(s, 500, s % 3 == 0) for s in order], [(s, 0, True) for s in order if s % 3]]
    with mod.pool(34, 700) as one, mod.pool(34, 700) as two:
        a = _run_yin(one, xs, steps)
        b = _run_yin(two, xs, [part for items in steps for part in (items[:32], items[32:])])
    alone = mod(torch.stack(xs[:2]))
    for s in range(34):
        assert np.array_equal(_cat(a[s], 0), _cat(b[s], 0)) and np.array_equal(_cat(a[s], 1), _cat(b[s], 1)), s
        assert _cat(a[s], 0).shape == (n // hop,)
    for s in range(2):
        assert np.array_equal(_cat(a[s], 0), _bits(alone[0][s])) and np.array_equal(_cat(a[s], 1), _bits(alone[1][s]))
    assert not np.array_equal(_cat(a[33], 0), _cat(a[0], 0))                              # the sessions differ


def test_refused_tracker_steps_move_nothing():
    sr, W, hop, fmin, fmax, L = _cfg(0)
    xs, mod, whole = _case(0)
    L_ = _lib.lib()
    with mod.pool(3, 700) as pool:
        got = _run_yin(pool, xs, [[(0, 700, False), (1, 500, False), (2, 2 * hop + 3, False)], [(2, 0, True)]])
        at = [700, 500, 2 * hop + 3]
        state = lambda: [(pool.received(s), pool.emitted(s), pool.pending(s)) for s in range(3)]      # noqa: E731
        before, py_before = state(), (list(pool.counters.received), list(pool.counters.emitted), list(pool.counters.flushed))
        x = xs[0][700:1400]
        with pytest.raises(ValueError, match=r"duplicate session 0 \(item 1\)"):
            pool.step([(0, x, False), (0, x, False)])
        with pytest.raises(ValueError, match=r"item 1 \(session 1\) has 701 samples"):
            pool.step([(0, x, False), (1, xs[1][:701], False)])
        with pytest.raises(PoolStateError, match=r"session 2 was flushed \(item 1\)"):
            pool.step([(0, x, False), (2, None, False)])
        # the library's own refusals, below the Python plan
        items = (_lib.WavPoolItem * 2)(_lib.WavPoolItem(0, 700, 0), _lib.WavPoolItem(1, 100, 0))
        k = pool.counters.plan([(0, 700, False), (1, 100, False)])
        assert max(k) >= 2
        chunks = torch.zeros((2, 700), device="cuda")
        chunks[0], chunks[1, :100] = x, xs[1][500:600]
        out = torch.empty((2, 2, max(k)), device="cuda")
        emit = (ctypes.c_int64 * 2)()
        for args, pattern in (
                ((chunks.data_ptr(), 700, out[0].data_ptr(), max(k) - 1, max(k) - 1),
                 "out_cols = %d, but item %d (session %d) emits %d frames" % (max(k) - 1, k.index(max(k)), k.index(max(k)), max(k))),
                ((chunks.data_ptr(), 700, out[0].data_ptr(), max(k) - 1, max(k)), "out_stride = %d is shorter" % (max(k) - 1)),
                ((chunks.data_ptr(), 700, None, max(k), max(k)), "null output although item"),
                ((None, 700, out[0].data_ptr(), max(k), max(k)), "null chunk buffer although item 0 (session 0) has 700 samples"),
                ((chunks.data_ptr(), 699, out[0].data_ptr(), max(k), max(k)), "row stride 699 is shorter"),
        ):
            st = L_.fv_yinpool_step(pool._h, items, 2, args[0], args[1], args[2], out[1].data_ptr(), args[3], args[4], emit, None)
            msg = L_.fv_last_error().decode()
            assert st == _lib.FV_ERR_INVALID and msg.startswith("fv_yinpool_step:") and pattern in msg, (st, msg)
            assert list(emit) == [0, 0]
        done = (_lib.WavPoolItem * 1)(_lib.WavPoolItem(2, 0, 0))
        assert L_.fv_yinpool_step(pool._h, done, 1, None, 0, None, None, 0, 0, emit, None) == _lib.FV_ERR_STATE
        assert "session 2 was flushed (item 0); fv_yinpool_reset" in L_.fv_last_error().decode()
        assert state() == before and (pool.counters.received, pool.counters.emitted, pool.counters.flushed) == py_before
        # ... and the run goes on to its end, bit-identical
        _run_yin(pool, xs, [[(1, 700, False), (0, 700, False)], [(0, 700, False), (1, 700, False)], [(0, 700, False), (1, L - 517 - 1900, True)],
                            [(0, L - 2800, True)]], at, got)
    for s in range(3):
        assert np.array_equal(_cat(got[s], 0), whole[s][0]) and np.array_equal(_cat(got[s], 1), whole[s][1]), s


# ---- the oscillator pool ----
OSC_SR, OSC_HOP = 8000, 128                                   # kTmplChunk = 2048 samples = 16 frames


@functools.lru_cache(maxsize=None)
def _tracks():
    """Four F0 tracks of 90, 61, 1 and 40 frames, 80 - 1900 Hz, with unvoiced frames written as 0, negative and NaN; track 0 starts and ends
    unvoiced, track 1 voiced."""
    rng = np.random.default_rng(11)
    out = []
    for T in (90, 61, 1, 40):
        f0 = rng.uniform(80.0, 1900.0, T).astype(np.float32)
        for at in rng.integers(2, max(T - 6, 3), 5):
            f0[at:at + int(rng.integers(1, 5))] = 0.0
        out.append(f0)
    out[0][[0, 1, -1]] = 0.0
    out[0][17], out[0][40] = np.nan, -5.0
    out[1][0], out[1][-1], out[1][30] = 150.0, 1700.0, 2.0 * OSC_SR
    out[2][0] = 440.0
    return tuple(torch.from_numpy(f).cuda() for f in out)


def _run_osc(pool, xs, steps, at=None, got=None, ref=None):
    hop, n = pool.hop_length, len(xs)
    at = [0] * n if at is None else at
    got = [[] for _ in range(n)] if got is None else got
    for items in steps:
        plan = pool.counters.plan(items)
        if ref is not None:
            assert ref.step(items) == plan, items
        out = torch.full((len(items), max(plan, default=0) * hop + 5), float("nan"), device="cuda")
        res, emit = pool.step_padded(items, _chunks(items, xs, at), out)
        assert emit == plan and res is out and bool(torch.isfinite(out).all()), items
        for i, ((s, c, _), k) in enumerate(zip(items, emit)):
            assert not _bits(out[i, k * hop:]).any(), (items, i)
            at[s] += c
            got[s].append(out[i, :k * hop].clone())
            assert (pool.received(s), pool.emitted(s), pool.pending(s)) == (at[s], pool.counters.emitted[s], at[s] - pool.counters.emitted[s])
    return got


@pytest.mark.parametrize("kind", ["sine", "sawtooth"])
def test_oscillator_sessions_equal_each_track_alone(kind):
    xs = _tracks()
    osc = f0mod.PitchTemplate(OSC_SR, OSC_HOP, kind=kind, amplitude=0.5)
    whole = [_bits(osc(x[None])[0, 0]) for x in xs]
    assert float(osc(xs[0][None]).abs().max()) > 0.49
    steps = [
        [(2, 1, False), (0, 1, False)],                        # a first push of one frame: nothing comes out, the phase starts at 0
        [(1, 40, False)],                                      # 39 frames: three chunks of 2048 samples
        [(0, 3, False), (1, 0, False)],                        # inside one chunk; an item without frames
        [(2, 0, True), (1, 2, False), (0, 40, False)],         # a flush that brings no new frame and emits the pending one
        [(0, 40, False)],
        [(1, 19, True), (0, 6, False)],
        [(0, 0, True)],
    ]
    with osc.pool(3, 40) as pool:
        assert pool.max_frames == pool.counters.max_frames == 41
        got = _run_osc(pool, xs, steps, ref=pref.osc_slots(3, 40))
        assert [len(g[0]) for g in got[:3]] == [0, 39 * OSC_HOP, 0] and len(got[2][1]) == OSC_HOP
        for s in range(3):
            assert np.array_equal(_bits(torch.cat(got[s])), whole[s]), s
        # a reset followed by a second utterance in the same slots, whatever the phases and carried frames hold; one push that also ends
        with pytest.raises(PoolStateError, match=r"session 1 was flushed"):
            pool.step([(1, xs[1][:2], False)])
        for s in (0, 1, 2):
            pool.reset(s)
        again = _run_osc(pool, [xs[3], xs[0], xs[1]], [[(1, 40, False), (0, 40, True)], [(2, 1, False), (1, 40, False)], [(2, 40, False)],
                                                       [(1, 10, True), (2, 20, True)]])
        for s, t in enumerate((3, 0, 1)):
            assert np.array_equal(_bits(torch.cat(again[s])), whole[t]), s
    unvoiced = np.repeat(~((xs[0].cpu().numpy() > 0) & (xs[0].cpu().numpy() < OSC_SR)), OSC_HOP)
    assert unvoiced.sum() >= 5 * OSC_HOP and not _bits(torch.cat(got[0]))[unvoiced].any()            # +0.0 in unvoiced frames


def test_thirty_four_oscillator_sessions_cross_two_launch_blocks():
    base = _tracks()[0].cpu().numpy()[:64]
    xs = [torch.from_numpy(np.roll(base, 5 * s).copy()).cuda() for s in range(34)]
    osc = f0mod.PitchTemplate(OSC_SR, OSC_HOP, amplitude=0.5)
    order = list(range(33, -1, -1))
    steps = [[(s, 30, False) for s in order], [(s, 34, s % 2 == 0) for s in order], [(s, 0, True) for s in order if s % 2]]
    with osc.pool(34, 34) as one, osc.pool(34, 34) as two:
        a = _run_osc(one, xs, steps)
        b = _run_osc(two, xs, [part for items in steps for part in (items[:32], items[32:])])
    whole = osc(torch.stack(xs))[:, 0]
    for s in range(34):
        assert np.array_equal(_bits(torch.cat(a[s])), _bits(whole[s])) and np.array_equal(_bits(torch.cat(b[s])), _bits(whole[s])), s
    assert not np.array_equal(_bits(whole[33]), _bits(whole[0]))


def test_refused_oscillator_steps_move_nothing():
    xs = _tracks()
    osc = f0mod.PitchTemplate(OSC_SR, OSC_HOP)
    L_ = _lib.lib()
    with osc.pool(2, 50) as pool:
        got = _run_osc(pool, xs, [[(0, 50, False), (1, 30, False)]])
        before = [(pool.received(s), pool.emitted(s)) for s in range(2)]
        with pytest.raises(ValueError, match=r"duplicate session 1 \(item 1\)"):
            pool.step([(1, xs[1][30:31], False), (1, xs[1][30:31], False)])
        with pytest.raises(ValueError, match=r"item 0 \(session 0\) has 51 samples"):
            pool.step([(0, torch.zeros(51, device="cuda"), False)])
        items = (_lib.WavPoolItem * 1)(_lib.WavPoolItem(0, 40, 0))
        out = torch.empty((1, 40 * OSC_HOP), device="cuda")
        emit = (ctypes.c_int64 * 1)()
        st = L_.fv_oscpool_step(pool._h, items, 1, xs[0][50:].data_ptr(), 40, out.data_ptr(), 40 * OSC_HOP, 40 * OSC_HOP - 1, emit, None)
        assert st == _lib.FV_ERR_INVALID and "out_cols = %d, but item 0 (session 0) emits %d samples" % (40 * OSC_HOP - 1, 40 * OSC_HOP) \
            in L_.fv_last_error().decode()
        assert [(pool.received(s), pool.emitted(s)) for s in range(2)] == before and emit[0] == 0
        _run_osc(pool, xs, [[(1, 31, True), (0, 40, True)]], [50, 30], got)
    for s in range(2):
        assert np.array_equal(_bits(torch.cat(got[s])), _bits(osc(xs[s][None])[0, 0])), s


# ---- the two chained ----
def test_template_pool_equals_template_from_audio_per_session():
    sr, W, hop, fmin, fmax, L = _cfg(0)
    xs, _, _ = _case(0)
    lengths = tuple(int(x.shape[0]) for x in xs)
    kw = dict(frame_length=W, fmin=fmin, fmax=fmax, kind="sawtooth", amplitude=0.7)
    whole = [f0mod.template_from_audio(x[None], sr, hop, **kw)[0] for x in xs]
    assert float(whole[0].abs().max()) > 0.6 and all(tuple(w.shape) == (1, (n // hop) * hop) for w, n in zip(whole, lengths))
    steps = _schedule(5, lengths, 500, hop)
    at, got = [0] * S, [[] for _ in range(S)]
    with f0mod.TemplatePool(sr, hop, S, 500, **kw) as pool:
        assert pool.max_frames == pool.tracker.max_frames + 1
        for items in steps:
            frames, plan = pool.counters.plan(items)
            ys = pool.step([(s, xs[s][at[s]:at[s] + c] if c else None, end) for s, c, end in items])
            for (s, c, _), y, k in zip(items, ys, plan):
                assert tuple(y.shape) == (1, k * hop)
                at[s] += c
                got[s].append(y.clone())
                assert pool.received(s) == at[s] and pool.emitted(s) == pool.counters.template.emitted[s]
        assert all(pool.emitted(s) == lengths[s] // hop and pool.pending(s) == 0 for s in range(S))
    for s in range(S):
        assert np.array_equal(_bits(torch.cat(got[s], dim=-1)), _bits(whole[s])), s


# ---- the chain: [ResamplePool ->] WavPool + TemplatePool -> SessionPool, on the tiny use_template HiFiGAN of test_gpu_f0_stream.py ----
TINY_GEN = dict(hop_length=64, num_mels=20, upsample_initial_channel=32, upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4],
                resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]], pre_conv_kernel_size=7, post_conv_kernel_size=7,
                use_template=True)
CHAIN_SR, CHAIN_HOP = 16000, 64
TRACKER = dict(frame_length=1024, fmin=60.0, fmax=800.0)
CHAIN_TOL = 2e-5      # of max(1, peak): the generator pool's own bar (tests/test_gpu_pool.py, tests/test_gpu_stream.py)


@functools.lru_cache(maxsize=None)
def _chain_parts():
    from vocoder_amd.data.transforms import LogMelSpectrogram
    from vocoder_amd.modules.generators import HiFiGANGenerator
    gen = HiFiGANGenerator(**TINY_GEN).eval()
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(TINY_GEN, 5).items()})
    front = LogMelSpectrogram(sample_rate=CHAIN_SR, n_fft=256, win_length=256, hop_length=CHAIN_HOP, n_mels=20, f_min=0, f_max=CHAIN_SR // 2)
    return front.eval().cuda(), gen.cuda()


@pytest.mark.parametrize("client", [CHAIN_SR, 24000])
def test_wav_session_pool_with_a_template_equals_the_whole_file_forward(client, monkeypatch):
    from vocoder_amd import inference
    from vocoder_amd import resample as rs
    front, gen = _chain_parts()
    to_model = None if client == CHAIN_SR else rs.Resample(client, CHAIN_SR)
    lengths = (9617, 4000, 6300) if to_model is None else (9617 * 3 // 2, 6000, 9450)          # client samples
    xs = [torch.from_numpy(fref.glide(n, client, seed=3 + s)[0].astype(np.float32)).cuda() for s, n in enumerate(lengths)]
    chunk = 1400
    steps = _schedule(13 + client, lengths, chunk, CHAIN_HOP)
    with inference.WavSessionPool(front, gen, 3, chunk, input_resample=to_model, template=dict(TRACKER)) as chain:
        tp = chain.template_pool
        assert tp is not None and tp.max_chunk_samples == chain.wav_pool.max_chunk_samples
        assert chain.gen_pool.max_chunk_frames == max(chain.wav_pool.max_frames, tp.max_frames)
        # a mismatching frame count at the end is refused before anything moves: the template branch plans one frame short
        at, got = [0] * 3, [[] for _ in xs]

        def feed(items):
            ys = chain.step([(s, xs[s][at[s]:at[s] + c] if c else None, end) for s, c, end in items])
            for (s, c, _), y in zip(items, ys):
                at[s] += c
                got[s].append(y.clone())

        real = tp.counters.plan
        state = lambda: [(chain.wav_pool.received_samples(s), tp.received(s), chain.gen_pool.received_frames(s),      # noqa: E731
                          None if chain.in_pool is None else chain.in_pool.received(s)) for s in range(3)]
        feed(steps[0])
        before = state()
        monkeypatch.setattr(tp.counters, "plan", lambda items: (real(items)[0], [k - 1 for k in real(items)[1]]))
        with pytest.raises(ValueError, match=r"session 1 \(item 0\) ends with \d+ frames from the log-mel front-end and \d+ from the pitch"):
            chain.step([(1, xs[1][at[1]:at[1] + 700], True)])
        monkeypatch.undo()
        assert state() == before and not chain.wav_pool.counters.flushed[1] and not tp.counters.tracker.flushed[1]
        for items in steps[1:]:
            feed(items)
        rest = [torch.cat(g, dim=-1) for g in got]
    with torch.no_grad():
        for s in range(3):
            y = xs[s][None] if to_model is None else to_model(xs[s][None])
            mel = front(y)
            template = f0mod.template_from_audio(y, CHAIN_SR, CHAIN_HOP, **TRACKER)
            assert mel.shape[-1] * CHAIN_HOP == template.shape[-1] and float(template.abs().max()) > 0.9
            whole = gen(mel, template)[0]
            peak = float(whole.abs().max())
            d = float((rest[s] - whole).abs().max()) if rest[s].shape == whole.shape else float("inf")
            print(f"session {s} ({lengths[s]} client samples, {mel.shape[-1]} frames): chain vs the whole file {d:.3e}, "
                  f"bar {CHAIN_TOL * max(1.0, peak):.3e}, peak {peak:.3f}")
            assert tuple(rest[s].shape) == tuple(whole.shape) == (1, mel.shape[-1] * CHAIN_HOP)
            assert d <= CHAIN_TOL * max(1.0, peak), (s, d, peak)
            assert float((whole - gen(mel, torch.zeros_like(template))[0]).abs().max()) > 1e-3      # the template matters
