"""GPU: the pitch-shift pool (fv_pvpool_* in vocoder_amd/csrc/pitch_shift.hip) through ``vocoder_amd.pitch_shift.PitchShiftPool`` and
``inference.WavSessionPool(pitch_shift=...)``.

Every comparison of the pool is on bits, against ``PitchShift(batch_invariant=True).forward`` of each session's whole utterance alone: the two
DFT convs are fixed-order sums per column, the phase is a wrapping integer sum, the overlap-add sums a sample's frames in one order and the
resample pool is bit-identical to its rows, so a session has nothing to be approximately equal about, whatever stands beside it in a step.
Every chunk buffer holds NaN past each item's samples and has a stride longer than the longest chunk; the output and the workspace are filled
with NaN before every step, so a slot that is neither written nor provably unread shows up as a NaN or as one changed bit.  After every step
each session's E is the counting rule's (pitch_shift_pool_reference).  The chain's bar is the generator pool's own, 2e-5 * max(1, peak)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pitch_shift_pool_reference as pool_ref
import pitch_shift_reference as pref
from vocoder_amd import _lib
from vocoder_amd import pitch_shift as ps

pytestmark = pytest.mark.gpu

SR = 44100
STEPS = (3, -4, 12, -12, 0.5)
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 300, 1000)
NAN = float("nan")


def _bits(a) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _shifter(n_steps, n_fft):
    mod = ps.PitchShift(SR, n_steps, n_fft=n_fft, batch_invariant=True)
    return mod, pool_ref.Rule(SR, n_steps, mod.n_fft, mod.hop_length)


@functools.lru_cache(maxsize=None)
def _utterance(n_steps, n_fft, L, seed):
    """One utterance on the device and the whole-row GPU result of it alone (computed once, never changed)."""
    mod, _ = _shifter(n_steps, n_fft)
    x = torch.from_numpy(pref.broadband(L, SR, seed).astype(np.float32)).cuda() if L else torch.zeros(0, device="cuda")
    whole = mod(x[None])[0] if L else x
    assert tuple(whole.shape) == (L,) and not bool(torch.isnan(whole).any())
    return x, whole


def _step(pool, items, xs, at, extra_cols=3):
    """One step on NaN-filled buffers: items (session, c, flush) take xs[session][at[session]:+c].  Returns each item's outputs (clones)."""
    count = len(items)
    longest = max((c for _, c, _ in items), default=0)
    chunks = torch.full((max(count, 1), longest + 5), NAN, device="cuda")
    for i, (s, c, _) in enumerate(items):
        chunks[i, :c] = xs[s][at[s]:at[s] + c]
    plan = pool.counters.plan(items)
    out = torch.full((count, max(plan, default=0) + extra_cols), NAN, device="cuda")
    pool._ws.fill_(0xFF)                                            # every float of the workspace a NaN
    got, emit = pool.step_padded(items, chunks, out)
    assert emit == plan and got is out
    res = []
    for i, ((s, c, _), k) in enumerate(zip(items, emit)):
        at[s] += c
        assert not bool(torch.isnan(out[i, :k]).any()), (items[i], k)
        assert bool((_bits(out[i, k:]) == 0).all()), (items[i], k)  # exact zeros behind the outputs, every column written
        res.append(out[i, :k].clone())
    return res


def _run(pool, rule, steps, xs, wholes, mod=None, twin_stream=True):
    """Runs a schedule of steps; checks E against the counting rule after every step, every finished session against its utterance alone
    and against a PitchShiftStream(batch=1) fed the same chunks."""
    S = pool.sessions
    ref = pool_ref.Sessions(rule, S)
    at, got, fed = [0] * S, [[] for _ in range(S)], [[] for _ in range(S)]
    for items in steps:
        ys = _step(pool, items, xs, at)
        counted = ref.step(items)
        for (s, c, flush), y, k in zip(items, ys, counted):
            assert y.shape[0] == k, (s, c, flush, y.shape[0], k)
            got[s].append(y)
            fed[s].append(c)
        for s in range(S):
            assert (pool.received(s), pool.emitted(s), pool.pending(s)) == (ref.N[s], ref.E[s], ref.N[s] - ref.E[s]), s
    for s in range(S):
        if not ref.flushed[s]:
            continue
        y = torch.cat(got[s]) if got[s] else torch.zeros(0, device="cuda")
        assert np.array_equal(_bits(y), _bits(wholes[s])), (s, int(wholes[s].shape[0]), int((_bits(y) != _bits(wholes[s])).sum()))
        if twin_stream and mod is not None and wholes[s].shape[0]:
            with mod.stream(1, pool.max_chunk) as st:
                a, parts = 0, []
                for c in fed[s]:
                    parts.append(st.push(xs[s][None, a:a + c].contiguous()))
                    a += c
                parts.append(st.flush())
            assert np.array_equal(_bits(torch.cat(parts, dim=1)[0]), _bits(y)), s
    return got


def _random_schedule(rng, lengths, max_chunk, hop):
    """Seeded steps over subsets of the unfinished sessions; chunk sizes include 0 and 1; an utterance ends with its last samples or with a
    later flush-only item."""
    left, done, steps = list(lengths), [False] * len(lengths), []
    while not all(done):
        items = []
        for s in rng.permutation(len(lengths)):
            s = int(s)
            if done[s] or rng.random() < 0.4:
                continue
            c = min(left[s], int(rng.choice([0, 1, hop, int(rng.integers(0, max_chunk + 1)), max_chunk])))
            flush = c == left[s] and rng.random() < 0.6
            left[s] -= c
            done[s] = flush
            items.append((s, c, flush))
        steps.append(items)
    return steps


@pytest.mark.parametrize("n_steps", STEPS)
def test_sessions_of_every_length_under_a_random_schedule_equal_their_utterances_alone(n_steps):
    mod, rule = _shifter(n_steps, 64)
    assert mod.hop_length == 16
    pairs = [_utterance(n_steps, 64, L, 100 + i) for i, L in enumerate(LENGTHS)]
    xs, wholes = [p[0] for p in pairs], [p[1] for p in pairs]
    max_chunk = 3 * 16 + 5
    steps = _random_schedule(np.random.default_rng(abs(int(n_steps * 10)) + 77), LENGTHS, max_chunk, 16)
    assert any(len(it) > 1 for it in steps) and any(c == 0 and f for it in steps for _, c, f in it)
    with mod.pool(len(LENGTHS), max_chunk) as pool:
        assert pool.max_outputs == pool.counters.max_outputs
        _run(pool, rule, steps, xs, wholes, mod)


@pytest.mark.parametrize("n_steps", [3, -4])
def test_default_frame_three_sessions(n_steps):
    mod, rule = _shifter(n_steps, 2048)
    assert (mod.n_fft, mod.hop_length) == (2048, 512)
    lengths = (20000, 9000, 4097)
    pairs = [_utterance(n_steps, 2048, L, 7 + i) for i, L in enumerate(lengths)]
    xs, wholes = [p[0] for p in pairs], [p[1] for p in pairs]
    steps = _random_schedule(np.random.default_rng(5), lengths, 4096, 512)
    with mod.pool(3, 4096) as pool:
        _run(pool, rule, steps, xs, wholes, mod, twin_stream=n_steps == 3)


@pytest.mark.parametrize("short_first", [True, False])
def test_a_short_flushing_item_beside_a_long_pushing_item(short_first):
    """The step's STFT conv is padded to the long item's dA; the short item's column dA_short reads real polyphase slots and must be written
    as zero: its flush reads it as the row's column T."""
    mod, rule = _shifter(3, 64)
    (xa, wa), (xb, wb) = _utterance(3, 64, 45, 31), _utterance(3, 64, 500, 32)
    A0 = mod.stream_ready(40)[0]
    dA_short, dA_long = mod.lengths(45)[0] - A0, mod.stream_ready(160)[0]
    assert 0 < dA_short < dA_long
    a, b = (0, 5, True), (1, 160, False)
    steps = [[(0, 40, False)], [a, b] if short_first else [b, a], [(1, 160, False)], [(1, 180, True)]]
    with mod.pool(2, 200) as pool:
        _run(pool, rule, steps, [xa, xb], [wa, wb], mod)


def test_items_in_different_phases_in_one_step():
    mod, rule = _shifter(3, 64)
    lengths = (200, 232, 248, 900)
    pairs = [_utterance(3, 64, L, 50 + i) for i, L in enumerate(lengths)]
    xs, wholes = [p[0] for p in pairs], [p[1] for p in pairs]
    r = mod.stream_ready
    assert r(10)[0] == 0                                                            # no frame
    assert r(32)[0] > 0 and r(32)[1] == 0                                           # frames, no stretched frame
    assert r(48)[1] > 0 and r(48)[2] == 0                                           # stretched frames, no stretched sample
    assert mod.stream_emitted(650) > mod.stream_emitted(600)                        # emitting
    steps = [[(3, 200, False)], [(3, 200, False)], [(3, 200, False)],
             [(0, 10, False), (1, 32, False), (2, 48, False), (3, 50, False)],
             [(0, 190, True), (1, 200, True), (2, 200, True), (3, 200, False)], [(3, 50, True)]]
    with mod.pool(4, 200) as pool:
        got = _run(pool, rule, steps, xs, wholes, mod)
    assert [int(y.shape[0]) for y in (got[0][0], got[1][0], got[2][0])] == [0, 0, 0] and got[3][3].shape[0] > 0


def test_a_slot_untouched_for_several_steps_then_resumed():
    """Sample, polar and frame carries each have a bit per slot: the idle slot's halves stay where its own bits say while the others flip."""
    mod, rule = _shifter(-4, 64)
    lengths = (700, 640, 655)
    pairs = [_utterance(-4, 64, L, 60 + i) for i, L in enumerate(lengths)]
    xs, wholes = [p[0] for p in pairs], [p[1] for p in pairs]
    steps = [[(0, 100, False), (1, 90, False)], [(0, 100, False), (2, 33, False)]]
    steps += [[(1, 50, False), (2, 37, False)], [(1, 49, False)], [(2, 100, False), (1, 51, False)], [(1, 100, False), (2, 85, False)],
              [(2, 100, False)]]                                                     # session 0 idle: an odd and an even number of flips beside it
    steps += [[(0, 100, False), (1, 100, False)], [(0, 100, False), (2, 100, False)], [(0, 300, True), (1, 200, True), (2, 200, True)]]
    with mod.pool(3, 300) as pool:
        _run(pool, rule, steps, xs, wholes, mod)


def test_34_sessions_in_one_step_equal_the_same_sessions_stepped_32_and_2():
    mod, rule = _shifter(3, 64)
    S, L = 34, 260
    pairs = [_utterance(3, 64, L, 200 + s) for s in range(S)]
    xs, wholes = [p[0] for p in pairs], [p[1] for p in pairs]
    sizes = [50, 33, 64, 1, 60, 52]
    with mod.pool(S, 64) as one, mod.pool(S, 64) as two:
        at1, at2, got1, got2 = [0] * S, [0] * S, [[] for _ in range(S)], [[] for _ in range(S)]
        for j, c in enumerate(sizes):
            items = [(s, c, j == len(sizes) - 1) for s in range(S)]
            for s, y in enumerate(_step(one, items, xs, at1)):
                got1[s].append(y)
            for part in (items[:32], items[32:]):
                for (s, _, _), y in zip(part, _step(two, part, xs, at2)):
                    got2[s].append(y)
    for s in range(S):
        y1, y2 = torch.cat(got1[s]), torch.cat(got2[s])
        assert np.array_equal(_bits(y1), _bits(y2)) and np.array_equal(_bits(y1), _bits(wholes[s])), s


def test_edges_flush_only_empty_short_reset_and_identity():
    """The utterance shorter than n_fft / 2 emits nothing before its end and its N samples with it — frame 0 holds them, so they are the
    whole row's bits, zeros only where the whole row has zeros; the utterance whose stretch is empty (Ls = 0) gives zeros."""
    mod, rule = _shifter(3, 64)
    (xa, wa), (xb, wb), (xc, wc) = _utterance(3, 64, 300, 71), _utterance(3, 64, 20, 72), _utterance(3, 64, 0, 73)
    with mod.pool(3, 300) as pool:
        # a flush-only item ends session 0; session 2 is flushed at N = 0; session 1 is shorter than n_fft / 2
        got = _run(pool, rule, [[(0, 300, False), (1, 20, False), (2, 0, True)], [(0, 0, True), (1, 0, True)]], [xa, xb, xc], [wa, wb, wc], mod)
        assert got[1][0].shape[0] == 0 and got[1][1].shape[0] == 20 and got[2][0].shape[0] == 0
        # reset and reuse: a loud utterance fills every carry of slot 0; the next one has the bits of a fresh slot
        pool.reset(0)
        loud = torch.full((300,), 1e3, device="cuda")
        at = [0]
        _step(pool, [(0, 300, False)], [loud], at)
        _step(pool, [(0, 0, True)], [loud], at)
        for s in (0, 1, 2):
            pool.reset(s)
        _run(pool, rule, [[(0, 150, False)], [(0, 150, True), (1, 20, True)]], [xa, xb, xc], [wa, wb, wc], mod)
    low, lrule = _shifter(-12, 64)                               # Ls = 0: L = 1 an octave down, one zero at the flush
    assert low.lengths(1)[2] == 0
    one = torch.full((1,), 0.5, device="cuda")
    with low.pool(2, 8) as pool:
        got = _run(pool, lrule, [[(1, 1, True)]], [one, one], [low(one[None])[0]] * 2, low)
        assert got[1][0].shape[0] == 1 and float(got[1][0][0]) == 0.0
    ident = ps.PitchShift(SR, 0, n_fft=64, batch_invariant=True)  # every item's samples back bit for bit, no carry work
    x, _ = _utterance(3, 64, 300, 71)
    with ident.pool(2, 200) as pool:
        assert pool._need == 0 and pool.max_outputs == 200
        at = [0, 0]
        a = _step(pool, [(0, 200, False), (1, 7, True)], [x, x], at)
        b = _step(pool, [(0, 100, True)], [x, x], at)
        assert np.array_equal(_bits(torch.cat([a[0], b[0]])), _bits(x)) and np.array_equal(_bits(a[1]), _bits(x[:7]))
        assert pool.pending(0) == 0 and pool.emitted(0) == 300


def _raw_step(pool, items, chunks, out, ws_bytes=None):
    """fv_pvpool_step itself, past the Python plan -> (status, message)."""
    L = _lib.lib()
    n = len(items)
    arr = (_lib.WavPoolItem * max(n, 1))(*[_lib.WavPoolItem(int(s), int(c), int(f)) for s, c, f in items])
    got = (ctypes.c_int64 * max(n, 1))()
    st = L.fv_pvpool_step(pool._h, arr, n, chunks.data_ptr(), int(chunks.stride(0)), out.data_ptr(), int(out.stride(0)), int(out.shape[1]), got,
                          pool._ws.data_ptr(), pool._need if ws_bytes is None else ws_bytes, int(torch.cuda.current_stream().cuda_stream))
    return int(st), L.fv_last_error().decode()


def test_refused_steps_change_nothing():
    """Each refusal is followed by a valid step; the pool equals a twin that was never refused, on bits, to the end of both utterances."""
    mod, rule = _shifter(3, 64)
    (xa, wa), (xb, wb) = _utterance(3, 64, 400, 81), _utterance(3, 64, 330, 82)
    xs = [xa, xb, xa]
    with mod.pool(3, 100) as pool, mod.pool(3, 100) as twin:
        at, tat = [0] * 3, [0] * 3
        got, tgot = [[], []], [[], []]

        def both(items):
            for (s, _, _), y, t in zip(items, _step(pool, items, xs, at), _step(twin, items, xs, tat)):
                assert np.array_equal(_bits(y), _bits(t)), items
                if s < 2:
                    got[s].append(y), tgot[s].append(t)

        both([(0, 100, False), (1, 90, False), (2, 10, True)])
        chunks, out = torch.full((3, 120), NAN, device="cuda"), torch.full((3, 150), NAN, device="cuda")
        chunks[:, :101] = 0.25
        state = lambda: [(pool.received(s), pool.emitted(s)) for s in range(3)]      # noqa: E731
        before = state()
        cases = [([(0, 50, False), (1, 50, False), (0, 10, False)], _lib.FV_ERR_INVALID, r"duplicate session 0 (item 2)", None, out),
                 ([(0, 50, False), (2, 0, False)], _lib.FV_ERR_STATE, r"session 2 was flushed (item 1)", None, out),
                 ([(1, 50, False), (0, 101, False)], _lib.FV_ERR_INVALID, r"item 1 (session 0) has 101 samples", None, out),
                 ([(1, 100, False), (0, 100, False)], _lib.FV_ERR_INVALID, r"out_cols = 3, but item", None, out[:, :3]),
                 ([(1, 100, False), (0, 100, False)], _lib.FV_ERR_INVALID, r"workspace too small", pool._need - 256, out)]
        for items, status, text, ws_bytes, o in cases:
            st, msg = _raw_step(pool, items, chunks, o, ws_bytes)
            assert st == status and msg.startswith("fv_pvpool_step:") and text in msg, (items, st, msg)
            assert re_names(msg), msg
            assert state() == before and pool.counters.received == [b[0] for b in before]
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all())                                     # nothing was written
            both([(0, 20, False), (1, 15, False)])                                  # a valid step after every refusal
            before = state()
        with pytest.raises(ValueError, match="duplicate session 1"):                 # the Python plan refuses the same before the library
            pool.step_padded([(1, 1, False), (1, 1, False)], chunks)
        with pytest.raises(_lib.FishVocError, match="out_cols"):                     # ... and hands the library's refusals on
            pool.step_padded([(0, 100, False)], chunks, out[:1, :3].contiguous())
        assert state() == before and pool.counters.received[0] == before[0][0]
        both([(0, 100, False), (1, 100, False)])
        both([(0, 100, False), (1, 65, True)])
        both([(0, 400 - at[0], True)])
    for s, w in ((0, wa), (1, wb)):
        assert np.array_equal(_bits(torch.cat(got[s])), _bits(w)) and np.array_equal(_bits(torch.cat(tgot[s])), _bits(w)), s


def re_names(msg: str) -> bool:
    """Does a refusal name an item and a session?"""
    return "item" in msg and "session" in msg


# ---- the chain: [ResamplePool ->] PitchShiftPool -> WavPool [+ TemplatePool] -> SessionPool, on the synthetic HiFiGAN-V1-44k ----
TRACKER = dict(frame_length=2048, fmin=40.0, fmax=1100.0)


@functools.lru_cache(maxsize=None)
def _chain_parts(use_template):
    from vocoder_amd import synthetic as syn
    from vocoder_amd.data.transforms import LogMelSpectrogram
    from vocoder_amd.modules.generators.hifigan import HiFiGANGenerator
    cfg = dict(syn.HIFIGAN_V1_44K, use_template=use_template)
    gen = HiFiGANGenerator(**cfg).eval()
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(cfg, 3).items()})
    hop = cfg["hop_length"]
    front = LogMelSpectrogram(sample_rate=SR, n_fft=2048, win_length=2048, hop_length=hop, n_mels=80, f_min=0, f_max=SR // 2)
    return front.eval().cuda(), gen.cuda(), hop


@pytest.mark.parametrize("client", [SR, 24000])
@pytest.mark.parametrize("use_template", [False, True])
def test_wav_session_pool_with_a_pitch_shift_matches_the_whole_file_path(use_template, client):
    from vocoder_amd import f0 as f0mod, inference
    from vocoder_amd import resample as rs
    front, gen, hop = _chain_parts(use_template)
    shifter = ps.PitchShift(SR, 3, batch_invariant=True)
    to_model = None if client == SR else rs.Resample(client, SR)
    lengths = (int(0.3 * client), int(0.2 * client) + 17)                                # client samples
    xs = [torch.from_numpy((0.3 * pref.broadband(n, client, seed=1 + s)).astype(np.float32).clip(-1, 1)).cuda() for s, n in enumerate(lengths)]
    chunk = 8 * hop * client // SR
    sizes = ([chunk] * (lengths[0] // chunk) + [lengths[0] % chunk], [chunk // 2 + 3] * (lengths[1] // (chunk // 2 + 3)) + [lengths[1] % (chunk // 2 + 3)])
    template = dict(TRACKER) if use_template else None
    with pytest.raises(ValueError, match=r"pitch_shift has sample_rate = 48000 Hz.*44100 Hz"):     # a shifter at another rate, by name
        inference.WavSessionPool(front, gen, 2, chunk, input_resample=to_model, template=template, pitch_shift=ps.PitchShift(48000, 3))
    got = [[], []]
    with inference.WavSessionPool(front, gen, 2, chunk, input_resample=to_model, template=template, pitch_shift=shifter) as chain:
        sp = chain.shift_pool
        assert sp is not None and chain.wav_pool.max_chunk_samples == sp.max_outputs
        assert sp.max_chunk == (chunk if to_model is None else chain.in_pool.max_outputs)
        at, j = [0, 0], [0, 0]
        while j[0] < len(sizes[0]) or j[1] < len(sizes[1]):
            items = []
            for s in (0, 1):
                if j[s] < len(sizes[s]):
                    c = sizes[s][j[s]]
                    items.append((s, xs[s][at[s]:at[s] + c] if c else None, j[s] == len(sizes[s]) - 1))
                    at[s] += c
                    j[s] += 1
            for (s, _, _), y in zip(items, chain.step(items)):
                got[s].append(y.clone())
        assert all(sp.received(s) == sp.emitted(s) and sp.pending(s) == 0 for s in (0, 1))       # as many samples out as went in
    with torch.no_grad():
        for s in (0, 1):
            x = xs[s][None] if to_model is None else to_model(xs[s][None])
            y = shifter(x)
            assert y.shape == x.shape
            mel = front(y)
            tm = f0mod.template_from_audio(y, SR, hop, **TRACKER) if use_template else None
            whole = (gen(mel, tm) if use_template else gen(mel))[0]
            plain = (gen(front(x), tm) if use_template else gen(front(x)))[0]
            rest = torch.cat(got[s], dim=-1)
            peak = float(whole.abs().max())
            bar = 2e-5 * max(1.0, peak)
            d = float((rest - whole).abs().max()) if rest.shape == whole.shape else float("inf")
            print(f"session {s} ({lengths[s]} client samples at {client} Hz{', template' if use_template else ''}): chain vs the whole file "
                  f"{d:.3e}, bar {bar:.1e}, peak {peak:.3f}")
            assert tuple(rest.shape) == tuple(whole.shape) == (1, mel.shape[-1] * hop)
            assert d <= bar, (s, d, bar)
            assert float((whole - plain).abs().max()) > 1e-2                             # the shift matters
