"""GPU: the log-mel front-end as a pool of sessions that advance independently (fv_wavpool_*, WavPool) and the wav -> wav chain on top of it
(WavSessionPool).  The checker is the module's whole-row forward of each utterance alone — bit for bit under batch_invariant, where every
output column is one fixed-order sum — and the CPU oracle within the front-end's bar, 2e-4, without it."""
import ctypes
import random
import re

import numpy as np
import pytest

from oracle import oracle as orc
from vocoder_amd import _lib, framing, synthetic as syn
from vocoder_amd._lib import FishVocError
from vocoder_amd.sessions import PoolStateError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = 2e-4

# (n_fft, hop, n_mels): plain; win - hop odd (pad_l != pad_r); LinearSpectrogram; a carry (n_fft samples) wider than one 256-thread block
CONFIGS = [(256, 64, 20), (256, 51, 20), (256, 64, 0), (320, 80, 16)]
LENGTHS = [1777, 600, 3000, 1283, 2048]      # utterances of 600 - 3000 samples
MAX_CHUNK = 700
TINY_GEN = dict(hop_length=64, num_mels=20, upsample_initial_channel=128, upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4],
                resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, pre_conv_kernel_size=7, post_conv_kernel_size=7,
                use_template=False)
_modules: dict = {}
_cache: dict = {}


def _module(cfg, invariant=True):
    """One front-end per (config, mode) for the whole file."""
    key = (cfg, invariant)
    if key not in _modules:
        from vocoder_amd.data.transforms import LogMelSpectrogram
        from vocoder_amd.data.transforms.spectrogram import LinearSpectrogram
        n_fft, hop, n_mels = cfg
        m = (LinearSpectrogram(n_fft, n_fft, hop) if n_mels == 0 else
             LogMelSpectrogram(sample_rate=24000, n_fft=n_fft, win_length=n_fft, hop_length=hop, n_mels=n_mels, f_min=0.0, f_max=12000))
        m = m.eval().cuda()
        m.batch_invariant = invariant
        _modules[key] = m
    return _modules[key]


def _waves(cfg, S, scale=0.2, seed=0):
    """White noise at 0.2, as the front-end's other tests: ``S`` utterances of ``LENGTHS``."""
    rng = np.random.default_rng(sum(cfg) + 31 * S + seed)
    return [(scale * rng.normal(size=LENGTHS[(s + seed) % len(LENGTHS)])).astype(np.float32) for s in range(S)]


def _whole(cfg, invariant, wave):
    """The module's whole-row forward of one utterance alone, (C, frames(L)) on the device, computed once."""
    key = ("whole", cfg, invariant, wave.tobytes())
    if key not in _cache:
        _cache[key] = _module(cfg, invariant)(torch.from_numpy(wave[None]).cuda())[0].clone()
    return _cache[key]


def _oracle(cfg, wave):
    key = ("oracle", cfg, wave.tobytes())
    if key not in _cache:
        n_fft, hop, n_mels = cfg
        if n_mels == 0:
            ref = orc.linear_spectrogram(wave[None], n_fft, n_fft, hop)
        else:
            ref = orc.logmel_forward(wave[None], dict(sample_rate=24000, n_fft=n_fft, win_length=n_fft, hop_length=hop, n_mels=n_mels,
                                                      f_min=0.0, f_max=12000))
        _cache[key] = ref[0]
    return _cache[key]


def _schedule(seed, lengths, hop, idle=1):
    """A seeded random schedule over ``len(lengths)`` slots: a list of steps, each a list of ``(session, samples, flush)``.  Step 0 gives the
    slots 1, hop - 1, hop and MAX_CHUNK samples, step 1 an empty push to slot 0; then slot ``idle`` sits out four steps in which random
    subsets of the others push; from step 6 on every step takes a random subset (it may be empty) with sizes in [0, MAX_CHUNK].  Even slots
    end with a flush on their last, non-empty chunk, odd slots with a flush on an empty one."""
    rng = random.Random(seed)
    S = len(lengths)
    at, done, steps = [0] * S, [False] * S, []
    while not all(done):
        t = len(steps)
        live = [s for s in range(S) if not done[s] and not (s == idle and 2 <= t < 6)]
        chosen = live if t < 2 else rng.sample(live, rng.randint(0 if t >= 6 and rng.random() < 0.15 else min(1, len(live)), len(live)))
        items = []
        for s in chosen:
            left = lengths[s] - at[s]
            if t == 0:
                c = [1, hop - 1, hop, MAX_CHUNK][s % 4]
            elif t < 6:
                c = 0 if (t, s) == (1, 0) else rng.randint(1, 2 * hop)
            else:
                c = rng.choice([rng.randint(0, MAX_CHUNK), rng.randint(0, 2 * hop), hop])
            c = min(c, left)
            flush = c == left and (s % 2 == 0 or c == 0)
            items.append((s, c, flush))
            at[s] += c
            done[s] = flush
        rng.shuffle(items)
        steps.append(items)
    return steps


def _check_schedule(steps, S, hop, idle):
    sizes = {c for items in steps for _, c, _ in items}
    assert {0, 1, hop - 1, hop, MAX_CHUNK} <= sizes
    flushes = [(s, c) for items in steps for s, c, f in items if f]
    assert len(flushes) == S and any(c > 0 for _, c in flushes) and any(c == 0 for _, c in flushes)
    assert all(c > 0 for items in steps[:2] for s, c, _ in items if s == idle)                 # the idle slot has samples in its carry ...
    quiet = [t for t, items in enumerate(steps) if idle not in {s for s, _, _ in items} and any(c > 0 for _, c, _ in items)]
    assert {2, 3, 4, 5} <= set(quiet)                                                         # ... sits out four steps while others push ...
    assert any(idle == s and c > 0 for items in steps[6:] for s, c, _ in items)               # ... and goes on
    assert any(len(items) < S for items in steps)


def _serve(pool, waves, steps, nan_stride=0):
    """Drive ``pool`` through ``steps``; returns the frames per session, concatenated.  ``nan_stride``: through ``step_padded`` with chunk rows
    ``nan_stride`` wider than the longest chunk and NaN wherever no sample is, and an output of ``max_frames`` columns that starts as NaN."""
    S = len(waves)
    xs = [torch.from_numpy(w).cuda() for w in waves]
    at, got = [0] * S, [[] for _ in range(S)]
    C = pool.out_channels
    for items in steps:
        want = pool.counters.plan(items)
        before = {s: (pool.received_samples(s), pool.emitted_frames(s)) for s in range(S)}
        if nan_stride:
            stride = max((c for _, c, _ in items), default=0) + nan_stride
            chunks = torch.full((len(items), stride), float("nan"), device="cuda")
            for i, (s, c, _) in enumerate(items):
                chunks[i, :c] = xs[s][at[s]:at[s] + c]
            out = torch.full((len(items), C, pool.max_frames), float("nan"), device="cuda")
            y, emit = pool.step_padded(items, chunks, out=out)
            assert y is out and bool(torch.isfinite(out).all())
            for i, k in enumerate(emit):
                assert not bool(out[i, :, k:].any()), (items, i)      # exact zeros after the item's frames; a zero row for k = 0
            ys = [out[i, :, :k] for i, k in enumerate(emit)]
        else:
            ys = pool.step([(s, xs[s][at[s]:at[s] + c] if c else None, f) for s, c, f in items])
            emit = [int(y.shape[1]) for y in ys]
        assert emit == want and all(tuple(y.shape) == (C, k) for y, k in zip(ys, emit))
        for (s, c, f), y in zip(items, ys):
            at[s] += c
            got[s].append(y.clone())
            assert (pool.received_samples(s), pool.emitted_frames(s)) == (at[s], before[s][1] + y.shape[1])
            assert pool.pending_samples(s) == pool.counters.pending_samples(s)
        for s in set(range(S)) - {s for s, _, _ in items}:
            assert (pool.received_samples(s), pool.emitted_frames(s)) == before[s]
    return [torch.cat(g, dim=1) if g else torch.empty((C, 0), device="cuda") for g in got]


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("invariant", [True, False])
def test_sessions_equal_each_utterance_alone(cfg, invariant):
    m = _module(cfg, invariant)
    S = 5 if cfg[1] == 51 else 4
    waves = _waves(cfg, S)
    lengths = [len(w) for w in waves]
    steps = _schedule(sum(cfg), lengths, cfg[1], idle=1)
    _check_schedule(steps, S, cfg[1], 1)
    with m.wav_pool(S, MAX_CHUNK) as pool:
        assert pool.max_frames == (cfg[0] + MAX_CHUNK) // cfg[1] + 2 and pool.workspace_bytes % 256 == 0
        got = _serve(pool, waves, steps)
        assert [pool.received_samples(s) for s in range(S)] == lengths
    for s, w in enumerate(waves):
        assert got[s].shape[1] == m.frames(len(w))
        if invariant:
            assert torch.equal(got[s], _whole(cfg, True, w)), (cfg, s)
            _cache[("served", cfg, s)] = got[s]
        ref = _oracle(cfg, w)
        err = float(np.abs(got[s].cpu().numpy() - ref).max())
        print(f"cfg {cfg} invariant {invariant} session {s} ({len(w)} samples): max|d| vs oracle {err:.2e}")
        assert ref.shape == tuple(got[s].shape) and err <= TOL, (cfg, s, err)


def test_thirty_four_sessions_pass_one_launchs_table_entries():
    """34 sessions, more than the 32 entries one launch carries: a step in which every session pushes less than a hop (34 carry entries, no
    frame), a step in which all 34 push the rest and emit (34 rows), a flush of all.  Sessions 0, 31, 32 and 33 — either side of the edge
    between the first and the second launch — are the whole-row forward of their utterance bit for bit; so are the others."""
    cfg = CONFIGS[0]
    m = _module(cfg, True)
    S, hop = 34, cfg[1]
    rng = np.random.default_rng(34)
    waves = [(0.2 * rng.normal(size=300 + 11 * s)).astype(np.float32) for s in range(S)]
    first = [1 + s % (hop - 1) for s in range(S)]
    steps = [[(s, first[s], False) for s in range(S)], [(s, len(waves[s]) - first[s], False) for s in range(S)],
             [(s, 0, True) for s in range(S)]]
    with m.wav_pool(S, MAX_CHUNK) as pool:
        assert pool.counters.plan(steps[0]) == [0] * S
        got = _serve(pool, waves, steps)
        assert pool.emitted_frames(33) == m.frames(len(waves[33])) > m.frames_ready(len(waves[33])) > 0      # steps 1 and 2 both emit
    for s in [0, 31, 32, 33] + list(range(1, 31)):
        assert torch.equal(got[s], _whole(cfg, True, waves[s])), s


@pytest.mark.parametrize("cfg", CONFIGS)
def test_lockstep_sessions_equal_a_batched_stream(cfg):
    m = _module(cfg)
    S, hop = 4, cfg[1]
    L = 1200
    wave = np.stack([w[:L] for w in _waves(cfg, S, seed=2)])
    assert wave.shape == (S, L)
    x = torch.from_numpy(wave).cuda()
    rng = random.Random(sum(cfg))
    sizes = [1, hop - 1, hop, MAX_CHUNK, 0]
    while sum(sizes) < L:
        sizes.append(min(L - sum(sizes), rng.randint(0, 3 * hop)))
    with m.stream(batch=S, max_chunk_samples=MAX_CHUNK) as st, m.wav_pool(S, MAX_CHUNK) as pool:
        at = 0
        for c in sizes:
            want = st.push(x[:, at:at + c])
            ys = pool.step([(s, x[s, at:at + c] if c else None, False) for s in range(S)])
            assert all(torch.equal(ys[s], want[s]) for s in range(S)), (cfg, at, c)
            at += c
        want = st.flush()
        ys = pool.step([(s, None, True) for s in range(S)])
        assert want.shape[2] > 0 and all(torch.equal(ys[s], want[s]) for s in range(S))


@pytest.mark.parametrize("cfg", CONFIGS)
def test_padding_is_never_read_and_the_rest_of_the_output_is_zero(cfg):
    m = _module(cfg)
    S = 5 if cfg[1] == 51 else 4
    waves = _waves(cfg, S)
    steps = _schedule(sum(cfg), [len(w) for w in waves], cfg[1], idle=1)
    assert any(c == 0 and not f for items in steps for _, c, f in items)      # items that emit nothing
    with m.wav_pool(S, MAX_CHUNK) as pool:
        got = _serve(pool, waves, steps, nan_stride=7)
    for s, w in enumerate(waves):
        assert torch.equal(got[s], _whole(cfg, True, w)), (cfg, s)
        if ("served", cfg, s) in _cache:
            assert torch.equal(got[s], _cache[("served", cfg, s)])


@pytest.mark.parametrize("cfg", CONFIGS)
def test_a_reset_slot_starts_the_next_utterance_from_zeros(cfg):
    m = _module(cfg)
    hop = cfg[1]
    first = (1e6 * np.random.default_rng(5).normal(size=900)).astype(np.float32)      # poisons the slot's carry
    second, other = _waves(cfg, 2, seed=3)
    x1, x2, xo = (torch.from_numpy(w).cuda() for w in (first, second, other))
    with m.wav_pool(2, MAX_CHUNK) as pool:
        a = [pool.step([(0, xo[:500], False), (1, x1[:MAX_CHUNK], False)])[0]]
        a.append(pool.step([(1, x1[MAX_CHUNK:], True), (0, xo[500:501], False)])[1])
        with pytest.raises(PoolStateError, match="session 1 was flushed"):
            pool.step([(1, x2[:10], False)])
        pool.reset(1)
        assert (pool.received_samples(1), pool.emitted_frames(1), pool.pending_samples(1)) == (0, 0, 0)
        assert (pool.received_samples(0), pool.emitted_frames(0)) == (501, m.frames_ready(501))      # the other slot goes on through the reset
        b, at, ao = [], 0, 501
        for c in (hop - 1, 1, MAX_CHUNK, 2 * hop + 1):
            ys = pool.step([(1, x2[at:at + c], False), (0, xo[ao:ao + 300], False)])
            b.append(ys[0])
            a.append(ys[1])
            at, ao = at + c, ao + 300
        ys = pool.step([(0, xo[ao:], True), (1, x2[at:], True)])
        a.append(ys[0])
        b.append(ys[1])
    assert torch.equal(torch.cat(b, dim=1), _whole(cfg, True, second))
    assert torch.equal(torch.cat(a, dim=1), _whole(cfg, True, other))


def _raw_step(pool, items, chunks, out_frames, ws_bytes=None):
    """fv_wavpool_step itself -> (status, message, frames_out)."""
    n = len(items)
    arr = (_lib.WavPoolItem * max(n, 1))(*[_lib.WavPoolItem(s, c, int(f)) for s, c, f in items])
    got = (ctypes.c_int64 * max(n, 1))()
    out = torch.full((n, pool.out_channels, max(out_frames, 1)), 7.0, device="cuda")
    st = pool._lib.fv_wavpool_step(pool._h, arr, n, chunks.data_ptr() if chunks is not None else None,
                                   chunks.shape[1] if chunks is not None else 0, out.data_ptr(), out_frames, got, pool._ws.data_ptr(),
                                   pool._ws.numel() * 4 if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return st, pool._lib.fv_last_error().decode(), [int(got[i]) for i in range(n)], out


@pytest.mark.parametrize("cfg", CONFIGS)
def test_refused_steps_move_nothing(cfg):
    m = _module(cfg)
    fr = m._framing()
    hop, pad = cfg[1], max(fr.pad_l, fr.pad_r)
    S = 4
    waves = _waves(cfg, S)
    xs = [torch.from_numpy(w).cuda() for w in waves]
    with m.wav_pool(S, MAX_CHUNK) as pool:
        # sessions 0 and 1 are under way, 2 has ended, 3 has not begun
        got = {s: [] for s in range(S)}
        ys = pool.step([(0, xs[0][:400], False), (1, xs[1][:133], False), (2, xs[2][:MAX_CHUNK], True)])
        got[0].append(ys[0])
        got[1].append(ys[1])
        state = [(pool.received_samples(s), pool.emitted_frames(s), pool.pending_samples(s)) for s in range(S)]
        lib_state = [(int(pool._lib.fv_wavpool_received_samples(pool._h, s)), int(pool._lib.fv_wavpool_emitted_frames(pool._h, s)))
                     for s in range(S)]
        assert lib_state == [(n, e) for n, e, _ in state]
        chunks = torch.zeros((3, MAX_CHUNK), device="cuda")
        chunks[0, :300] = xs[0][400:700]
        chunks[1, :300] = xs[1][133:433]
        chunks[2, :pad] = xs[3][:pad]
        cases = [
            ([(0, 300, False), (1, 300, False), (0, 5, False)], _lib.FV_ERR_INVALID, ValueError, r"duplicate session 0 \(item 2\)"),
            ([(0, 300, False), (1, 300, False), (2, 5, False)], _lib.FV_ERR_STATE, PoolStateError, r"session 2 was flushed \(item 2\)"),
            ([(0, 300, False), (1, 300, False), (3, pad, True)], _lib.FV_ERR_INVALID, ValueError, r"session 3 \(item 2\) ends after %d" % pad),
        ]
        for items, status, exc, pattern in cases:
            with pytest.raises(exc, match=pattern):                   # the Python plan refuses first ...
                pool.step_padded(items, chunks)
            st, msg, frames, out = _raw_step(pool, items, chunks, pool.max_frames)      # ... and the library refuses the same step by name
            assert st == status and "fv_wavpool_step" in msg, (st, msg)
            assert re.search(pattern, msg), msg
            assert frames == [0, 0, 0] and bool((out == 7.0).all())   # nothing was written
            assert [(pool.received_samples(s), pool.emitted_frames(s), pool.pending_samples(s)) for s in range(S)] == state
        # buffers: a missing chunk buffer, a short row stride, a short output, a workspace that is too small
        ok = [(0, 300, False), (1, 300, False)]
        for kw, pattern in ((dict(chunks=None), r"null chunk buffer although item 0 \(session 0\) has 300 samples"),
                            (dict(chunks=chunks[:2, :299].contiguous()), r"row stride 299 is shorter than the longest chunk"),
                            (dict(out_frames=1), r"out_frames = 1, but an item of this step emits"),
                            (dict(ws_bytes=pool.workspace_bytes - 256), r"workspace too small")):
            args = dict(chunks=chunks[:2].contiguous(), out_frames=pool.max_frames)
            args.update(kw)
            st, msg, frames, out = _raw_step(pool, ok, args["chunks"], args["out_frames"], args.get("ws_bytes"))
            assert st == _lib.FV_ERR_INVALID and re.search(pattern, msg), (st, msg)
            assert frames == [0, 0] and bool((out == 7.0).all())
            assert [(pool.received_samples(s), pool.emitted_frames(s), pool.pending_samples(s)) for s in range(S)] == state
        assert pool._lib.fv_wavpool_reset(pool._h, S) == _lib.FV_ERR_INVALID
        # the next valid steps still give each utterance alone: the refused ones moved nothing on the device
        ys = pool.step([(0, xs[0][400:700], False), (1, xs[1][133:], True), (3, xs[3][:pad], False)])
        got[0].append(ys[0])
        got[1].append(ys[1])
        got[3].append(ys[2])
        ys = pool.step([(3, xs[3][pad:pad + MAX_CHUNK], False), (0, xs[0][700:1400], False)])
        got[3].append(ys[0])
        got[0].append(ys[1])
        ys = pool.step([(0, xs[0][1400:], True), (3, xs[3][pad + MAX_CHUNK:], True)])
        got[0].append(ys[0])
        got[3].append(ys[1])
        for s in (0, 1, 3):
            assert torch.equal(torch.cat(got[s], dim=1), _whole(cfg, True, waves[s])), (cfg, s)


def test_engines_and_handles_that_cannot_serve_a_pool_are_refused():
    cfg = CONFIGS[0]
    from vocoder_amd.engine import Engine, upsampler_config
    gen = Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**TINY_GEN), state_dict=syn.hifigan_state_dict(TINY_GEN, 1))
    with pytest.raises(FishVocError, match="log-mel") as ei:
        gen.wav_pool(2, 64)
    assert ei.value.status == _lib.FV_ERR_UNSUPPORTED
    h = ctypes.c_void_p()
    assert gen._lib.fv_wavpool_create(gen._h, 2, 64, ctypes.byref(h)) == _lib.FV_ERR_UNSUPPORTED and not h.value
    assert "fv_wavpool_create" in gen._lib.fv_last_error().decode() and "FV_MODEL_LOGMEL" in gen._lib.fv_last_error().decode()
    gen.close()
    m = _module(cfg)
    for sessions in (0, 65536):
        with pytest.raises(FishVocError, match=r"sessions \(%d\)" % sessions) as ei:
            m.wav_pool(sessions, 64)
        assert ei.value.status == _lib.FV_ERR_INVALID
    with pytest.raises(FishVocError, match="log-mel"):                # the frame-windowed pool keeps refusing a front-end
        m.session_pool(sessions=2, max_chunk_frames=4)
    pool = m.wav_pool(2, 64)
    m.invalidate_engine()                                             # a rebuilt engine closes its pools
    with pytest.raises(FishVocError, match="create a new pool"):
        pool.step([(0, torch.zeros(8, device="cuda"), False)])
    with pytest.raises(FishVocError, match="create a new pool"):
        pool.reset(0)


def test_wav_session_pool_equals_the_generator_pool_fed_by_hand():
    from vocoder_amd import inference
    from vocoder_amd.modules.generators import HiFiGANGenerator
    cfg = CONFIGS[0]
    front = _module(cfg)
    fr = front._framing()
    hop = cfg[1]
    gen = HiFiGANGenerator(**TINY_GEN)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(TINY_GEN, 5).items()}, strict=True)
    gen = gen.eval().cuda()
    gen.batch_invariant = True
    S = 3
    waves = _waves(cfg, S, seed=1)
    lengths = [len(w) for w in waves]
    xs = [torch.from_numpy(w).cuda() for w in waves]
    steps = _schedule(11, lengths, hop, idle=2)
    mels = [_whole(cfg, True, w) for w in waves]
    with inference.WavSessionPool(front, gen, S, MAX_CHUNK) as chain:
        assert chain.gen_pool.max_chunk_frames == chain.wav_pool.max_frames and chain.hop == 64
        at, got = [0] * S, [[] for _ in range(S)]
        for items in steps:
            ys = chain.step([(s, xs[s][at[s]:at[s] + c] if c else None, f) for s, c, f in items])
            for (s, c, _), y in zip(items, ys):
                at[s] += c
                got[s].append(y.clone())
        with pytest.raises(PoolStateError, match="session 0 was flushed"):
            chain.step([(0, xs[0][:10], False)])
        chain.reset(0)
        assert chain.wav_pool.received_samples(0) == 0 and chain.gen_pool.received_frames(0) == 0
        max_frames = chain.wav_pool.max_frames
    # by hand: the whole-row mel's frames in the counts PoolCounters gives, each item's `end` passed on as the generator pool's flush
    pc = framing.PoolCounters(fr, S, MAX_CHUNK)
    with gen.session_pool(S, max_chunk_frames=max_frames) as pool:
        want = [[] for _ in range(S)]
        for items in steps:
            ks = pc.plan(items)
            hand = [(s, mels[s][:, pc.emitted[s]:pc.emitted[s] + k] if k else None, f) for (s, _, f), k in zip(items, ks)]
            pc.commit(items, ks)
            for (s, _, _), y in zip(items, pool.step(hand)):
                want[s].append(y.clone())
    for s in range(S):
        a, b = torch.cat(got[s], dim=1), torch.cat(want[s], dim=1)
        assert a.shape == b.shape == (1, fr.frames(lengths[s]) * 64) and torch.equal(a, b), s
        alone = gen(mels[s][None])[0]
        peak = float(alone.abs().max())
        d = float((a - alone).abs().max())
        print(f"session {s} ({lengths[s]} samples, {fr.frames(lengths[s])} frames): chain vs the utterance alone {d:.3e}, peak {peak:.3e}")
        assert d <= 2e-5 * peak, (s, d, peak)
    with pytest.raises(ValueError, match="HiFiGANGenerator takes a pitch template"):
        inference.WavSessionPool(front, HiFiGANGenerator(**dict(TINY_GEN, use_template=True)).eval().cuda(), S, MAX_CHUNK)
