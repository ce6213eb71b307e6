"""GPU: the resample pool (fv_respool_*, vocoder_amd.resample.ResamplePool; resample_pool_kernel in vocoder_amd/csrc/resample.hip) and the
wav -> wav chain with a resampler on either side (inference.WavSessionPool).  Every comparison of the pool is ``torch.equal`` against
``Resample.forward`` of the session's whole utterance: an output is one ascending fp32 sum whatever workgroup forms it."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

from vocoder_amd import _lib
from vocoder_amd import resample as rs
from vocoder_amd import synthetic as syn
from vocoder_amd._lib import FishVocError
from vocoder_amd.sessions import PoolStateError

pytestmark = pytest.mark.gpu

PAIRS = [(44100, 48000), (48000, 8000), (2, 3)]
LENGTHS = [0, 1, 37, 5000, 9001]
MAX_CHUNK = 9000                                  # one item spans three 4096-sample tiles


@functools.lru_cache(maxsize=None)
def _mod(orig, new, table="lds"):
    return rs.Resample(orig, new, table=table)


def _utterances(lengths, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.uniform(-1, 1, size=L).astype(np.float32)).cuda() for L in lengths]


@functools.lru_cache(maxsize=None)
def _whole(orig, new, lengths, seed):
    """Resample.forward of every utterance alone (the LDS form), computed once and never modified."""
    mod = _mod(orig, new)
    return tuple(mod(x[None])[0] if x.numel() else torch.zeros(0, device="cuda") for x in _utterances(lengths, seed))


def _schedule(seed, lengths, max_chunk, small=64):
    """A seeded random schedule: a list of steps, each a list of ``(session, samples, end)``.  Step 0 names every session (the last one with a
    full max_chunk), step 1 names session 0 alone with no samples, step 2 one session; then random subsets (some empty) with sizes in
    [0, max_chunk], zero-sample items among them.  Even sessions end on their last chunk, odd ones on an empty item."""
    rng = random.Random(seed)
    S = len(lengths)
    at, done, steps = [0] * S, [False] * S, []
    while not all(done):
        t = len(steps)
        live = [s for s in range(S) if not done[s]]
        if t == 0:
            chosen = live
        elif t == 1:
            chosen = [0] if not done[0] else live[:1]
        elif t == 2:
            chosen = [live[-1]]
        else:
            chosen = rng.sample(live, rng.randint(0 if rng.random() < 0.15 else 1, len(live)))
        items = []
        for s in chosen:
            left = lengths[s] - at[s]
            c = max_chunk if t == 0 and s == S - 1 else 0 if t == 1 else rng.choice([0, rng.randint(0, max_chunk), rng.randint(0, small), small])
            c = min(c, left)
            end = c == left and (s % 2 == 0 or c == 0) and t != 1
            items.append((s, c, end))
            at[s] += c
            done[s] = end
        rng.shuffle(items)
        steps.append(items)
    return steps


def _run(pool, xs, steps, got=None, at=None):
    S = len(xs)
    at = [0] * S if at is None else at
    got = [[] for _ in range(S)] if got is None else got
    for items in steps:
        ys = pool.step([(s, xs[s][at[s]:at[s] + c] if c else None, f) for s, c, f in items])
        for (s, c, _), y in zip(items, ys):
            at[s] += c
            got[s].append(y.clone())
    return got


@pytest.mark.parametrize("table", ["lds", "global"])
@pytest.mark.parametrize("orig,new", PAIRS)
def test_sessions_equal_each_utterance_alone(orig, new, table):
    mod = _mod(orig, new, table)
    lengths = tuple(LENGTHS)
    xs, want = _utterances(lengths, orig + new), _whole(orig, new, lengths, orig + new)
    steps = _schedule(orig * 3 + new, lengths, MAX_CHUNK)
    assert len(steps[0]) == 5 and len(steps[1]) == 1 and (0, 0, True) in steps[0]                # all, one; a flush at N' = 0
    assert any(c == 0 and not f for items in steps for _, c, f in items) and any(c == MAX_CHUNK for items in steps for _, c, _ in items)
    with mod.pool(len(lengths), MAX_CHUNK) as pool:
        assert pool.max_outputs == pool.counters.max_outputs == mod.design.max_step_outputs(MAX_CHUNK)
        got = _run(pool, xs, steps)
        for s, L in enumerate(lengths):
            assert pool.received(s) == L and pool.emitted(s) == mod.output_length(L) and pool.pending(s) == 0
    for s, L in enumerate(lengths):
        y = torch.cat(got[s])
        assert y.shape == want[s].shape == (mod.output_length(L),) and torch.equal(y, want[s]), (s, L)


@pytest.mark.parametrize("table", ["lds", "global"])
def test_seventy_sessions_cross_three_table_blocks(table):
    orig, new = 44100, 48000
    mod = _mod(orig, new, table)
    rng = random.Random(70)
    lengths = tuple(rng.randint(100, 400) for _ in range(70))
    xs, want = _utterances(lengths, 700), _whole(orig, new, lengths, 700)
    at, got = [0] * 70, [[] for _ in range(70)]
    with mod.pool(70, 64) as pool:
        t = 0
        while any(a < L for a, L in zip(at, lengths)) or t == 0:
            chosen = list(range(70)) if t % 3 == 0 else rng.sample(range(70), rng.randint(33, 70))
            items = []
            for s in chosen:
                left = lengths[s] - at[s]
                if pool.counters.flushed[s]:
                    continue
                c = min(rng.randint(1, 64), left)
                items.append((s, c, c == left))
            rng.shuffle(items)
            _run(pool, xs, [items], got, at)
            t += 1
    for s in range(70):
        assert torch.equal(torch.cat(got[s]), want[s]), s


@pytest.mark.parametrize("orig,new", [(44100, 48000), (48000, 8000)])
def test_lockstep_sessions_equal_a_stream_push_for_push(orig, new):
    mod = _mod(orig, new)
    S, L = 4, 6000
    x = torch.stack(_utterances((L,) * S, 9))
    rng = random.Random(orig)
    with mod.stream(S, 4500) as st, mod.pool(S, 4500) as pool:
        at = 0
        while at < L:
            c = min(rng.choice([1, 63, 4500, rng.randint(1, 4500)]), L - at)
            a = st.push(x[:, at:at + c])
            b, emit = pool.step_padded([(s, c, False) for s in range(S)], x[:, at:at + c])
            assert emit == [a.shape[1]] * S and torch.equal(a, b), (at, c)
            at += c
        a = st.flush()
        b, emit = pool.step_padded([(s, 0, True) for s in range(S)], None)
        assert emit == [a.shape[1]] * S and a.shape[1] > 0 and torch.equal(a, b)


def test_padding_is_never_read_and_the_rest_is_zero():
    orig, new = 44100, 48000
    mod = _mod(orig, new)
    lengths = (700, 300, 0, 450)
    S = len(lengths)
    steps = [[(0, 200, False), (1, 0, False), (2, 0, True), (3, 450, False)], [(3, 0, False), (0, 300, False)],
             [(1, 300, True), (0, 200, True), (3, 0, True)]]

    def run(seed_others):
        xs = _utterances(lengths, 5)
        if seed_others:
            xs = [xs[0]] + _utterances(lengths, seed_others)[1:]
        at, got = [0] * S, [[] for _ in range(S)]
        with mod.pool(S, 512) as pool:
            for items in steps:
                count, stride = len(items), max(c for _, c, _ in items) + 7
                chunks = torch.full((count + 2, stride), float("nan"), device="cuda")      # taller than count, NaN wherever no sample lies
                for i, (s, c, _) in enumerate(items):
                    chunks[i, :c] = xs[s][at[s]:at[s] + c]
                plan = pool.counters.plan(items)
                out = torch.full((count, max(plan) + 9), float("nan"), device="cuda")
                res, emit = pool.step_padded(items, chunks, out)
                assert res is out and emit == plan
                assert bool(torch.isfinite(out).all())
                for i, ((s, c, _), k) in enumerate(zip(items, emit)):
                    assert bool((out[i, k:] == 0).all()), (items, i)       # exact zeros behind the outputs, a row of zeros for k = 0
                    at[s] += c
                    got[s].append(out[i, :k].clone())
        return [torch.cat(g) for g in got], xs

    a, xs = run(0)
    for s in range(S):
        want = mod(xs[s][None])[0] if lengths[s] else torch.zeros(0, device="cuda")
        assert torch.equal(a[s], want), s
    b, _ = run(77)                                                             # other audio in the other sessions
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


def test_a_reset_slot_starts_from_zeros():
    orig, new = 48000, 8000
    mod = _mod(orig, new)
    A, B = _utterances((1000, 777), 21)
    with mod.pool(4, 400) as pool:
        _run(pool, [None, None, A], [[(2, 400, False)], [(2, 400, False)], [(2, 200, True)]])
        assert pool.counters.flushed[2] and pool.emitted(2) == mod.output_length(1000)
        pool.reset(2)
        assert pool.received(2) == pool.emitted(2) == pool.pending(2) == 0
        got = _run(pool, [None, None, B], [[(2, 3, False)], [(2, 400, False)], [(2, 374, True)]])     # the carry still holds A's tail
    assert torch.equal(torch.cat(got[2]), mod(B[None])[0])


def test_refused_steps_move_nothing():
    orig, new = 44100, 48000
    mod = _mod(orig, new)
    lengths = (900, 600, 300)
    xs, want = _utterances(lengths, 3), _whole(orig, new, lengths, 3)
    L = _lib.lib()
    with mod.pool(3, 256) as pool:
        got = _run(pool, xs, [[(0, 256, False), (1, 200, False), (2, 256, False)], [(2, 44, True)]])
        at = [256, 200, 300]
        state = lambda: [(pool.received(s), pool.emitted(s), pool.pending(s)) for s in range(3)]      # noqa: E731
        before, py_before = state(), (list(pool.counters.received), list(pool.counters.emitted), list(pool.counters.flushed))
        x = xs[0][256:512]
        with pytest.raises(ValueError, match=r"duplicate session 0 \(item 1\)"):
            pool.step([(0, x, False), (0, x, False)])
        with pytest.raises(ValueError, match=r"item 1 \(session 1\) has 257 samples"):
            pool.step([(0, x, False), (1, xs[1][:257], False)])
        with pytest.raises(PoolStateError, match=r"session 2 was flushed \(item 1\)"):
            pool.step([(0, x, False), (2, None, False)])
        # the library's own refusals, below the Python plan
        items = (_lib.WavPoolItem * 2)(_lib.WavPoolItem(0, 256, 0), _lib.WavPoolItem(1, 100, 0))
        k = pool.counters.plan([(0, 256, False), (1, 100, False)])
        chunks = torch.zeros((2, 256), device="cuda")
        chunks[0], chunks[1, :100] = x, xs[1][200:300]
        out = torch.empty((2, max(k)), device="cuda")
        emit = (ctypes.c_int64 * 2)()
        for args, status, pattern in (
                ((chunks.data_ptr(), 256, out.data_ptr(), max(k) - 1, max(k) - 1), _lib.FV_ERR_INVALID,
                 "out_cols = %d, but item %d (session %d) emits %d outputs" % (max(k) - 1, k.index(max(k)), k.index(max(k)), max(k))),
                ((chunks.data_ptr(), 256, out.data_ptr(), max(k) - 1, max(k)), _lib.FV_ERR_INVALID, "out_stride = %d is shorter" % (max(k) - 1)),
                ((chunks.data_ptr(), 256, None, max(k), max(k)), _lib.FV_ERR_INVALID, "null output although item"),
                ((None, 256, out.data_ptr(), max(k), max(k)), _lib.FV_ERR_INVALID, "null chunk buffer although item 0 (session 0) has 256 samples"),
                ((chunks.data_ptr(), 255, out.data_ptr(), max(k), max(k)), _lib.FV_ERR_INVALID, "row stride 255 is shorter"),
        ):
            st = L.fv_respool_step(pool._h, items, 2, args[0], args[1], args[2], args[3], args[4], emit, None)
            msg = L.fv_last_error().decode()
            assert st == status and msg.startswith("fv_respool_step:") and pattern in msg, (st, msg)
            assert list(emit) == [0, 0]
        dup = (_lib.WavPoolItem * 2)(_lib.WavPoolItem(1, 1, 0), _lib.WavPoolItem(1, 1, 0))
        assert L.fv_respool_step(pool._h, dup, 2, chunks.data_ptr(), 256, out.data_ptr(), max(k), max(k), emit, None) == _lib.FV_ERR_INVALID
        assert "duplicate session 1 (item 1)" in L.fv_last_error().decode()
        done = (_lib.WavPoolItem * 1)(_lib.WavPoolItem(2, 0, 0))
        assert L.fv_respool_step(pool._h, done, 1, None, 0, None, 0, 0, emit, None) == _lib.FV_ERR_STATE
        assert "session 2 was flushed (item 0); fv_respool_reset" in L.fv_last_error().decode()
        assert state() == before and (pool.counters.received, pool.counters.emitted, pool.counters.flushed) == py_before
        with pytest.raises(FishVocError, match=r"session 7 lies outside \[0, 3\)"):
            pool.reset(7)
        # ... and the run goes on to its end, bit-identical
        _run(pool, xs, [[(0, 256, False), (1, 100, False)], [(1, 256, False), (0, 256, False)], [(0, 132, True), (1, 44, True)]], got, at)
    for s in range(3):
        assert torch.equal(torch.cat(got[s]), want[s]), s


# ---- the chain: ResamplePool -> WavPool -> SessionPool -> ResamplePool ----
TINY_GEN = dict(hop_length=64, num_mels=20, upsample_initial_channel=128, upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4],
                resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, pre_conv_kernel_size=7, post_conv_kernel_size=7,
                use_template=False)
SR, CLIENT = 24000, 48000
CHAIN_TOL = 2e-5      # of the peak: the bar of test_wav_session_pool_equals_the_generator_pool_fed_by_hand (tests/test_gpu_wavpool.py)


def test_the_chain_with_a_resampler_on_either_side():
    from vocoder_amd import inference
    from vocoder_amd.data.transforms import LogMelSpectrogram
    from vocoder_amd.modules.generators import HiFiGANGenerator
    front = LogMelSpectrogram(sample_rate=SR, n_fft=256, win_length=256, hop_length=64, n_mels=20, f_min=0.0, f_max=12000).eval().cuda()
    front.batch_invariant = True
    gen = HiFiGANGenerator(**TINY_GEN)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(TINY_GEN, 5).items()}, strict=True)
    gen = gen.eval().cuda()
    gen.batch_invariant = True
    to_model, to_client = rs.Resample(CLIENT, SR), rs.Resample(SR, CLIENT)
    S, chunk = 3, 1400
    lengths = (3554, 1200, 6000)                                            # client samples
    rng = np.random.default_rng(8)
    xs = [torch.from_numpy((0.2 * rng.normal(size=L)).astype(np.float32)).cuda() for L in lengths]
    steps = _schedule(13, lengths, chunk, small=128)

    def feed(step):
        at, got = [0] * S, [[] for _ in range(S)]
        for items in steps:
            ys = step(items, [xs[s][at[s]:at[s] + c] if c else None for s, c, _ in items])
            for (s, c, _), y in zip(items, ys):
                at[s] += c
                got[s].append(y.clone())
        return [torch.cat(g, dim=-1) for g in got]

    with inference.WavSessionPool(front, gen, S, chunk, input_resample=to_model, output_resample=to_client) as chain:
        assert chain.wav_pool.max_chunk_samples == chain.in_pool.max_outputs
        assert chain.out_pool.max_chunk == (chain.gen_pool.max_chunk_frames + chain.gen_pool.lookahead_frames) * 64
        wav_chunk, out_chunk = chain.in_pool.max_outputs, chain.out_pool.max_chunk
        a = feed(lambda items, rows: chain.step([(s, x, f) for (s, _, f), x in zip(items, rows)]))
        state = [(chain.in_pool.received(s), chain.wav_pool.received_samples(s), chain.gen_pool.received_frames(s), chain.out_pool.received(s))
                 for s in range(S)]
        with pytest.raises(PoolStateError, match=r"session 0 was flushed \(item 0\)"):
            chain.step([(0, xs[0][:10], False)])
        chain.reset(0)
        assert chain.in_pool.received(0) == chain.wav_pool.received_samples(0) == chain.gen_pool.received_frames(0) == chain.out_pool.received(0) == 0
        # refused by the second plan (20 samples at the model's rate end an utterance too short for one frame): the first pool has not moved
        with pytest.raises(ValueError, match=r"session 0 \(item 0\) ends after 20 samples"):
            chain.step([(0, xs[0][:40], True)])
        assert chain.in_pool.received(0) == chain.in_pool.counters.received[0] == 0 and not chain.in_pool.counters.flushed[0]
        assert state[1:] == [(chain.in_pool.received(s), chain.wav_pool.received_samples(s), chain.gen_pool.received_frames(s),
                              chain.out_pool.received(s)) for s in range(1, S)]

    # (a) by hand: a ResamplePool, the plain WavSessionPool and a ResamplePool, step by step with the same schedule
    with to_model.pool(S, chunk) as ip, inference.WavSessionPool(front, gen, S, wav_chunk) as plain, to_client.pool(S, out_chunk) as op:
        def by_hand(items, rows):
            mid = ip.step([(s, x, f) for (s, _, f), x in zip(items, rows)])
            audio = plain.step([(s, y if y.numel() else None, f) for (s, _, f), y in zip(items, mid)])
            out = op.step([(s, y[0] if y.shape[1] else None, f) for (s, _, f), y in zip(items, audio)])
            return [y[None] for y in out]
        b = feed(by_hand)
    for s in range(S):
        assert a[s].shape == b[s].shape and torch.equal(a[s], b[s]), s

    # (b) the whole utterance: output_resample(gen(frontend(input_resample(x)))), within the chain's bar times the output filter's gain
    gain = float(np.abs(to_client.design.taps.astype(np.float64)).sum(axis=1).max())      # sum |h| of the widest phase bounds a linear filter's gain
    with torch.no_grad():
        for s in range(S):
            alone = gen(front(to_model(xs[s][None])))                                      # (1, 1, frames * hop)
            want = to_client(alone[0])
            peak = float(alone.abs().max())
            d = float((a[s] - want).abs().max())
            print(f"session {s} ({lengths[s]} client samples): chain vs the utterance alone {d:.3e}, bar {CHAIN_TOL * peak * gain:.3e}")
            assert a[s].shape == want.shape and d <= CHAIN_TOL * peak * gain, (s, d, peak, gain)

    # the plain chain (no keyword) still runs as before
    with inference.WavSessionPool(front, gen, 2, 700) as plain:
        assert plain.in_pool is None and plain.out_pool is None
        y = plain.step([(0, torch.from_numpy((0.2 * rng.normal(size=700)).astype(np.float32)).cuda(), True)])
        assert y[0].shape == (1, front._framing().frames(700) * 64) and bool(torch.isfinite(y[0]).all())
