"""GPU: the posterior encoder for sessions that advance independently (fv_wnpool_*, ``PosteriorEncoder.pool``) and the codec's encode pool.

Every comparison is ``torch.equal`` against the module's own ``forward`` on a session's whole utterance — one ragged ``forward(x_padded,
lengths)`` gives every row's bits at once, a row being bit-identical alone or in a batch — so there is no tolerance.  The configs are the
stream tests' (tests/test_gpu_posterior_stream.py), by value: the folded k = 5, d = 1 taps (``k5``, ``default``), the run-time taps
(``dilated``, ``bnvae``, ``k1``), R = 0, and the real widths with 16 layers (``default``).  The pool's rings hold pow2(2 p_i + max_chunk + R)
frames (an item may flush with its last frames): 32 for ``k5`` with max_chunk 8, so 300 frames are more than 9 laps."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from vocoder_amd import _lib, codec
from vocoder_amd import synthetic as syn
from vocoder_amd._lib import FV_ERR_INVALID, FV_ERR_STATE, FishVocError
from vocoder_amd.modules.encoders import PosteriorEncoder, PosteriorPool
from vocoder_amd.sessions import PoolStateError

pytestmark = pytest.mark.gpu

TABLE = 128         # entries of one launch table (fv_wnpool_*: "a by-value table of 128 entries")


def make_cfg(cin, out, C, k, rate, cycle, nl, mode):
    return dict(in_channels=cin, out_channels=out, hidden_channels=C, kernel_size=k, dilation_rate=rate, dilation_cycle=cycle, n_layers=nl, mode=mode)


# name -> (config, seed of its weights, R)
CONFIGS = {
    "k5": (make_cfg(20, 8, 48, 5, 1, 1, 4, "vqvae"), 21, 8),
    "dilated": (make_cfg(20, 8, 48, 5, 2, 3, 4, "vae"), 12, 16),
    "bnvae": (make_cfg(20, 8, 32, 3, 3, 2, 1, "bnvae"), 13, 1),
    "k1": (make_cfg(20, 8, 32, 1, 1, 1, 2, "vqvae"), 23, 0),
    "default": (dict(syn.POSTERIOR_DEFAULT), 11, 32),
}
NAMES = sorted(CONFIGS)


def new_module(name):
    cfg, seed, _ = CONFIGS[name]
    m = PosteriorEncoder(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in syn.posterior_state_dict(cfg, seed).items()}, strict=True)
    return m.eval().cuda()


@functools.lru_cache(maxsize=None)
def module(name):
    m = new_module(name)
    assert m.reach_frames == CONFIGS[name][2]
    return m


@functools.lru_cache(maxsize=None)
def case(name, lengths, seed=0):
    """(the utterances, forward's tensors per utterance): one ragged forward, computed once, shared, never written."""
    cfg = CONFIGS[name][0]
    T = max(lengths)
    x = torch.from_numpy(np.random.default_rng(1000 * seed + T + len(lengths)).standard_normal((len(lengths), cfg["in_channels"], T))
                         .astype(np.float32)).cuda()
    res = module(name)(x, list(lengths))
    res = (res,) if cfg["mode"] == "vqvae" else tuple(res[:3])
    return [x[b, :, :n] for b, n in enumerate(lengths)], [tuple(t[b, :, :n] for t in res) for b, n in enumerate(lengths)]


def tensors(res):
    """What a step returns for one item -> its tensors without the mask."""
    if isinstance(res, tuple):
        assert len(res) == 4 and res[3].shape == (1, res[0].shape[1]) and bool((res[3] == 1).all())
        return tuple(res[:3])
    return (res,)


def assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, f"{what}: tensor {i} has shape {tuple(g.shape)}, expected {tuple(w.shape)}"
        assert torch.equal(g, w), f"{what}: tensor {i} differs, max |d| = {float((g - w).abs().max()):.3e}"


class Driver:
    """Feeds utterances to slots of a pool step by step and collects every session's output; checks each item's shape against the plan."""

    def __init__(self, pool, xs):
        self.pool, self.xs = pool, dict(xs)               # slot -> (in_channels, T)
        self.pos = {s: 0 for s in self.xs}
        self.done = {s: False for s in self.xs}
        self.parts = {s: [] for s in self.xs}
        self.sent = {s: [] for s in self.xs}              # the chunk sizes, for the same chunks through a stream

    def step(self, asks, reverse=False):
        """asks: (slot, frames, flush) -> one pool step."""
        items = []
        for s, c, flush in asks:
            x = self.xs[s]
            items.append((s, x[:, self.pos[s]:self.pos[s] + c] if c else None, flush))
        if reverse:
            items = items[::-1]
            asks = list(asks)[::-1]
        plan = self.pool.counters.plan([(s, c, f) for s, c, f in asks])
        res = self.pool.step(items)
        assert len(res) == len(items)
        for (s, c, flush), r, k in zip(asks, res, plan):
            ts = tensors(r)
            for t in ts:
                assert t.shape == (self.pool.out_channels, k) and t.dtype == torch.float32, (t.shape, k)
            self.parts[s].append(ts)
            self.sent[s].append(c)
            self.pos[s] += c
            self.done[s] = flush
            assert self.pool.received_frames(s) == self.pos[s] and self.pool.pending_frames(s) == self.pos[s] - self.pool.emitted_frames(s)

    def restart(self, s, x):
        """Slot s is reset and begins the utterance x."""
        self.pool.reset(s)
        self.xs[s], self.pos[s], self.done[s], self.parts[s], self.sent[s] = x, 0, False, [], []

    def left(self, s):
        return self.xs[s].shape[1] - self.pos[s]

    def output(self, s):
        assert self.done[s] and self.left(s) == 0 and self.pool.emitted_frames(s) == self.pos[s]
        return tuple(torch.cat([p[i] for p in self.parts[s]], dim=1) for i in range(len(self.parts[s][0])))


def random_schedule(d, rng, max_chunk, flush_with_frames):
    """Steps of a random non-empty subset of the unfinished slots, chunks in [0, max_chunk]; slot s ends with a flush that accompanies its
    last frames where flush_with_frames[s], else with a zero-frame flush item of its own."""
    steps = 0
    while not all(d.done.values()):
        free = [s for s in d.xs if not d.done[s]]
        chosen = sorted(rng.permutation(free)[: rng.integers(1, len(free) + 1)].tolist())
        asks = []
        for s in chosen:
            left = d.left(s)
            if left == 0:
                asks.append((s, 0, True))
                continue
            c = min(int(rng.integers(0, max_chunk + 1)), left)
            asks.append((s, c, c == left and flush_with_frames[s]))
        d.step(asks)
        steps += 1
        assert steps < 5000
    return steps


def through_stream(m, x, chunks):
    """The same chunks through stream(1, 8), then its flush (the pool's flush item, where it had no frames, is a push of none)."""
    parts, a = [], 0
    with m.stream(1, 8) as st:
        for c in list(chunks) + [None]:
            res = st.flush() if c is None else st.push(x[None, :, a:a + c])
            parts.append(tuple(t[0] for t in (res[:3] if isinstance(res, tuple) else (res,))))
            a += c or 0
    return tuple(torch.cat([p[i] for p in parts], dim=1) for i in range(len(parts[0])))


@pytest.mark.parametrize("name", NAMES)
def test_whole_utterance_bits(name):
    m, R = module(name), CONFIGS[name][2]
    lengths = (2 * R + 37, R + 5, 1, 70)
    xs, want = case(name, lengths)
    with m.pool(4, 8) as pool:
        assert isinstance(pool, PosteriorPool) and pool.lookahead_frames == R and pool.sessions == 4 and pool.max_chunk_frames == 8
        assert pool.max_frames == 8 + R
        d = Driver(pool, enumerate(xs))
        steps = random_schedule(d, np.random.default_rng(7), 8, {0: True, 1: False, 2: True, 3: False})
        assert steps > 8
        for s in range(4):
            got = d.output(s)
            assert_same(got, want[s], f"session {s}")
            assert_same(through_stream(m, xs[s], d.sent[s]), got, f"session {s} through stream(1, 8)")


@pytest.mark.parametrize("name", ["k5", "dilated"])
def test_independence_and_reuse(name):
    m, R = module(name), CONFIGS[name][2]
    xs, want = case(name, (2 * R + 37, R + 5, 1, 70))
    (long_x,), (long_want,) = case(name, (300,), seed=3)
    short_xs, short_want = case(name, (R + 5, max(R // 2, 1)), seed=4)

    def eights(d, s):
        c = min(8, d.left(s))
        return (s, c, c == d.left(s))

    def run(d, slots, until, reverse_odd=False):
        step = 0
        while not until():
            d.step([eights(d, s) for s in slots if not d.done[s]], reverse=reverse_odd and bool(step % 2))
            step += 1

    with m.pool(4, 8) as pool:
        # slot 1 with the other slots idle
        d = Driver(pool, {1: xs[1]})
        run(d, [1], lambda: d.done[1])
        alone = d.output(1)
        assert_same(alone, want[1], "slot 1 alone")
        pool.reset(1)
        # all four busy, the items in reverse order on every other step; slot 3 runs the 300-frame utterance
        d = Driver(pool, {0: xs[0], 1: xs[1], 2: xs[2], 3: long_x})
        run(d, range(4), lambda: all(d.done.values()), reverse_odd=True)
        assert_same(d.output(1), alone, "slot 1 with the others busy")
        assert_same(d.output(0), want[0], "slot 0")
        assert_same(d.output(2), want[2], "slot 2")
        assert_same(d.output(3), long_want, "300 frames in slot 3")
        # slot 3 is reset and reused while slot 0 is mid-utterance: the short utterances read nothing the long one left in the rings
        d.restart(0, xs[0])
        d.step([eights(d, 0)])
        for i in range(2):
            d.restart(3, short_xs[i])
            assert (pool.received_frames(3), pool.emitted_frames(3), pool.pending_frames(3)) == (0, 0, 0)
            run(d, [0, 3], lambda: d.done[3])
            assert_same(d.output(3), short_want[i], f"{short_xs[i].shape[1]} frames in slot 3 after reset {i + 1}")
            assert not d.done[0] and 0 < d.pos[0] < xs[0].shape[1]
        run(d, [0], lambda: d.done[0])
        assert_same(d.output(0), want[0], "slot 0, mid-utterance through both resets of slot 3")


def test_ring_wrap_under_unequal_pace():
    """k5, max_chunk 8: slot 0 takes 300 frames in chunks of 8 while slot 1 advances one frame per step: more than 9 laps of the 32-frame
    rings for slot 0, and the two slots' frame numbers drift apart by hundreds."""
    (x0,), (want0,) = case("k5", (300,), seed=3)
    (x1,), (want1,) = case("k5", (38,), seed=5)
    with module("k5").pool(2, 8) as pool:
        d = Driver(pool, {0: x0, 1: x1})
        while not (d.done[0] and d.done[1]):
            asks = []
            if not d.done[0]:
                c = min(8, d.left(0))
                asks.append((0, c, c == d.left(0)))
            if not d.done[1]:
                asks.append((1, 1, d.left(1) == 1))
            d.step(asks)
        assert_same(d.output(0), want0, "slot 0: 300 frames in eights")
        assert_same(d.output(1), want1, "slot 1: one frame per step")


def test_both_tiles_in_one_launch():
    """dilated, max_chunk 160: 150 frames beside 3 (the 128-column tile, chosen by the widest item), then 70 | 64 | 16 beside 1 | 1 | 1."""
    xs, want = case("dilated", (150, 3), seed=6)
    xs2, want2 = case("dilated", (150, 3), seed=7)
    with module("dilated").pool(2, 160) as pool:
        d = Driver(pool, enumerate(xs))
        d.step([(0, 150, True), (1, 3, True)])
        assert_same(d.output(0), want[0], "150 frames in one item")
        assert_same(d.output(1), want[1], "3 frames beside them")
        pool.reset(0), pool.reset(1)
        d = Driver(pool, enumerate(xs2))
        for c, last in ((70, False), (64, False), (16, True)):
            d.step([(0, c, last), (1, 1, last)])
        assert_same(d.output(0), want2[0], "70 | 64 | 16")
        assert_same(d.output(1), want2[1], "1 | 1 | 1")


def test_more_items_than_one_table():
    name, S = "bnvae", TABLE + 5
    m = module(name)
    nl = CONFIGS[name][0]["n_layers"]
    lengths = tuple(1 + (7 * s) % 23 for s in range(S))
    xs, want = case(name, lengths)
    with m.pool(S, 8) as pool:
        d = Driver(pool, enumerate(xs))
        most = 0
        while not all(d.done.values()):
            asks = []
            for s in range(S):
                if not d.done[s]:
                    c = min(8, d.left(s))
                    asks.append((s, c, c == d.left(s)))
            d.step(asks)
            if len(asks) > TABLE:
                most = max(most, pool.last_step_launches)
                assert pool.last_step_launches <= (2 * nl + 2) * 2
        assert most > 2 * nl + 2                                    # two blocks did run
        for s in range(S):
            assert_same(d.output(s), want[s], f"session {s} of {S}")
        # one full table takes the launches of a single session
        for s in range(S):
            pool.reset(s)
        x8 = xs[lengths.index(max(lengths))][:, :8]
        assert x8.shape[1] == 8
        pool.step([(0, x8, False)])
        single = pool.last_step_launches
        assert 0 < single <= 2 * nl + 2
        pool.reset(0)
        pool.step([(s, x8, False) for s in range(TABLE)])
        assert pool.last_step_launches == single


@pytest.mark.parametrize("name", ["k5", "bnvae"])
def test_padding_is_never_read_and_outputs_end_in_zeros(name):
    m, R = module(name), CONFIGS[name][2]
    cfg = CONFIGS[name][0]
    xs, want = case(name, (R + 9, 5, 3))
    vae = cfg["mode"] != "vqvae"
    with m.pool(3, 8) as pool:
        pos, outs = [0, 0, 0], [[], [], []]
        done = [False] * 3
        while not all(done):
            items, chunks = [], torch.full((3, cfg["in_channels"], 11), float("nan"), device="cuda")
            rows = [s for s in range(3) if not done[s]]
            chunks = chunks[:len(rows)]
            for i, s in enumerate(rows):
                c = min(8 if s == 0 else 2, xs[s].shape[1] - pos[s])
                chunks[i, :, :c] = xs[s][:, pos[s]:pos[s] + c]
                pos[s] += c
                done[s] = pos[s] == xs[s].shape[1]
                items.append((s, c, done[s]))
            cols = pool.max_frames
            new = lambda: torch.full((len(rows), cfg["out_channels"], cols), float("nan"), device="cuda")      # noqa: E731
            out = (new(), new(), new()) if vae else new()
            got, emit = pool.step_padded(items, chunks, out=out)
            for t in (got if vae else (got,)):
                assert not bool(torch.isnan(t).any())
                for i, k in enumerate(emit):
                    assert bool((t[i, :, k:] == 0).all()) and not bool(torch.signbit(t[i, :, k:]).any())
            for i, s in enumerate(rows):
                outs[s].append(tuple(t[i, :, :emit[i]].clone() for t in (got if vae else (got,))))
        for s in range(3):
            assert_same(tuple(torch.cat([p[i] for p in outs[s]], dim=1) for i in range(len(outs[s][0]))), want[s], f"session {s}")


def test_refusals_change_no_counter():
    m = new_module("k5")
    xs, _ = case("k5", (24, 24, 24))
    pool = m.pool(3, 8)
    pool.step([(0, xs[0][:, :8], False), (1, xs[1][:, :5], False)])
    pool.step([(0, xs[0][:, 8:13], False), (2, xs[2][:, :3], True)])

    def counters():
        return [(pool.received_frames(s), pool.emitted_frames(s), pool.pending_frames(s)) for s in range(3)]
    state = [(13, 5, 8), (5, 0, 5), (3, 3, 0)]
    assert counters() == state
    good = (1, xs[1][:, 5:9], False)
    with pytest.raises(ValueError, match="duplicate session 0"):
        pool.step([good, (0, xs[0][:, :2], False), (0, None, True)])
    with pytest.raises(ValueError, match="session 3, outside"):
        pool.step([good, (3, xs[0][:, :2], False)])
    with pytest.raises(ValueError, match="max_chunk = 8"):
        pool.step([good, (0, xs[0][:, :9], False)])
    with pytest.raises(PoolStateError, match="session 2 was flushed"):
        pool.step([good, (2, xs[2][:, :1], False)])
    with pytest.raises(ValueError, match=r"\(20, n\)"):
        pool.step([good, (0, xs[0][:19, :4], False)])
    with pytest.raises(ValueError, match=r"\(2, 20, stride\)"):
        pool.step_padded([(1, 4, False), (0, 4, False)], torch.zeros(2, 19, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        pool.step([good, (0, xs[0][:, :4].cpu(), False)])
    assert counters() == state
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        pool.step([good])
    with pytest.raises(RuntimeError, match="inference-only"):
        m.pool(3, 8)
    m.eval()
    assert counters() == state
    # the library's own refusals, past the Python plan: the same statuses and names, and no counter moves
    L = _lib.lib()
    buf = torch.zeros(2, 20, 8, device="cuda")
    out = torch.zeros(2, 8, 16, device="cuda")
    got = (ctypes.c_int64 * 2)(-1, -1)

    def c_step(items, x=buf, z=out, mean=None, cols=16, rstride=8):
        arr = (_lib.WavPoolItem * len(items))(*[_lib.WavPoolItem(s, c, int(f)) for s, c, f in items])
        return L.fv_wnpool_step(pool._h, arr, len(items), x.data_ptr() if x is not None else None, 160, rstride, z.data_ptr() if z is not None else None,
                                mean.data_ptr() if mean is not None else None, None, cols, got, None)
    for items, kw, status, words in (
            ([(1, 4, False), (2, 1, False)], {}, FV_ERR_STATE, ("session 2", "flushed", "item 1")),
            ([(1, 4, False), (1, 0, True)], {}, FV_ERR_INVALID, ("duplicate session 1",)),
            ([(1, 4, False), (7, 1, False)], {}, FV_ERR_INVALID, ("session 7",)),
            ([(1, 4, False), (0, 9, False)], {}, FV_ERR_INVALID, ("9 frames", "max_chunk = 8")),
            ([(1, 4, False)], {"mean": out}, FV_ERR_INVALID, ("d_mean", "vqvae")),
            ([(1, 4, False)], {"x": None}, FV_ERR_INVALID, ("null chunk buffer",)),
            ([(1, 4, False)], {"rstride": 3}, FV_ERR_INVALID, ("row stride 3",)),
            ([(0, 8, True)], {"cols": 15}, FV_ERR_INVALID, ("out_cols = 15", "emits 16")),
            ([(0, 8, True)], {"z": None}, FV_ERR_INVALID, ("null",)),
    ):
        assert c_step(items, **kw) == status, (items, kw)
        msg = L.fv_last_error().decode()
        assert msg.startswith("fv_wnpool_step:") and all(w in msg for w in words), (msg, words)
        assert got[0] == -1 and got[1] == -1
        assert [(L.fv_wnpool_received(pool._h, s), L.fv_wnpool_emitted(pool._h, s), L.fv_wnpool_pending(pool._h, s)) for s in range(3)] == state
    # the good item alone is accepted afterwards: its session had not moved
    assert pool.step([good])[0].shape == (8, 1)
    state[1] = (9, 1, 8)
    assert counters() == state
    with pytest.raises(FishVocError, match="session 3 lies outside"):
        pool.reset(3)
    pool.reset(2)
    assert pool.step([(2, xs[2][:, :8], False)])[0].shape == (8, 0)
    # the engine is rebuilt: the pool is closed, and says so
    m.load_state_dict(m.state_dict())
    with pytest.raises(FishVocError, match="load_state_dict") as e:
        pool.step([good])
    assert e.value.status == FV_ERR_STATE
    with pytest.raises(FishVocError, match="closed"):
        pool.reset(0)
    with m.pool(3, 8) as p2:               # a new one works
        assert p2.step([(0, xs[0][:, :8], True)])[0].shape == (8, 8)
    p3 = m.pool(3, 8)
    m.to("cuda")                           # .to() rebuilds as well
    with pytest.raises(FishVocError, match="closed"):
        p3.step([good])


def make_codec(nq):
    torch.manual_seed(5)
    c = codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, num_quantizers=nq, decoder_depths=(1,),
                          decoder_dims=(32,), encoder="posterior", hidden_channels=32, posterior_layers=4)
    c = c.eval().cuda()
    c.frontend.batch_invariant = True       # the mode in which the front-end's stream and pool have their whole-row bits
    return c


@pytest.mark.parametrize("nq", [1, 3])
def test_codec_encode_pool_gives_encodes_codes(nq):
    c = make_codec(nq)
    lengths = (5000, 1203, 2600)
    g = torch.Generator().manual_seed(nq)
    waves = [(0.1 * torch.randn(n, generator=g)).cuda() for n in lengths]
    want = [c.encode(w[None])[..., 0, :] for w in waves]
    assert all(w.shape == ((w.shape[-1],) if nq == 1 else (3, w.shape[-1])) and w.dtype == torch.int64 for w in want)
    sizes = (1000, 1, 37)
    pos, parts, sent0 = [0, 0, 0], [[], [], []], []
    done = [False] * 3
    with c.encode_pool(3, 1000) as pool:
        step = 0
        while not all(done):
            items = []
            for s in range(3):
                if done[s]:
                    continue
                n = min(sizes[(step + s) % 3], lengths[s] - pos[s])        # staggered: the sessions are never in phase
                last = pos[s] + n == lengths[s]
                items.append((s, waves[s][pos[s]:pos[s] + n], last))
                if s == 0:
                    sent0.append(n)
                pos[s] += n
                done[s] = last
            res = pool.step(items)
            for (s, _, _), r in zip(items, res):
                assert r.dtype == torch.int64 and r.shape[:-1] == want[s].shape[:-1]
                parts[s].append(r)
            step += 1
        for s in range(3):
            got = torch.cat(parts[s], dim=-1)
            assert got.shape == want[s].shape and torch.equal(got, want[s]), f"session {s}"
            assert pool.received_samples(s) == lengths[s] and pool.emitted_frames(s) == want[s].shape[-1]
        assert any(p.shape[-1] == 0 for p in parts[0]) and sum(p.shape[-1] > 0 for p in parts[0]) > 2
        # a refused step moves neither pool
        before = [(pool.wav_pool.received_samples(s), pool.enc_pool.received_frames(s)) for s in range(3)]
        pool.reset(1)
        with pytest.raises(ValueError, match="flushed"):
            pool.step([(1, waves[1][:100], False), (0, waves[0][:100], False)])
        assert [(pool.wav_pool.received_samples(s), pool.enc_pool.received_frames(s)) for s in range(3)] == [before[0], (0, 0), before[2]]
    with c.encode_stream(1, 1000) as st:
        a, sp = 0, []
        for n in sent0:
            sp.append(st.push(waves[0][None, a:a + n]))
            a += n
        sp.append(st.flush())
        got = torch.cat(sp, dim=-1)[..., 0, :]
        assert torch.equal(got, want[0])
