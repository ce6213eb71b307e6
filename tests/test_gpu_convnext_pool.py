"""GPU: the ConvNeXt backbone layer by layer for sessions that advance independently (fv_cnxpool_*, ``ConvNeXtEncoder.layer_pool``), and the
codec's ``encode_pool(layers=True)`` / ``decode_pool(backbone="layers")`` on top.

Every comparison is ``torch.equal`` against the module's own whole-row ``forward`` in batch-invariant mode, of one session's utterance run
alone, unless a test says otherwise.  The modules carry random layer scales and LayerNorm weights (the 1e-6 initialisation hides the
blocks).  Each config picks another instantiation of the depthwise pool kernel or another path of the engine:

  one      in 20, dims (32,), depths (1,)      one block, half a 64-row chunk, R = 6
  two      dims (64, 96), depths (2, 2)        the stage change on packed columns
  c320     dims (320,), depths (1,)            <7, 512, 16> with never-computed chunks
  square   32 -> (32, 64), depths (1, 1)       a C -> C stem: direct sums, the bits of forward with conv_algorithm = "direct"
  default  513 -> (512,) x 6                   the default encoder shape, R = 21
"""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

from vocoder_amd import _lib, codec
from vocoder_amd import synthetic as syn
from vocoder_amd._lib import FishVocError
from vocoder_amd.modules.encoders.convnext import ConvNeXtEncoder, ConvNeXtPool
from vocoder_amd.sessions import PoolStateError

pytestmark = pytest.mark.gpu

# name -> (input_channels, dims, depths, seed)
CONFIGS = {
    "one": (20, (32,), (1,), 1),
    "two": (20, (64, 96), (2, 2), 2),
    "c320": (20, (320,), (1,), 3),
    "square": (32, (32, 64), (1, 1), 6),
    "default": (513, (512,), (6,), 5),
}
NAMES = list(CONFIGS)


def reach(name):
    return 3 * (1 + sum(CONFIGS[name][2]))


def randomise(m, seed):
    """Layer scales, LayerNorm weights and biases that let every block show."""
    from vocoder_amd.modules.encoders.convnext import LayerNorm
    g = torch.Generator().manual_seed(seed)
    norms = {id(p) for mod in m.modules() if isinstance(mod, LayerNorm) for p in mod.parameters()}
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("gamma"):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif id(p) in norms:
                p.copy_((1.0 if n.endswith("weight") else 0.0) + 0.3 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return m


def new_module(name, **kw):
    cin, dims, depths, seed = CONFIGS[name]
    torch.manual_seed(seed)
    m = randomise(ConvNeXtEncoder(input_channels=cin, depths=depths, dims=dims, **kw), seed).eval().cuda()
    m.batch_invariant = True
    if m.stem_has_winograd_form:
        m.conv_algorithm = "direct"
    assert m.stream_is_bit_exact
    return m


@functools.lru_cache(maxsize=None)
def module(name):
    return new_module(name)


@functools.lru_cache(maxsize=None)
def case(name, T, seed=0):
    """(x (C_in, T), the whole-row batch-invariant forward of it alone (C_out, T)): computed once, shared, never written."""
    cin = CONFIGS[name][0]
    x = torch.from_numpy(np.random.default_rng(1000 * seed + T).standard_normal((cin, T)).astype(np.float32)).cuda()
    if T == 0:
        return x, torch.empty((CONFIGS[name][1][-1], 0), device="cuda")
    return x, module(name)(x[None])[0]


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        d = (got - want).abs().amax(dim=0)
        bad = torch.nonzero(d > 0).flatten().tolist()
        nan = torch.nonzero(torch.isnan(got).any(dim=0)).flatten().tolist()
        raise AssertionError(f"{what}: differs at frames {bad[:12]} ({len(bad)} of {got.shape[1]}), NaN at {nan[:12]}, max |d| = {float(d.max()):.3e}")


def random_steps(rng, sessions, lengths, max_chunk):
    """Steps of (session, a, n, flush) that take every session of ``sessions`` through its ``lengths[s]`` frames: random subsets in random
    order, zero-frame items, sessions left out for several steps, and the flush either with the last frames or alone."""
    pos, over, idle, steps = {s: 0 for s in sessions}, set(), {s: 0 for s in sessions}, []
    while len(over) < len(sessions):
        items = []
        for s in sessions:
            if s in over:
                continue
            if idle[s] > 0:
                idle[s] -= 1
                continue
            if rng.random() < 0.15:
                idle[s] = rng.randint(1, 4)                # skipped for several steps
                continue
            left = lengths[s] - pos[s]
            n = min(left, rng.choice([0, 1, max_chunk, rng.randint(0, max_chunk), rng.randint(0, max_chunk)]))
            flush = n == left and rng.random() < 0.5        # with the last frames, or — n = 0 once nothing is left — alone
            items.append((s, pos[s], n, flush))
            pos[s] += n
            if flush:
                over.add(s)
        rng.shuffle(items)
        if items:
            steps.append(items)
    return steps


def drive(pool, xs, steps, outs=None):
    """Runs ``steps`` of (session, a, n, flush) over the utterances ``xs[s]``; every item's shape and the counters are the plan's.
    -> the outputs per session, step by step."""
    outs = {} if outs is None else outs
    for items in steps:
        plan = pool.counters.plan([(s, n, f) for s, _, n, f in items])
        res = pool.step([(s, xs[s][:, a:a + n] if n else None, f) for s, a, n, f in items])
        for (s, a, n, f), k, y in zip(items, plan, res):
            assert y.shape == (pool.out_channels, k) and y.dtype == torch.float32, (s, a, n, f, y.shape, k)
            N = a + n
            E = N if f else max(0, N - pool.lookahead_frames)
            assert (pool.received_frames(s), pool.emitted_frames(s), pool.pending_frames(s)) == (N, E, N - E)
            outs.setdefault(s, []).append(y)
    return outs


def cat(parts, co):
    return torch.cat(parts, dim=1) if parts else torch.empty((co, 0), device="cuda")


# ---- 1: whole-utterance bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_session_has_its_whole_utterances_bits(name):
    m, R = module(name), reach(name)
    lengths = [2 * R + 37, 0, R - 1, R + 5]
    if name == "default":
        lengths = [2 * R + 37, 0, R - 1]
    xs = [case(name, T)[0] for T in lengths]
    big = case(name, lengths[0])[1]
    assert bool(torch.isfinite(big).all()) and float(big.abs().max()) > 0.1
    with m.layer_pool(len(lengths), 8) as pool:
        assert isinstance(pool, ConvNeXtPool) and pool.lookahead_frames == R == m.lookahead_frames and pool.max_frames == 8 + R
        assert pool.sessions == len(lengths) and pool.max_chunk_frames == 8 and pool.state_bytes > 0
        steps = random_steps(random.Random(len(name)), list(range(len(lengths))), lengths, 8)
        kinds = {("flush with frames" if n else "flush alone") if f else ("frames" if n else "zero frames") for st in steps for _, _, n, f in st}
        assert {"frames", "zero frames"} <= kinds and kinds & {"flush with frames", "flush alone"}
        outs = drive(pool, xs, steps)
        for s, T in enumerate(lengths):
            assert_same(cat(outs[s], pool.out_channels), case(name, T)[1], f"session {s}, {T} frames")
        # both kinds of flush, deterministically: with the last frames, and alone
        for s in range(len(lengths)):
            pool.reset(s)
        T = lengths[0]
        T2 = lengths[2]
        outs = drive(pool, {0: xs[0], 2: xs[2]}, [[(0, a, min(8, T - a), a + 8 >= T)] for a in range(0, T, 8)]
                     + [[(2, a, min(8, T2 - a), False)] for a in range(0, T2, 8)] + [[(2, T2, 0, True)]])
        assert_same(cat(outs[0], pool.out_channels), big, "flush with the last frames")
        assert_same(cat(outs[2], pool.out_channels), case(name, lengths[2])[1], "flush alone")


# ---- 2: independence and reuse ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "two", "square"])
def test_a_session_does_not_see_the_others_or_the_item_order(name):
    m, R = module(name), reach(name)
    T = 2 * R + 37
    lengths = [T, R + 9, 2 * R + 11]
    xs = [case(name, n, seed=2)[0] for n in lengths]
    mine = [(0, a, min(n, T - a), a + n >= T) for a, n in zip(range(0, T, 5), [5] * T)]       # session 0: fives, flush with the last
    runs = []
    for trial in range(2):
        rng = random.Random(10 * trial + 1)
        others = random_steps(rng, [1, 2], lengths, 8)
        steps = []
        for i, it in enumerate(mine):
            rest = others[i] if i < len(others) else []
            items = rest + [it] if trial == 0 else [it] + rest[::-1]
            if trial == 1 and len(items) > 1:
                rng.shuffle(items)
            steps.append(items)
        steps += others[len(mine):]
        with m.layer_pool(3, 8) as pool:
            outs = drive(pool, xs, steps)
            runs.append(outs[0])
            for s, n in enumerate(lengths):
                assert_same(cat(outs[s], pool.out_channels), case(name, n, seed=2)[1], f"trial {trial} session {s}")
            if trial == 1:
                # the slots' rings are stale now: a second, other utterance in slot 1 and a NaN one before it in slot 2
                pool.reset(1), pool.reset(2)
                x2, want2 = case(name, R + 14, seed=3)
                bad = torch.full_like(xs[2], float("nan"))
                drive(pool, {2: bad}, [[(2, a, min(8, lengths[2] - a), a + 8 >= lengths[2])] for a in range(0, lengths[2], 8)])
                pool.reset(2)
                outs = drive(pool, {1: x2, 2: x2}, [[(1, a, min(7, R + 14 - a), a + 7 >= R + 14), (2, a, min(7, R + 14 - a), False)]
                                                    for a in range(0, R + 14, 7)] + [[(2, R + 14, 0, True)]])
                assert_same(cat(outs[1], pool.out_channels), want2, "a second utterance in a stale slot")
                assert_same(cat(outs[2], pool.out_channels), want2, "after an all-NaN utterance")
    assert len(runs[0]) == len(runs[1]) == len(mine)
    for i, (a, b) in enumerate(zip(*runs)):
        assert a.shape == b.shape and torch.equal(a, b), f"step {i}"


# ---- 3: ring wrap at the smallest rings ----------------------------------------------------------------------------------------------------------
def test_many_laps_through_the_smallest_rings():
    from vocoder_amd.modules.encoders.convnext import pool_ring_cap
    cap = pool_ring_cap(1, 1)
    assert cap == 16
    fast, slow = 5 * cap * 3 + 7, 5 * cap + 3            # paces 1 and 1 every third step: both go through their rings five times
    xs = [case("one", fast)[0], case("one", slow)[0]]
    steps = []
    for t in range(fast):
        items = [(0, t, 1, t == fast - 1)]
        if t % 3 == 0 and t // 3 < slow:
            items.insert(t % 2, (1, t // 3, 1, False))
        steps.append(items)
    steps.append([(1, slow, 0, True)])
    with module("one").layer_pool(2, 1) as pool:
        outs = drive(pool, xs, steps)
        assert_same(cat(outs[0], pool.out_channels), case("one", fast)[1], "pace 1")
        assert_same(cat(outs[1], pool.out_channels), case("one", slow)[1], "pace 1 / 3")


# ---- 4: tile edges in one launch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "two", "c320"])
def test_tile_edges_in_one_launch(name):
    m, R = module(name), reach(name)
    MAX = 40
    lengths = [R + MAX, R + 4, 5 + R + 3, 5]
    xs = [case(name, n, seed=4)[0] for n in lengths]
    with m.layer_pool(4, MAX) as pool:
        outs = drive(pool, xs, [[(0, 0, R, False), (1, 0, R + 3, False), (3, 0, 5, False)]])
        assert all(y.shape[1] == k for y, k in zip([outs[0][0], outs[1][0], outs[3][0]], [0, 3, 0]))
        # one step: more than 32 new columns at every level (a flush with max_chunk frames after R pending); a single frame; 5 frames that
        # give the stem 2 columns, which block 1 only files (no output column yet); a flush with no frames
        step = [(0, R, MAX, True), (1, R + 3, 1, False), (2, 0, 5, False), (3, 5, 0, True)]
        assert pool.counters.plan([(s, n, f) for s, _, n, f in step]) == [R + MAX, 1, 0, 5] and R + MAX > 32
        drive(pool, xs, [step], outs)
        drive(pool, xs, [[(2, 5, R + 3, True), (1, R + 4, 0, True)]], outs)
        for s, n in enumerate(lengths):
            assert_same(cat(outs[s], pool.out_channels), case(name, n, seed=4)[1], f"session {s}")


# ---- 5: more items than one table --------------------------------------------------------------------------------------------------------------------
def test_a_step_of_more_than_one_launch_table():
    m, R = module("one"), reach("one")
    table = _lib.lib().fv_cnxpool_table_size()
    S = table + 3
    first = [1 + (5 * i) % 8 for i in range(S)]
    second = [1 + (3 * i + 2) % 8 for i in range(S)]
    xs = [case("one", a + b, seed=5 + i % 3)[0] for i, (a, b) in enumerate(zip(first, second))]
    with m.layer_pool(S, 8) as pool:
        order = list(range(S))
        random.Random(3).shuffle(order)
        outs = drive(pool, xs, [[(s, 0, first[s], False) for s in order], [(s, first[s], second[s], True) for s in order[::-1]]])
        # every level has work in the second step: T (1 + L) + 2 + 2 L + 2 (stages - 1) + 1 + ceil(count / 32), T = 2, L = 1, one stage
        T, L = 2, 1
        assert -(-S // table) == T
        assert pool.last_step_launches == T * (1 + L) + 2 + 2 * L + 0 + 1 + -(-S // 32)
        for s in range(S):
            assert_same(cat(outs[s], pool.out_channels), case("one", first[s] + second[s], seed=5 + s % 3)[1], f"session {s}")


def test_launches_with_one_table_are_the_streams_plus_the_crop():
    for name, want in (("default", 22 + 1), ("two", 1 + 2 + 4 * 3 + 2 + 1 + 1)):
        R = reach(name)
        x = case(name, R + 8)[0]
        with module(name).layer_pool(2, 8) as pool:
            drive(pool, [x, x], [[(0, a, n, False), (1, a, n, False)] for a, n in zip(range(0, R, 8), [8] * R)])
            pool.step([(0, x[:, -8:], False)])             # past R frames: every level has a new column
            assert pool.last_step_launches == want, name
            pool.step([(1, None, False)])                  # nothing new at any level: the crop's launch alone (a row of zero columns: none)
            assert pool.last_step_launches == 0


# ---- 6: padding and zeros ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "two"])
def test_padding_is_never_read_and_the_rest_of_out_is_zero(name):
    m, R = module(name), reach(name)
    cin = CONFIGS[name][0]
    lengths = [R + 21, R + 6, 3]
    xs = [case(name, n, seed=6)[0] for n in lengths]
    with m.layer_pool(3, 8) as pool:
        pos, parts = [0, 0, 0], [[], [], []]
        sizes = ([8, 3, 8], [5, 8, 1], [3])
        step = 0
        while any(p < n for p, n in zip(pos, lengths)):
            items, rows = [], []
            for s in (2, 0, 1):
                if pos[s] < lengths[s]:
                    n = min(sizes[s][step % len(sizes[s])], lengths[s] - pos[s])
                    items.append((s, n, pos[s] + n == lengths[s]))
                    rows.append(xs[s][:, pos[s]:pos[s] + n])
                    pos[s] += n
            # a strided view into a wider NaN-filled buffer, NaN after every item's own frames
            wide = torch.full((len(items), cin + 2, 8 + 5), float("nan"), device="cuda")
            for i, r in enumerate(rows):
                wide[i, 1:-1, 2:2 + r.shape[1]] = r
            chunks = wide[:, 1:-1, 2:10]
            assert not chunks.is_contiguous()
            plan = pool.counters.plan(items)
            out = torch.full((len(items), pool.out_channels, max(plan) + 3), float("nan"), device="cuda")
            got, emit = pool.step_padded(items, chunks, out)
            assert got is out and emit == plan
            assert not bool(torch.isnan(out).any())                             # every element written
            for i, ((s, _, _), k) in enumerate(zip(items, emit)):
                assert bool((out[i, :, k:] == 0).all()) and not bool(torch.signbit(out[i, :, k:]).any())
                parts[s].append(out[i, :, :k].clone())
            step += 1
        for s, n in enumerate(lengths):
            assert_same(cat(parts[s], pool.out_channels), case(name, n, seed=6)[1], f"session {s}")


# ---- 7: refusals change nothing -------------------------------------------------------------------------------------------------------------------
def test_refused_steps_change_nothing():
    m, R = module("two"), reach("two")
    T = 2 * R + 20
    x, want = case("two", T, seed=7)
    with m.layer_pool(3, 8) as pool:
        outs = drive(pool, [x, x, x], [[(0, 0, 8, False), (1, 0, 3, True)]])
        state = lambda: [(pool.received_frames(s), pool.emitted_frames(s), pool.pending_frames(s)) for s in range(3)]      # noqa: E731
        before = state()
        c = x[:, 8:16]
        with pytest.raises(ValueError, match="duplicate session 0"):
            pool.step([(0, c, False), (2, c, False), (0, c, False)])
        with pytest.raises(PoolStateError, match="flushed"):
            pool.step([(0, c, False), (1, c, False)])
        with pytest.raises(ValueError, match="max_chunk"):
            pool.step([(2, c, False), (0, x[:, 8:17], False)])
        with pytest.raises(RuntimeError, match="CUDA/HIP"):
            pool.step([(0, c.cpu(), False)])
        with pytest.raises(ValueError, match="expected"):
            pool.step([(0, x[:5, 8:16], False)])
        with pytest.raises(ValueError, match="expected out"):
            pool.step_padded([(0, 8, False)], c[None].contiguous(), torch.empty(1, pool.out_channels + 1, 8, device="cuda"))
        # past the Python plan, to the library's own refusals
        chunks = torch.zeros(2, 20, 30, device="cuda")
        with pytest.raises(FishVocError, match="fv_cnxpool_step.*out_cols = 2.*item 1 \\(session 2\\)"):
            pool.step_padded([(0, 8, False), (2, 8, True)], chunks, torch.empty(2, pool.out_channels, 2, device="cuda"))
        assert state() == before
        L, got = _lib.lib(), (ctypes.c_int64 * 2)(-7, -7)
        arr = (_lib.WavPoolItem * 2)(_lib.WavPoolItem(0, 8, 0), _lib.WavPoolItem(0, 1, 0))
        out = torch.empty(2, pool.out_channels, 8, device="cuda")
        for bad, word in ((arr, "duplicate session 0"),
                          ((_lib.WavPoolItem * 2)(_lib.WavPoolItem(0, 8, 0), _lib.WavPoolItem(1, 1, 0)), "flushed"),
                          ((_lib.WavPoolItem * 2)(_lib.WavPoolItem(2, 8, 0), _lib.WavPoolItem(0, 9, 0)), "max_chunk = 8"),
                          ((_lib.WavPoolItem * 2)(_lib.WavPoolItem(2, 8, 0), _lib.WavPoolItem(3, 1, 0)), "session 3")):
            rc = L.fv_cnxpool_step(pool._h, bad, 2, chunks.data_ptr(), chunks.stride(0), chunks.stride(1), out.data_ptr(), 8, got, None)
            assert rc != 0 and word in L.fv_last_error().decode() and list(got) == [-7, -7], (word, L.fv_last_error().decode())
        rc = L.fv_cnxpool_step(pool._h, arr, 1, chunks.data_ptr(), chunks.stride(0), 7, out.data_ptr(), 8, got, None)
        assert rc == _lib.FV_ERR_INVALID and "row stride 7" in L.fv_last_error().decode()
        assert state() == before
        torch.cuda.synchronize()
        # the next valid steps still give forward's bits
        drive(pool, [x, x, x], [[(0, a, min(8, T - a), a + 8 >= T)] for a in range(8, T, 8)], outs)
        assert_same(cat(outs[0], pool.out_channels), want, "after the refused steps")


def test_create_refusals_by_name():
    from vocoder_amd.modules.generators import HiFiGANGenerator
    with pytest.raises(FishVocError, match="fv_cnxpool_create.*kernel_size"):
        new_module("one", kernel_size=5).layer_pool(2, 8)
    m = new_module("one")
    m.precision = "f16x3"
    with pytest.raises(FishVocError, match="fv_cnxpool_create.*f16x3"):
        m.layer_pool(2, 8)
    for sessions, chunk, word in ((0, 8, "sessions = 0"), (65536, 8, "sessions"), (2, 0, "max_chunk"), (60000, 1 << 16, "32-bit addressing")):
        with pytest.raises(FishVocError, match=word):
            module("one").layer_pool(sessions, chunk)
    cfg = dict(hop_length=64, upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4], resblock_kernel_sizes=[3, 7, 11],
               resblock_dilation_sizes=[[1, 3, 5]] * 3, num_mels=80, upsample_initial_channel=128, use_template=False, pre_conv_kernel_size=7,
               post_conv_kernel_size=7)
    gen = HiFiGANGenerator(**cfg)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(cfg, seed=1).items()}, strict=True)
    eng = gen.eval().cuda().engine(torch.device("cuda", torch.cuda.current_device()))
    L, p = _lib.lib(), ctypes.c_void_p()
    assert L.fv_cnxpool_create(eng._h, 2, 8, ctypes.byref(p)) == _lib.FV_ERR_INVALID and not p.value
    assert "FV_MODEL_CONVNEXT" in L.fv_last_error().decode()


def test_a_rebuilt_engine_closes_the_pool():
    m = new_module("one")
    pool = m.layer_pool(2, 8)
    m.load_state_dict(m.state_dict())
    with pytest.raises(FishVocError, match="closed"):
        pool.step([(0, torch.zeros(20, 4, device="cuda"), False)])


# ---- 8, 9: the codec: the tiny one the other tests use (n_fft 64, hop 16, latent 32, K 48) -------------------------------------------------
def make_codec(nq, **kw):
    torch.manual_seed(5)
    kw.setdefault("decoder_depths", (1,))
    kw.setdefault("decoder_dims", (32,))
    c = codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, num_quantizers=nq, encoder_depths=(2,),
                          encoder_dims=(32,), **kw)
    randomise(c.encoder, 7), randomise(c.decoder.backbone, 8)
    c = c.eval().cuda()
    c.encoder.batch_invariant = c.frontend.batch_invariant = True
    return c


@pytest.mark.parametrize("nq", [1, 3])
def test_codec_encode_pool_by_layers_gives_encodes_codes(nq):
    c = make_codec(nq)
    lengths = (5000, 1203, 2600)
    g = torch.Generator().manual_seed(nq)
    waves = [(0.1 * torch.randn(n, generator=g)).cuda() for n in lengths]
    want = [c.encode(w[None])[..., 0, :] for w in waves]
    assert all(w.shape == ((w.shape[-1],) if nq == 1 else (3, w.shape[-1])) and w.dtype == torch.int64 for w in want)
    sizes = (1000, 1, 37)
    pos, parts, done = [0, 0, 0], [[], [], []], [False] * 3
    with pytest.raises(ValueError, match="pool form is not built"):
        c.encode_pool(3, 1000)
    with c.encode_pool(3, 1000, layers=True) as pool:
        assert isinstance(pool.enc_pool, ConvNeXtPool)
        step = 0
        while not all(done):
            items = []
            for s in range(3):
                if done[s]:
                    continue
                n = min(sizes[(step + s) % 3], lengths[s] - pos[s])        # staggered: the sessions are never in phase
                last = pos[s] + n == lengths[s]
                items.append((s, waves[s][pos[s]:pos[s] + n], last))
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
    c.encoder.batch_invariant = False
    with pytest.raises(ValueError, match="not bit-exact"):
        c.encode_pool(3, 1000, layers=True)


WINDOW_TOL = 2e-5      # of the output's peak: tests/test_gpu_codec_decode.py's bound for a decode_pool against decode()


def decode_steps(lengths):
    """(session, a, n, flush) steps for three sessions: staggered sizes, the third one arriving late in one flushing item."""
    steps, pos = [], [0, 0]
    while pos[0] < lengths[0]:
        t, items = len(steps), []
        for s, sizes in ((0, [8, 1, 5, 8]), (1, [3, 0, 8])):
            if pos[s] < lengths[s]:
                n = min(sizes[t % len(sizes)], lengths[s] - pos[s])
                items.append((s, pos[s], n, pos[s] + n == lengths[s]))
                pos[s] += n
        if t == 6:
            items.insert(0, (2, 0, lengths[2], True))
        steps.append(items[::-1] if t % 2 else items)
    return steps


@pytest.mark.parametrize("nq", [1, 2])
def test_decode_pool_by_layers(nq):
    """``backbone="layers"``: per session bit-identical to ``head.session_pool`` fed, under the same schedule, the frames of the backbone's
    whole-row batch-invariant direct-sum ``forward`` of ``from_codes(codes)``; and, with only the head windowed, within 2e-5 of
    ``decode()``'s peak."""
    MAX = 8
    m = make_codec(nq, decoder_depths=(1, 1), decoder_dims=(32, 64))
    bb, head = m.decoder.backbone, m.decoder.head
    with m.decode_pool(3, MAX, backbone="layers") as dp:
        A = bb.lookahead_frames
        assert dp.backbone == "layers" and dp.codes.lookahead_frames == A == 9 and isinstance(dp.codes.pool, ConvNeXtPool)
        assert dp.lookahead_frames == A + dp.head.lookahead_frames and dp.head.max_chunk_frames == MAX + A and (dp.hop, dp.out_channels) == (16, 1)
        assert dp.ring_bytes > 0
        lengths = [2 * dp.lookahead_frames + 21, dp.lookahead_frames + 3, 4]
        g = torch.Generator().manual_seed(6)
        utts = [torch.randint(0, 48, (n,) if nq == 1 else (nq, n), generator=g).cuda() for n in lengths]
        as_batch = lambda u: u[None] if nq == 1 else u[:, None, :]      # noqa: E731
        assert bb.stem_has_winograd_form
        bb.batch_invariant, bb.conv_algorithm = True, "direct"
        frames = [bb(m.vq.from_codes(as_batch(u))[0])[0] for u in utts]
        bb.batch_invariant, bb.conv_algorithm = False, "auto"      # the layer pool has those bits whatever the module's settings
        E, outs = [0, 0, 0], [[] for _ in lengths]
        with head.session_pool(3, MAX + A) as p2:
            for items in decode_steps(lengths):
                got = dp.step([(s, utts[s][..., a:a + n] if n else None, fl) for s, a, n, fl in items])
                feed = []
                for s, a, n, fl in items:
                    E1 = a + n if fl else max(E[s], a + n - A)
                    feed.append((s, frames[s][:, E[s]:E1].contiguous() if E1 > E[s] else None, fl))
                    E[s] = E1
                want = p2.step(feed)
                for (s, a, n, fl), x, y in zip(items, got, want):
                    assert x.shape == y.shape and torch.equal(x, y), (s, a, n, fl)
                    outs[s].append(x)
            before = [(dp.received_frames(s), dp.emitted_frames(s), dp.codes.emitted_frames(s)) for s in range(3)]
            with pytest.raises(ValueError, match="flushed"):                     # planned before any stage is launched: no pool moves
                dp.step([(1, utts[1][..., :2], False), (0, utts[0][..., :2], False)])
            with pytest.raises(ValueError, match="max_chunk"):
                dp.step([(0, utts[0][..., :MAX + 1], False)])
            assert [(dp.received_frames(s), dp.emitted_frames(s), dp.codes.emitted_frames(s)) for s in range(3)] == before
        for s, n in enumerate(lengths):
            y, whole = torch.cat(outs[s], dim=1), m.decode(as_batch(utts[s]))[0]
            assert y.shape == whole.shape == (1, n * 16) and dp.received_frames(s) == dp.emitted_frames(s) == n
            d, peak = float((y - whole).abs().max()), float(whole.abs().max())
            print(f"decode_pool(backbone='layers') n_q={nq} session {s}: max|d| to decode = {d:.3e}, peak = {peak:.3e}, ratio = {d / peak:.3e}")
            assert d <= WINDOW_TOL * peak
        dp.reset(2)
        assert dp.received_frames(2) == 0 and dp.emitted_frames(2) == 0
        assert torch.equal(dp.step([(2, utts[2], True)])[0], outs[2][0])


def test_decode_pool_by_windows_is_what_it_was():
    MAX = 8
    m = make_codec(2, decoder_depths=(1, 1), decoder_dims=(32, 64))
    with m.decode_pool(3, MAX) as dp, m.decode_pool(3, MAX, backbone="window") as dp2:
        assert dp.backbone == dp2.backbone == "window" and type(dp.codes).__name__ == type(dp2.codes).__name__ == "CodeSessionPool"
        lengths = [2 * dp.lookahead_frames + 21, dp.lookahead_frames + 3, 4]
        g = torch.Generator().manual_seed(6)
        utts = [torch.randint(0, 48, (2, n), generator=g).cuda() for n in lengths]
        with m.decoder.backbone.session_pool(3, MAX) as p1, m.decoder.head.session_pool(3, MAX + dp.codes.lookahead_frames) as p2:
            for items in decode_steps(lengths):
                step = [(s, utts[s][:, a:a + n] if n else None, fl) for s, a, n, fl in items]
                got, got2 = dp.step(step), dp2.step(step)
                z = p1.step([(s, m.vq.from_codes(utts[s][:, None, a:a + n])[0][0] if n else None, fl) for s, a, n, fl in items])
                want = p2.step([(s, zi if zi.shape[1] else None, fl) for (s, _, _, fl), zi in zip(items, z)])
                for x, x2, y in zip(got, got2, want):
                    assert x.shape == y.shape and torch.equal(x, y) and torch.equal(x2, y)
    with pytest.raises(ValueError, match="'window' or 'layers'"):
        m.decode_pool(3, MAX, backbone="rings")
    with pytest.raises(ValueError, match="two-stage"):
        codec.CodecDecodePool(m.decoder.head, m.vq, 3, MAX, "layers")
