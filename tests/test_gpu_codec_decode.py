"""GPU: the decode direction of the codec served chunk by chunk — code streams and code session pools (fv_stream_*_codes, fv_pool_*_codes,
vocoder_amd.engine.CodeStream / CodeSessionPool), VQVAECodec.decode_stream / decode_pool, UnifyGenerator.decode_stream and the command
line's --chunk-frames.  The yardstick is the chain that existed before: vq.from_codes into a float Stream / SessionPool, bit for bit; and the
whole-row decode within the project's window bound."""
import ctypes
import functools

import numpy as np
import pytest

from vocoder_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WINDOW_TOL = 2e-5      # of the output's peak: the project's bound for a window against the whole clip
B, K_CODES, MAX_CHUNK = 2, 48, 8
HIFI = dict(hop_length=16, upsample_rates=[4, 2, 2], upsample_kernel_sizes=[8, 4, 4], resblock_kernel_sizes=[3, 7, 11],
            resblock_dilation_sizes=[[1, 3, 5]] * 3, upsample_initial_channel=64, use_template=False, pre_conv_kernel_size=7,
            post_conv_kernel_size=7)
# (decoder, D, n_q, codes of -1 pushed with validate=False): D = 32 lies below one 64-channel slice, D = 72 has a partial last slice
CASES = [("head", 32, 1, False), ("head", 32, 3, False), ("head", 72, 1, True), ("head", 72, 3, False), ("hifigan", 32, 3, True),
         ("hifigan", 72, 1, False)]
IDS = [f"{d}-D{D}-q{q}{'-holes' if h else ''}" for d, D, q, h in CASES]


def _t(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def _quantiser(D, nq, seed, K=K_CODES):
    from vocoder_amd.modules.quantizers import ResidualVectorQuantization, VectorQuantization
    rng = np.random.default_rng(seed)
    embeds = [(0.5 * rng.standard_normal((K, D))).astype(np.float32) for _ in range(nq)]
    if nq > 1:
        m = ResidualVectorQuantization(num_quantizers=nq, dim=D, codebook_size=K, kmeans_init=False)
        sd = {f"layers.{q}._codebook.embed": torch.from_numpy(e) for q, e in enumerate(embeds)}
    else:
        m = VectorQuantization(dim=D, codebook_size=K, kmeans_init=False)
        sd = {"_codebook.embed": torch.from_numpy(embeds[0])}
    m.load_state_dict({**m.state_dict(), **sd}, strict=True)
    return m.eval().cuda()


@functools.lru_cache(maxsize=None)
def _decoder(kind, D):
    from vocoder_amd.modules.generators import HiFiGANGenerator, ISTFTHead
    if kind == "head":
        cfg = dict(dim=D, n_fft=64, hop_length=16, win_length=64, padding="same")
        m, sd = ISTFTHead(**cfg), syn.istft_head_state_dict(cfg, seed=11)
    else:
        cfg = dict(HIFI, num_mels=D)
        m, sd = HiFiGANGenerator(**cfg), syn.hifigan_state_dict(cfg, seed=5)
    m.load_state_dict(_t(sd), strict=True)
    return m.eval().cuda()


@functools.lru_cache(maxsize=None)
def _setup(kind, D, nq, holes=False):
    """(decoder module, quantiser, codes (B, T) or (n_q, B, T) int64 of an utterance of 2R + 37 frames, R)"""
    dec, vq = _decoder(kind, D), _quantiser(D, nq, seed=D + nq)
    R = dec.engine(torch.device("cuda", torch.cuda.current_device())).reach_frames
    T = 2 * R + 37
    g = torch.Generator().manual_seed(100 * D + nq)
    codes = torch.randint(0, K_CODES, (nq, B, T), generator=g)
    if holes:      # frames without a code in some layer, and (n_q = 1) without any
        codes[torch.rand((nq, B, T), generator=g) < 0.15] = -1
    codes = codes.cuda()
    return dec, vq, (codes[0] if nq == 1 else codes), R


def _spans(T):
    """1, 8, 3, 8, 8, ... up to T: with max_chunk = 8 the ring of 2R + 8 frames wraps several times and windows straddle the wrap"""
    sizes, at, out = [1, 8, 3], 0, []
    while at < T:
        n = min(sizes[len(out)] if len(out) < len(sizes) else MAX_CHUNK, T - at)
        out.append((at, at + n))
        at += n
    return out


def _whole(dec, vq, codes):
    y = dec(vq.from_codes(codes)[0])
    return y[:, None, :] if y.ndim == 2 else y


def _within_window_bound(got, whole, what):
    peak = float(whole.abs().max())
    err = float((got - whole).abs().max())
    print(f"{what}: max|d| = {err:.3e}, peak = {peak:.3e}, bound = {WINDOW_TOL * peak:.3e}")
    assert got.shape == whole.shape and err <= WINDOW_TOL * peak, (what, err, peak)


# ---- 1 / 2: the code stream against the float stream (bits) and against the whole-row decode (window bound) ---------------------------------
@pytest.mark.parametrize("kind,D,nq,holes", CASES, ids=IDS)
def test_code_stream_has_the_float_streams_bits_and_decodes_the_utterance(kind, D, nq, holes):
    dec, vq, codes, R = _setup(kind, D, nq, holes)
    T = codes.shape[-1]
    assert T == 2 * R + 37
    outs = []
    with dec.code_stream(vq, B, MAX_CHUNK) as cs, dec.stream(B, MAX_CHUNK) as fs:
        assert (cs.context_frames, cs.lookahead_frames, cs.hop) == (fs.context_frames, fs.lookahead_frames, fs.hop) == (R, R, 16)
        assert T > 2 * R + MAX_CHUNK, "the ring wraps"
        for a, b in _spans(T):
            got = cs.push(codes[..., a:b], validate=not holes)
            want = fs.push(vq.from_codes(codes[..., a:b])[0])
            assert got.shape == want.shape and torch.equal(got, want), (a, b)
            assert (cs.received_frames, cs.emitted_frames, cs.pending_frames) == (fs.received_frames, fs.emitted_frames, fs.pending_frames)
            outs.append(got)
        got, want = cs.flush(), fs.flush()
        assert got.shape[2] == R * 16 and torch.equal(got, want)
        outs.append(got)
    _within_window_bound(torch.cat(outs, dim=2), _whole(dec, vq, codes), f"code stream {kind} D={D} n_q={nq}")


def test_code_stream_takes_int32_and_the_first_layers_alone_and_validates():
    dec, vq, codes, R = _setup("head", 72, 3)
    with dec.code_stream(vq, B, MAX_CHUNK) as cs, dec.stream(B, MAX_CHUNK) as fs, dec.code_stream(vq, B, MAX_CHUNK) as c2:
        for a, b in _spans(R + 20):
            want = fs.push(vq.from_codes(codes[:2, :, a:b])[0])                 # two of three layers, as from_codes takes them
            assert torch.equal(cs.push(codes[:2, :, a:b].to(torch.int32)), want)
            assert torch.equal(c2.push(codes[:2, :, a:b]), want)
        before = (cs.received_frames, cs.emitted_frames, cs.pending_frames)
        for bad in (K_CODES, -2):
            chunk = codes[:, :, :4].clone()
            chunk[1, 0, 2] = bad
            with pytest.raises(IndexError, match="out of range"):
                cs.push(chunk)
            with pytest.raises(IndexError):
                vq.from_codes(chunk) if bad > 0 else cs.push(chunk)
        assert (cs.received_frames, cs.emitted_frames, cs.pending_frames) == before
        # validate=False: a code outside [0, K) contributes nothing, exactly as a -1
        a, b = R + 20, R + 24
        chunk, holes = codes[:, :, a:b].clone(), codes[:, :, a:b].clone()
        chunk[1, 0, 2], holes[1, 0, 2] = K_CODES + 7, -1
        assert torch.equal(cs.push(chunk, validate=False), c2.push(holes))
        assert torch.equal(cs.flush(), c2.flush())


# ---- 3: the code pool against the float pool (bits) and every session against its whole decode ------------------------------------------------
def _pool_schedule(R, A):
    """Steps for 4 slots: ("step", [(slot, utterance, first frame, n, flush)]) / ("reset", slot).  Utterance 0 is long and ends with a bare
    flush; 1 ends together with its last frames; 2 is a whole short utterance in one item, placed in a step where a longer row exists (a group
    of its own); 3 ends, its slot is reset and serves utterance 4.  Chunk sizes differ within a step (0 included) and items are permuted."""
    lengths = [2 * R + 37, R + 11, 5, 9, R + 13]
    sizes = {0: [8, 3, 0, 8, 1, 8, 8, 5], 1: [2, 8, 0, 7, 8], 3: [4, 5], 4: [8, 6, 0, 8]}
    pos, live, slot_utt = {0: 0, 1: 0, 3: 0}, {0, 1, 3}, {0: 0, 1: 1, 3: 3}
    out, t, short_done, ended = [], 0, False, set()
    while live or not short_done:
        items = []
        for s in sorted(live):
            u = slot_utt[s]
            if u in ended:                                   # utterance 0: the bare flush one step after its last frames
                items.append((s, u, lengths[u], 0, True))
                continue
            n = min(sizes[u][t % len(sizes[u])], lengths[u] - pos[s])
            last = pos[s] + n == lengths[u]
            items.append((s, u, pos[s], n, last and u != 0))
            pos[s] += n
            if last and u == 0:
                ended.add(0)
        if not short_done and pos[0] > A + 2 * MAX_CHUNK and any(s == 0 and n > 0 for s, _, _, n, _ in items):   # slot 0 has a longer row
            items.append((2, 2, 0, lengths[2], True))
            short_done = True
        items = items[t % len(items):] + items[:t % len(items)]          # permuted order
        out.append(("step", items))
        for s, u, _, _, flush in items:
            if flush and s in live:
                if u == 3:
                    out.append(("reset", 3))
                    slot_utt[3], pos[3] = 4, 0
                else:
                    live.discard(s)
        t += 1
        assert t < 200
    return lengths, out


@pytest.mark.parametrize("kind,D,nq", [("head", 72, 3), ("hifigan", 32, 1)])
def test_code_pool_has_the_float_pools_bits_and_decodes_every_session(kind, D, nq):
    dec, vq, _, R = _setup(kind, D, nq)
    with dec.code_pool(vq, 4, MAX_CHUNK) as cp, dec.session_pool(4, MAX_CHUNK) as fp:
        lengths, sched = _pool_schedule(R, cp.lookahead_frames)
        g = torch.Generator().manual_seed(7)
        utts = [torch.randint(0, K_CODES, (nq, n), generator=g).cuda() for n in lengths]
        outs = [[] for _ in lengths]
        saw_own_group = saw_empty_chunk = False
        for what, arg in sched:
            if what == "reset":
                cp.reset(arg), fp.reset(arg)
                continue
            plan = cp.state.plan([(s, n, fl) for s, _, _, n, fl in arg])
            saw_own_group |= len(plan.groups) > 1
            saw_empty_chunk |= any(n == 0 and not fl for _, _, _, n, fl in arg)
            code_items, float_items = [], []
            for s, u, a, n, fl in arg:
                c = utts[u][:, a:a + n]
                code_items.append((s, (c[0] if nq == 1 else c) if n else None, fl))
                float_items.append((s, vq.from_codes(c[:, None, :])[0][0] if n else None, fl))
            got, want = cp.step(code_items), fp.step(float_items)
            for i, (s, u, a, n, fl) in enumerate(arg):
                assert got[i].shape == want[i].shape and torch.equal(got[i], want[i]), (s, u, a, n, fl)
                assert (cp.received_frames(s), cp.emitted_frames(s), cp.pending_frames(s)) == \
                       (fp.received_frames(s), fp.emitted_frames(s), fp.pending_frames(s))
                outs[u].append(got[i])
        assert saw_own_group and saw_empty_chunk
        for u, n in enumerate(lengths):
            whole = _whole(dec, vq, utts[u][:, None, :])[0]
            _within_window_bound(torch.cat(outs[u], dim=1), whole, f"code pool {kind} utterance {u} ({n} frames)")


def test_a_step_of_more_than_one_launch_table():
    """36 items on a 40-slot pool (kPoolBlock = 32 entries travel per launch): 34 whole utterances of 7 frames in one group and 2 items that
    only file their frames; the next step ends those two."""
    dec, vq, _, R = _setup("head", 32, 1)
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, K_CODES, (36, 7), generator=g).cuda()
    with dec.code_pool(vq, 40, MAX_CHUNK) as cp, dec.session_pool(40, MAX_CHUNK) as fp:
        slots = [39 - s for s in range(36)]
        z = vq.from_codes(codes[None])[0]                                        # (36, D, 7): row i is item i's frames
        first = [(slots[i], i, 0, 3, False) if i in (5, 33) else (slots[i], i, 0, 7, True) for i in range(36)]
        second = [(slots[i], i, 3, 4, True) for i in (33, 5)]
        for arg in (first, second):
            got = cp.step([(s, codes[i, a:a + n], fl) for s, i, a, n, fl in arg])
            want = fp.step([(s, z[i, :, a:a + n], fl) for s, i, a, n, fl in arg])
            assert len(got) == len(arg)
            for x, y in zip(got, want):
                assert x.shape == y.shape and torch.equal(x, y)
        assert all(cp.emitted_frames(s) == 7 for s in slots) and got[0].shape == (1, 7 * 16)


# ---- 4: a refused step moves nothing -------------------------------------------------------------------------------------------------------
def _counters(pool, S):
    return [(pool.received_frames(s), pool.emitted_frames(s), pool.pending_frames(s), pool.state.flushed[s]) for s in range(S)]


def test_a_refused_pool_step_moves_nothing():
    from vocoder_amd import _lib
    from vocoder_amd._lib import FishVocError
    dec, vq, codes, R = _setup("head", 72, 3)
    L = _lib.lib()
    c = codes[:, 0]                                                              # (n_q, T): one session's codes
    with dec.code_pool(vq, 3, MAX_CHUNK) as cp, dec.code_pool(vq, 3, MAX_CHUNK) as twin, dec.session_pool(3, MAX_CHUNK) as fp:
        def both(items):
            got, want = cp.step(items), twin.step(items)
            assert all(torch.equal(x, y) for x, y in zip(got, want))
        both([(0, c[:, :8], False), (1, c[:, :5], True), (2, c[:, :8], False)])
        both([(0, c[:, 8:16], False), (2, c[:, 8:11], False)])
        before = _counters(cp, 3)
        stream = int(torch.cuda.current_stream().cuda_stream)
        with pytest.raises(ValueError, match="duplicate session 0"):
            cp.step([(0, c[:, 16:20], False), (2, c[:, 11:12], False), (0, c[:, 20:21], False)])
        with pytest.raises(ValueError, match="max_chunk_frames"):
            cp.step([(2, c[:, 11:12], False), (0, c[:, 16:16 + MAX_CHUNK + 1], False)])
        with pytest.raises(ValueError, match="flushed"):
            cp.step([(0, c[:, 16:20], False), (1, c[:, 5:6], False)])
        # the library's own refusals, past the Python plan: the same step through the entry points themselves
        items = (_lib.PoolItem * 3)(_lib.PoolItem(0, 4, 0), _lib.PoolItem(2, 1, 0), _lib.PoolItem(0, 1, 0))
        c32 = torch.zeros((3, 3, 4), dtype=torch.int32, device="cuda")
        out = torch.zeros((3, 1, 8 * 16), device="cuda")
        got = (ctypes.c_int64 * 3)()
        tail = (out.data_ptr(), 8, got, cp._ws.data_ptr(), cp._ws.numel() * 4, stream)
        assert L.fv_codepool_step(cp._h, items, 3, c32.data_ptr(), None, 4, *tail) == _lib.FV_ERR_INVALID
        assert b"duplicate session 0" in L.fv_last_error()
        items[2] = _lib.PoolItem(1, 1, 0)
        assert L.fv_codepool_step(cp._h, items, 3, c32.data_ptr(), None, 4, *tail) == _lib.FV_ERR_STATE
        assert b"flushed" in L.fv_last_error()
        items[2] = _lib.PoolItem(1, MAX_CHUNK + 1, 0)
        assert L.fv_codepool_step(cp._h, items, 3, c32.data_ptr(), None, MAX_CHUNK + 1, *tail) == _lib.FV_ERR_INVALID
        # a code handle given floats, a float handle given codes
        mel = torch.zeros((1, 72, 4), device="cuda")
        assert L.fv_pool_step(cp._h, items, 1, mel.data_ptr(), None, 4, *tail) == _lib.FV_ERR_STATE
        assert b"fv_codepool_step" in L.fv_last_error()
        fbefore = _counters(fp, 3)
        assert L.fv_codepool_step(fp._h, items, 1, c32.data_ptr(), None, 4, out.data_ptr(), 8, got, fp._ws.data_ptr(), fp._ws.numel() * 4,
                                    stream) == _lib.FV_ERR_STATE
        assert b"fv_pool_step" in L.fv_last_error() and b"floats" in L.fv_last_error()
        assert _counters(fp, 3) == fbefore
        assert _counters(cp, 3) == before
        both([(2, c[:, 11:19], False), (0, c[:, 16:24], True)])                  # the bits of the undisturbed run
        both([(2, None, True)])
    # a quantiser of another width is refused at creation, by name; so is none at all
    wrong = _quantiser(40, 1, seed=1)
    with pytest.raises(FishVocError, match="dim = 40") as ei:
        dec.code_pool(wrong, 2, MAX_CHUNK)
    assert ei.value.status == _lib.FV_ERR_INVALID
    with pytest.raises(FishVocError, match="dim = 40"):
        dec.code_stream(wrong, 2, MAX_CHUNK)
    eng, h = dec.engine(codes.device), ctypes.c_void_p()
    assert L.fv_stream_create_codes(eng._h, None, ctypes.byref(_lib.StreamConfig(1, 8, -1, -1)), ctypes.byref(h)) == _lib.FV_ERR_INVALID
    assert b"null vq" in L.fv_last_error() and not h.value
    assert L.fv_codepool_create(eng._h, None, ctypes.byref(_lib.PoolConfig(1, 8, -1, -1)), ctypes.byref(h)) == _lib.FV_ERR_INVALID
    assert b"null vq" in L.fv_last_error() and not h.value


def test_a_refused_push_moves_nothing():
    from vocoder_amd import _lib
    dec, vq, codes, R = _setup("head", 32, 3)
    L = _lib.lib()
    with dec.code_stream(vq, B, MAX_CHUNK) as cs, dec.code_stream(vq, B, MAX_CHUNK) as twin, dec.stream(B, MAX_CHUNK) as fs:
        for a, b in _spans(R + 9):
            assert torch.equal(cs.push(codes[:, :, a:b]), twin.push(codes[:, :, a:b]))
        at = R + 9
        before = (cs.received_frames, cs.emitted_frames, cs.pending_frames)
        stream = int(torch.cuda.current_stream().cuda_stream)
        with pytest.raises(ValueError, match="max_chunk_frames"):
            cs.push(codes[:, :, at:at + MAX_CHUNK + 1])
        got = ctypes.c_int64(0)
        out = torch.zeros((B, 1, 9 * 16), device="cuda")
        c32 = torch.zeros((3, B, 9), dtype=torch.int32, device="cuda")
        tail = (out.data_ptr(), ctypes.byref(got), cs._ws.data_ptr(), cs._ws.numel() * 4, stream)
        assert L.fv_stream_push_codes(cs._h, c32.data_ptr(), None, MAX_CHUNK + 1, *tail) == _lib.FV_ERR_INVALID
        mel = torch.zeros((B, 32, 4), device="cuda")
        assert L.fv_stream_push(cs._h, mel.data_ptr(), None, 4, *tail) == _lib.FV_ERR_STATE
        assert b"fv_stream_push_codes" in L.fv_last_error()
        assert L.fv_stream_push_codes(fs._h, c32.data_ptr(), None, 4, out.data_ptr(), ctypes.byref(got), fs._ws.data_ptr(), fs._ws.numel() * 4,
                                      stream) == _lib.FV_ERR_STATE
        assert b"fv_stream_push" in L.fv_last_error() and b"floats" in L.fv_last_error()
        assert (fs.received_frames, fs.pending_frames) == (0, 0)
        assert (cs.received_frames, cs.emitted_frames, cs.pending_frames) == before
        assert torch.equal(cs.push(codes[:, :, at:at + 8]), twin.push(codes[:, :, at:at + 8]))
        assert torch.equal(cs.flush(), twin.flush())
        with pytest.raises(_lib.FishVocError) as ei:                              # after the flush, as a float stream
            cs.push(codes[:, :, :1])
        assert ei.value.status == _lib.FV_ERR_STATE
    # the codebooks are read at every push: a quantiser that was reloaded closes the handle they live in, and the stream says so
    vq2 = _quantiser(32, 1, seed=9)
    with dec.code_stream(vq2, 1, MAX_CHUNK) as cs:
        vq2.invalidate_engine()
        with pytest.raises(_lib.FishVocError, match="create a new one"):
            cs.push(codes[0, :1, :4])


# ---- 5: what the rings cost ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,D,nq", [("head", 72, 3), ("hifigan", 32, 1)])
def test_ring_bytes(kind, D, nq):
    dec, vq, _, R = _setup(kind, D, nq)
    cap = R + R + MAX_CHUNK
    with dec.code_stream(vq, B, MAX_CHUNK) as cs, dec.stream(B, MAX_CHUNK) as fs:
        assert cs.ring_bytes == B * nq * cap * 4 and fs.ring_bytes == B * D * cap * 4
        assert cs.workspace_bytes == fs.workspace_bytes
    with dec.code_pool(vq, 5, 3, context_frames=R + 2, lookahead_frames=R) as cp, dec.session_pool(5, 3, context_frames=R + 2,
                                                                                                   lookahead_frames=R) as fp:
        assert cp.ring_bytes == 5 * nq * (2 * R + 5) * 4 and fp.ring_bytes == 5 * D * (2 * R + 5) * 4
        assert cp.workspace_bytes == fp.workspace_bytes


# ---- 6: the codec's own objects ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_codec(nq):
    """The tiny codec of test_posterior_stream_host.py (a two-stage Vocos decoder), untrained initialisation"""
    from vocoder_amd import codec
    torch.manual_seed(nq)
    return codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, num_quantizers=nq, encoder_depths=(1,),
                             encoder_dims=(32,), decoder_depths=(1,), decoder_dims=(32,)).eval().cuda()


@pytest.mark.parametrize("nq", [1, 2])
def test_decode_stream_of_a_two_stage_decoder_is_the_hand_made_chain(nq):
    m = _tiny_codec(nq)
    bb, head = m.decoder.backbone, m.decoder.head
    with m.decode_stream(B, MAX_CHUNK) as ds:
        assert ds.lookahead_frames == ds.codes.lookahead_frames + ds.head.lookahead_frames
        R_bb, R_head = ds.codes.reach_frames, ds.head.reach_frames
        assert ds.lookahead_frames == R_bb + R_head and (ds.hop, ds.out_channels) == (16, 1)
        assert ds.codes.ring_bytes == B * nq * (2 * R_bb + MAX_CHUNK) * 4
        T = 2 * (R_bb + R_head) + 37
        g = torch.Generator().manual_seed(5)
        codes = torch.randint(0, 48, (B, T) if nq == 1 else (nq, B, T), generator=g).cuda()
        outs = []
        with bb.stream(B, MAX_CHUNK) as s1, head.stream(B, max(MAX_CHUNK, R_bb)) as s2:
            for a, b in _spans(T):
                got = ds.push(codes[..., a:b])
                want = s2.push(s1.push(m.vq.from_codes(codes[..., a:b])[0]))
                assert got.shape == want.shape and torch.equal(got, want), (a, b)
                outs.append(got)
            got = ds.flush()
            want = torch.cat([s2.push(s1.flush()), s2.flush()], dim=2)
            assert torch.equal(got, want)
            outs.append(got)
        y, whole = torch.cat(outs, dim=2), m.decode(codes)
        assert y.shape == whole.shape == (B, 1, T * 16) and ds.emitted_frames == ds.received_frames == T
        # two windowed stages have no bar in the project yet: the distance is reported, not asserted
        print(f"two-stage decode_stream n_q={nq}: max|d| to decode = {float((y - whole).abs().max()):.3e}, peak = {float(whole.abs().max()):.3e}")
        ds.reset()                                                              # the next utterance
        assert torch.equal(ds.push(codes[..., :1]), outs[0]) and ds.received_frames == 1


def test_decode_pool_of_a_two_stage_decoder_is_the_hand_made_chain():
    m = _tiny_codec(2)
    bb, head = m.decoder.backbone, m.decoder.head
    with m.decode_pool(3, MAX_CHUNK) as dp:
        A = dp.codes.lookahead_frames
        assert dp.lookahead_frames == A + dp.head.lookahead_frames and dp.head.max_chunk_frames == MAX_CHUNK + A
        g = torch.Generator().manual_seed(6)
        lengths = [2 * dp.lookahead_frames + 21, dp.lookahead_frames + 3, 4]
        utts = [torch.randint(0, 48, (2, n), generator=g).cuda() for n in lengths]
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
        outs = [[] for _ in lengths]
        with bb.session_pool(3, MAX_CHUNK) as p1, head.session_pool(3, MAX_CHUNK + A) as p2:
            for items in steps:
                got = dp.step([(s, utts[s][:, a:a + n] if n else None, fl) for s, a, n, fl in items])
                z = p1.step([(s, m.vq.from_codes(utts[s][:, None, a:a + n])[0][0] if n else None, fl) for s, a, n, fl in items])
                want = p2.step([(s, zi if zi.shape[1] else None, fl) for (s, _, _, fl), zi in zip(items, z)])
                for (s, a, n, fl), x, y in zip(items, got, want):
                    assert x.shape == y.shape and torch.equal(x, y), (s, a, n, fl)
                    outs[s].append(x)
            before = [(dp.received_frames(s), dp.emitted_frames(s)) for s in range(3)]
            with pytest.raises(ValueError, match="flushed"):                     # planned before either stage is launched: neither pool moves
                dp.step([(0, utts[0][:, :2], False)])
            assert [(dp.received_frames(s), dp.emitted_frames(s)) for s in range(3)] == before
        for s, n in enumerate(lengths):
            y, whole = torch.cat(outs[s], dim=1), m.decode(utts[s][:, None, :])[0]
            assert y.shape == whole.shape == (1, n * 16)
            print(f"two-stage decode_pool session {s}: max|d| to decode = {float((y - whole).abs().max()):.3e}, peak = {float(whole.abs().max()):.3e}")
        dp.reset(2)
        assert dp.received_frames(2) == 0 and dp.emitted_frames(2) == 0


@pytest.mark.parametrize("nq", [1, 3])
def test_single_engine_decoders_through_the_codec_and_the_unify_generator(nq):
    from vocoder_amd.codec import VQVAECodec
    from vocoder_amd.modules.generators import UnifyGenerator
    from torch import nn
    dec, vq, codes, R = _setup("hifigan" if nq == 3 else "head", 32, nq)
    T = codes.shape[-1]
    c = VQVAECodec(nn.Identity(), dec, vq)
    u = UnifyGenerator(nn.Identity(), dec, vq) if nq == 1 else None
    whole = c.decode(codes)
    for obj in (c, u):
        if obj is None:
            continue
        with obj.decode_stream(B, MAX_CHUNK) as ds, dec.stream(B, MAX_CHUNK) as fs:
            assert ds.head is None and ds.lookahead_frames == R
            outs = []
            for a, b in _spans(T):
                outs.append(ds.push(codes[..., a:b]))
                assert torch.equal(outs[-1], fs.push(vq.from_codes(codes[..., a:b])[0]))
            outs.append(ds.flush())
            assert torch.equal(outs[-1], fs.flush())
        _within_window_bound(torch.cat(outs, dim=2), whole if obj is c else u.decode(codes), f"{type(obj).__name__}.decode_stream n_q={nq}")
        with obj.decode_pool(2, MAX_CHUNK) as dp, dec.session_pool(2, MAX_CHUNK) as fp:
            outs = [[], []]
            for t, (a, b) in enumerate(_spans(T)):
                last = b == T
                items = [(s, codes[..., s, a:b], last) for s in ((0, 1) if t % 2 else (1, 0))]
                got = dp.step(items)
                want = fp.step([(s, vq.from_codes(x[..., None, :])[0][0], fl) for s, x, fl in items])
                for (s, _, _), x, y in zip(items, got, want):
                    assert torch.equal(x, y)
                    outs[s].append(x)
        for s in range(2):
            _within_window_bound(torch.cat(outs[s], dim=1), whole[s], f"{type(obj).__name__}.decode_pool n_q={nq} session {s}")


def test_command_line_chunk_frames_writes_what_decode_stream_gives(tmp_path):
    from vocoder_amd import codec
    from vocoder_amd.inference import read_wav, write_wav
    arch = ["--n-fft", "64", "--hop-length", "16", "--win-length", "64", "--latent-size", "32", "--codebook-size", "48", "--num-quantizers", "2"]
    codes = np.random.default_rng(1).integers(0, 48, (2, 57)).astype(np.int64)
    np.save(tmp_path / "a.codes.npy", codes)
    torch.manual_seed(0)                      # no checkpoint: the untrained initialisation, the same for both
    assert codec.main(["decode", "-i", str(tmp_path / "a.codes.npy"), "-o", str(tmp_path / "cli"), "--chunk-frames", "5"] + arch) == 0
    torch.manual_seed(0)
    m = codec.build_vqvae(64, 16, 64, 32, 48, 2, encoder_dims=(32,), decoder_dims=(32, 64)).eval().cuda()
    c = torch.from_numpy(codes)[:, None, :].cuda()
    with m.decode_stream(1, 5) as ds:
        audio = torch.cat([ds.push(c[..., n:n + 5]) for n in range(0, 57, 5)] + [ds.flush()], dim=2)
    assert audio.shape == (1, 1, 57 * 16)
    write_wav(tmp_path / "want.wav", audio[0, 0].cpu().numpy(), 24000)
    assert (tmp_path / "cli" / "a.wav").read_bytes() == (tmp_path / "want.wav").read_bytes()
    got, sr = read_wav(tmp_path / "cli" / "a.wav")
    assert sr == 24000 and got.shape == (1, 57 * 16)
