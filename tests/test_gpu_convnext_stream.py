"""GPU: the ConvNeXt backbone layer by layer and chunk by chunk (fv_cnxstream_*, ``ConvNeXtEncoder.layer_stream``), and the codec on top.

Every comparison is ``torch.equal`` against the module's own whole-row ``forward`` in batch-invariant mode unless a test says otherwise: the
stream promises those bits under any chunking.  The modules carry random layer scales and LayerNorm weights (the 1e-6 initialisation hides
the blocks).  Each config picks another instantiation of the depthwise stream kernel or another path of the engine:

  one      in 20, dims (32,), depths (1,)      one block, half a 64-row chunk, R = 6
  two      dims (64, 96), depths (2, 2)        the stage change; a partial second chunk at <7, 256, 8>
  c320     dims (320,), depths (1,)            <7, 512, 16> with never-computed chunks
  c640     dims (640,), depths (1,)            <7, 1024, 16>
  default  513 -> (512,) x 6                   the default encoder shape, R = 21
  square   32 -> (32, 64), depths (1, 1)       a C -> C stem: the batch-invariant forward runs it on the Winograd pair lattice, whose bits
  square64 64 -> (64,), depths (1,)            depend on the window's alignment (quad lattice at 64); the stream runs direct sums and has
                                               the bits of forward with conv_algorithm = "direct" (the decoder backbone's case, 512 -> 512)

Chunks are pushed as slices ``x[:, :, a:b]``, strided views, unless a test says otherwise."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from vocoder_amd import _lib, codec
from vocoder_amd import synthetic as syn
from vocoder_amd._lib import FishVocError
from vocoder_amd.modules.encoders.convnext import ConvNeXtEncoder, ConvNeXtStream, schedule

pytestmark = pytest.mark.gpu

# name -> (input_channels, dims, depths, seed)
CONFIGS = {
    "one": (20, (32,), (1,), 1),
    "two": (20, (64, 96), (2, 2), 2),
    "c320": (20, (320,), (1,), 3),
    "c640": (20, (640,), (1,), 4),
    "default": (513, (512,), (6,), 5),
    "square": (32, (32, 64), (1, 1), 6),
    "square64": (64, (64,), (1,), 7),
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
    assert m.stem_has_winograd_form == name.startswith("square") and m.stream_is_bit_exact
    return m


@functools.lru_cache(maxsize=None)
def module(name):
    return new_module(name)


@functools.lru_cache(maxsize=None)
def case(name, B, T, seed=0):
    """(x, the whole-row batch-invariant forward): computed once, shared, never written."""
    x = torch.from_numpy(np.random.default_rng(1000 * seed + T).standard_normal((B, CONFIGS[name][0], T)).astype(np.float32)).cuda()
    return x, module(name)(x)


def run(st, x, chunks, contiguous=False):
    """Pushes ``chunks`` of ``x`` and flushes; every call's shape and the counters are the schedule's.  -> the concatenated frames."""
    B = x.shape[0]
    parts, a = [], 0
    for c, (e0, e1) in zip(list(chunks) + [None], st.schedule(chunks)):
        if c is None:
            y = st.flush()
        else:
            chunk = x[:, :, a:a + c]
            y = st.push(chunk.contiguous() if contiguous else chunk)
            a += c
        assert y.shape == (B, st.out_channels, e1 - e0) and y.dtype == torch.float32, (y.shape, e0, e1)
        assert (st.received_frames, st.emitted_frames, st.pending_frames) == (a, e1, a - e1)
        parts.append(y)
    assert a == x.shape[2] and st.emitted_frames == a
    return torch.cat(parts, dim=2)


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        d = (got - want).abs().amax(dim=(0, 1))
        bad = torch.nonzero(d > 0).flatten().tolist()
        nan = torch.nonzero(torch.isnan(got).any(dim=1).any(dim=0)).flatten().tolist()
        raise AssertionError(f"{what}: differs at frames {bad[:12]} ({len(bad)} of {got.shape[2]}), NaN at {nan[:12]}, max |d| = {float(d.max()):.3e}")


def in_eights(T, head=()):
    head = list(head)
    rest = T - sum(head)
    return head + [8] * (rest // 8) + ([rest % 8] if rest % 8 else [])


@pytest.mark.parametrize("name", NAMES)
def test_any_chunking_has_the_whole_rows_bits(name):
    m, R = module(name), reach(name)
    T = 2 * R + 37
    x, want = case(name, 3, T)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.1
    with m.layer_stream(3, 8) as st:
        assert isinstance(st, ConvNeXtStream) and st.lookahead_frames == R and st.batch == 3 and st.max_chunk_frames == 8
        assert st.state_bytes > 0
        assert_same(run(st, x, in_eights(T, [1, 8, 3])), want, "[1, 8, 3, 8, ...]")
        st.reset()
        assert_same(run(st, x, [1] * T), want, "all ones")
        st.reset()
        assert_same(run(st, x, in_eights(T, [5, 0, 8, 0])), want, "zero-frame pushes in the middle")
    with m.layer_stream(3, T) as st:
        assert_same(run(st, x, [T]), want, "one push")


@pytest.mark.parametrize("name", NAMES)
def test_tile_edges_inside_a_chunk(name):
    x, want = case(name, 2, 113)
    with module(name).layer_stream(2, 70) as st:
        assert_same(run(st, x, [33, 64, 16]), want, "33 | 64 | 16")
        st.reset()
        assert_same(run(st, x[:, :, :70], [70]), module(name)(x[:, :, :70].contiguous()), "one push of 70")


@pytest.mark.parametrize("name", NAMES)
def test_short_utterances(name):
    m, R = module(name), reach(name)
    with m.layer_stream(2, R + 1) as st:
        for T in sorted({1, 2, 3, R, R + 1}):
            x, want = case(name, 2, T, seed=1)
            st.reset()
            assert_same(run(st, x, [T]), want, f"T = {T} in one push")
            st.reset()
            assert_same(run(st, x, [1] * T), want, f"T = {T} frame by frame")


def test_many_laps_through_the_smallest_rings():
    x, want = case("one", 2, 300)
    with module("one").layer_stream(2, 8) as st:
        assert_same(run(st, x, in_eights(300)), want, "300 frames in eights")
    x, want = case("two", 2, 300)
    with module("two").layer_stream(2, 8) as st:
        assert_same(run(st, x, in_eights(300)), want, "300 frames in eights, two stages")


@pytest.mark.parametrize("name", ["one", "two", "c320"])
def test_a_reset_leaves_nothing_of_the_last_utterance(name):
    """The first utterance is all NaN: whatever the rings keep of it must not be read as the next utterance's padding."""
    R = reach(name)
    x, want = case(name, 2, 2 * R + 11)
    with module(name).layer_stream(2, 8) as st:
        bad = torch.full_like(x, float("nan"))
        got = run(st, bad, in_eights(x.shape[2]))
        assert bool(torch.isnan(got).all())
        st.reset()
        assert_same(run(st, x, in_eights(x.shape[2], [3])), want, "after an all-NaN utterance")
        st.reset()
        assert_same(run(st, x[:, :, :2], [2]), module(name)(x[:, :, :2].contiguous()), "a 2-frame utterance after a long one")


@pytest.mark.parametrize("name", ["one", "two", "default"])
def test_rows_alone_and_in_a_batch(name):
    R = reach(name)
    x, want = case(name, 3, 2 * R + 37)
    with module(name).layer_stream(1, 8) as st:
        for b in (0, 2):
            st.reset()
            assert_same(run(st, x[b:b + 1], in_eights(x.shape[2], [2])), want[b:b + 1], f"row {b} alone")


@pytest.mark.parametrize("name", ["one", "c640"])
def test_views_and_copies(name):
    R = reach(name)
    x, want = case(name, 2, 2 * R + 37)
    wide = torch.full((2, x.shape[1] + 3, x.shape[2] + 10), float("nan"), device="cuda")
    wide[:, 1:-2, 4:-6] = x
    with module(name).layer_stream(2, 8) as st:
        assert_same(run(st, x, in_eights(x.shape[2]), contiguous=True), want, "copies")
        st.reset()
        assert_same(run(st, wide[:, 1:-2, 4:-6], in_eights(x.shape[2], [1])), want, "views into a NaN-filled wider tensor")


def test_refused_calls_change_nothing():
    x, want = case("two", 2, 2 * reach("two") + 37)
    m = module("two")
    with m.layer_stream(2, 8) as st, m.layer_stream(2, 8) as twin:
        first = st.push(x[:, :, :8])
        assert torch.equal(first, twin.push(x[:, :, :8]))
        with pytest.raises(FishVocError, match="max_chunk"):
            st.push(x[:, :, 8:17])
        assert (st.received_frames, st.emitted_frames, st.pending_frames) == (8, 0, 8)
        parts, tparts = [first], [first]
        for a in range(8, x.shape[2], 8):
            parts.append(st.push(x[:, :, a:a + 8]))
            tparts.append(twin.push(x[:, :, a:a + 8]))
            assert torch.equal(parts[-1], tparts[-1])
        parts.append(st.flush())
        assert_same(torch.cat(parts, dim=2), want, "after a refused push")
        N, E = st.received_frames, st.emitted_frames
        with pytest.raises(FishVocError, match="flushed"):
            st.push(x[:, :, :1])
        assert (st.received_frames, st.emitted_frames) == (N, E) and st.pending_frames == 0
        st.reset()
        assert torch.equal(torch.cat([st.push(x[:, :, :8]), st.flush()], dim=2), m(x[:, :, :8].contiguous()))


def test_create_refusals_by_name():
    from vocoder_amd.modules.generators import HiFiGANGenerator
    with pytest.raises(FishVocError, match="kernel_size"):
        new_module("one", kernel_size=5).layer_stream(1, 8)
    m = new_module("one")
    m.precision = "f16x3"
    with pytest.raises(FishVocError, match="f16x3"):
        m.layer_stream(1, 8)
    for batch, chunk, word in ((0, 8, "batch"), (1, 0, "max_chunk")):
        with pytest.raises(FishVocError, match=word):
            module("one").layer_stream(batch, chunk)
    cfg = dict(hop_length=64, upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4], resblock_kernel_sizes=[3, 7, 11],
               resblock_dilation_sizes=[[1, 3, 5]] * 3, num_mels=80, upsample_initial_channel=128, use_template=False, pre_conv_kernel_size=7,
               post_conv_kernel_size=7)
    gen = HiFiGANGenerator(**cfg)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(cfg, seed=1).items()}, strict=True)
    eng = gen.eval().cuda().engine(torch.device("cuda", torch.cuda.current_device()))
    L, s = _lib.lib(), ctypes.c_void_p()
    assert L.fv_cnxstream_create(eng._h, 1, 8, ctypes.byref(s)) == _lib.FV_ERR_INVALID and not s.value
    assert "FV_MODEL_CONVNEXT" in L.fv_last_error().decode()


def test_a_wider_output_through_the_c_abi():
    """``y_row_stride`` wider than the frames a call emits (the Python wrapper never asks for that): the frames land in the first columns of
    every row and the rest of the caller's buffer is left alone."""
    m = module("two")
    x, want = case("two", 2, 2 * reach("two") + 37)
    T, Co, pad = x.shape[2], want.shape[1], 5
    eng = m.engine(torch.device("cuda", torch.cuda.current_device()))
    L, s, got = _lib.lib(), ctypes.c_void_p(), ctypes.c_int64(-1)
    _lib.check(L.fv_cnxstream_create(eng._h, 2, 16, ctypes.byref(s)))
    try:
        parts, E = [], 0
        for a in list(range(0, T, 16)) + [None]:
            c = 0 if a is None else min(16, T - a)
            k = T - E if a is None else max(E, a + c - reach("two")) - E
            y = torch.full((2, Co, k + pad), -7.0, device="cuda")
            if a is None:
                _lib.check(L.fv_cnxstream_flush(s, y.data_ptr(), k + pad, ctypes.byref(got), None))
            else:
                chunk = x[:, :, a:a + c]
                _lib.check(L.fv_cnxstream_push(s, chunk.data_ptr(), chunk.stride(0), chunk.stride(1), c, y.data_ptr(), k + pad, ctypes.byref(got), None))
            torch.cuda.synchronize()
            assert got.value == k and bool((y[:, :, k:] == -7.0).all())
            parts.append(y[:, :, :k])
            E += k
        assert_same(torch.cat(parts, dim=2), want, "y_row_stride = k + 5")
    finally:
        torch.cuda.synchronize()
        L.fv_cnxstream_destroy(s)


@pytest.mark.parametrize("name", NAMES)
def test_lookahead_is_the_backbones_reach(name):
    """R = 3 (1 + sum depths): the backbone's own reach.  ``Engine.reach_frames`` is that plus the 2 frames of margin the engine's windows keep."""
    m = module(name)
    eng = m.engine(torch.device("cuda", torch.cuda.current_device()))
    with m.layer_stream(1, 8) as st:
        assert st.lookahead_frames == m.lookahead_frames == reach(name) == eng.reach_frames - 2
        assert st.schedule([8, 8]) == schedule([8, 8], reach(name))


def test_a_rebuilt_engine_closes_the_stream():
    m = new_module("one")
    st = m.layer_stream(1, 8)
    m.load_state_dict(m.state_dict())
    with pytest.raises(FishVocError, match="closed"):
        st.push(torch.zeros(1, 20, 4, device="cuda"))


# ---- the codec: the tiny one the other tests use (n_fft 64, hop 16, latent 32, K 48), with a ConvNeXt encoder in batch-invariant mode ----

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
def test_codec_encode_stream_gives_encodes_codes(nq):
    c = make_codec(nq)
    wave = 0.1 * torch.randn(2, 5000, generator=torch.Generator().manual_seed(nq)).cuda()
    want = c.encode(wave)
    assert want.shape == ((2, want.shape[-1]) if nq == 1 else (3, 2, want.shape[-1])) and want.shape[-1] > 2 * c.encoder.lookahead_frames
    sizes, a = [], 0
    while a < 5000:
        for n in (1000, 1, 37):
            n = min(n, 5000 - a)
            sizes.append(n)
            a += n
    with c.encode_stream(2, 1000) as st:
        assert isinstance(st._enc, ConvNeXtStream)
        parts, a = [], 0
        for i, n in enumerate(sizes):
            chunk = wave[:, a:a + n]
            parts.append(st.push(chunk[:, None, :] if i % 2 else chunk))
            a += n
        parts.append(st.flush())
        got = torch.cat(parts, dim=-1)
        assert got.shape == want.shape and torch.equal(got, want)
        assert any(p.shape[-1] == 0 for p in parts) and sum(p.shape[-1] > 0 for p in parts) > 2
        st.reset()
        short = wave[:, :1203]
        got = torch.cat([st.push(short[:, :1000]), st.push(short[:, 1000:]), st.flush()], dim=-1)
        assert torch.equal(got, c.encode(short))
    c.encoder.batch_invariant = False
    with pytest.raises(ValueError, match="not bit-exact"):
        c.encode_stream(2, 1000)


def test_codec_command_line_with_a_square_stem(tmp_path):
    """n_fft / 2 + 1 == latent_size: the encoder's stem is a C -> C conv, and ``--batch-invariant`` sets direct sums with it."""
    from vocoder_amd.inference import write_wav
    arch = ["--n-fft", "62", "--hop-length", "16", "--win-length", "62", "--latent-size", "32", "--codebook-size", "48", "--batch-invariant"]
    write_wav(tmp_path / "a.wav", 0.1 * np.random.default_rng(1).standard_normal(3000).astype(np.float32), 24000)
    torch.manual_seed(0)
    assert codec.main(["encode", "-i", str(tmp_path / "a.wav"), "-o", str(tmp_path / "whole")] + arch) == 0
    torch.manual_seed(0)
    assert codec.main(["encode", "-i", str(tmp_path / "a.wav"), "-o", str(tmp_path / "chunked"), "--chunk-samples", "777"] + arch) == 0
    whole, chunked = np.load(tmp_path / "whole" / "a.codes.npy"), np.load(tmp_path / "chunked" / "a.codes.npy")
    assert whole.shape == chunked.shape and whole.shape[-1] > 64 and np.array_equal(whole, chunked)


def test_codec_command_line_chunked_writes_the_same_file(tmp_path):
    from vocoder_amd.inference import write_wav
    arch = ["--n-fft", "64", "--hop-length", "16", "--win-length", "64", "--latent-size", "32", "--codebook-size", "48", "--num-quantizers", "2",
            "--batch-invariant"]
    write_wav(tmp_path / "a.wav", 0.1 * np.random.default_rng(0).standard_normal(5000).astype(np.float32), 24000)
    torch.manual_seed(0)                      # no checkpoint: the untrained initialisation, the same for both calls
    assert codec.main(["encode", "-i", str(tmp_path / "a.wav"), "-o", str(tmp_path / "whole")] + arch) == 0
    torch.manual_seed(0)
    assert codec.main(["encode", "-i", str(tmp_path / "a.wav"), "-o", str(tmp_path / "chunked"), "--chunk-samples", "777"] + arch) == 0
    whole, chunked = np.load(tmp_path / "whole" / "a.codes.npy"), np.load(tmp_path / "chunked" / "a.codes.npy")
    assert whole.dtype == chunked.dtype == np.int64 and whole.shape == chunked.shape and whole.shape[0] == 2 and whole.shape[1] > 64
    assert np.array_equal(whole, chunked)


def _spans(T, sizes=(8, 1, 5, 8, 0, 3)):
    out, a, i = [], 0, 0
    while a < T:
        n = min(sizes[i % len(sizes)], T - a)
        out.append((a, a + n))
        a, i = a + n, i + 1
    return out


WINDOW_TOL = 2e-5      # of the output's peak: the project's bound for ONE windowed stage against the whole clip


@pytest.mark.parametrize("nq", [1, 2])
def test_decode_stream_by_layers(nq):
    """``backbone="layers"``: equal to ``head.stream()`` fed, in the same chunks, the frames of the backbone's whole-row batch-invariant
    forward of ``from_codes(codes)`` — with direct sums in its 32 -> 32 stem, which has a Winograd form (``stem_has_winograd_form``) —; and,
    with only the head windowed, within 2e-5 of ``decode()``'s peak (``decode()`` itself runs as it always did).  Measured on an MI355X:
    see profiles/LOG.md R41.1."""
    B, MAX = 2, 8
    m = make_codec(nq, decoder_depths=(1, 1), decoder_dims=(32, 64))
    bb, head = m.decoder.backbone, m.decoder.head
    with m.decode_stream(B, MAX, backbone="layers") as ds:
        R_bb = bb.lookahead_frames
        assert ds.backbone == "layers" and ds.codes.lookahead_frames == R_bb == 9
        assert ds.lookahead_frames == R_bb + ds.head.lookahead_frames and (ds.hop, ds.out_channels) == (16, 1)
        T = 2 * ds.lookahead_frames + 37
        codes = torch.randint(0, 48, (B, T) if nq == 1 else (nq, B, T), generator=torch.Generator().manual_seed(5)).cuda()
        assert bb.stem_has_winograd_form
        bb.batch_invariant, bb.conv_algorithm = True, "direct"
        frames = bb(m.vq.from_codes(codes)[0])
        bb.batch_invariant, bb.conv_algorithm = False, "auto"      # the layer stream has those bits whatever the module's settings
        sched = schedule([b - a for a, b in _spans(T)], R_bb)
        outs = []
        with head.stream(B, max(MAX, R_bb)) as s2:
            for (a, b), (e0, e1) in zip(_spans(T), sched):
                got = ds.push(codes[..., a:b])
                want = s2.push(frames[:, :, e0:e1].contiguous())
                assert got.shape == want.shape and torch.equal(got, want), (a, b)
                outs.append(got)
            got = ds.flush()
            want = torch.cat([s2.push(frames[:, :, sched[-1][0]:].contiguous()), s2.flush()], dim=2)
            assert torch.equal(got, want)
            outs.append(got)
        y, whole = torch.cat(outs, dim=2), m.decode(codes)
        assert y.shape == whole.shape == (B, 1, T * 16) and ds.emitted_frames == ds.received_frames == T
        d, peak = float((y - whole).abs().max()), float(whole.abs().max())
        print(f"decode_stream(backbone='layers') n_q={nq}: max|d| to decode = {d:.3e}, peak = {peak:.3e}, ratio = {d / peak:.3e}")
        assert d <= WINDOW_TOL * peak
        with pytest.raises(ValueError, match="max_chunk_frames"):
            ds.push(codes[..., :MAX + 1])
        ds.reset()
        assert torch.equal(ds.push(codes[..., :1]), outs[0]) and ds.received_frames == 1


def test_decode_stream_by_windows_is_what_it_was():
    """The default ``backbone="window"`` is the hand-made chain of float streams, as before."""
    B, MAX = 2, 8
    m = make_codec(2, decoder_depths=(1, 1), decoder_dims=(32, 64))
    bb, head = m.decoder.backbone, m.decoder.head
    with m.decode_stream(B, MAX) as ds, m.decode_stream(B, MAX, backbone="window") as ds2:
        assert ds.backbone == ds2.backbone == "window"
        R_bb = ds.codes.reach_frames
        T = 2 * ds.lookahead_frames + 21
        codes = torch.randint(0, 48, (2, B, T), generator=torch.Generator().manual_seed(6)).cuda()
        with bb.stream(B, MAX) as s1, head.stream(B, max(MAX, R_bb)) as s2:
            for a, b in _spans(T):
                got = ds.push(codes[..., a:b])
                want = s2.push(s1.push(m.vq.from_codes(codes[..., a:b])[0]))
                assert torch.equal(got, want) and torch.equal(ds2.push(codes[..., a:b]), want), (a, b)
            assert torch.equal(ds.flush(), torch.cat([s2.push(s1.flush()), s2.flush()], dim=2))
    with pytest.raises(ValueError, match="backbone"):
        m.decode_stream(B, MAX, backbone="rings")
    with pytest.raises(ValueError, match="two-stage"):
        codec.CodecDecodeStream(m.decoder.head, m.vq, B, MAX, "layers")
