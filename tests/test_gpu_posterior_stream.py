"""GPU: the posterior encoder chunk by chunk (fv_wnstream_*, ``PosteriorEncoder.stream``) and the codec's streaming encode.

Every comparison is ``torch.equal`` against the module's own whole-row ``forward``: a stream promises the whole utterance's bits under any
chunking, so there is no tolerance.  The configs are the smallest that reach each code path — the folded k = 5, d = 1 taps (``k5``,
``default``), the run-time taps (``dilated``, ``bnvae``, ``k1``), the 32-column tile (chunks up to 64 frames) and the 128-column one (a push
of 150), R = 0, and the real widths with 16 layers (``default``).  Chunks are pushed as slices ``x[:, :, a:b]``, strided views, unless a test
says otherwise."""
import functools

import numpy as np
import pytest
import torch

from vocoder_amd import codec
from vocoder_amd import synthetic as syn
from vocoder_amd._lib import FV_ERR_STATE, FishVocError
from vocoder_amd.modules.encoders import PosteriorEncoder, PosteriorStream
from vocoder_amd.modules.encoders.posterior_encoder import schedule

pytestmark = pytest.mark.gpu


def make_cfg(cin, out, C, k, rate, cycle, nl, mode):
    return dict(in_channels=cin, out_channels=out, hidden_channels=C, kernel_size=k, dilation_rate=rate, dilation_cycle=cycle, n_layers=nl, mode=mode)


# name -> (config, seed of its weights, R)
CONFIGS = {
    "k5": (make_cfg(20, 8, 48, 5, 1, 1, 4, "vqvae"), 21, 8),
    "dilated": (make_cfg(20, 8, 48, 5, 2, 3, 4, "vae"), 12, 16),        # tests/golden/posterior_vae.npz's config: dilations 1, 2, 4, 1
    "bnvae": (make_cfg(20, 8, 32, 3, 3, 2, 1, "bnvae"), 13, 1),         # tests/golden/posterior_bnvae.npz's config
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
def case(name, B, T, seed=0):
    """(x, the whole-row forward's tensors): computed once, shared, never written."""
    cfg = CONFIGS[name][0]
    x = torch.from_numpy(np.random.default_rng(1000 * seed + T).standard_normal((B, cfg["in_channels"], T)).astype(np.float32)).cuda()
    res = module(name)(x)
    return x, ((res,) if cfg["mode"] == "vqvae" else tuple(res[:3]))


def run(st, x, chunks, contiguous=False):
    """Pushes ``chunks`` of ``x`` and flushes; every call's shape and the counters are the schedule's.  -> the concatenated tensors."""
    R, B = st.lookahead_frames, x.shape[0]
    sched = schedule(chunks, R)
    vae = st._module.mode != "vqvae"
    parts, a = [], 0
    for c, (e0, e1) in zip(list(chunks) + [None], sched):
        if c is None:
            res = st.flush()
        else:
            chunk = x[:, :, a:a + c]
            res = st.push(chunk.contiguous() if contiguous else chunk)
            a += c
        res = res if vae else (res,)
        assert len(res) == (4 if vae else 1)
        for t in res[:3]:
            assert t.shape == (B, st.out_channels, e1 - e0) and t.dtype == torch.float32, (t.shape, e0, e1)
        if vae:
            assert res[3].shape == (B, 1, e1 - e0) and bool((res[3] == 1).all())
        assert (st.received_frames, st.emitted_frames, st.pending_frames) == (a, e1, a - e1)
        parts.append(res[:3])
    assert a == x.shape[2] and st.emitted_frames == a
    return tuple(torch.cat([p[i] for p in parts], dim=2) for i in range(len(parts[0])))


def assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g, w), f"{what}: tensor {i} differs, max |d| = {float((g - w).abs().max()):.3e}"


def in_eights(T, head=()):
    head = list(head)
    rest = T - sum(head)
    return head + [8] * (rest // 8) + ([rest % 8] if rest % 8 else [])


@pytest.mark.parametrize("name", NAMES)
def test_any_chunking_has_the_whole_rows_bits(name):
    m, R = module(name), CONFIGS[name][2]
    T = 2 * R + 37
    x, want = case(name, 3, T)
    with m.stream(3, 8) as st:
        assert isinstance(st, PosteriorStream) and st.lookahead_frames == R and st.batch == 3 and st.max_chunk_frames == 8
        assert_same(run(st, x, in_eights(T, [1, 8, 3])), want, "[1, 8, 3, 8, ...]")
        st.reset()
        assert_same(run(st, x, [1] * T), want, "all ones")
        st.reset()
        assert_same(run(st, x, in_eights(T, [5, 0, 8, 0])), want, "zero-frame pushes in the middle")
    with m.stream(3, T) as st:
        assert_same(run(st, x, [T]), want, "one push")


def test_one_wide_push_runs_the_128_column_tile():
    x, want = case("dilated", 3, 150)
    with module("dilated").stream(3, 160) as st:
        assert_same(run(st, x, [150]), want, "one push of 150")
        st.reset()
        assert_same(run(st, x, [70, 64, 16]), want, "70 | 64 | 16: the wide tile, then the narrow one at its widest")


@pytest.mark.parametrize("name", NAMES)
def test_short_utterances(name):
    m, R = module(name), CONFIGS[name][2]
    with m.stream(2, max(R + 1, 1)) as st:
        for T in sorted({1, R, R + 1, R // 2} - {0}):
            x, want = case(name, 2, T, seed=1)
            st.reset()
            got = run(st, x, [T])
            assert_same(got, want, f"T = {T} in one push")
            st.reset()
            assert_same(run(st, x, [1] * T), want, f"T = {T} frame by frame")
    # T < R: every frame comes from the flush (run() has checked each push's empty shape)
    if R > 1:
        assert schedule([R // 2], R) == [(0, 0), (0, R // 2)]


def test_ring_wrap():
    """max_chunk = 8 on k5: rings of 16 frames (2 p + max(8, R) = 12, R + max(8, R) = 16), so 300 frames are more than 18 laps."""
    x, want = case("k5", 3, 300)
    with module("k5").stream(3, 8) as st:
        assert_same(run(st, x, in_eights(300, [1, 8, 3])), want, "T = 300")


@pytest.mark.parametrize("name", ["k5", "dilated"])
def test_reset_between_utterances(name):
    R = CONFIGS[name][2]
    x1, want1 = case(name, 3, 2 * R + 37)
    x2, want2 = case(name, 3, R + 5, seed=2)
    with module(name).stream(3, 8) as st:
        assert_same(run(st, x1, in_eights(x1.shape[2])), want1, "first utterance")
        st.reset()
        assert (st.received_frames, st.emitted_frames, st.pending_frames) == (0, 0, 0)
        assert_same(run(st, x2, in_eights(x2.shape[2], [3])), want2, "second, shorter utterance")


@pytest.mark.parametrize("name", ["k5", "dilated"])
def test_rows_are_independent_and_strides_do_not_matter(name):
    m, R = module(name), CONFIGS[name][2]
    T = 2 * R + 37
    x, _ = case(name, 3, T)
    chunks = in_eights(T, [1, 8, 3])
    with m.stream(3, 8) as st:
        strided = run(st, x, chunks)                        # slices of x: the row stride is T
        st.reset()
        assert_same(run(st, x, chunks, contiguous=True), strided, "contiguous copies against strided views")
        wide = torch.full((3, x.shape[1], T + 9), float("nan"), device=x.device)
        wide[:, :, 4:4 + T] = x
        st.reset()
        assert_same(run(st, wide[:, :, 4:4 + T], chunks), strided, "views of a wider tensor whose other frames are NaN")
    with m.stream(1, 8) as st:
        for b in range(3):
            st.reset()
            assert_same(run(st, x[b:b + 1], chunks), tuple(t[b:b + 1] for t in strided), f"row {b} alone")


def test_refusals_change_no_counter():
    m = new_module("k5")
    x, _ = case("k5", 2, 24)
    st = m.stream(2, 8)
    st.push(x[:, :, :8])
    st.push(x[:, :, 8:13])
    state = (13, 5, 8)

    def counters():
        return st.received_frames, st.emitted_frames, st.pending_frames
    assert counters() == state
    with pytest.raises(FishVocError, match="max_chunk = 8"):
        st.push(x[:, :, :9])
    assert counters() == state
    with pytest.raises(ValueError, match=r"\(2, 20, c\)"):
        st.push(x[:, :19, :4])
    with pytest.raises(ValueError, match=r"\(2, 20, c\)"):
        st.push(x[:1, :, :4])
    assert counters() == state
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        st.push(x[:, :, :4].cpu())
    assert counters() == state
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        st.push(x[:, :, :4])
    with pytest.raises(RuntimeError, match="inference-only"):
        st.flush()
    with pytest.raises(RuntimeError, match="inference-only"):
        m.stream()
    m.eval()
    assert counters() == state
    assert st.flush().shape == (2, 8, 8)
    state = (13, 13, 0)
    with pytest.raises(FishVocError, match="flushed") as e:
        st.push(x[:, :, :4])
    assert e.value.status == FV_ERR_STATE
    with pytest.raises(FishVocError, match="flushed"):
        st.flush()
    assert counters() == state
    st.reset()
    assert st.push(x[:, :, :8]).shape == (2, 8, 0) and counters() == (8, 0, 8)
    # the engine is rebuilt: the stream is closed, and says so
    m.load_state_dict(m.state_dict())
    with pytest.raises(FishVocError, match="load_state_dict") as e:
        st.push(x[:, :, :4])
    assert e.value.status == FV_ERR_STATE
    with pytest.raises(FishVocError, match="closed"):
        st.flush()
    with m.stream(2, 8) as st2:           # a new one works
        assert st2.push(x[:, :, :8]).shape == (2, 8, 0) and st2.flush().shape == (2, 8, 8)
    st3 = m.stream(2, 8)
    m.to("cuda")                           # .to() rebuilds as well
    with pytest.raises(FishVocError, match="closed"):
        st3.push(x[:, :, :4])
    with pytest.raises(FishVocError, match="d_mean"):       # the C ABI's own rule, as fv_posterior_forward has it
        c_push_with_mean(m)


def c_push_with_mean(m):
    import ctypes

    from vocoder_amd import _lib
    L, s = _lib.lib(), ctypes.c_void_p()
    eng = m.engine(torch.device("cuda", torch.cuda.current_device()))
    _lib.check(L.fv_wnstream_create(eng.handle, 1, 8, ctypes.byref(s)))
    try:
        buf = torch.zeros(1, 20, 8, device="cuda")
        got = ctypes.c_int64(-1)
        st = L.fv_wnstream_push(s, buf.data_ptr(), 160, 8, 8, buf.data_ptr(), buf.data_ptr(), None, 8, ctypes.byref(got), None)
        assert got.value == -1 and L.fv_wnstream_pending(s) == 0
        _lib.check(st)
    finally:
        L.fv_wnstream_destroy(s)


def make_codec(nq):
    torch.manual_seed(5)
    c = codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, num_quantizers=nq, decoder_depths=(1,),
                          decoder_dims=(32,), encoder="posterior", hidden_channels=32, posterior_layers=4)
    c = c.eval().cuda()
    c.frontend.batch_invariant = True       # the mode in which the front-end's stream has its whole-row bits
    return c


@pytest.mark.parametrize("nq", [1, 3])
def test_codec_encode_stream_gives_encodes_codes(nq):
    c = make_codec(nq)
    wave = 0.1 * torch.randn(2, 5000, generator=torch.Generator().manual_seed(nq)).cuda()
    want = c.encode(wave)
    assert want.shape == ((2, want.shape[-1]) if nq == 1 else (3, 2, want.shape[-1])) and want.shape[-1] > 2 * c.encoder.reach_frames
    sizes, a = [], 0
    while a < 5000:
        for n in (1000, 1, 37):
            n = min(n, 5000 - a)
            sizes.append(n)
            a += n
    with c.encode_stream(2, 1000) as st:
        parts = []
        a = 0
        for i, n in enumerate(sizes):
            chunk = wave[:, a:a + n]
            parts.append(st.push(chunk[:, None, :] if i % 2 else chunk))
            a += n
            assert parts[-1].dtype == want.dtype and parts[-1].shape[:-1] == want.shape[:-1]
        assert st.received_samples == 5000
        parts.append(st.flush())
        got = torch.cat(parts, dim=-1)
        assert got.shape == want.shape and torch.equal(got, want)
        assert any(p.shape[-1] == 0 for p in parts) and sum(p.shape[-1] > 0 for p in parts) > 2
        st.reset()                       # and once more on the same stream, another utterance
        short = wave[:, :1203]
        got = torch.cat([st.push(short[:, :1000]), st.push(short[:, 1000:]), st.flush()], dim=-1)
        assert torch.equal(got, c.encode(short))
    with pytest.raises(FishVocError):
        c.encode_stream(2, 64).push(wave[:, :65])


def test_codec_command_line_chunked_writes_the_same_file(tmp_path):
    from vocoder_amd.inference import write_wav
    arch = ["--n-fft", "64", "--hop-length", "16", "--win-length", "64", "--latent-size", "32", "--codebook-size", "48", "--num-quantizers", "2",
            "--encoder", "posterior", "--hidden-channels", "32"]
    write_wav(tmp_path / "a.wav", 0.1 * np.random.default_rng(0).standard_normal(5000).astype(np.float32), 24000)
    torch.manual_seed(0)                      # no checkpoint: the untrained initialisation, the same for both calls
    assert codec.main(["encode", "-i", str(tmp_path / "a.wav"), "-o", str(tmp_path / "whole")] + arch) == 0
    torch.manual_seed(0)
    assert codec.main(["encode", "-i", str(tmp_path / "a.wav"), "-o", str(tmp_path / "chunked"), "--chunk-samples", "777"] + arch) == 0
    whole, chunked = np.load(tmp_path / "whole" / "a.codes.npy"), np.load(tmp_path / "chunked" / "a.codes.npy")
    assert whole.dtype == chunked.dtype == np.int64 and whole.shape == chunked.shape and whole.shape[0] == 2 and whole.shape[1] > 64
    assert np.array_equal(whole, chunked)
