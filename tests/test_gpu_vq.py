"""GPU: the vector quantiser (vocoder_amd/csrc/vq.hip) through ``vocoder_amd.modules.quantizers``, ``UnifyGenerator(vq=...)``,
``vocoder_amd.codec`` and the C ABI.

Codes are compared with the fp64 restatement (vq_reference.py) on every DECIDABLE frame — one whose fp64 gap between the best and the
second-best score exceeds, at every layer, the dot-product error bound tau (any summation order) — exactly; at most 1 % of a case's frames
may be undecidable (more is a failure of the inputs), and every frame's chosen code must score within tau of the best along the GPU's own
path.  Values are bit-exact: z against a CPU gather-and-add of the GPU's codes, decode against z, and every invariance (alone / batch /
chunked along T / slice count / both frame tilings).  Each case prints what it measured."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import vq_reference as vref
from vocoder_amd import _lib
from vocoder_amd import synthetic as syn
from vocoder_amd.modules.quantizers import ResidualVectorQuantization, VectorQuantization

pytestmark = pytest.mark.gpu

SHAPES = [(64, 256, 1), (96, 320, 3), (7, 5, 2), (128, 1024, 8)]
# N frames as (B, T): one frame; below and above one 32-frame tile; several tiles over three rows
LAYOUTS = {1: (1, 1), 31: (1, 31), 33: (3, 11), 375: (3, 125), 64: (2, 32)}
CASES = [(D, K, nq, N) for (D, K, nq) in SHAPES for N in (1, 31, 33, 375)] + [(512, 4096, 1, 64)]      # the codec's own shape: 64 frames only


def make_vq(D, K, nq, embeds, rvq=None):
    """A loaded quantiser on the device; the residual class for nq > 1 (vae.py:66-78), or on request."""
    if nq > 1 or rvq:
        m = ResidualVectorQuantization(num_quantizers=nq, dim=D, codebook_size=K, kmeans_init=False)
        sd = {f"layers.{q}._codebook.embed": torch.from_numpy(e) for q, e in enumerate(embeds)}
    else:
        m = VectorQuantization(dim=D, codebook_size=K, kmeans_init=False)
        sd = {"_codebook.embed": torch.from_numpy(embeds[0])}
    m.load_state_dict({**m.state_dict(), **sd}, strict=True)
    return m.eval().cuda()


def to_bdt(x: np.ndarray, B: int, T: int) -> torch.Tensor:
    """Frames (N, D), n = b T + t  ->  (B, D, T) on the device."""
    return torch.from_numpy(np.ascontiguousarray(x.reshape(B, T, -1).transpose(0, 2, 1))).cuda()


def frames_of(z: torch.Tensor) -> np.ndarray:
    return z.cpu().numpy().transpose(0, 2, 1).reshape(-1, z.shape[1])


def codes_of(codes: torch.Tensor) -> np.ndarray:
    c = codes.cpu().numpy()
    return c.reshape(1, -1) if c.ndim == 2 else c.reshape(c.shape[0], -1)


def bits(a) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def reference(D, K, nq, N):
    """The case's inputs and their fp64 codes.  With N < 100 a single undecidable frame is above the 1 % the inputs may leave, so the seed of a
    case is the first of 0 .. 3 at which the restatement ALONE (CPU, nothing of the code under test) leaves at most 1 %; the test still
    asserts the share."""
    for seed in range(4):
        x, embeds = vref.make_case(D, K, nq, N, seed)
        ref = vref.encode(x, embeds)
        if 1.0 - ref[2].mean() <= 0.01:
            break
    return (x, embeds) + ref


@pytest.mark.parametrize("D,K,nq,N", CASES)
def test_codes_and_values_against_the_reference(D, K, nq, N):
    x, embeds, ref_codes, ref_z, dec = reference(D, K, nq, N)
    B, T = LAYOUTS[N]
    vq = make_vq(D, K, nq, embeds)
    res = vq(to_bdt(x, B, T))
    z, codes, loss = res
    assert codes.dtype == torch.int64 and codes.shape == ((B, T) if nq == 1 else (nq, B, T)) and z.shape == (B, D, T)
    assert loss.shape == ((1,) if nq == 1 else (nq, 1)) and not loss.any()
    c = codes_of(codes)
    undecidable = 1.0 - dec.mean()
    mism = (c != ref_codes).any(axis=0)
    excess = vref.path_excess(x, embeds, c)
    print(f"(D {D}, K {K}, n_q {nq}, N {N}): undecidable {100 * undecidable:.2f} %, mismatching frames {int(mism.sum())} "
          f"(decidable: {int((mism & dec).sum())}), worst (score deficit - tau) {excess.max():.3e}")
    assert undecidable <= 0.01, "the inputs leave too many frames undecidable"
    assert c.min() >= 0 and c.max() < K
    assert not (mism & dec).any()
    assert (excess <= 0).all()
    # values: the GPU's own codes, gathered and added on the CPU in layer order
    assert np.array_equal(bits(frames_of(z)), bits(vref.gather_sum(c, embeds)))
    assert np.array_equal(bits(vq.decode(codes)), bits(z))
    z2, codes2 = vq.from_codes(codes)
    assert codes2 is codes and np.array_equal(bits(z2), bits(z))
    assert torch.equal(vq.encode(to_bdt(x, B, T)), codes)


def test_exact_cases():
    D, K = 24, 40
    rng = np.random.default_rng(5)
    # rows duplicated at j < j': j' never comes back
    base = rng.standard_normal((K // 2, D)).astype(np.float32)
    embed = np.concatenate([base, base])[rng.permutation(K)]
    first = {}
    for j, row in enumerate(embed):
        first.setdefault(row.tobytes(), j)
    x = rng.standard_normal((200, D)).astype(np.float32)
    vq = make_vq(D, K, 1, [embed])
    c = codes_of(vq.encode(to_bdt(x, 2, 100)))[0]
    assert all(first[embed[j].tobytes()] == j for j in c)
    # frames that ARE rows of a well-separated codebook: that row's index, z == x bit for bit
    embed = (4.0 * rng.standard_normal((K, D))).astype(np.float32)
    pick = rng.integers(0, K, 70)
    z, codes, _ = make_vq(D, K, 1, [embed])(to_bdt(embed[pick], 1, 70))
    assert np.array_equal(codes_of(codes)[0], pick) and np.array_equal(bits(frames_of(z)), bits(embed[pick]))
    # a frame of NaNs takes code 0 (at every layer: its residual stays NaN); its neighbours are untouched
    x, embeds = vref.make_case(D, K, 2, 9, seed=1)
    want = vref.encode(x, embeds)[0]
    x[4] = np.nan
    z, codes, _ = make_vq(D, K, 2, embeds)(to_bdt(x, 1, 9))
    c = codes_of(codes)
    assert c[:, 4].tolist() == [0, 0] and np.array_equal(np.delete(c, 4, 1), np.delete(want, 4, 1))
    assert np.array_equal(bits(frames_of(z)), bits(vref.gather_sum(c, embeds)))
    # decode: a negative code contributes nothing, an all-negative frame is exact zeros, a code >= K is an IndexError
    vq = make_vq(D, K, 2, embeds)
    cc = torch.tensor([[[3, -1, -1, 5]], [[7, 2, -1, -1]]], device="cuda")
    assert np.array_equal(bits(frames_of(vq.decode(cc))), bits(vref.gather_sum(cc.cpu().numpy().reshape(2, -1), embeds)))
    assert not vq.decode(cc)[0, :, 2].any()
    assert np.array_equal(bits(frames_of(vq.decode(cc[:1]))), bits(vref.gather_sum(cc[:1].cpu().numpy().reshape(1, -1), embeds)))
    with pytest.raises(IndexError):
        vq.decode(torch.tensor([[[K]], [[0]]], device="cuda"))


def test_invariance_alone_batch_chunks_and_slices():
    D, K, nq, B, T = 96, 320, 3, 3, 40
    x, embeds = vref.make_case(D, K, nq, B * T, seed=2)
    xt = to_bdt(x, B, T)
    vq = make_vq(D, K, nq, embeds)
    z, codes, _ = vq(xt)
    for b in range(B):      # a batch of one
        zb, cb, _ = vq(xt[b:b + 1])
        assert torch.equal(cb, codes[:, b:b + 1]) and np.array_equal(bits(zb), bits(z[b:b + 1]))
    for b, t in ((0, 0), (1, 17), (2, 39)):      # a frame alone
        zf, cf, _ = vq(xt[b:b + 1, :, t:t + 1])
        assert torch.equal(cf, codes[:, b:b + 1, t:t + 1]) and np.array_equal(bits(zf), bits(z[b:b + 1, :, t:t + 1]))
    cuts = [0, 1, 5, 32, 33, T]                  # chunks along T: strided views of the batch, as a stream would pass them
    zs, cs = zip(*[vq(xt[:, :, a:b])[:2] for a, b in zip(cuts, cuts[1:])])
    assert torch.equal(torch.cat(cs, dim=2), codes) and np.array_equal(bits(torch.cat(zs, dim=2)), bits(z))
    assert np.array_equal(bits(torch.cat([vq.decode(codes[:, :, a:b]) for a, b in zip(cuts, cuts[1:])], dim=2)), bits(z))
    for slices in (1, 2):                        # K = 320 is 10 code tiles: two slicing granules
        vq.slices = slices
        z2, c2, _ = vq(xt)
        assert torch.equal(c2, codes) and np.array_equal(bits(z2), bits(z))
    # K = 1024 has four granules: 1, 3 (uneven) and 4 slices
    x, embeds = vref.make_case(128, 1024, 2, 70, seed=4)
    vq = make_vq(128, 1024, 2, embeds)
    z, codes, _ = vq(to_bdt(x, 1, 70))
    for slices in (1, 3, 4):
        vq.slices = slices
        z2, c2, _ = vq(to_bdt(x, 1, 70))
        assert torch.equal(c2, codes) and np.array_equal(bits(z2), bits(z))


def test_large_launches_take_two_frame_tiles_with_the_same_bits():
    """A workgroup takes two 32-frame tiles where that still leaves two workgroups per compute unit (K = 1024: four slicing granules): same
    codes, same bits.  D = 40 is five chunks of 8 channels, padded to two groups of four."""
    D, K, nq = 40, 1024, 2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 64 * (2 * cus // 4) + 5 - 64          # just enough 64-frame tiles; the last one is partial
    x, embeds = vref.make_case(D, K, nq, N, seed=6)
    ref_codes, _, dec = vref.encode(x, embeds)
    vq = make_vq(D, K, nq, embeds)
    z, codes, _ = vq(to_bdt(x, 1, N))
    assert _lib.last_kernel() == "vq_search_kernel<2>"
    c = codes_of(codes)
    print(f"N {N}: undecidable {100 * (1 - dec.mean()):.2f} %, mismatching decidable frames {int(((c != ref_codes).any(0) & dec).sum())}")
    assert 1 - dec.mean() <= 0.01 and not ((c != ref_codes).any(0) & dec).any()
    assert (vref.path_excess(x, embeds, c) <= 0).all()
    assert np.array_equal(bits(frames_of(z)), bits(vref.gather_sum(c, embeds)))
    for a, b in ((0, N - 64), (0, 100), (N - 41, N)):        # the same frames in launches below the threshold
        zs, cs, _ = vq(to_bdt(x[a:b], 1, b - a))
        assert _lib.last_kernel() == "vq_search_kernel<1>"
        assert torch.equal(cs, codes[:, :, a:b]) and np.array_equal(bits(zs), bits(z[:, :, a:b]))


def test_ragged_rows():
    D, K, nq, T = 96, 320, 3, 12
    lengths = [0, 5, 12]
    x, embeds = vref.make_case(D, K, nq, 3 * T, seed=7)
    xt = to_bdt(x, 3, T)
    for b, n in enumerate(lengths):
        xt[b, :, n:] = float("nan")             # a NaN in the output, or a changed code, means padding was read
    vq = make_vq(D, K, nq, embeds)
    z, codes, _ = vq(xt, lengths)
    for b, n in enumerate(lengths):
        assert (codes[:, b, n:] == -1).all() and not bits(z[b, :, n:]).any()
        if n:
            zb, cb, _ = vq(xt[b:b + 1, :, :n])
            assert torch.equal(cb, codes[:, b:b + 1, :n]) and np.array_equal(bits(zb), bits(z[b:b + 1, :, :n]))
    assert np.array_equal(bits(vq.decode(codes)), bits(z))
    assert np.array_equal(bits(vq.decode(codes.clamp(min=0), lengths)), bits(z))
    assert torch.equal(vq.encode(xt, torch.tensor(lengths)), codes)
    with pytest.raises(ValueError, match="lengths"):
        vq(xt, [0, 5, 13])
    # more rows than one launch carries lengths for (256)
    B, T = 300, 2
    x, embeds = vref.make_case(7, 5, 2, B * T, seed=8)
    lengths = np.random.default_rng(0).integers(0, T + 1, B)
    xt = to_bdt(x, B, T)
    for b, n in enumerate(lengths):
        xt[b, :, n:] = float("nan")
    vq = make_vq(7, 5, 2, embeds)
    z, codes, _ = vq(xt, lengths.tolist())
    valid = (np.arange(T)[None, :] < lengths[:, None]).reshape(-1)
    full = codes_of(vq(to_bdt(x, B, T)).codes)
    assert np.array_equal(codes_of(codes), np.where(valid[None, :], full, -1))
    assert np.array_equal(bits(frames_of(z)), bits(vref.gather_sum(codes_of(codes), embeds)))
    assert np.array_equal(bits(vq.decode(codes)), bits(z))


def _t(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def _tiny_pairs():
    from vocoder_amd.modules.encoders import ConvNeXtEncoder
    from vocoder_amd.modules.generators import HiFiGANGenerator, ISTFTHead
    fire = dict(backbone=dict(input_channels=20, depths=[1, 1], dims=[32, 64], kernel_size=7),
                head=dict(hop_length=16, upsample_rates=[4, 2, 2], upsample_kernel_sizes=[8, 4, 4], resblock_kernel_sizes=[3, 7, 11],
                          resblock_dilation_sizes=[[1, 3, 5]] * 3, num_mels=64, upsample_initial_channel=64, use_template=False,
                          pre_conv_kernel_size=13, post_conv_kernel_size=13))
    vocos = dict(backbone=dict(input_channels=20, depths=[1, 1], dims=[32, 64], kernel_size=7),
                 head=dict(dim=64, n_fft=64, hop_length=16, win_length=64, padding="same"))
    yield "convnext + hifigan", fire, syn.firefly_state_dict(fire, 4), lambda: (ConvNeXtEncoder(**fire["backbone"]), HiFiGANGenerator(**fire["head"]))
    yield "vocos pair", vocos, syn.vocos_state_dict(vocos, 3), lambda: (ConvNeXtEncoder(**vocos["backbone"]), ISTFTHead(**vocos["head"]))


@pytest.mark.parametrize("nq", [1, 3])
def test_unify_generator_with_a_quantiser(nq):
    from vocoder_amd.modules.generators import UnifyGenerator
    for name, cfg, sd, make in _tiny_pairs():
        D, K = 64, 48
        embeds = [(0.5 * 0.6 ** q * np.random.default_rng(q).standard_normal((K, D))).astype(np.float32) for q in range(nq)]
        backbone, head = make()
        u = UnifyGenerator(backbone, head, vq=make_vq(D, K, nq, embeds).cpu())
        vsd = {f"vq.{k}": v for k, v in u.vq.state_dict().items()}
        u.load_state_dict({**_t(sd), **vsd}, strict=True)
        u = u.eval().cuda()
        mel = torch.from_numpy(syn.synthetic_mel(2, 20, 9, 3)).cuda()
        audio, res = u(mel)
        lat = u.backbone(mel)
        want = u.vq(lat)
        y = u.head(want.z)
        y = y[:, None, :] if y.ndim == 2 else y
        assert audio.shape == (2, 1, 9 * 16), name
        assert torch.equal(res.codes, want.codes) and np.array_equal(bits(res.z), bits(want.z)) and np.array_equal(bits(audio), bits(y)), name
        codes = u.encode(mel)
        assert torch.equal(codes, want.codes) and np.array_equal(bits(u.decode(codes)), bits(audio)), name


def test_codec_round_trip_lengths_and_checkpoint_keys(tmp_path):
    from vocoder_amd import codec
    kw = dict(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, encoder_depths=(1,), encoder_dims=(32,), decoder_depths=(1, 1),
              decoder_dims=(32, 64))
    for nq in (1, 2):
        src = codec.build_vqvae(num_quantizers=nq, **kw)
        # a Lightning-style dict: generator.* / vq.* next to keys of other modules, which are dropped
        ckpt = {"state_dict": {**{f"generator.{k}": v for k, v in src.state_dict().items() if k.startswith(("encoder.", "decoder."))},
                               **{k: v for k, v in src.state_dict().items() if k.startswith("vq.")},
                               "discriminators.mpd.weight": torch.zeros(3)}}
        path = tmp_path / f"vqvae{nq}.pt"
        torch.save(ckpt, path)
        m = codec.build_vqvae(num_quantizers=nq, **kw)
        res = m.load_checkpoint(path)
        assert not res.missing_keys and not res.unexpected_keys
        for k, v in src.state_dict().items():
            assert torch.equal(m.state_dict()[k], v), k
        with pytest.raises(RuntimeError):      # strict: a quantiser of another depth does not load
            codec.build_vqvae(num_quantizers=nq + 1, **kw).load_checkpoint(path)
        m = m.eval().cuda()
        for L in (16 * 9, 16 * 9 + 7, 16 * 9 - 5):
            audio = (0.1 * torch.randn(2, 1, L, generator=torch.Generator().manual_seed(L))).cuda()
            fake, aux = m(audio)
            assert fake.shape == audio.shape and aux == 0 and torch.isfinite(fake).all()
        audio = (0.1 * torch.randn(2, 1, 16 * 9, generator=torch.Generator().manual_seed(1))).cuda()
        codes = m.encode(audio)
        assert codes.dtype == torch.int64 and codes.shape == ((2, 9) if nq == 1 else (nq, 2, 9))
        assert np.array_equal(bits(m.decode(codes)), bits(m(audio)[0]))
        assert torch.equal(m.encode(m.frontend(audio)), codes)          # a spectrogram goes straight into the encoder


def test_c_abi_refusals_enqueue_nothing():
    L = _lib.lib()
    D, K, nq, B, T = 16, 40, 2, 2, 10
    x, embeds = vref.make_case(D, K, nq, B * T, seed=9)
    h = ctypes.c_void_p()
    assert L.fv_vq_create(ctypes.byref(_lib.VQConfig(D, K, nq)), ctypes.byref(h)) == 0
    try:
        for q, e in enumerate(embeds):
            assert L.fv_vq_load_codebook(h, q, e.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
        xt = to_bdt(x, B, T)
        need = int(L.fv_vq_workspace_bytes(h, B, T))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        codes = torch.full((nq, B, T), -7, dtype=torch.int32, device="cuda")
        z = torch.full((B, D, T), 3.5, device="cuda")
        stream = int(torch.cuda.current_stream().cuda_stream)

        def call(stride=T, frames=None, bytes_=need):
            return L.fv_vq_encode(h, xt.data_ptr(), stride, frames, codes.data_ptr(), z.data_ptr(), B, T, ws.data_ptr(), bytes_, stream)

        for kwargs, word in ((dict(bytes_=need - 1), "workspace"), (dict(stride=T - 1), "stride"),
                             (dict(frames=(ctypes.c_int32 * B)(3, T + 1)), "host_frames[1]")):
            assert call(**kwargs) == _lib.FV_ERR_INVALID and word in L.fv_last_error().decode(), (kwargs, L.fv_last_error())
            torch.cuda.synchronize()
            assert (codes == -7).all() and (z == 3.5).all()         # nothing was enqueued
        assert L.fv_vq_decode(h, codes.data_ptr(), (ctypes.c_int32 * B)(-1, 2), z.data_ptr(), B, T, stream) == _lib.FV_ERR_INVALID
        assert "host_frames[0]" in L.fv_last_error().decode()
        torch.cuda.synchronize()
        assert (z == 3.5).all()
        assert call() == 0
        torch.cuda.synchronize()
        want = vref.encode(x, embeds)
        got = codes.cpu().numpy().reshape(nq, -1)
        assert not ((got != want[0]).any(0) & want[2]).any()
        assert np.array_equal(bits(frames_of(z)), bits(vref.gather_sum(got, embeds)))
    finally:
        torch.cuda.synchronize()
        L.fv_vq_destroy(h)


def test_codec_command_line_round_trip(tmp_path):
    """``python -m vocoder_amd.codec encode`` writes ``<stem>.codes.npy``, ``decode`` reads it back into ``<stem>.wav`` (in process: the test is
    about the files, not the interpreter start)."""
    from vocoder_amd import codec
    from vocoder_amd.inference import read_wav, write_wav
    arch = ["--n-fft", "64", "--hop-length", "16", "--win-length", "64", "--latent-size", "32", "--codebook-size", "48", "--num-quantizers", "2"]
    wav = 0.1 * np.random.default_rng(0).standard_normal(16 * 11).astype(np.float32)
    write_wav(tmp_path / "a.wav", wav, 24000)
    torch.manual_seed(0)                      # no checkpoint: the untrained initialisation, the same for both calls
    assert codec.main(["encode", "-i", str(tmp_path / "a.wav"), "-o", str(tmp_path / "out")] + arch) == 0
    codes = np.load(tmp_path / "out" / "a.codes.npy")
    assert codes.dtype == np.int64 and codes.shape == (2, 11) and codes.min() >= 0 and codes.max() < 48
    torch.manual_seed(0)
    m = codec.build_vqvae(64, 16, 64, 32, 48, 2, encoder_dims=(32,), decoder_dims=(32, 64)).eval().cuda()
    pcm, sr = read_wav(tmp_path / "a.wav")
    assert sr == 24000 and np.array_equal(m.encode(torch.from_numpy(pcm)[None].cuda())[:, 0].cpu().numpy(), codes)
    torch.manual_seed(0)
    assert codec.main(["decode", "-i", str(tmp_path / "out" / "a.codes.npy"), "-o", str(tmp_path / "out")] + arch) == 0
    audio, sr = read_wav(tmp_path / "out" / "a.wav")
    want = m.decode(torch.from_numpy(codes)[:, None, :].cuda())[0, 0].cpu().numpy()
    assert sr == 24000 and audio.shape == (1, 16 * 11)
    assert np.abs(audio[0] - np.clip(want, -1, 1)).max() <= 1.0 / 32767          # 16-bit PCM on the way
