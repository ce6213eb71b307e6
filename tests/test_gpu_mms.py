"""GPU: MMSEncoder's two kernels (vocoder_amd/csrc/mms_front.hip) through the C ABI, and ``vocoder_amd.modules.encoders.MMSEncoder``.

The normalisation is held to the float64 restatement (mms_reference.py) by a bound derived from its own roundings; the interpolation is a
pure gather and is held to bit equality with ``torch.nn.functional.interpolate`` on the CPU; the module is held to the reference's goldens
(every row run ALONE through the reference on the CPU) at the project's parity bar, max |d| <= 1e-4 of the expected tensor's own peak.
Everything else is bit-exact: a row alone / in a batch / in another order / padded, exact zeros past a row's counts, poisoned padding.
Each parity case prints what it measured.  Nothing here reads the reference or imports ``transformers``."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import mms_reference as mref
from resample_reference import Filter
from vocoder_amd import _lib
from vocoder_amd import synthetic as syn
from vocoder_amd.modules.encoders import MMSEncoder

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("tiny", "rate")
BAR = 1e-4
U, E64 = 2.0 ** -24, 2.0 ** -53
SEG = 4096          # samples per segment of the normalisation's sums


def bits(a) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b) -> bool:
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def golden(name):
    g = np.load(os.path.join(GOLDEN, f"mms_{name}.npz"))
    cfg = json.loads(bytes(g["config"]).decode())
    return cfg, syn.mms_state_dict(cfg, int(g["seed"])), {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def module(name, hop):
    cfg, sd, g = golden(name)
    m = MMSEncoder(sampling_rate=int(g["sampling_rate"]), hop_length=hop, config=cfg)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().cuda()


@functools.lru_cache(maxsize=None)
def sample_rows():
    """The rows the normalisation kernel sees on the fixtures: mms_tiny's waves (1500, 613 and 40 samples) and mms_rate's waves at 16 kHz
    (8000 — two segments —, 4322 and 436 samples), then the longest with a DC offset of 100 x its deviation."""
    rows = []
    for name in FIXTURES:
        _, _, g = golden(name)
        rate = int(g["sampling_rate"])
        for b, n in enumerate(g["lengths"]):
            x = g["waves"][b, : int(n)]
            rows.append(x if rate == 16000 else Filter(rate, 16000)(x).astype(np.float32))
    long = max(rows, key=len)
    rows.append((long + np.float32(100.0 * long.std())).astype(np.float32))
    return rows


def normalize(x: torch.Tensor, lengths=None, out=None) -> torch.Tensor:
    """fv_mms_normalize on a (B, T) device tensor; the output starts as NaN, so every element must be written."""
    L = _lib.lib()
    B, T = x.shape
    y = torch.full_like(x, float("nan")) if out is None else out
    need = int(L.fv_mms_normalize_workspace_bytes(B, T))
    ws = torch.full((max(need, 16),), 0xA5, dtype=torch.uint8, device="cuda")
    lp = None if lengths is None else (ctypes.c_int32 * B)(*lengths)
    _lib.check(L.fv_mms_normalize(x.data_ptr(), T, lp, B, y.data_ptr(), ws.data_ptr(), need, int(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return y


def interpolate(x: torch.Tensor, N: int, frames=None, out_frames=None) -> torch.Tensor:
    """fv_mms_interpolate on a (B, F, H) device tensor -> (B, H, N); the output starts as NaN."""
    L = _lib.lib()
    B, F, H = x.shape
    y = torch.full((B, H, N), float("nan"), device="cuda")
    arr = lambda v: None if v is None else (ctypes.c_int32 * B)(*v)      # noqa: E731
    _lib.check(L.fv_mms_interpolate(x.data_ptr(), F, H, arr(frames), arr(out_frames), B, y.data_ptr(), N, int(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return y


def padded(rows, T, fill=0.0):
    x = np.full((len(rows), T), fill, np.float32)
    for b, r in enumerate(rows):
        x[b, : len(r)] = r
    return torch.from_numpy(x).cuda()


def test_normalize_against_float64_within_its_own_roundings():
    """With z = (x - m) r, r = 1 / sqrt(var + 1e-7), exact, the kernel computes y = fl(fl(x - m^) r^) in fp32 where
      m^ = fl32(m64), |m^ - m| <= u |m| + d e64 mean|x|      the cast of the mean, and the fp64 sum behind it: every partial sum passes
                                                              through at most d = 16 + 6 + 3 + segments additions (a thread's 16 samples, the
                                                              butterfly, the four waves, the segments), each with relative error e64 = 2^-53
      r^ = fl32(r64), |r^ / r - 1| <= u + k                   the cast of the reciprocal deviation; k = (1.5 d + 4) e64 E[x^2] / (var + 1e-7)
                                                              from the same bound on sum x^2 (x^2 is exact in fp64) and on m^2, halved by
                                                              the square root, plus the division, the root and the reciprocal
    and the subtraction and the product round once each (u = 2^-24).  So
      |y - z| <= (|z| (3 u + k) + (u |m| + d e64 mean|x|) r) (1 + 8 u)
    The first term is the three roundings that scale the value, the second the rounded mean, which a DC offset of 100 deviations raises
    to 100 u.  Nothing in the bound is fitted to the kernel's output."""
    rows = sample_rows()
    T = max(len(r) for r in rows)
    got = normalize(padded(rows, T), [len(r) for r in rows]).cpu().numpy()
    worst = 0.0
    for b, x in enumerate(rows):
        x64 = x.astype(np.float64)
        z = mref.normalize(x64)
        m, var = x64.mean(), x64.var()
        r = 1.0 / np.sqrt(var + mref.EPS)
        d = 16 + 6 + 3 + -(-len(x) // SEG)
        k = (1.5 * d + 4) * E64 * (x64 ** 2).mean() / (var + mref.EPS)
        bound = (np.abs(z) * (3 * U + k) + (U * abs(m) + d * E64 * np.abs(x64).mean()) * r) * (1 + 8 * U)
        err = np.abs(got[b, : len(x)] - z)
        ratio = float((err / bound).max())
        worst = max(worst, float(err.max()))
        print(f"normalize row {b} ({len(x)} samples, mean / deviation = {m * r:.3g}): max |d| = {err.max():.3e}, max |d| / bound = {ratio:.3f}")
        assert np.isfinite(got[b]).all() and (err <= bound).all(), (b, ratio)
        assert not bits(got[b, len(x):]).any()                          # exact zeros past the row's length
    print(f"normalize: largest |d| over all rows = {worst:.3e}")


def test_normalize_constant_and_empty_rows_give_zeros():
    rows = [np.full(613, 3.25, np.float32), np.zeros(0, np.float32), np.full(5000, -1e-3, np.float32), sample_rows()[1]]
    x = padded(rows, 5001, fill=float("nan"))           # padding is poison: it is never read
    y = normalize(x, [len(r) for r in rows])
    assert not bits(y[:3]).any()
    assert not torch.isnan(y).any() and float(y[3, :613].abs().max()) > 1 and not bits(y[3, 613:]).any()


def test_normalize_a_row_has_the_same_bits_alone_batched_reordered_padded_and_in_place():
    rows = sample_rows()
    lengths = [len(r) for r in rows]
    T = max(lengths)                                    # 8000: whole quads, 16-byte accesses
    batch = normalize(padded(rows, T), lengths)
    order = list(range(len(rows)))[::-1]
    rev = normalize(padded([rows[i] for i in order], T), [lengths[i] for i in order])
    odd = normalize(padded(rows, T + 777, fill=float("nan")), lengths)          # 8777: single floats, and poisoned padding
    wide = normalize(padded(rows, T + 4100), lengths)                           # one more segment than any row has
    inplace = padded(rows, T)
    normalize(inplace, lengths, out=inplace)
    for b, n in enumerate(lengths):
        alone = normalize(padded([rows[b]], n))                                 # no lengths: the row fills its tensor
        assert same(alone[0], batch[b, :n])
        assert same(rev[order.index(b)], batch[b])
        assert same(odd[b, :n], batch[b, :n]) and not bits(odd[b, n:]).any()
        assert same(wide[b, :n], batch[b, :n]) and not bits(wide[b, n:]).any()
        assert same(inplace[b], batch[b])


INTERP_CASES = [        # (F, N, H): the fixtures' own frame counts, then the edges
    (149, 375, 128), (60, 153, 128), (3, 10, 128),      # mms_tiny at hop 4: N > F, frames repeat 2 and 3 times
    (149, 46, 128), (60, 19, 128), (3, 1, 128),         # mms_tiny at hop 32: N < F, frames are skipped
    (24, 43, 192), (13, 23, 192), (1, 2, 192),          # mms_rate; the last has F = 1
    (60, 60, 128), (149, 149, 128),                     # N = F
    (149, 376, 128), (24, 44, 192),                     # N a multiple of 4: 16-byte stores
    (24, 43, 100), (24, 44, 68), (13, 64, 4),           # H not a multiple of the 64-channel tile, with either store
]


@pytest.mark.parametrize("F,N,H", INTERP_CASES)
def test_interpolate_is_bit_equal_to_torch_on_the_cpu(F, N, H):
    x = torch.from_numpy(np.random.default_rng(F * 1000 + N).standard_normal((2, F, H)).astype(np.float32))
    want = torch.nn.functional.interpolate(x.transpose(1, 2), size=N, mode="nearest")
    got = interpolate(x.cuda(), N)
    assert got.shape == (2, H, N) and same(got, want)
    assert same(got[0], mref.interpolate(x[0].numpy(), N))


@pytest.mark.parametrize("N", (375, 376))
def test_interpolate_ragged_rows(N):
    """Rows with their own (F_b, N_b): zeros past N_b, nothing read past F_b (poison), the bits of the row alone."""
    H, F = 128, 149
    counts = [(149, N), (60, 153), (3, 10), (0, 0), (1, 2), (149, 46)]
    rng = np.random.default_rng(77)
    x = np.full((len(counts), F, H), np.nan, np.float32)
    for b, (fb, _) in enumerate(counts):
        x[b, :fb] = rng.standard_normal((fb, H)).astype(np.float32)
    got = interpolate(torch.from_numpy(x).cuda(), N, [c[0] for c in counts], [c[1] for c in counts])
    assert not torch.isnan(got).any()
    for b, (fb, nb) in enumerate(counts):
        assert not bits(got[b, :, nb:]).any()
        if nb == 0:
            continue
        row = torch.from_numpy(x[b:b + 1, :fb])
        want = torch.nn.functional.interpolate(row.transpose(1, 2), size=nb, mode="nearest")
        assert same(got[b, :, :nb], want[0])
        assert same(interpolate(row.cuda(), nb)[0], got[b, :, :nb])


def parity(tag, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
    print(f"{tag}: max |d| / peak = {err:.2e} (peak {np.abs(want).max():.3g})")
    assert got.shape == want.shape and np.isfinite(got).all() and err <= BAR, (tag, err)
    return err


def fixture_modules():
    return [(name, int(hop)) for name in FIXTURES for hop in golden(name)[2]["hops"]]


@pytest.mark.parametrize("name,hop", fixture_modules())
def test_goldens_through_the_module(name, hop):
    cfg, _, g = golden(name)
    m, lengths, waves = module(name, hop), g["lengths"].tolist(), torch.from_numpy(g["waves"]).cuda()
    batch = m(waves, lengths=lengths)
    assert batch.shape == (len(lengths), cfg["hidden_size"], waves.shape[1] // hop)
    for b, n in enumerate(lengths):
        want = g[f"out_h{hop}_{b}"]
        alone = m(waves[b:b + 1, :n])
        assert alone.shape == (1,) + want.shape
        parity(f"golden mms_{name} hop {hop} row {b} alone", alone[0].cpu().numpy(), want)
        parity(f"golden mms_{name} hop {hop} row {b} in the ragged batch", batch[b, :, : want.shape[1]].cpu().numpy(), want)


@pytest.mark.parametrize("name,hop", fixture_modules())
def test_a_row_has_the_same_bits_alone_ragged_listed_and_with_a_channel_axis(name, hop):
    _, _, g = golden(name)
    m, lengths, waves = module(name, hop), g["lengths"].tolist(), torch.from_numpy(g["waves"]).cuda()
    batch = m(waves, lengths=lengths)
    listed = m.forward_list([waves[b, :n] for b, n in enumerate(lengths)])
    poisoned = waves.clone()
    for b, n in enumerate(lengths):
        poisoned[b, n:] = float("nan")
    assert same(m(poisoned, lengths=torch.tensor(lengths)), batch)            # padding is never read; lengths may be a tensor
    for b, n in enumerate(lengths):
        nb = n // hop
        alone = m(waves[b:b + 1, :n])
        assert same(alone[0], batch[b, :, :nb]) and not bits(batch[b, :, nb:]).any()
        assert listed[b].shape == (batch.shape[1], nb) and same(listed[b], alone[0])
    assert same(m(waves[:, None], lengths=lengths), batch)                    # (B, 1, L) is the same call
    full = m(waves[:2, : lengths[1]])                                         # no lengths: every row holds L samples
    assert same(m(waves[:2, None, : lengths[1]]), full) and same(full[1], batch[1, :, : lengths[1] // hop])


def test_codec_with_an_mms_encoder_encodes_audio_to_codes():
    from vocoder_amd.codec import VQVAECodec
    from vocoder_amd.modules.quantizers import VectorQuantization
    cfg, _, g = golden("tiny")
    hop, H, K = 32, cfg["hidden_size"], 64
    m = module("tiny", hop)
    vq = VectorQuantization(dim=H, codebook_size=K, kmeans_init=False)
    embed = torch.from_numpy(np.random.default_rng(5).standard_normal((K, H)).astype(np.float32))
    vq.load_state_dict({**vq.state_dict(), "_codebook.embed": embed}, strict=True)
    codec = VQVAECodec(m, torch.nn.Identity(), vq.eval().cuda(), hop_length=hop)
    audio = torch.from_numpy(g["waves"][:2, :613]).cuda()
    codes = codec.encode(audio[:, None])
    assert codes.shape == (2, 613 // hop) and codes.dtype == torch.int64
    assert torch.equal(codes, codec.encode(audio))
    latent = m(audio)                                                          # the encoder slot received the audio itself
    want = torch.cdist(latent.transpose(1, 2).cpu().double(), embed.double()[None]).argmin(-1)
    assert torch.equal(codes.cpu(), want)
