"""GPU: the resampler kernel (vocoder_amd/csrc/resample.hip) through ``vocoder_amd.resample.Resample`` — parity with the float64 restatement
under the derived bound, exact impulses, ragged rows, streaming bit-identity, a row whose indices pass 2^31, the error returns and the CLI.

The bar of every comparison with the restatement is ``Filter.bound``: (Kp + 2) 2^-24 max_p sum_j |h[p][j]| max|x| — the rounding of a Kp-term fp32
dot product plus that of the taps; it is derived, not measured."""
import functools
import random

import numpy as np
import pytest
import torch

from resample_reference import Filter
from vocoder_amd import _lib
from vocoder_amd import resample as rs

pytestmark = pytest.mark.gpu

HANN, KAISER = "sinc_interp_hann", "sinc_interp_kaiser"
PAIRS = [(44100, 48000, HANN), (44100, 16000, HANN), (48000, 8000, HANN), (22050, 44100, HANN), (3, 2, HANN), (2, 3, HANN),
         (44100, 48000, KAISER)]


@functools.lru_cache(maxsize=None)
def _pair(orig, new, method):
    """One module, restatement and native design per rate pair, shared by the tests (never modified)."""
    return rs.Resample(orig, new, resampling_method=method), Filter(orig, new, resampling_method=method), rs.native_design(
        orig, new, resampling_method=method)


def _strided(x: np.ndarray, extra: int = 5, fill: float = float("nan")) -> torch.Tensor:
    """(B, L) on the device as a view of a wider tensor (row stride L + extra); the columns beside it hold ``fill``."""
    B, L = x.shape
    big = torch.full((B, L + extra), fill, dtype=torch.float32, device="cuda")
    big[:, :L] = torch.from_numpy(x)
    return big[:, :L]


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("orig,new,method", PAIRS)
def test_parity_with_the_restatement(orig, new, method):
    mod, ref, d = _pair(orig, new, method)
    tile = _lib.resample_input_tile()
    bound = ref.bound(1.0)
    assert 1e-6 <= bound <= 8e-6
    rng = np.random.default_rng(orig + 3 * new)
    for L in sorted({1, 5, max(ref.o - 1, 1), ref.o, ref.o + 1, 2 * tile + 3}):
        x = rng.uniform(-1, 1, size=(3, L)).astype(np.float32)
        y = mod(_strided(x))
        assert tuple(y.shape) == (3, ref.output_length(L))
        err = float(np.abs(y.cpu().numpy().astype(np.float64) - ref(x)).max())
        print(f"{orig} -> {new} {method} L = {L}: max|d| = {err:.2e}, bound {bound:.2e}")
        assert err <= bound, (L, err, bound)


@pytest.mark.parametrize("orig,new,method", [(44100, 48000, HANN), (44100, 16000, HANN), (48000, 8000, HANN), (2, 3, HANN)])
def test_impulses_return_the_designed_taps_bit_for_bit(orig, new, method):
    """x = delta at 0, at L - 1 and on both sides of a tile boundary: y[m] is the designed fp32 tap h[p][pos - first_input(m)] where that lies in
    the band of m's phase and 0.0 elsewhere, exactly (products with 1 and sums with 0 do not round)."""
    mod, ref, d = _pair(orig, new, method)
    tile = _lib.resample_input_tile()
    L = 2 * tile + 3
    M = d.output_length(L)
    m = np.arange(M)
    f, p = m // d.n, m % d.n
    start = f * d.o + np.asarray(d.first)[p] - d.width
    count = np.asarray(d.count)[p]
    positions = [0, L - 1, tile - 1, tile, tile + d.first[0]]
    x = np.zeros((len(positions), L), dtype=np.float32)
    want = np.zeros((len(positions), M), dtype=np.float32)
    for r, pos in enumerate(positions):
        x[r, pos] = 1.0
        i = pos - start
        hit = (i >= 0) & (i < count)
        want[r, hit] = d.taps[p[hit], i[hit]]
        assert hit.any()
    y = mod(_strided(x, fill=0.0)).cpu().numpy()
    assert np.array_equal(_bits(y), _bits(want))


def test_ragged_rows_equal_the_rows_alone():
    orig, new, method = 44100, 16000, HANN
    mod, ref, d = _pair(orig, new, method)
    L = _lib.resample_input_tile() + 2 * d.o + 7
    lengths = [L, 1, 0, L - d.o + 1]
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, size=(4, L)).astype(np.float32)
    for b, n in enumerate(lengths):
        x[b, n:] = np.nan                                     # never loaded
    xd = _strided(x)
    y = mod(xd, lengths=lengths).cpu().numpy()
    assert y.shape == (4, d.output_length(L)) and not np.isnan(y).any()
    for b, n in enumerate(lengths):
        k = d.output_length(n)
        assert not y[b, k:].any() and not np.signbit(y[b, k:]).any()
        if n:
            alone = mod(xd[b:b + 1, :n].contiguous()).cpu().numpy()
            assert np.array_equal(_bits(y[b, :k]), _bits(alone[0]))
    y2 = mod(xd, lengths=torch.tensor(lengths, dtype=torch.int32, device="cuda")).cpu().numpy()      # device lengths: the same call
    assert np.array_equal(_bits(y2), _bits(y))


def _schedules(L, o):
    rng = random.Random(5)
    irregular, left = [], L
    while left > 0:
        c = min(left, rng.randint(1, 2 * o))
        irregular.append(c)
        left -= c
    return {"all-1": [1] * L, "all-7": [7] * (L // 7) + ([L % 7] if L % 7 else []), "all-o": [o] * (L // o) + ([L % o] if L % o else []),
            "all-(o+1)": [o + 1] * (L // (o + 1)) + ([L % (o + 1)] if L % (o + 1) else []), "irregular": irregular}


@pytest.mark.parametrize("orig,new", [(44100, 48000), (48000, 8000)])
def test_streaming_is_bit_identical_to_the_whole_row(orig, new):
    mod, ref, d = _pair(orig, new, HANN)
    o = d.o
    L = 5 * o + 3 if o > 50 else 40 * o + 3
    rng = np.random.default_rng(orig)
    xs = [torch.from_numpy(rng.uniform(-1, 1, size=(2, L)).astype(np.float32)).cuda() for _ in range(2)]
    whole = [_bits(mod(x).cpu().numpy()) for x in xs]
    for name, chunks in _schedules(L, o).items():
        assert sum(chunks) == L
        with mod.stream(batch=2, max_chunk=max(chunks)) as st:
            for x, want in zip(xs, whole):                      # the second utterance after a reset
                outs, N = [], 0
                for c in chunks:
                    y = st.push(x[:, N:N + c])
                    N += c
                    assert y.shape[1] == d.emit_count(N) - d.emit_count(N - c), (name, N)
                    assert st.received_samples == N and st.emitted_samples == d.emit_count(N)
                    outs.append(y)
                assert st.pending_samples == d.output_length(L) - d.emit_count(L)
                outs.append(st.flush())
                got = _bits(torch.cat(outs, dim=1).cpu().numpy())
                assert got.shape == want.shape and np.array_equal(got, want), name
                st.reset()


def test_stream_with_the_smallest_carry_uneven_chunks_and_strided_rows():
    """2 -> 3 Hz has the smallest carry, H samples: chunks below, at and above H, each a strided slice of one (2, L) tensor (the row stride
    exceeds the chunk), are bit-identical to the whole row; so is a second utterance after reset(), which starts from zeros whatever the
    first one left in the carry."""
    mod, ref, d = _pair(2, 3, HANN)
    H = (d.kp + 3) // 4 * 4                                     # the samples a stream carries (fv_resample_stream_create)
    chunks = [1, H - 1, H, H + 1, 1]
    L = sum(chunks)
    rng = np.random.default_rng(23)
    with mod.stream(batch=2, max_chunk=H + 1) as st:
        for _ in range(2):
            x = torch.from_numpy(rng.uniform(-1, 1, size=(2, L)).astype(np.float32)).cuda()
            want = _bits(mod(x).cpu().numpy())
            outs, N = [], 0
            for c in chunks:
                piece = x[:, N:N + c]
                assert piece.stride(0) == L > c
                outs.append(st.push(piece))
                N += c
                assert st.received_samples == N and st.emitted_samples == d.emit_count(N)
            outs.append(st.flush())
            got = _bits(torch.cat(outs, dim=1).cpu().numpy())
            assert got.shape == want.shape and np.array_equal(got, want)
            st.reset()


def test_a_refused_push_leaves_the_stream_intact():
    mod, ref, d = _pair(44100, 48000, HANN)
    x = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, size=(1, 400)).astype(np.float32)).cuda()
    want = _bits(mod(x).cpu().numpy())
    with mod.stream(batch=1, max_chunk=200) as st:
        a = st.push(x[:, :150])
        with pytest.raises(_lib.FishVocError) as ei:
            st.push(x[:, 150:400])                              # 250 > max_chunk
        assert ei.value.status == _lib.FV_ERR_INVALID and "max_chunk" in str(ei.value)
        assert st.received_samples == 150 and st.pending_samples == d.output_length(150) - d.emit_count(150)
        b = st.push(x[:, 150:350])
        c = st.push(x[:, 350:])
        e = st.flush()
        with pytest.raises(_lib.FishVocError) as ei:
            st.push(x[:, :10])                                  # after the flush, before a reset
        assert ei.value.status == _lib.FV_ERR_STATE
        assert np.array_equal(_bits(torch.cat([a, b, c, e], dim=1).cpu().numpy()), want)


def test_empty_chunks_and_empty_rows_are_no_ops():
    """A generator stream emits nothing until its lookahead has arrived: the (B, 0) chunk it hands on is a valid push."""
    mod, ref, d = _pair(44100, 48000, HANN)
    x = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, size=(2, 300)).astype(np.float32)).cuda()
    want = _bits(mod(x).cpu().numpy())
    with mod.stream(batch=2, max_chunk=300) as st:
        e0 = st.push(x[:, :0])
        assert tuple(e0.shape) == (2, 0) and st.received_samples == 0
        a = st.push(x)
        e1 = st.push(torch.empty((2, 1, 0), device="cuda")[:, 0])
        assert tuple(e1.shape) == (2, 0) and st.received_samples == 300
        assert np.array_equal(_bits(torch.cat([e0, a, e1, st.flush()], dim=1).cpu().numpy()), want)
    assert tuple(mod(x[:, :0]).shape) == (2, 0) and tuple(mod(torch.empty((2, 1, 0), device="cuda")).shape) == (2, 1, 0)


def test_long_row_whose_indices_pass_2_to_the_31():
    orig, new = 44100, 16000
    mod, ref, d = _pair(orig, new, HANN)
    L = 13_500_000
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand((1, L), generator=g, device="cuda") * 2 - 1
    y = mod(x)
    M = d.output_length(L)
    assert tuple(y.shape) == (1, M) and (M - 1) * d.o > 2 ** 31
    m0 = M - 2000
    a = max(0, d.first_input(m0) - d.o)
    want = ref.outputs(x[0, a:].cpu().numpy(), m0, M, start=a, total=L)
    err = float(np.abs(y[0, m0:].cpu().numpy().astype(np.float64) - want).max())
    print(f"long row: max|d| over the last 2000 outputs = {err:.2e}, bound {ref.bound(1.0):.2e}")
    assert err <= ref.bound(1.0)
    head = ref.outputs(x[0, :4096].cpu().numpy(), 0, 1000, start=0, total=L)
    assert float(np.abs(y[0, :1000].cpu().numpy().astype(np.float64) - head).max()) <= ref.bound(1.0)


def test_error_returns():
    mod, ref, d = _pair(44100, 48000, HANN)
    L = _lib.lib()
    x = torch.zeros((2, 300), dtype=torch.float32, device="cuda")
    mod(x)                                                                   # creates the handle
    h = mod._handle(x.device)
    st = L.fv_resample_forward(h, x.data_ptr(), 300, None, x.data_ptr() + 4 * 100, 400, 1, 300, None)   # y inside x
    assert st == _lib.FV_ERR_INVALID and b"overlaps" in L.fv_last_error()
    with pytest.raises(_lib.FishVocError) as ei:
        mod(x, lengths=[300, 301])
    assert ei.value.status == _lib.FV_ERR_INVALID and "lengths[1] = 301" in str(ei.value)
    with pytest.raises(_lib.FishVocError) as ei:
        rs.Resample(44101, 48000)(x)                                         # 48000 phases x 13 taps
    assert ei.value.status == _lib.FV_ERR_UNSUPPORTED and "44101 -> 48000" in str(ei.value) and "48000 phases x 13 taps" in str(ei.value)
    with pytest.raises(ValueError, match="CUDA"):
        mod(torch.zeros(2, 10))
    same = rs.Resample(44100, 44100)
    assert same(x) is x


def test_cli_resamples_the_input_and_the_output(tmp_path):
    """--resample: a 22050 Hz stereo wav gives what Resample -> model give directly; --output-rate 48000: ceil(160 T / 147) samples at 48 kHz, and
    the streamed file (--chunk-frames 8) equals the unstreamed one within 1 LSB."""
    from vocoder_amd import inference, synthetic as syn
    sd = syn.hifigan_state_dict(dict(syn.HIFIGAN_V1_44K), 3)
    torch.save({"state_dict": {f"generator.{k}": torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "g.ckpt")
    rng = np.random.default_rng(1)
    wav = (0.3 * rng.normal(size=(256 * 9, 2))).astype(np.float32).clip(-1, 1)
    (tmp_path / "in").mkdir()
    inference.write_wav(tmp_path / "in" / "b.wav", wav, 22050)
    common = ["--generator", "hifigan", "--num-mels", "80", "--ckpt-path", str(tmp_path / "g.ckpt"), "--input-path", str(tmp_path / "in")]
    inference.main(common + ["--output-path", str(tmp_path / "out"), "--resample"])
    got, sr = inference.read_wav(tmp_path / "out" / "b.wav")
    model = inference.build_model("hifigan", overrides={"num_mels": 80}, ckpt_path=tmp_path / "g.ckpt")
    y, _ = inference.read_wav(tmp_path / "in" / "b.wav")
    up = rs.Resample(22050, 44100)(torch.from_numpy(y)[:, None].cuda())
    assert up.shape[-1] == 512 * 9
    want = model(up)[0].squeeze(1)
    T = want.shape[-1]
    assert sr == 44100 and got.shape == (2, T)
    assert np.abs(got - np.clip(want.cpu().numpy(), -1, 1)).max() <= 2.0 / 32767

    inference.main(common + ["--output-path", str(tmp_path / "out48"), "--resample", "--output-rate", "48000"])
    got48, sr48 = inference.read_wav(tmp_path / "out48" / "b.wav")
    assert sr48 == 48000 and got48.shape == (2, -((-160 * T) // 147))
    want48 = rs.Resample(44100, 48000)(want).cpu().numpy()
    assert np.abs(got48 - np.clip(want48, -1, 1)).max() <= 2.0 / 32767

    inference.main(common + ["--output-path", str(tmp_path / "out48s"), "--resample", "--output-rate", "48000", "--chunk-frames", "8"])
    got48s, sr48s = inference.read_wav(tmp_path / "out48s" / "b.wav")
    assert sr48s == 48000 and got48s.shape == got48.shape
    assert np.abs(got48s - got48).max() <= 1.0 / 32768 + 1e-9
