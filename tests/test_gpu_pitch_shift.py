"""GPU: the pitch shift (vocoder_amd/csrc/pitch_shift.hip) through ``vocoder_amd.pitch_shift.PitchShift`` and the global-table resampler
(resample.hip) through ``Resample(table="global")``.

The parity bar is the project's own: |d| <= 1e-4 x the peak of the reference output, against form (b) of the float64 restatement
(pitch_shift_reference.py).  Every parity input is broadband (uniform noise plus a 440 Hz tone): the phase of an empty bin is ill-conditioned in
any precision.  Rows are strided views with NaN beside them: a NaN in the output means padding was read.  Each case prints what it measured.

Measured on an MI355X (profiles/LOG.md, the pitch-shift entry): see there."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import pitch_shift_reference as pref
from resample_reference import Filter
from vocoder_amd import _lib
from vocoder_amd import pitch_shift as ps
from vocoder_amd import resample as rs

pytestmark = pytest.mark.gpu

SR = 44100
BAR = 1e-4
HANN, KAISER = "sinc_interp_hann", "sinc_interp_kaiser"
STEPS = (3, -4, 12, -12, 0.5)


def _strided(x: np.ndarray, extra: int = 5, fill: float = float("nan")) -> torch.Tensor:
    """(B, L) on the device as a view of a wider tensor (row stride L + extra); the columns beside it hold ``fill``."""
    B, L = x.shape
    big = torch.full((B, L + extra), fill, dtype=torch.float32, device="cuda")
    big[:, :L] = torch.from_numpy(x)
    return big[:, :L]


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _rows(B, L, seed):
    return np.stack([pref.broadband(L, SR, seed + b) for b in range(B)]).astype(np.float32)


def _stretch_error(mod, x):
    """max over the rows of |GPU - float64 form (b)| / peak of the reference; checks the shape and that no padding was read."""
    B, L = x.shape
    y = mod.time_stretch(_strided(x)).cpu().numpy()
    assert y.shape == (B, mod.lengths(L)[2]) and not np.isnan(y).any()
    worst = 0.0
    if y.shape[1] == 0:          # round(L o / n) = 0 (L = 1 at -12 semitones: 881 / 882): nothing to compare
        return worst
    for b in range(B):
        ref = pref.time_stretch(x[b], mod.o, mod.n, mod.n_fft, mod.hop_length)
        assert ref.shape == y[b].shape
        worst = max(worst, float(np.abs(y[b] - ref).max() / np.abs(ref).max()))
    return worst


@pytest.mark.parametrize("n_steps", STEPS)
def test_stretch_parity_small_frames(n_steps):
    """n_fft 64, hop 16: rows shorter than a hop, than a frame, on and beside both, and several chunks of frames."""
    mod = ps.PitchShift(SR, n_steps, n_fft=64)
    assert mod.hop_length == 16
    for L in (1, 15, 16, 17, 63, 64, 1000):
        err = _stretch_error(mod, _rows(1, L, seed=L))
        print(f"stretch n_fft = 64, n_steps = {n_steps}, L = {L}: {err:.2e} of peak")
        assert err <= BAR, (L, err)


@pytest.mark.parametrize("n_steps", STEPS)
def test_stretch_parity_at_the_default_frame(n_steps):
    mod = ps.PitchShift(SR, n_steps)
    assert (mod.n_fft, mod.hop_length) == (2048, 512)
    err = _stretch_error(mod, _rows(3, 20000, seed=7))
    print(f"stretch n_fft = 2048, n_steps = {n_steps}, B = 3, L = 20000: {err:.2e} of peak")
    assert err <= BAR, err


def test_no_drift_over_a_long_row():
    """391 analysis frames: librosa's accumulator holds ~1e6 rad at the end; held in fp32 it is off by 0.12 of peak here."""
    mod = ps.PitchShift(SR, 3)
    err = _stretch_error(mod, _rows(1, 200000, seed=3))
    print(f"drift n_fft = 2048, n_steps = 3, L = 200000: {err:.2e} of peak")
    assert err <= BAR, err


def test_forward_parity_with_the_whole_restatement():
    """The two stages together against pitch_shift_reference.pitch_shift (form (b), then Filter): the same bar."""
    mod = ps.PitchShift(SR, 3)
    x = _rows(2, 20000, seed=21)
    y = mod(_strided(x)).cpu().numpy()
    assert y.shape == x.shape and not np.isnan(y).any()
    for b in range(2):
        ref = pref.pitch_shift(x[b], SR, 3)
        err = float(np.abs(y[b] - ref).max() / np.abs(ref).max())
        print(f"forward n_steps = 3, L = 20000, row {b}: {err:.2e} of peak")
        assert err <= BAR, err


def test_a_sine_moves_by_the_ratio_and_the_edge_cases_are_exact():
    L, k0 = 32768, 64
    f0 = k0 * SR / 2048                                       # on a bin centre
    x = np.sin(2 * np.pi * f0 * np.arange(L) / SR).astype(np.float32)[None]
    for n_steps in (3, -4):
        mod = ps.PitchShift(SR, n_steps)
        y = mod(_strided(x))
        assert tuple(y.shape) == (1, L)
        y2 = mod(_strided(x))
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(y2.cpu().numpy()))       # two runs, identical bits
        mid = y.cpu().numpy()[0, L // 4:L // 4 + L // 2].astype(np.float64)
        peak = float(np.argmax(np.abs(np.fft.rfft(mid * np.hanning(L // 2)))) * SR / (L // 2))
        want = f0 * mod.orig_freq / SR
        print(f"sine {f0:.1f} Hz, n_steps = {n_steps}: peak at {peak:.1f} Hz, want {want:.1f} Hz")
        assert abs(peak - want) <= SR / (L // 2)
        z = mod(torch.zeros((2, 5000), dtype=torch.float32, device="cuda")).cpu().numpy()
        assert z.shape == (2, 5000) and not z.any()          # silence in, exact zeros out
    same = ps.PitchShift(SR, 0)
    xd = _strided(x)
    assert np.array_equal(_bits(same(xd).cpu().numpy()), _bits(x)) and np.array_equal(_bits(same.time_stretch(xd).cpu().numpy()), _bits(x))
    # n_steps = 0 through the C entry as well: a copy
    h = ctypes.c_void_p()
    cfg = same.config()
    _lib.check(_lib.lib().fv_pitch_shift_create(ctypes.byref(cfg), ctypes.byref(h)))
    out = torch.full((1, L), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().fv_pitch_shift_forward(h, xd.data_ptr(), L, out.data_ptr(), L, 1, L, None, 0, None))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(x))
    _lib.lib().fv_pitch_shift_destroy(h)


def test_forward_is_stretch_then_the_global_resampler_then_fix_length():
    for n_steps in (3, -4):
        mod = ps.PitchShift(SR, n_steps, n_fft=256)
        x = _rows(2, 5000, seed=9)
        xd = _strided(x)
        y = mod(xd).cpu().numpy()
        st = mod.time_stretch(xd)
        res = rs.Resample(mod.orig_freq, SR, resampling_method=KAISER, lowpass_filter_width=64, rolloff=ps.KAISER_BEST_ROLLOFF, table="global")
        r = res(st).cpu().numpy()
        assert r.shape[1] == mod.lengths(5000)[3]
        want = np.zeros_like(x)
        k = min(r.shape[1], 5000)
        want[:, :k] = r[:, :k]
        assert np.array_equal(_bits(y), _bits(want))


def test_errors_of_the_device_calls():
    L = _lib.lib()
    mod = ps.PitchShift(SR, 3, n_fft=64)
    x = torch.zeros((2, 100), dtype=torch.float32, device="cuda")
    h = mod._handle(x.device)
    need = L.fv_pitch_shift_workspace_bytes(h, 2, 100)
    assert need > 0 and need % 256 == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    y = torch.zeros((2, 100), dtype=torch.float32, device="cuda")
    assert L.fv_pitch_shift_forward(h, x.data_ptr(), 100, x.data_ptr(), 100, 2, 100, ws.data_ptr(), need, None) == _lib.FV_ERR_INVALID
    assert "overlaps" in L.fv_last_error().decode()
    assert L.fv_pitch_shift_forward(h, x.data_ptr(), 100, y.data_ptr(), 100, 2, 100, ws.data_ptr(), need - 256, None) == _lib.FV_ERR_INVALID
    assert "workspace" in L.fv_last_error().decode()
    assert L.fv_pitch_shift_forward(h, x.data_ptr(), 99, y.data_ptr(), 100, 2, 100, ws.data_ptr(), need, None) == _lib.FV_ERR_INVALID
    assert "stride" in L.fv_last_error().decode()
    assert L.fv_pitch_shift_forward(h, None, 100, y.data_ptr(), 100, 2, 100, ws.data_ptr(), need, None) == _lib.FV_ERR_INVALID
    assert L.fv_pitch_shift_forward(h, x.data_ptr(), 100, y.data_ptr(), 100, 0, 100, None, 0, None) == _lib.FV_OK      # no rows: a no-op
    with pytest.raises(ValueError, match="CUDA"):
        mod(torch.zeros(10))
    assert tuple(mod(torch.zeros((2, 3, 0), dtype=torch.float32, device="cuda")).shape) == (2, 3, 0)
    # a row so short that the stretch has no sample (Ls = (2 * 220 + 441) // 882 = 0): the stretch is empty and the shift a row of exact zeros
    low = ps.PitchShift(SR, -12, n_fft=64)
    assert low.lengths(1)[2:] == (0, 0)
    one = _strided(np.ones((2, 1), dtype=np.float32))
    assert tuple(low.time_stretch(one).shape) == (2, 0)
    z = torch.full((2, 1), float("nan"), dtype=torch.float32, device="cuda")
    need1 = L.fv_pitch_shift_workspace_bytes(low._handle(one.device), 2, 1)
    ws1 = torch.empty(max(need1, 1), dtype=torch.uint8, device="cuda")
    _lib.check(L.fv_pitch_shift_forward(low._handle(one.device), one.data_ptr(), one.stride(0), z.data_ptr(), 1, 2, 1, ws1.data_ptr(), need1, None))
    torch.cuda.synchronize()
    assert z.cpu().numpy().tobytes() == np.zeros((2, 1), dtype=np.float32).tobytes()
    assert not low(one).cpu().numpy().any()
    assert tuple(mod(torch.zeros((2, 1, 300), dtype=torch.float32, device="cuda")).shape) == (2, 1, 300)     # stereo (C, 1, L): two rows


# ---- the resampler with its table in global memory ----

@functools.lru_cache(maxsize=None)
def _both(orig, new):
    return rs.Resample(orig, new), rs.Resample(orig, new, table="global"), rs.native_design(orig, new)


@pytest.mark.parametrize("orig,new", [(44100, 48000), (44100, 16000), (3, 2)])
def test_global_table_is_bit_identical_to_the_lds_table(orig, new):
    lds, glb, d = _both(orig, new)
    tile = _lib.resample_input_tile()
    rng = np.random.default_rng(orig + new)
    L = 2 * tile + 3
    x = rng.uniform(-1, 1, size=(3, L)).astype(np.float32)
    xd = _strided(x)
    a, b = lds(xd), glb(xd)
    assert _lib.last_kernel() == "resample_global_kernel"
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    # ragged rows
    lengths = [L, 1, L - d.o + 1]
    xr = x.copy()
    for r, n in enumerate(lengths):
        xr[r, n:] = np.nan
    xrd = _strided(xr)
    ra, rb = lds(xrd, lengths=lengths).cpu().numpy(), glb(xrd, lengths=lengths).cpu().numpy()
    assert not np.isnan(rb).any() and np.array_equal(_bits(ra), _bits(rb))
    # a stream's pushes
    Ls = 5 * d.o + 3 if d.o > 50 else 40 * d.o + 3
    xs = xd[:2, :Ls].contiguous()
    want = _bits(lds(xs).cpu().numpy())
    chunks, left, step = [], Ls, max(1, d.o // 3 + 1)
    while left > 0:
        chunks.append(min(left, step))
        left -= chunks[-1]
        step = step * 2 if step < 2 * d.o else 1
    with glb.stream(batch=2, max_chunk=max(chunks)) as st:
        outs, N = [], 0
        for c in chunks:
            outs.append(st.push(xs[:, N:N + c]))
            N += c
        outs.append(st.flush())
    assert np.array_equal(_bits(torch.cat(outs, dim=1).cpu().numpy()), want)


def test_the_lds_form_still_refuses_what_only_the_global_form_takes():
    with pytest.raises(_lib.FishVocError) as ei:
        rs.Resample(44101, 48000)(torch.zeros((1, 10), dtype=torch.float32, device="cuda"))
    assert ei.value.status == _lib.FV_ERR_UNSUPPORTED and "44101" in str(ei.value)


def _banded_reference(d, kwargs, x):
    """The float64 restatement evaluated on the band alone, for a pair whose dense (n, 2 width + o) matrix does not fit in memory (44101 ->
    48000: 17 GB): the expressions of resample_reference.Filter for the taps j in [first[p], first[p] + count[p]) of each output's phase; the
    taps outside the band are below 1e-30 (the window's edge).  Returns (y float64, the bound of Filter.bound)."""
    lpw, rolloff, method, beta = kwargs["lowpass_filter_width"], kwargs["rolloff"], kwargs["resampling_method"], kwargs.get("beta")
    o, n, width, kp = d.o, d.n, d.width, d.kp
    base = min(o, n) * rolloff
    L = x.shape[-1]
    M = d.output_length(L)
    m = np.arange(M)
    f, p = m // n, m % n
    first, count = np.asarray(d.first)[p], np.asarray(d.count)[p]
    j = first[:, None] + np.arange(kp)[None, :]
    t = np.clip(((j - width) / o - p[:, None] / n) * base, -lpw, lpw)
    win = np.cos(t * math.pi / lpw / 2) ** 2 if method == HANN else np.i0((beta or 14.769656459379492) * np.sqrt(1 - (t / lpw) ** 2)) / np.i0(
        beta or 14.769656459379492)
    tp = t * math.pi
    safe = np.where(tp == 0, 1.0, tp)
    h = np.where(tp == 0, 1.0, np.sin(safe) / safe) * win * (base / o)
    h = np.where(np.arange(kp)[None, :] < count[:, None], h, 0.0)
    idx = f[:, None] * o + j - width
    ok = (idx >= 0) & (idx < L)
    xs = np.where(ok[None], x.astype(np.float64)[:, np.clip(idx, 0, L - 1)], 0.0)
    return (xs * h[None]).sum(axis=2), (kp + 2) * 2.0 ** -24 * float(np.abs(h).sum(axis=1).max())


def test_global_table_parity_on_a_pair_whose_table_passes_lds():
    """44101 -> 48000 (hann, width 6): 48000 phases of 13 taps.  L = o visits every phase once."""
    kwargs = dict(lowpass_filter_width=6, rolloff=0.99, resampling_method=HANN)
    mod = rs.Resample(44101, 48000, table="global", **kwargs)
    d = rs.native_design(44101, 48000, **kwargs)
    tile = _lib.resample_input_tile()
    rng = np.random.default_rng(5)
    for L in (1, d.o, 2 * tile + 3):
        x = rng.uniform(-1, 1, size=(2, L)).astype(np.float32)
        y = mod(_strided(x)).cpu().numpy()
        ref, bound = _banded_reference(d, kwargs, x)
        assert y.shape == ref.shape == (2, d.output_length(L)) and not np.isnan(y).any()
        err = float(np.abs(y - ref).max())
        print(f"44101 -> 48000 hann global L = {L}: max|d| = {err:.2e}, bound {bound:.2e}")
        assert err <= bound, (L, err, bound)
    # impulses return the designed taps exactly: the uploaded table is fv_resample_design's
    L = 2 * tile + 3
    M = d.output_length(L)
    m = np.arange(M)
    f, p = m // d.n, m % d.n
    start = f * d.o + np.asarray(d.first)[p] - d.width
    count = np.asarray(d.count)[p]
    positions = [0, L - 1, tile - 1, tile]
    x = np.zeros((len(positions), L), dtype=np.float32)
    want = np.zeros((len(positions), M), dtype=np.float32)
    for r, pos in enumerate(positions):
        x[r, pos] = 1.0
        i = pos - start
        hit = (i >= 0) & (i < count)
        want[r, hit] = d.taps[p[hit], i[hit]]
        assert hit.any()
    assert np.array_equal(_bits(mod(_strided(x, fill=0.0)).cpu().numpy()), _bits(want))


def test_global_table_parity_on_the_pitch_shift_pair():
    """52400 -> 44100 (kaiser, width 64): 441 phases of 163 taps, the resample of a +3 semitone shift, against Filter under its bound."""
    kwargs = dict(lowpass_filter_width=64, rolloff=ps.KAISER_BEST_ROLLOFF, resampling_method=KAISER)
    mod = rs.Resample(52400, 44100, table="global", **kwargs)
    ref = Filter(52400, 44100, **kwargs)
    bound = ref.bound(1.0)
    tile = _lib.resample_input_tile()
    rng = np.random.default_rng(6)
    for L in (1, ref.o, 2 * tile + 3):
        x = rng.uniform(-1, 1, size=(2, L)).astype(np.float32)
        y = mod(_strided(x)).cpu().numpy()
        assert y.shape == (2, ref.output_length(L)) and not np.isnan(y).any()
        err = float(np.abs(y - ref(x)).max())
        print(f"52400 -> 44100 kaiser global L = {L}: max|d| = {err:.2e}, bound {bound:.2e}")
        assert err <= bound, (L, err, bound)


# ---- the CLI ----

def test_cli_pitch_shift(tmp_path):
    """--pitch-shift 3 on a 0.3 s wav: a wav of the same length as without it, other content; mel inputs and --chunk-frames are refused by name."""
    from vocoder_amd import inference, synthetic as syn
    sd = syn.hifigan_state_dict(dict(syn.HIFIGAN_V1_44K), 3)
    torch.save({"state_dict": {f"generator.{k}": torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "g.ckpt")
    n = int(0.3 * SR)
    wav = (0.3 * pref.broadband(n, SR, seed=1)).astype(np.float32).clip(-1, 1)
    (tmp_path / "in").mkdir()
    inference.write_wav(tmp_path / "in" / "a.wav", wav, SR)
    common = ["--generator", "hifigan", "--num-mels", "80", "--ckpt-path", str(tmp_path / "g.ckpt")]
    wav_in = ["--input-path", str(tmp_path / "in" / "a.wav")]
    inference.main(common + wav_in + ["--output-path", str(tmp_path / "plain")])
    inference.main(common + wav_in + ["--output-path", str(tmp_path / "shift"), "--pitch-shift", "3"])
    inference.main(common + wav_in + ["--output-path", str(tmp_path / "batch"), "--pitch-shift", "3", "--batch-size", "2"])
    a, sra = inference.read_wav(tmp_path / "plain" / "a.wav")
    b, srb = inference.read_wav(tmp_path / "shift" / "a.wav")
    c, _ = inference.read_wav(tmp_path / "batch" / "a.wav")
    assert sra == srb == SR and a.shape == b.shape == c.shape and a.shape[1] == (n // 512) * 512
    assert np.abs(a - b).max() > 1e-2
    assert np.abs(c - b).max() <= 2.0 / 32768          # the ragged call gives the one-by-one wav within 1 LSB, as without the option
    torch.save(torch.zeros(80, 12), tmp_path / "m.pt")
    with pytest.raises(ValueError, match="--pitch-shift"):
        inference.main(common + ["--input-path", str(tmp_path / "m.pt"), "--output-path", str(tmp_path / "o"), "--pitch-shift", "3"])
    with pytest.raises(ValueError, match="--pitch-shift"):      # under --batch-size too: a mel is refused, not passed through unshifted
        inference.main(common + ["--input-path", str(tmp_path / "m.pt"), "--output-path", str(tmp_path / "o"), "--pitch-shift", "3",
                                 "--batch-size", "2"])
    torch.save(torch.zeros(80, 12), tmp_path / "in" / "m.pt")   # a directory that mixes wav and mel
    with pytest.raises(ValueError, match="--pitch-shift"):
        inference.main(common + ["--input-path", str(tmp_path / "in"), "--output-path", str(tmp_path / "o"), "--pitch-shift", "3",
                                 "--batch-size", "2"])
    assert not (tmp_path / "o").exists()                         # refused before anything is written
    with pytest.raises(ValueError, match="--pitch-shift"):
        inference.main(common + wav_in + ["--output-path", str(tmp_path / "o"), "--pitch-shift", "3", "--chunk-frames", "8"])
