"""GPU: the streaming pitch shift (fv_pv_stream_* in vocoder_amd/csrc/pitch_shift.hip) through ``vocoder_amd.pitch_shift`` and the wav -> wav chain
of ``vocoder_amd.inference``.

Every comparison against the whole-row GPU result is on bits, with ``PitchShift(batch_invariant=True)`` on both sides: the two DFT convs are then
fixed-order sums per column, the phase is a wrapping integer sum, the overlap-add sums a sample's frames in one order and the resampler's stream
is bit-identical to its rows, so a stream has nothing to be approximately equal about.  Every pushed chunk is a strided view with NaN beside it:
a NaN in the output, or one changed bit, means a sample outside the chunk was read.  After every push the emitted count is the counting rule's
(pitch_shift_stream_reference) and N - E stays inside its latency bound.  The chain's bar is the generator stream's own, 2e-5 * max(1, peak)
(test_gpu_stream.py)."""
import functools

import numpy as np
import pytest
import torch

import pitch_shift_reference as pref
import pitch_shift_stream_reference as sref
from vocoder_amd import _lib
from vocoder_amd import pitch_shift as ps

pytestmark = pytest.mark.gpu

SR = 44100
BAR = 1e-4
STEPS = (3, -4, 12, -12, 0.5)
SMALL_L = (1, 15, 16, 17, 63, 64, 300, 1000)


def _bits(a) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _strided(x: torch.Tensor, extra: int = 5) -> torch.Tensor:
    """A copy of x (B, c) as a view of a wider tensor whose other columns hold NaN."""
    big = torch.full((x.shape[0], x.shape[1] + extra), float("nan"), dtype=torch.float32, device="cuda")
    big[:, :x.shape[1]] = x
    return big[:, :x.shape[1]]


def _rows(B, L, seed):
    return np.stack([pref.broadband(L, SR, seed + b) for b in range(B)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _shifter(n_steps, n_fft):
    """The module (batch-invariant), the float64 filter of its second stage, and the latency bound: made once per configuration."""
    mod = ps.PitchShift(SR, n_steps, n_fft=n_fft, batch_invariant=True)
    filt = sref.resampler(SR, n_steps) if mod.orig_freq != SR else None
    return mod, filt, (sref.latency_bound(filt, mod.n_fft, mod.hop_length) if filt is not None else 0)


@functools.lru_cache(maxsize=None)
def _case(n_steps, n_fft, B, L):
    """Rows on the device and the whole-row GPU result (computed once, never changed)."""
    mod, _, _ = _shifter(n_steps, n_fft)
    host = _rows(B, L, seed=L + n_fft)
    rows = torch.from_numpy(host).cuda()
    whole = mod(_strided(rows))
    assert tuple(whole.shape) == (B, L) and not bool(torch.isnan(whole).any())
    return host, rows, whole, _bits(whole)


def _sizes(name, L, hop):
    if name == "random":
        sizes = sref.chunk_sizes(L, np.random.default_rng(L), 3 * hop)
        if 0 not in sizes:
            sizes.insert(len(sizes) // 2, 0)
        return sizes
    c = {"one": L, "hop": hop, "37": 37, "1": 1}[name]
    return [c] * (L // c) + ([L % c] if L % c else [])


def _expected(mod, filt, N):
    if filt is None:
        return N
    E, raw = sref.emitted(filt, sref.ready(N, mod.o, mod.n, mod.n_fft, mod.hop_length)[2], N)
    assert raw <= N                                       # the cap at N does not bind
    return E


def _stream_all(st, mod, filt, bound, rows, sizes):
    """Pushes rows in `sizes`, then flushes, checking every count against the counting rule; returns the concatenated output."""
    B, L = rows.shape
    outs, at, E = [], 0, 0
    for c in sizes:
        y = st.push(_strided(rows[:, at:at + c]))
        at += c
        E2 = max(E, _expected(mod, filt, at))
        assert tuple(y.shape) == (B, E2 - E), (at, c, tuple(y.shape), E2 - E)
        E = E2
        assert (st.received_samples, st.emitted_samples) == (at, E)
        assert st.pending_samples == at - E <= bound, (at, E, bound)
        outs.append(y)
    y = st.flush()
    assert tuple(y.shape) == (B, L - E) and st.emitted_samples == L == st.received_samples and st.pending_samples == 0
    return torch.cat(outs + [y], dim=1)


def _check(n_steps, n_fft, B, L, name):
    mod, filt, bound = _shifter(n_steps, n_fft)
    _, rows, _, whole_bits = _case(n_steps, n_fft, B, L)
    sizes = _sizes(name, L, mod.hop_length)
    assert sum(sizes) == L and (name != "random" or 0 in sizes)
    with mod.stream(B, max(sizes)) as st:
        y = _stream_all(st, mod, filt, bound, rows, sizes)
    assert not bool(torch.isnan(y).any()), (n_steps, L, name)
    got = _bits(y)
    assert np.array_equal(got, whole_bits), (n_steps, L, name, int((got != whole_bits).sum()), float((y.cpu() - _case(n_steps, n_fft, B, L)[2].cpu()).abs().max()))


@pytest.mark.parametrize("n_steps", STEPS)
def test_small_frames_every_chunking_equals_the_whole_rows_bit_for_bit(n_steps):
    """n_fft 64, hop 16, B = 3: rows shorter than a hop, than half a frame, than a frame, on and beside each, and many frames."""
    assert _shifter(n_steps, 64)[0].hop_length == 16
    for L in SMALL_L:
        for name in ("one", "hop", "37", "random"):
            _check(n_steps, 64, 3, L, name)


def test_small_frames_one_sample_per_push():
    _check(3, 64, 3, 300, "1")


@pytest.mark.parametrize("name", ["one", "4096", "random"])
@pytest.mark.parametrize("n_steps", [3, -4])
def test_default_frame_equals_the_whole_rows_bit_for_bit(n_steps, name):
    mod, filt, bound = _shifter(n_steps, 2048)
    assert (mod.n_fft, mod.hop_length) == (2048, 512)
    B, L = 2, 20000
    _, rows, _, whole_bits = _case(n_steps, 2048, B, L)
    sizes = [4096] * 4 + [L - 4 * 4096] if name == "4096" else _sizes(name, L, 512)
    assert sum(sizes) == L
    with mod.stream(B, max(sizes)) as st:
        y = _stream_all(st, mod, filt, bound, rows, sizes)
    assert not bool(torch.isnan(y).any())
    assert np.array_equal(_bits(y), whole_bits), (n_steps, name, int((_bits(y) != whole_bits).sum()))


@pytest.mark.parametrize("n_steps", [3, -4])
def test_parity_of_the_whole_rows_under_the_switch(n_steps):
    """The mode the stream is compared with keeps the project's bar: batch_invariant=True against pitch_shift_reference.pitch_shift."""
    host, _, whole, _ = _case(n_steps, 2048, 2, 20000)
    y = whole.cpu().numpy()
    for b in range(2):
        ref = pref.pitch_shift(host[b], SR, n_steps)
        err = float(np.abs(y[b] - ref).max() / np.abs(ref).max())
        print(f"batch-invariant forward n_steps = {n_steps}, L = 20000, row {b}: {err:.2e} of peak")
        assert err <= BAR, err


def test_ends_refusals_and_reset():
    mod, filt, bound = _shifter(3, 2048)
    B, L = 2, 20000
    _, rows, _, whole_bits = _case(3, 2048, B, L)
    with mod.stream(B, 4096) as st:
        y = st.flush()                                        # a flush at N = 0 emits nothing
        assert tuple(y.shape) == (B, 0) and st.emitted_samples == 0
        st.reset()
        short = rows[:, :1000]                                # L < n_fft / 2: nothing leaves before the flush
        y = st.push(_strided(short))
        assert tuple(y.shape) == (B, 0) and st.pending_samples == 1000
        y = st.flush()
        assert tuple(y.shape) == (B, 1000) and np.array_equal(_bits(y), _bits(mod(_strided(short))))
        # a push and a flush after a flush are refused and change nothing
        before = (st.received_samples, st.emitted_samples, st.pending_samples)
        with pytest.raises(_lib.FishVocError) as ei:
            st.push(_strided(short))
        assert ei.value.status == _lib.FV_ERR_STATE and "fv_pv_stream_reset" in str(ei.value)
        with pytest.raises(_lib.FishVocError) as ei:
            st.flush()
        assert ei.value.status == _lib.FV_ERR_STATE and "fv_pv_stream_reset" in str(ei.value)
        assert (st.received_samples, st.emitted_samples, st.pending_samples) == before
        st.reset()
        with pytest.raises(_lib.FishVocError) as ei:          # a chunk above max_chunk, on a fresh utterance
            st.push(_strided(torch.zeros((B, 4097), device="cuda")))
        assert ei.value.status == _lib.FV_ERR_INVALID and st.received_samples == 0 and st.pending_samples == 0
        with pytest.raises(ValueError):
            st.push(rows[:1, :100])
        with pytest.raises(_lib.FishVocError) as ei:          # a workspace that is too small
            st._call(rows[:, :4096].contiguous(), 4096, flush=False, workspace_bytes=st._need - 256)
        assert ei.value.status == _lib.FV_ERR_INVALID and "workspace" in str(ei.value) and st.received_samples == 0
        # silence in, exact zeros out
        quiet = torch.zeros((B, 6000), device="cuda")
        y = torch.cat([st.push(_strided(quiet[:, :4096])), st.push(_strided(quiet[:, 4096:])), st.flush()], dim=1)
        assert tuple(y.shape) == (B, 6000) and bool((y == 0).all())
        # a loud first utterance fills every carry; after reset() the second one has the bits of a fresh stream
        st.reset()
        loud = torch.full((B, 4096), 1e3, device="cuda")
        for _ in range(3):
            st.push(_strided(loud))
        st.flush()
        st.reset()
        y = _stream_all(st, mod, filt, bound, rows, _sizes("random", L, 512))
        assert np.array_equal(_bits(y), whole_bits)
    with pytest.raises(_lib.FishVocError):                    # closed
        st.push(_strided(rows[:, :100]))


def test_a_row_whose_stretch_is_empty_and_the_pass_through():
    # Ls = 0: L = 1 at -12 semitones (round(220 / 441) = 0): one zero, at the flush
    mod, filt, bound = _shifter(-12, 64)
    assert mod.lengths(1)[2] == 0
    one = torch.full((3, 1), 0.5, device="cuda")
    with mod.stream(3, 8) as st:
        assert st.push(_strided(one)).shape[1] == 0
        y = st.flush()
        assert tuple(y.shape) == (3, 1) and bool((y == 0).all()) and np.array_equal(_bits(y), _bits(mod(_strided(one))))
    # n_steps = 0: every push hands its own samples back, the flush has nothing left
    ident = ps.PitchShift(SR, 0, batch_invariant=True)
    x = torch.from_numpy(_rows(2, 777, seed=5)).cuda()
    with ident.stream(2, 512) as st:
        a = st.push(_strided(x[:, :512]))
        assert st.pending_samples == 0 and st.emitted_samples == 512
        b = st.push(_strided(x[:, 512:]))
        c = st.flush()
        assert tuple(c.shape) == (2, 0) and st.emitted_samples == 777
    assert np.array_equal(_bits(torch.cat([a, b], dim=1)), _bits(x))


# ---- the chain, on the synthetic HiFiGAN-V1-44k of test_gpu_pitch_shift.py::test_cli_pitch_shift ----
@pytest.mark.parametrize("use_template", [False, True])
def test_the_wav_chain_with_a_pitch_shift_matches_the_whole_file_path(use_template):
    from vocoder_amd import f0 as f0mod, inference, synthetic as syn
    from vocoder_amd.data.transforms import LogMelSpectrogram
    from vocoder_amd.modules.generators.hifigan import HiFiGANGenerator
    cfg = dict(syn.HIFIGAN_V1_44K, use_template=use_template)
    hop, chunk_frames = cfg["hop_length"], 8
    gen = HiFiGANGenerator(**cfg).eval()
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(cfg, 3).items()})
    front = LogMelSpectrogram(sample_rate=SR, n_fft=2048, win_length=2048, hop_length=hop, n_mels=80, f_min=0, f_max=SR // 2)
    model = inference.InferenceModel(gen, SR, 80, hop, mel_transform=front).eval().cuda()
    n = int(0.3 * SR)
    x = (0.3 * pref.broadband(n, SR, seed=1)).astype(np.float32).clip(-1, 1)
    shifter = ps.PitchShift(SR, 3, batch_invariant=True)
    tracker = dict(frame_length=2048, fmin=40.0, fmax=1100.0)

    # the whole-file path: shift, pad, log-mel, forward (test.py:61-71)
    y = shifter(torch.from_numpy(x)[None].cuda())
    y = torch.nn.functional.pad(y, (0, inference._pad_samples(hop, y.shape[-1])))
    mel = model.mel_transform(y)
    template = f0mod.template_from_audio(y, SR, hop, **tracker) if use_template else None
    whole = model(None, None, input_spec=mel, template=template)[0]
    plain = model(None, None, input_spec=model.mel_transform(torch.from_numpy(x)[None].cuda()), template=template)[0]
    peak = float(whole.abs().max())
    bar = 2e-5 * max(1.0, peak)
    assert tuple(whole.shape) == (1, 1, (n // hop) * hop) and float((whole - plain).abs().max()) > 1e-2       # the shift matters

    limit = chunk_frames * hop
    chunks = [torch.from_numpy(x[at:at + limit])[None] for at in range(0, n, limit)]
    got, stats = inference.stream_wav_synthesis(model, iter(chunks), n, chunk_frames=chunk_frames, pitch_shift=shifter,
                                                template=dict(tracker) if use_template else None)
    d = float((got - whole).abs().max())
    print(f"wav -> wav with a pitch shift{' and a template' if use_template else ''}, {chunk_frames}-frame chunks: max|d| = {d:.2e} "
          f"(bar {bar:.1e}, peak {peak:.3f}); {stats['reads']} reads")
    assert tuple(got.shape) == tuple(whole.shape) and d <= bar
    assert stats["reads"] == len(chunks)
    with pytest.raises(ValueError, match="Hz"):
        inference.stream_wav_synthesis(model, iter(chunks), n, chunk_frames=chunk_frames, pitch_shift=ps.PitchShift(48000, 3))
