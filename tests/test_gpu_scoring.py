"""GPU: scoring generated audio (vocoder_amd.scoring, fv_spec_distance, python -m vocoder_amd.eval).  The kernel against float32 terms summed
with math.fsum, at every stride and in every batch bit for bit; the two metrics against the CPU oracle / the float64 formulas; the CLI.
Every bar is derived from the number formats, not measured."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from vocoder_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHANNELS = (5, 20)          # fewer and more than the 16 channels a workgroup takes per step
# fp64 accumulation of n <= 4e4 non-negative terms: relative error <= n * 2^-53 = 4.4e-12
REL_SUM = 1e-9
# S_log / count: logf is within 2 ulp where |log| <= 6.91 (ulp 9.5e-7 at most), twice per term, plus half an ulp of the difference:
# (2 + 2 + 0.5) * 9.5e-7 = 4.3e-6 per term at worst, and a mean of terms errs no more than its worst term
ABS_LOG = 5e-6
MEL_TOL = 4e-4              # twice the front-end's own 2e-4 bar (test_gpu_logmel_windows.TOL): |a - b| - |a' - b'| <= |a - a'| + |b - b'|
MEL_CONFIGS = [(256, 64, 20), (96, 64, 12), (256, 51, 20)]      # (n_fft, hop, n_mels) of test_gpu_logmel_windows.py
_cache: dict = {}


def _K():
    return _lib.spec_distance_tile()


def _frames():
    K = _K()
    return [0, 1, K - 1, K, K + 1, 2 * K + 1]


def _kernel_case(C):
    """est / ref (B, C, T) float32 with NaN at and past frames[b], and the float64 reference of the four sums; made once per C."""
    if ("case", C) not in _cache:
        frames = _frames()
        B, T = len(frames), max(frames) + 3
        rng = np.random.default_rng(100 + C)
        ref = np.exp(rng.uniform(math.log(1e-3), math.log(1e3), size=(B, C, T))).astype(np.float32)
        est = (ref * np.exp(0.3 * rng.normal(size=(B, C, T)))).astype(np.float32)
        want = np.zeros((B, 4))
        for b, n in enumerate(frames):
            e, r = est[b, :, :n], ref[b, :, :n]
            d = e - r                                                     # float32 throughout: one rounding per operation
            with np.errstate(all="ignore"):
                terms = (np.abs(d), d * d, r * r, np.abs(np.log(r) - np.log(e)))
            assert all(t.dtype == np.float32 for t in terms)
            want[b] = [math.fsum(t.astype(np.float64).ravel().tolist()) for t in terms]
            est[b, :, n:] = np.nan
            ref[b, :, n:] = np.nan
        _cache["case", C] = (est, ref, frames, want)
    return _cache["case", C]


def _batch_result(C):
    """The kernel on the whole batch of ``_kernel_case(C)``, contiguous, with the log term; computed once and never modified."""
    if ("got", C) not in _cache:
        from vocoder_amd.scoring import spec_distance
        est, ref, frames, _ = _kernel_case(C)
        got = spec_distance(torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda(), frames, log_term=True).cpu().numpy()
        got.setflags(write=False)
        _cache["got", C] = got
    return _cache["got", C]


@pytest.mark.parametrize("C", CHANNELS)
def test_kernel_against_float32_terms_summed_in_float64(C):
    from vocoder_amd.scoring import spec_distance
    est, ref, frames, want = _kernel_case(C)
    got = _batch_result(C)
    assert got.dtype == np.float64 and got.shape == (len(frames), 4)
    for b, n in enumerate(frames):
        rel = [abs(got[b, k] - want[b, k]) / want[b, k] if want[b, k] else abs(got[b, k]) for k in range(3)]
        err_log = abs(got[b, 3] - want[b, 3]) / max(C * n, 1)
        print(f"C={C} frames={n}: rel(S_l1, S_sq, S_ref) = {rel}, |S_log / count error| = {err_log:.3e}")
        if n == 0:
            assert got[b].tobytes() == np.zeros(4).tobytes()              # four zeros exactly, and no NaN from the unread columns
            continue
        assert np.all(np.isfinite(got[b]))
        assert max(rel) <= REL_SUM, (b, n, rel)
        assert err_log <= ABS_LOG, (b, n, err_log)
    # log flag off: S_log is exactly 0.0, the other three are the same bits, and negative inputs (log-mels) give finite sums
    e, r = torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda()
    off = spec_distance(e, r, frames).cpu().numpy()
    assert off[:, 3].tobytes() == np.zeros(len(frames)).tobytes() and off[:, :3].tobytes() == got[:, :3].tobytes()
    neg = spec_distance(-e, torch.log(r) - 3.0, frames).cpu().numpy()
    assert np.all(np.isfinite(neg)) and np.all(neg[1:, 0] > 0) and neg[:, 3].tobytes() == np.zeros(len(frames)).tobytes()
    # frames = None scores every column: the NaN padding then reaches the result, which is how the test knows the masking above is real
    assert np.isnan(spec_distance(e, r).cpu().numpy()[0, 0])


@pytest.mark.parametrize("C", CHANNELS)
def test_strided_views_give_the_same_bits(C):
    """``base[:, :, 1:]`` of a tensor one column wider: ld = T + 1 is odd for one C and even for the other, the base pointer is 4 bytes off a
    16-byte boundary, so the scalar-load path runs; then a row stride with a gap and a channel slice."""
    from vocoder_amd.scoring import _layout, spec_distance
    est, ref, frames, _ = _kernel_case(C)
    B, _, T = est.shape
    want = _batch_result(C)
    for wider, gap in ((1, 0), (3, 2)):
        be = torch.full((B + gap, C + gap, T + wider), float("nan"), device="cuda")
        br = torch.full((B + gap, C + gap, T + wider), float("nan"), device="cuda")
        ve, vr = be[:B, :C, wider:], br[:B, :C, wider:]
        ve.copy_(torch.from_numpy(est)), vr.copy_(torch.from_numpy(ref))
        assert _layout(ve) == (T + wider, (C + gap) * (T + wider)) and ve.data_ptr() % 16 != 0 and not ve.is_contiguous()
        got = spec_distance(ve, vr, frames, log_term=True).cpu().numpy()
        assert got.tobytes() == want.tobytes(), (wider, gap)
    # a layout the entry cannot express is copied, not refused
    te = torch.from_numpy(est).cuda().transpose(1, 2).contiguous().transpose(1, 2)
    assert _layout(te) is None
    assert spec_distance(te, torch.from_numpy(ref).cuda(), frames, log_term=True).cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("C", CHANNELS)
def test_a_row_scores_the_same_alone_in_any_batch_at_any_width_and_on_every_run(C):
    from vocoder_amd.scoring import spec_distance
    est, ref, frames, _ = _kernel_case(C)
    want = _batch_result(C)
    B, _, T = est.shape
    e, r = torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda()
    again = spec_distance(e, r, frames, log_term=True).cpu().numpy()                  # two consecutive calls
    assert again.tobytes() == want.tobytes()
    rev = spec_distance(e.flip(0).contiguous(), r.flip(0).contiguous(), frames[::-1], log_term=True).cpu().numpy()
    assert rev[::-1].tobytes() == want.tobytes()
    pad = torch.full((B, C, _K()), float("nan"), device="cuda")
    wide = spec_distance(torch.cat([e, pad], 2), torch.cat([r, pad], 2), frames, log_term=True).cpu().numpy()     # T + K
    assert wide.tobytes() == want.tobytes()
    for i in range(B):
        alone = spec_distance(e[i:i + 1], r[i:i + 1], frames[i:i + 1], log_term=True).cpu().numpy()
        assert alone[0].tobytes() == want[i].tobytes(), i
        # and cut to its own width (T = frames[i]: no padding at all)
        own = spec_distance(e[i:i + 1, :, :frames[i]].contiguous(), r[i:i + 1, :, :frames[i]].contiguous(), None, log_term=True).cpu().numpy()
        assert own[0].tobytes() == want[i].tobytes(), i
    # more rows than one launch carries by value (64): the blocks of rows do not disturb one another
    many = 70
    idx = [k % B for k in range(many)]
    big = spec_distance(e[idx].contiguous(), r[idx].contiguous(), [frames[k] for k in idx], log_term=True).cpu().numpy()
    assert big.tobytes() == want[idx].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------------
def _ragged_lengths(fr):
    """test_gpu_logmel_windows._ragged_cases' pattern without its 0-length row."""
    hop, pad = fr.hop_length, max(fr.pad_l, fr.pad_r)
    shortest = max(pad + 1, hop)
    one_frame = shortest
    while fr.frames(one_frame + 1) == fr.frames(shortest):
        one_frame += 1
    return [[shortest, 7 * hop, 9 * hop + 3], [one_frame, 7 * hop - 1, 7 * hop + 1, 12 * hop]]


def _pair(cfg, case, B, L):
    rng = np.random.default_rng(sum(cfg) + 31 * case + 7 * B + L)
    target = (0.2 * rng.normal(size=(B, L))).astype(np.float32)
    preds = (target + 0.05 * rng.normal(size=(B, L))).astype(np.float32)
    return target, preds


def _mel_distance(cfg):
    if ("mel", cfg) not in _cache:
        from vocoder_amd.scoring import MelDistance
        n_fft, hop, n_mels = cfg
        _cache["mel", cfg] = MelDistance(24000, n_fft=n_fft, win_length=n_fft, hop_length=hop, n_mels=n_mels, f_min=0.0, f_max=12000).cuda()
    return _cache["mel", cfg]


@pytest.mark.parametrize("cfg", MEL_CONFIGS, ids=lambda c: "x".join(map(str, c)))
def test_mel_distance_against_the_oracle_and_its_three_forms_agree(cfg):
    n_fft, hop, n_mels = cfg
    m = _mel_distance(cfg)
    fr = m.mel._framing()
    ocfg = dict(sample_rate=24000, n_fft=n_fft, win_length=n_fft, hop_length=hop, n_mels=n_mels, f_min=0.0, f_max=12000)
    for case, lengths in enumerate(_ragged_lengths(fr)):
        B, L = len(lengths), max(lengths)
        target, preds = _pair(cfg, case, B, L)
        t, p = torch.from_numpy(target).cuda(), torch.from_numpy(preds).cuda()
        pt = torch.where(torch.arange(L, device="cuda")[None] < torch.tensor(lengths, device="cuda")[:, None], t, float("nan"))
        pp = torch.where(torch.arange(L, device="cuda")[None] < torch.tensor(lengths, device="cuda")[:, None], p, float("nan"))
        got = m.forward_ragged(pt, pp, lengths)                         # the padding holds NaN: it must never be read
        assert got.dtype == torch.float64 and got.shape == (B,)
        lst = m.forward_list([t[b, :n] for b, n in enumerate(lengths)], [p[b, :n] for b, n in enumerate(lengths)])
        assert lst.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
        got = got.cpu().numpy()
        for b, n in enumerate(lengths):
            want = float(np.mean(np.abs(orc.logmel_forward(preds[b:b + 1, :n], ocfg).astype(np.float64) -
                                        orc.logmel_forward(target[b:b + 1, :n], ocfg).astype(np.float64))))
            print(f"cfg={cfg} L={n}: oracle {want:.6f} got {got[b]:.6f} diff {abs(got[b] - want):.2e}")
            assert want >= 0.05, (cfg, n, want)
            assert abs(got[b] - want) <= MEL_TOL, (cfg, n, got[b], want)
            one = m(t[b:b + 1, :n], p[b:b + 1, :n])                     # eval.py:29-33's own call: one pair, whole rows
            assert one.shape == (1,) and one.cpu().numpy().tobytes() == got[b:b + 1].tobytes(), (cfg, n)
            assert m(t[b:b + 1, None, :n], p[b:b + 1, None, :n]).cpu().numpy().tobytes() == got[b:b + 1].tobytes()
    # rows of one length: forward on the batch, forward_ragged and forward_list agree bit for bit
    target, preds = _pair(cfg, 9, 3, 9 * hop + 3)
    t, p = torch.from_numpy(target).cuda(), torch.from_numpy(preds).cuda()
    a, b, c = m(t, p), m.forward_ragged(t, p, [9 * hop + 3] * 3), m.forward_list(list(t), list(p))
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()
    # forward_list crops each pair to the shorter of the two (eval.py:70-74)
    d = m.forward_list([t[0], t[1, :8 * hop]], [p[0, :7 * hop + 5], p[1]])
    e = m.forward_list([t[0, :7 * hop + 5], t[1, :8 * hop]], [p[0, :7 * hop + 5], p[1, :8 * hop]])
    assert d.cpu().numpy().tobytes() == e.cpu().numpy().tobytes()
    # a length of 0 scores NaN, not an error; a row the front-end refuses is refused with its index
    z = m.forward_ragged(t, p, [9 * hop + 3, 0, 7 * hop]).cpu().numpy()
    assert z[0].tobytes() == a.cpu().numpy()[0].tobytes() and np.isnan(z[1]) and np.isfinite(z[2])
    assert np.isnan(m.forward_ragged(t, p, [0, 0, 0]).cpu().numpy()).all()
    with pytest.raises(ValueError, match="row 2 holds"):
        m.forward_ragged(t, p, [9 * hop + 3, 7 * hop, max(fr.pad_l, fr.pad_r)])


def test_multi_resolution_stft_distance_against_the_float64_formulas():
    from vocoder_amd.scoring import MultiResolutionSTFTDistance
    res = ((256, 64), (96, 64))
    m = MultiResolutionSTFTDistance(res).cuda()
    cfg = MEL_CONFIGS[0]
    fr = _mel_distance(cfg).mel._framing()
    for case, lengths in enumerate(_ragged_lengths(fr)):
        B, L = len(lengths), max(lengths)
        target, preds = _pair(cfg, case, B, L)
        t, p = torch.from_numpy(target).cuda(), torch.from_numpy(preds).cuda()
        sc, mag = m.forward_ragged(t, p, lengths)
        assert sc.dtype == mag.dtype == torch.float64 and sc.shape == mag.shape == (B,)
        lsc, lmag = m.forward_list([t[b, :n] for b, n in enumerate(lengths)], [p[b, :n] for b, n in enumerate(lengths)])
        assert lsc.cpu().numpy().tobytes() == sc.cpu().numpy().tobytes() and lmag.cpu().numpy().tobytes() == mag.cpu().numpy().tobytes()
        sc, mag = sc.cpu().numpy(), mag.cpu().numpy()
        # the module's own magnitudes, through stft.py:55 and :74 in float64, per row over its valid frames
        specs = []
        for s in m.spectrograms:
            y, fl = s.forward_ragged(t, lengths)
            x, _ = s.forward_ragged(p, lengths)
            specs.append((y.cpu().numpy().astype(np.float64), x.cpu().numpy().astype(np.float64), fl))
        for b, n in enumerate(lengths):
            want_sc = np.mean([np.sqrt(np.sum((y[b, :, :fl[b]] - x[b, :, :fl[b]]) ** 2)) / np.sqrt(np.sum(y[b, :, :fl[b]] ** 2)) for y, x, fl in specs])
            want_mag = np.mean([np.mean(np.abs(np.log(y[b, :, :fl[b]]) - np.log(x[b, :, :fl[b]]))) for y, x, fl in specs])
            print(f"L={n}: sc {sc[b]:.8f} (float64 {want_sc:.8f}), mag {mag[b]:.8f} (float64 {want_mag:.8f})")
            # the float32 terms d * d and ref * ref carry 2^-24 each against float64 squares (and d itself 2^-24): far inside 1e-6
            assert abs(sc[b] - want_sc) <= 1e-6 * want_sc, (n, sc[b], want_sc)
            assert abs(mag[b] - want_mag) <= ABS_LOG, (n, mag[b], want_mag)
            assert 0.05 < sc[b] < 0.5 and 0.05 < mag[b] < 0.5, (n, sc[b], mag[b])
            one_sc, one_mag = m(t[b:b + 1, :n], p[b:b + 1, :n])
            assert one_sc.cpu().numpy().tobytes() == sc[b:b + 1].tobytes() and one_mag.cpu().numpy().tobytes() == mag[b:b + 1].tobytes()
    with pytest.raises(ValueError, match="row 0 holds"):
        m.forward_ragged(t, p, [96] + lengths[1:])           # long enough for (96, 64), not for (256, 64)


def test_cli_scores_a_directory_and_reports_what_it_skipped(tmp_path):
    from vocoder_amd import eval as ev
    from vocoder_amd.inference import write_wav
    from vocoder_amd.scoring import MelDistance
    rng = np.random.default_rng(5)
    src, gen = tmp_path / "src", tmp_path / "gen"

    def noise(n, channels=1, scale=0.2):
        return (scale * rng.normal(size=(n, channels))).astype(np.float32)
    a = noise(12000)
    write_wav(src / "a.wav", a, 48000), write_wav(gen / "a.wav", a[::2] + noise(6000, scale=0.05), 24000)      # the source at another rate
    b = noise(6500, channels=2)
    write_wav(src / "sub" / "b.wav", b, 24000), write_wav(gen / "sub" / "b.wav", b.mean(1) + noise(6500, scale=0.05)[:, 0], 24000)    # stereo
    write_wav(src / "c.wav", noise(6000), 24000)                                                                  # no partner
    out = tmp_path / "scores.json"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "vocoder_amd.eval", str(src), str(gen), "--json", str(out)],
                       capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "Average scores:" in r.stdout and "scored 2 pairs, skipped 1" in r.stdout
    assert "skipped c.wav" in r.stdout and "does not exist" in r.stdout
    for k in ev.METRICS:
        assert f"    {k}: " in r.stdout
    j = json.loads(out.read_text())
    names = ["a.wav", os.path.join("sub", "b.wav")]
    assert sorted(j["files"]) == names and [s["name"] for s in j["skipped"]] == ["c.wav"] and j["sr"] == 24000
    # the per-file values are MelDistance.forward_list's on the same data (and do not depend on the batch: each pair alone here)
    m = MelDistance(24000).cuda()
    res: dict = {}
    for name in names:
        s, g = ev.load_mono(src / name, 24000, "cuda", res), ev.load_mono(gen / name, 24000, "cuda", res)
        want = float(m.forward_list([s], [g])[0])
        assert abs(j["files"][name]["spec_diff"] - want) <= 1e-12, (name, j["files"][name], want)
        assert 0.01 < want < 1.0 and all(math.isfinite(j["files"][name][k]) and j["files"][name][k] > 0 for k in ev.METRICS)
    assert abs(j["mean"]["spec_diff"] - np.mean([j["files"][n]["spec_diff"] for n in names])) <= 1e-12
