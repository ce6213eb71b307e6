"""Host (no GPU): the scoring entries (include/fishvoc.h fv_spec_distance*) — the ABI surface, the workspace rule, every validation case of
fv_spec_distance (refused before any device call, so it runs here), and the pairing rule of ``python -m vocoder_amd.eval``."""
import ctypes
import os
import re

import numpy as np
import pytest

from vocoder_amd import _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SCORING_API = ("fv_spec_distance_tile", "fv_spec_distance_workspace_bytes", "fv_spec_distance")


def test_entry_points_are_declared_listed_exported_and_the_abi_stays_5():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in SCORING_API:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert {d for d in declared if d.startswith("fv_spec_distance")} == set(SCORING_API)
    assert {n for n in _lib.EXPORTS if n.startswith("fv_spec_distance")} == set(SCORING_API)
    assert "#define FV_ABI_VERSION 5" in hdr and _lib.FV_ABI_VERSION == 5 and L.fv_abi_version() == 5
    assert "#define FV_SPEC_DISTANCE_LOG 1" in hdr and _lib.FV_SPEC_DISTANCE_LOG == 1
    # every entry names the reference code it stands in for
    for name in SCORING_API:
        at = re.search(r"FV_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr).start()
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "eval.py" in comment or "stft.py" in comment, name


def test_tile_and_workspace_rule():
    L = _lib.lib()
    K = L.fv_spec_distance_tile()
    assert K >= 1 and _lib.spec_distance_tile() == K
    ws = L.fv_spec_distance_workspace_bytes
    grid_b, grid_t = (0, 1, 2, 3, 31, 32, 33, 64, 65, 1000), (0, 1, K - 1, K, K + 1, 2 * K + 1, 861, 10 ** 6)
    for b in grid_b:
        col = [ws(b, t) for t in grid_t]
        assert col == sorted(col), (b, col)                  # non-decreasing in T
    for t in grid_t:
        row = [ws(b, t) for b in grid_b]
        assert row == sorted(row), (t, row)                  # non-decreasing in the batch
    assert ws(1000, 10 ** 6) > ws(32, 861) > 0 and ws(32, 861) % 256 == 0
    # room for four doubles per (row, tile)
    for b, t in ((1, 1), (3, K + 1), (32, 861)):
        assert ws(b, t) >= b * -(-t // K) * 32


def _call(L, est=0x1000, ref=0x2000, row_stride=None, ld=10, channels=3, T=10, frames=(10, 4), flags=0, out=0x3000, ws=0x4000, ws_bytes=None,
          host_frames=True):
    """fv_spec_distance with dummy non-null device pointers: a refused call never touches them."""
    B = len(frames)
    arr = (ctypes.c_int32 * max(B, 1))(*frames) if host_frames else None
    row_stride = channels * ld if row_stride is None else row_stride
    ws_bytes = L.fv_spec_distance_workspace_bytes(B, T) if ws_bytes is None else ws_bytes
    return L.fv_spec_distance(est, ref, row_stride, ld, channels, T, arr, B, flags, out, ws, ws_bytes, None)


def test_every_validation_case_is_refused_without_a_gpu():
    L = _lib.lib()
    bad = [dict(est=None), dict(ref=None), dict(out=None), dict(ws=None), dict(host_frames=False),
           dict(channels=0), dict(channels=-2), dict(ld=9), dict(row_stride=29), dict(row_stride=-30),
           dict(ws_bytes=L.fv_spec_distance_workspace_bytes(2, 10) - 1), dict(ws_bytes=0), dict(flags=2), dict(T=-1)]
    for kw in bad:
        assert _call(L, **kw) == _lib.FV_ERR_INVALID, kw
        assert L.fv_last_error().startswith(b"fv_spec_distance:"), kw
    # a bad frame count names its row
    for frames, row in (((10, -1), 1), ((11, 4), 0), ((0, 3, 2 ** 31 - 1, 1), 2), ((1, 2, 3, 4, 5, -7), 5)):
        assert _call(L, frames=frames) == _lib.FV_ERR_INVALID, frames
        msg = L.fv_last_error().decode()
        assert f"frames[{row}]" in msg and f"row {row}" in msg, msg
    # the Python wrapper of the status carries the message
    with pytest.raises(_lib.FishVocError, match=r"frames\[1\]"):
        _lib.check(_call(L, frames=(10, 11)))
    # an empty batch is a no-op whatever else is passed (nothing is enqueued: this machine has no device to enqueue on)
    assert _call(L, frames=(), est=None, ref=None, out=None, ws=None) == _lib.FV_OK


def test_python_wrapper_refuses_cpu_tensors_and_shape_mismatches():
    torch = pytest.importorskip("torch")
    from vocoder_amd import scoring
    with pytest.raises(ValueError, match="no CPU fallback"):
        scoring.spec_distance(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3))
    # the in-place layouts: contiguous, a column slice, a row slice; not a transposed or a column-strided view
    base = torch.zeros(4, 5, 9)
    assert scoring._layout(base) == (9, 45)
    assert scoring._layout(base[:, :, 1:]) == (9, 45) and scoring._layout(base[:, 1:4, 2:7]) == (9, 45)
    assert scoring._layout(base[:1, :, 1:]) == (9, 45) and scoring._layout(base[::2]) == (9, 90)
    assert scoring._layout(base[:, :, ::2]) is None and scoring._layout(base.transpose(1, 2)) is None
    assert scoring._layout(base.expand(4, 5, 9)[:, :1].expand(4, 5, 9)) is None
    # the defaults of the reference: eval.py:55's front-end, gan.yaml:49-53's resolutions
    m = scoring.MelDistance(24000)
    assert (m.mel.n_fft, m.mel.win_length, m.mel.hop_length, m.mel.n_mels, m.mel.batch_invariant, m.training) == (1024, 1024, 256, 128, True, False)
    r = scoring.MultiResolutionSTFTDistance()
    assert r.resolutions == ((1024, 120), (2048, 240), (4096, 480), (512, 50))
    assert all(s.batch_invariant and s.win_length == s.n_fft for s in r.spectrograms)
    assert m.too_short(384) and not m.too_short(385) and r.too_short(1808) and not r.too_short(1809)
    for bad in (1, 384):
        with pytest.raises(ValueError, match="row 1 holds"):
            m._check_lengths([5000, bad, 0], "forward_ragged")
    m._check_lengths([5000, 0, 385], "forward_ragged")         # a length of 0 is an empty row, not an error


def _write(path, n, sr=24000, channels=1):
    from vocoder_amd.inference import write_wav
    write_wav(path, np.zeros((n, channels), np.float32), sr)


def test_cli_pairing_rule(tmp_path):
    from vocoder_amd import eval as ev
    src, gen = tmp_path / "src", tmp_path / "gen"
    _write(src / "a.wav", 5000), _write(gen / "a.wav", 5000)                       # equal
    _write(src / "sub" / "b.wav", 5000), _write(gen / "sub" / "b.wav", 5999)       # 999 longer: cropped to the shorter
    _write(src / "c.wav", 6000), _write(gen / "c.wav", 5000)                       # 1000 apart: skipped
    _write(src / "d.wav", 5000)                                                    # no partner
    _write(src / "e.wav", 5000), (gen / "e.flac").write_bytes(b"fLaC")             # the .flac fallback: no decoder
    _write(src / "f.wav", 10000, sr=48000), _write(gen / "f.wav", 5100, sr=24000)  # another rate: lengths compared at --sr
    _write(src / "g.wav", 5000, channels=2), _write(gen / "g.wav", 4001)           # stereo source, 999 shorter partner
    (gen / "only_generated.wav").parent.mkdir(exist_ok=True), _write(gen / "only_generated.wav", 100)
    pairs, skipped = ev.plan_pairs(src, gen, 24000)
    assert [(p.name, p.source_length, p.generated_length, p.length) for p in pairs] == [
        ("a.wav", 5000, 5000, 5000), ("f.wav", 5000, 5100, 5000), ("g.wav", 5000, 4001, 4001), (os.path.join("sub", "b.wav"), 5000, 5999, 5000)]
    assert all(p.source == src / p.name and p.generated == gen / p.name for p in pairs)
    reasons = dict(skipped)
    assert sorted(reasons) == ["c.wav", "d.wav", "e.wav"]
    assert "differ by 1000 samples" in reasons["c.wav"]
    assert "does not exist" in reasons["d.wav"] and "d.wav" in reasons["d.wav"]
    assert "e.flac" in reasons["e.wav"] and "not supported" in reasons["e.wav"]
    # the glob pattern selects the sources
    pairs, skipped = ev.plan_pairs(src, gen, 24000, "sub/*.wav")
    assert [p.name for p in pairs] == [os.path.join("sub", "b.wav")] and skipped == []
    # lengths at --sr follow the resampler's output length, ceil(sr * L / rate)
    assert ev.length_at(10000, 48000, 24000) == 5000 and ev.length_at(10001, 48000, 24000) == 5001 and ev.length_at(7, 24000, 24000) == 7
    from vocoder_amd.resample import design
    for L, rate in ((10001, 44100), (12345, 22050), (1, 48000)):
        assert ev.length_at(L, rate, 24000) == design(rate, 24000).output_length(L)


def test_cli_help_says_what_is_not_computed(capsys):
    from vocoder_amd import eval as ev
    with pytest.raises(SystemExit) as e:
        ev.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert out.count("PESQ is not computed") == 1 and "--no-stft" in out and "--json" in out and "--batch-size" in out
