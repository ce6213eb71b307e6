"""Host (no GPU): the posterior encoder stream's surface (include/fishvoc.h fv_wnstream_*, PosteriorEncoder.stream, the codec's
--chunk-samples) — the declared entry points, the emission rule against a brute-force simulation, and the refusals a host can see."""
import ctypes
import os
import re

import pytest

from vocoder_amd import _lib, codec
from vocoder_amd.modules.encoders import posterior_encoder as pe

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_wnstream_create", "fv_wnstream_push", "fv_wnstream_flush", "fv_wnstream_reset", "fv_wnstream_pending", "fv_wnstream_lookahead",
           "fv_wnstream_destroy")


def test_entry_points_are_declared_exported_and_present():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_wnstream_\w+)\s*\(", hdr))
    assert declared == set(ENTRIES)
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.fv_abi_version() == 5 and _lib.FV_ABI_VERSION == 5


def brute_force(chunks, R):
    """Frame by frame: latent frame t is final once the input frame t + R has arrived, or the utterance has ended."""
    out, N, E = [], 0, 0
    for c in chunks:
        N += c
        E0 = E
        while E + R < N:         # frame E reads inputs up to E + R <= N - 1
            E += 1
        out.append((E0, E))
    out.append((E, N))
    return out


@pytest.mark.parametrize("R", [0, 1, 8, 32])
def test_schedule_is_the_brute_force_rule(R):
    cases = [[], [0], [1], [0, 0, 5, 0], [1] * 70, [1, 8, 3, 8, 8, 8, 0, 8, 8], [R], [R + 1], [R, 0, 1], [100], [3, 0, 64, 0, 0, 2, 31, 33]]
    for chunks in cases:
        got = pe.schedule(chunks, R)
        assert got == brute_force(chunks, R), (chunks, R)
        assert len(got) == len(chunks) + 1
        assert got[-1][1] == sum(chunks)                                          # the flush ends at N
        assert got[-1][1] - got[-1][0] <= R                                       # and emits at most R frames
        assert all(a[1] == b[0] for a, b in zip(got, got[1:]))                    # no frame twice, none skipped
        assert all(e1 - e0 <= c for (e0, e1), c in zip(got, chunks))              # a push emits at most what it received


def test_create_refusals_name_their_cause():
    L = _lib.lib()
    s = ctypes.c_void_p()
    assert L.fv_wnstream_create(None, 1, 8, ctypes.byref(s)) == _lib.FV_ERR_INVALID
    assert L.fv_last_error().decode().startswith("fv_wnstream_create:") and "null" in L.fv_last_error().decode()
    cfg = _lib.PosteriorConfig(20, 8, 32, 5, 1, 1, 2, 0)
    h = ctypes.c_void_p()
    assert L.fv_posterior_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        assert L.fv_wnstream_create(h, 1, 8, None) == _lib.FV_ERR_INVALID and "null" in L.fv_last_error().decode()
        assert L.fv_wnstream_create(h, 1, 8, ctypes.byref(s)) == _lib.FV_ERR_STATE and not s.value
        msg = L.fv_last_error().decode()
        assert msg.startswith("fv_wnstream_create:") and "finalized" in msg, msg
    finally:
        L.fv_posterior_destroy(h)
    # calls on no stream
    got = ctypes.c_int64(7)
    assert L.fv_wnstream_push(None, None, 0, 0, 0, None, None, None, 1, ctypes.byref(got), None) == _lib.FV_ERR_INVALID
    assert "fv_wnstream_push" in L.fv_last_error().decode() and got.value == 7
    assert L.fv_wnstream_flush(None, None, None, None, 1, None, None) == _lib.FV_ERR_INVALID and "fv_wnstream_flush" in L.fv_last_error().decode()
    assert L.fv_wnstream_reset(None) == _lib.FV_ERR_INVALID
    assert L.fv_wnstream_pending(None) == -1 and L.fv_wnstream_lookahead(None) == -1
    L.fv_wnstream_destroy(None)


def test_python_stream_refusals_without_a_device():
    m = pe.PosteriorEncoder(20, 8, 32, n_layers=2).eval()
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.stream()
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.train().stream()              # the device comes first, as in forward
    assert m.stream_is_bit_exact


def test_cli_refuses_chunk_samples_without_the_posterior_encoder(capsys):
    with pytest.raises(SystemExit) as e:
        codec.main(["encode", "-i", "a.wav", "--chunk-samples", "777"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--chunk-samples" in err and "--encoder posterior" in err
    with pytest.raises(SystemExit) as e:
        codec.main(["decode", "-i", "a.codes.npy", "--encoder", "posterior", "--chunk-samples", "777"])
    assert e.value.code == 2 and "encode" in capsys.readouterr().err


def test_encode_stream_refuses_what_it_cannot_serve_by_name():
    class Audio:
        takes_audio = True
    c = codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, encoder_depths=(1,), encoder_dims=(32,),
                          decoder_depths=(1,), decoder_dims=(32,))
    with pytest.raises(ValueError, match="ConvNeXtEncoder"):
        c.encode_stream()
    c.encoder = torch_module(Audio)
    with pytest.raises(ValueError, match="takes_audio"):
        c.encode_stream()
    p = codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, encoder="posterior", hidden_channels=32,
                          posterior_layers=2, decoder_depths=(1,), decoder_dims=(32,))
    p.frontend = None
    with pytest.raises(ValueError, match="front-end"):
        p.encode_stream()


def torch_module(base):
    from torch import nn
    return type("AudioEncoder", (base, nn.Module), {})()
