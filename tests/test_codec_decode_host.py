"""Host (no GPU): the surface of the codec's decode direction (include/fishvoc.h fv_stream_*_codes / fv_pool_*_codes / fv_*_ring_bytes,
CodeStream / CodeSessionPool, VQVAECodec.decode_stream / decode_pool, the codec's --chunk-frames) — the declared entry points and the refusals
a host can see."""
import ctypes
import os
import re

import pytest

from vocoder_amd import _lib, codec
from vocoder_amd.engine import code_chunk

torch = pytest.importorskip("torch")
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRIES = ("fv_stream_create_codes", "fv_stream_push_codes", "fv_codepool_create", "fv_codepool_step", "fv_stream_ring_bytes",
           "fv_codepool_ring_bytes")


def test_entry_points_are_declared_exported_and_present_and_the_abi_stays():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    assert set(ENTRIES) <= declared and set(ENTRIES) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRIES:
        assert getattr(L, name).argtypes, name
    assert re.search(r"#define FV_ABI_VERSION 5\b", hdr) and _lib.FV_ABI_VERSION == 5 and L.fv_abi_version() == 5
    assert "must outlive the handle" in hdr and "FV_ABI_VERSION does not change" in hdr


def test_null_handles_are_refused_or_cost_nothing():
    L = _lib.lib()
    assert L.fv_stream_ring_bytes(None) == 0 and L.fv_codepool_ring_bytes(None) == 0
    h = ctypes.c_void_p()
    assert L.fv_stream_create_codes(None, None, ctypes.byref(_lib.StreamConfig(1, 8, -1, -1)), ctypes.byref(h)) == _lib.FV_ERR_INVALID
    assert L.fv_last_error().decode().startswith("fv_stream_create_codes:") and not h.value
    assert L.fv_codepool_create(None, None, ctypes.byref(_lib.PoolConfig(1, 8, -1, -1)), ctypes.byref(h)) == _lib.FV_ERR_INVALID
    assert L.fv_last_error().decode().startswith("fv_codepool_create:") and not h.value
    got = ctypes.c_int64(7)
    assert L.fv_stream_push_codes(None, None, None, 1, None, ctypes.byref(got), None, 0, None) == _lib.FV_ERR_INVALID
    assert "fv_stream_push_codes" in L.fv_last_error().decode() and got.value == 0
    assert L.fv_codepool_step(None, None, 0, None, None, 0, None, 0, None, None, 0, None) == _lib.FV_ERR_INVALID
    assert "fv_codepool_step" in L.fv_last_error().decode()


def test_command_line_refusals(capsys):
    with pytest.raises(SystemExit) as e:
        codec.main(["encode", "-i", "a.wav", "--chunk-frames", "5"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--chunk-frames" in err and "decode" in err
    for bad in ("0", "-3"):
        with pytest.raises(SystemExit) as e:
            codec.main(["decode", "-i", "a.codes.npy", "--chunk-frames", bad])
        assert e.value.code == 2 and "at least 1" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        codec.main(["decode", "-i", "a.codes.npy", "--chunk-samples", "777"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "encode" in err and "there is no decode stream" not in err


def test_chunks_of_codes_are_refused_before_any_device_is_asked():
    ok = torch.zeros((2, 2, 5), dtype=torch.int64)
    with pytest.raises(TypeError, match="int64 or int32"):
        code_chunk(ok.to(torch.float32), 2, 2, 8, "CodeStream.push")
    with pytest.raises(TypeError, match="tensor"):
        code_chunk([[1, 2]], 2, 2, 8, "CodeStream.push")
    with pytest.raises(ValueError, match="3 layers of codes for a quantiser of 2"):
        code_chunk(torch.zeros((3, 2, 5), dtype=torch.int64), 2, 2, 8, "CodeStream.push")
    with pytest.raises(ValueError, match="shape"):
        code_chunk(torch.zeros((2, 3, 5), dtype=torch.int64), 2, 2, 8, "CodeStream.push")       # three rows for a batch of two
    with pytest.raises(ValueError, match="shape"):
        code_chunk(torch.zeros((5,), dtype=torch.int64), 2, 2, 8, "CodeStream.push")
    with pytest.raises(ValueError, match="9 frames, more than max_chunk_frames = 8"):
        code_chunk(torch.zeros((2, 9), dtype=torch.int32), 2, 2, 8, "CodeStream.push")
    with pytest.raises(ValueError, match="max_chunk_frames"):
        code_chunk(torch.zeros((9,), dtype=torch.int32), 2, None, 8, "CodeSessionPool.step")      # a pool item: (c,) or (n_q, c)
    with pytest.raises(ValueError, match="shape"):
        code_chunk(torch.zeros((1, 2, 5), dtype=torch.int32), 2, None, 8, "CodeSessionPool.step")
    with pytest.raises(RuntimeError, match="HIP device"):                                        # a well-formed chunk: only the device is missing
        code_chunk(ok, 2, 2, 8, "CodeStream.push")
    with pytest.raises(RuntimeError, match="HIP device"):
        code_chunk(torch.zeros((2, 5), dtype=torch.int64), 2, None, 8, "CodeSessionPool.step")


def test_decoders_that_cannot_stream_are_refused_by_name():
    from torch import nn
    from vocoder_amd.modules.generators import UnifyGenerator
    c = codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, encoder_depths=(1,), encoder_dims=(32,),
                          decoder_depths=(1,), decoder_dims=(32,)).eval()
    with pytest.raises(RuntimeError, match="HIP device"):                    # the tiny codec is well-formed: only the device is missing
        c.decode_stream()
    with pytest.raises(RuntimeError, match="HIP device"):
        c.decode_pool(2)
    head, vq = c.decoder.head, c.vq
    for make in (lambda m: m.decode_stream(), lambda m: m.decode_pool(2)):
        with pytest.raises(ValueError, match="Identity has no engine"):
            make(codec.VQVAECodec(c.encoder, nn.Identity(), vq))
        with pytest.raises(ValueError, match="Linear has no engine"):
            make(codec.VQVAECodec(c.encoder, UnifyGenerator(nn.Linear(2, 2), head), vq))
        with pytest.raises(ValueError, match="no quantiser"):
            make(codec.VQVAECodec(c.encoder, head, None))
        with pytest.raises(ValueError, match="VQ module is not present"):
            make(UnifyGenerator(c.decoder.backbone, head))
        with pytest.raises(RuntimeError, match="HIP device"):
            make(UnifyGenerator(c.decoder.backbone, head, vq))
    from types import SimpleNamespace
    from vocoder_amd.engine import CodeSessionPool, CodeStream
    for handle in (CodeStream, CodeSessionPool):
        with pytest.raises(TypeError, match="quantiser"):                    # the quantiser is looked at before the engine is
            handle(SimpleNamespace(device=torch.device("cpu")), nn.Identity(), 1, 8)
