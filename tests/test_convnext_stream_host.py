"""Host (no GPU): the ConvNeXt layer stream's surface (include/fishvoc.h fv_cnxstream_*, ``ConvNeXtEncoder.layer_stream``, the codec's
options on top) — the declared entry points, the emission rule and the plan against a frame-by-frame ring simulation, and the refusals a
host can see."""
import ctypes
import os
import random
import re

import pytest
import torch

from vocoder_amd import _lib, codec
from vocoder_amd.modules.encoders import convnext
from vocoder_amd.modules.encoders.convnext import ConvNeXtEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_cnxstream_create", "fv_cnxstream_push", "fv_cnxstream_flush", "fv_cnxstream_reset", "fv_cnxstream_pending",
           "fv_cnxstream_lookahead", "fv_cnxstream_state_bytes", "fv_cnxstream_destroy", "fv_cnxstream_plan")


def test_entries_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_cnxstream_\w+)\s*\(", hdr))
    assert declared == set(ENTRIES)
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in ENTRIES)
    assert L.fv_abi_version() == 5 and int(re.search(r"#define\s+FV_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5


def test_null_handles_are_refused_by_name():
    L, s, got = _lib.lib(), ctypes.c_void_p(), ctypes.c_int64(7)
    assert L.fv_cnxstream_create(None, 1, 8, ctypes.byref(s)) == _lib.FV_ERR_INVALID
    assert L.fv_last_error().decode().startswith("fv_cnxstream_create:") and "null" in L.fv_last_error().decode()
    assert L.fv_cnxstream_push(None, None, 0, 0, 0, None, 1, ctypes.byref(got), None) == _lib.FV_ERR_INVALID
    assert "fv_cnxstream_push" in L.fv_last_error().decode() and got.value == 7
    assert L.fv_cnxstream_flush(None, None, 1, None, None) == _lib.FV_ERR_INVALID and "fv_cnxstream_flush" in L.fv_last_error().decode()
    assert L.fv_cnxstream_reset(None) == _lib.FV_ERR_INVALID
    assert L.fv_cnxstream_pending(None) == -1 and L.fv_cnxstream_lookahead(None) == -1 and L.fv_cnxstream_state_bytes(None) == -1
    L.fv_cnxstream_destroy(None)


def draws(n, seed):
    """(depths, max_chunk, chunks, T): a few hundred random streams, short utterances and long, small chunks and wide."""
    rng = random.Random(seed)
    for i in range(n):
        depths = [rng.randint(1, 4) for _ in range(rng.randint(1, 3))]
        max_chunk = rng.randint(1, 12) if i % 3 else rng.randint(1, 90)
        R = convnext.lookahead(depths)
        T = rng.randint(0, R + 2) if i % 4 == 0 else rng.randint(1, 300)
        chunks, left = [], T
        while left:
            c = min(left, max_chunk if rng.random() < 0.2 else rng.randint(0, max_chunk))
            chunks.append(c)
            left -= c
        yield depths, max_chunk, chunks, T


def test_schedule_counts():
    for depths, _, chunks, T in draws(300, 1):
        R = convnext.lookahead(depths)
        assert R == 3 * (1 + sum(depths))
        sched = convnext.schedule(chunks, R)
        assert len(sched) == len(chunks) + 1 and sum(b - a for a, b in sched) == T
        N = 0
        for c, (a, b) in zip(chunks, sched):
            N += c
            assert 0 <= a <= b == max(a, N - R)
            if N <= R:
                assert b == 0                      # k = 0 while N <= R
        assert sched[-1][1] == T and all(x[1] == y[0] for x, y in zip(sched, sched[1:]))


def test_ring_simulation_reads_the_frame_it_asks_for():
    """Frame by frame, with rings that keep the last utterance's frames across a reset: every ring read hits the frame asked for, no slot
    is read in the launch that writes it, every chunk frame is filed once and every output column computed once from frames that exist."""
    for depths, max_chunk, chunks, T in draws(300, 2):
        L = sum(depths)
        R, cap = convnext.lookahead(depths), convnext.ring_cap(max_chunk, L)
        step = max(max_chunk, R)
        assert cap >= 6 + step and cap & (cap - 1) == 0
        rings = [[("stale", s) for s in range(cap)] for _ in range(L + 1)]       # [0]: the input ring; [l]: block l's
        done, N, E = [0] * (L + 1), 0, 0
        for c, flush in [(c, False) for c in chunks] + [(0, True)]:
            N0, N1 = N, N + c
            # the stem: window [N0 - 6, N1), ring below N0
            out0, out1 = convnext.front(N0, 0), convnext.front(N1, 0, flush)
            assert out0 == done[0]
            read = {f & (cap - 1) for f in range(max(N0 - 6, 0), N0)}
            for f in range(max(N0 - 6, 0), N0):
                assert rings[0][f & (cap - 1)] == f
            assert not read & {f & (cap - 1) for f in range(N0, N1)}
            for f in range(N0, N1):
                rings[0][f & (cap - 1)] = f
            for t in range(out0, out1):
                assert t - 3 >= N0 - 6 and (t + 3 < N1 or (flush and t + 3 >= N1))
            done[0] = out1
            for lv in range(1, L + 1):
                q = convnext.level_plan(N0, N1, flush, lv)
                assert q["out0"] == done[lv] and q["in1"] == done[lv - 1]
                assert q["in1"] - q["in0"] <= step and q["out1"] - q["out0"] <= step
                if q["tiles"] == 0:
                    assert q["in1"] == q["in0"] and q["out1"] == q["out0"]
                    continue
                read, written = set(), set()
                filed, cols = [0] * (q["in1"] - q["in0"]), [0] * (q["out1"] - q["out0"])
                for j in range(q["tiles"]):
                    t0 = q["out0"] + 32 * j
                    for f in range(t0 - 3, t0 + 35):
                        if f < 0 or f >= q["in1"]:
                            continue                                   # zero by predicate: no slot is read
                        if f < q["in0"]:
                            assert f >= q["in0"] - 6 and rings[lv][f & (cap - 1)] == f, (lv, f)
                            read.add(f & (cap - 1))
                        elif f >= q["file_from"](j):
                            filed[f - q["in0"]] += 1
                            written.add(f & (cap - 1))
                    for t in range(t0, min(t0 + 32, q["out1"])):
                        cols[t - q["out0"]] += 1
                        assert all(t + d < q["in1"] or (flush and t + d >= N1) for d in range(-3, 4))
                assert all(v == 1 for v in filed) and all(v == 1 for v in cols) and not read & written
                for f in range(q["in0"], q["in1"]):
                    rings[lv][f & (cap - 1)] = f
                done[lv] = q["out1"]
            E1 = N1 if flush else max(E, N1 - R)
            assert done[L] == E1
            N, E = N1, E1
        assert N == E == T


def test_the_librarys_plan_is_the_mirror():
    """``fv_cnxstream_plan`` is csrc/cnx_stream_plan.h as the engine calls it: the Python mirror the simulation above runs must agree with it
    level by level, call by call."""
    L, out = _lib.lib(), (ctypes.c_int64 * 6)()
    assert L.fv_cnxstream_plan(0, 0, 0, 0, 8, 1, None) == -1 and L.fv_cnxstream_plan(3, 2, 0, 0, 8, 1, out) == -1
    assert L.fv_cnxstream_plan(0, 1, 0, 3, 8, 2, out) == -1 and L.fv_cnxstream_plan(0, 1, 0, 0, 0, 2, out) == -1
    for depths, max_chunk, chunks, T in draws(120, 3):
        levels, N = sum(depths), 0
        for c, flush in [(c, False) for c in chunks] + [(0, True)]:
            N0, N1 = N, N + c
            assert L.fv_cnxstream_plan(N0, N1, int(flush), 0, max_chunk, levels, out) == convnext.ring_cap(max_chunk, levels)
            out0 = convnext.front(N0, 0)
            assert list(out) == [N0, N1, out0, convnext.front(N1, 0, flush), c + 6, out0 - (N0 - 6)]
            for lv in range(1, levels + 1):
                q = convnext.level_plan(N0, N1, flush, lv)
                assert L.fv_cnxstream_plan(N0, N1, int(flush), lv, max_chunk, levels, out) == convnext.ring_cap(max_chunk, levels)
                assert list(out) == [q["in0"], q["in1"], q["out0"], q["out1"], q["tiles"], q["file_from"](1) if q["tiles"] > 1 else -1]
            N = N1


def test_cli_keeps_its_check_of_chunk_samples(capsys):
    for extra in (["--batch-invariant"], ["--encoder", "posterior"], ["--encoder", "posterior", "--batch-invariant"]):
        for bad in ("0", "-5"):
            with pytest.raises(SystemExit) as e:
                codec.main(["encode", "-i", "a.wav", "--chunk-samples", bad] + extra)
            assert e.value.code == 2 and "must be at least 1" in capsys.readouterr().err


def test_the_hint_names_both_settings_for_a_square_stem():
    c = codec.build_vqvae(n_fft=62, hop_length=16, win_length=62, latent_size=32, codebook_size=48, encoder_depths=(1,), encoder_dims=(32,),
                          decoder_depths=(1,), decoder_dims=(32,)).eval()
    assert c.encoder.stem_has_winograd_form
    with pytest.raises(ValueError, match="batch_invariant = True and encoder.conv_algorithm = 'direct'"):
        c.encode_stream(1)
    c.encoder.batch_invariant = True
    with pytest.raises(ValueError, match="conv_algorithm = 'direct'"):
        c.encode_stream(1)
    c.encoder.conv_algorithm = "direct"
    with pytest.raises(RuntimeError, match="HIP device|CUDA/HIP"):
        c.encode_stream(1)


def test_stream_is_bit_exact_follows_batch_invariant():
    m = ConvNeXtEncoder(input_channels=20, depths=(1, 2), dims=(32, 48))
    assert m.stream_is_bit_exact is False and m.lookahead_frames == 12
    m.batch_invariant = True
    assert m.stream_is_bit_exact is True
    m.batch_invariant = False
    assert m.stream_is_bit_exact is False
    sq = ConvNeXtEncoder(input_channels=32, depths=(1,), dims=(32,))       # a C -> C stem has a Winograd form: direct sums as well
    sq.batch_invariant = True
    assert sq.stem_has_winograd_form and not m.stem_has_winograd_form and sq.stream_is_bit_exact is False
    sq.conv_algorithm = "direct"
    assert sq.stream_is_bit_exact is True


def test_layer_stream_needs_the_device():
    m = ConvNeXtEncoder(input_channels=20, depths=(1,), dims=(32,)).eval()
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.layer_stream()
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.train().layer_stream()              # the device comes first, as in forward


def tiny_codec():
    return codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, encoder_depths=(1,), encoder_dims=(32,),
                             decoder_depths=(1,), decoder_dims=(32,)).eval()


def test_encode_stream_takes_a_batch_invariant_convnext_encoder():
    c = tiny_codec()
    with pytest.raises(ValueError, match="encode_stream: ConvNeXtEncoder") as e:
        c.encode_stream(1)
    assert "not bit-exact" in str(e.value) and "or set encoder.batch_invariant = True" in str(e.value)
    c.encoder.batch_invariant = True
    with pytest.raises(RuntimeError, match="HIP device|CUDA/HIP"):        # past the encoder check: the device refusal
        c.encode_stream(1)


def test_encode_pool_still_refuses_convnext():
    c = tiny_codec()
    with pytest.raises(ValueError, match="encode_pool: ConvNeXtEncoder") as e:
        c.encode_pool(3)
    assert "not bit-exact" in str(e.value) and "batch_invariant" not in str(e.value)
    c.encoder.batch_invariant = True
    with pytest.raises(ValueError, match="encode_pool: ConvNeXtEncoder") as e:
        c.encode_pool(3)
    assert "pool form is not built" in str(e.value)


def test_decode_stream_backbone_option_is_checked_on_the_host():
    c = tiny_codec()
    with pytest.raises(ValueError, match="'window' or 'layers'"):
        c.decode_stream(1, 8, backbone="rings")
    with pytest.raises(ValueError, match="two-stage"):
        codec.CodecDecodeStream(c.decoder.head, c.vq, 1, 8, "layers")
    with pytest.raises(RuntimeError, match="CUDA/HIP"):                  # a ConvNeXt backbone: past the option's check, to the device's
        c.decode_stream(1, 8, backbone="layers")


def test_cli_accepts_chunk_samples_with_batch_invariant(capsys, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        codec.main(["encode", "-i", "a.wav", "--chunk-samples", "777", "--batch-invariant"])
    assert e.value.code != 2 and "HIP device" in str(e.value.code)       # past the parser, up to the device check
    with pytest.raises(SystemExit) as e:
        codec.main(["encode", "-i", "a.wav", "--chunk-samples", "777"])
    assert e.value.code == 2 and "--batch-invariant" in capsys.readouterr().err


def test_cli_refuses_batch_invariant_for_decode(capsys):
    with pytest.raises(SystemExit) as e:
        codec.main(["decode", "-i", "a.codes.npy", "--batch-invariant", "--chunk-samples", "777"])
    assert e.value.code == 2 and "encode" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        codec.main(["decode", "-i", "a.codes.npy", "--batch-invariant"])
    assert e.value.code == 2 and "--batch-invariant belongs to encode" in capsys.readouterr().err
