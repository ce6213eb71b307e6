"""Host (no GPU): the ConvNeXt layer pool's surface (include/fishvoc.h fv_cnxpool_*, ``ConvNeXtEncoder.layer_pool``, the codec's options on
top) — the declared entry points, the plan in C and in Python, a frame-by-frame simulation of the per-slot rings and the packed buffers, and
the refusals a host can see."""
import ctypes
import os
import random
import re

import pytest

from vocoder_amd import _lib, codec
from vocoder_amd.modules.encoders import convnext
from vocoder_amd.modules.encoders.convnext import ConvNeXtEncoder, ConvNeXtPoolCounters
from vocoder_amd.modules.encoders.posterior_encoder import PosteriorPoolCounters
from vocoder_amd.sessions import PoolStateError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_cnxpool_create", "fv_cnxpool_plan", "fv_cnxpool_step", "fv_cnxpool_reset", "fv_cnxpool_received", "fv_cnxpool_emitted",
           "fv_cnxpool_pending", "fv_cnxpool_lookahead", "fv_cnxpool_max_frames", "fv_cnxpool_launches", "fv_cnxpool_state_bytes",
           "fv_cnxpool_table_size", "fv_cnxpool_destroy")


def test_entries_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_cnxpool_\w+)\s*\(", hdr))
    assert declared == set(ENTRIES)
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.fv_abi_version() == 5 and _lib.FV_ABI_VERSION == 5
    assert int(re.search(r"#define\s+FV_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5
    # a by-value table takes at most 2 KiB: entries of 8 ints
    assert 1 <= L.fv_cnxpool_table_size() <= 2048 // 32


def test_null_handles_are_refused_by_name():
    L, p = _lib.lib(), ctypes.c_void_p()
    assert L.fv_cnxpool_create(None, 1, 8, ctypes.byref(p)) == _lib.FV_ERR_INVALID and not p.value
    assert L.fv_last_error().decode().startswith("fv_cnxpool_create:") and "null" in L.fv_last_error().decode()
    got = (ctypes.c_int64 * 1)(7)
    assert L.fv_cnxpool_step(None, None, 0, None, 0, 0, None, 0, got, None) == _lib.FV_ERR_INVALID
    assert "fv_cnxpool_step" in L.fv_last_error().decode() and "null pool" in L.fv_last_error().decode() and got[0] == 7
    assert L.fv_cnxpool_reset(None, 0) == _lib.FV_ERR_INVALID and "fv_cnxpool_reset" in L.fv_last_error().decode()
    assert L.fv_cnxpool_received(None, 0) == -1 and L.fv_cnxpool_emitted(None, 0) == -1 and L.fv_cnxpool_pending(None, 0) == -1
    assert L.fv_cnxpool_lookahead(None) == -1 and L.fv_cnxpool_max_frames(None) == -1 and L.fv_cnxpool_launches(None) == -1
    assert L.fv_cnxpool_state_bytes(None) == -1
    L.fv_cnxpool_destroy(None)


def c_plan(R, S, max_chunk, counters, items):
    """fv_cnxpool_plan on the counters' state -> (its return value, the counts per item)."""
    L = _lib.lib()
    i64 = ctypes.c_int64 * S
    arr = (_lib.WavPoolItem * max(len(items), 1))(*[_lib.WavPoolItem(s, c, int(f)) for s, c, f in items])
    out = (ctypes.c_int64 * max(len(items), 1))(*([-7] * max(len(items), 1)))
    rc = L.fv_cnxpool_plan(R, S, max_chunk, i64(*counters.received), i64(*counters.emitted), (ctypes.c_int32 * S)(*map(int, counters.flushed)),
                           arr, len(items), out)
    return int(rc), [int(out[i]) for i in range(len(items))]


def random_step(rng, free, max_chunk, p_flush=0.15):
    """(session, frames, flush) for a random non-empty subset of ``free``, in random order: zero-frame items, full chunks, flushes alone and
    with frames."""
    chosen = rng.sample(free, rng.randint(1, len(free)))
    return [(s, rng.choice([0, 0, 1, min(3, max_chunk), max_chunk, rng.randint(0, max_chunk)]), rng.random() < p_flush) for s in chosen]


@pytest.mark.parametrize("depths", [(1,), (2, 1), (6, 3)])
def test_c_plan_python_plan_and_schedule_agree(depths):
    R, S, max_chunk = convnext.lookahead(depths), 5, 8
    rng = random.Random(200 + R)
    cn = ConvNeXtPoolCounters(R, S, max_chunk)
    assert isinstance(cn, PosteriorPoolCounters) and cn.max_frames == max_chunk + R
    history, done, kinds = [[] for _ in range(S)], [False] * S, set()
    for step in range(300):
        for s in range(S):
            if done[s] and rng.random() < 0.3:
                cn.reset(s)
                history[s], done[s] = [], False
                kinds.add("reset")
        free = [s for s in range(S) if not done[s] and (s != 4 or step >= 150)]
        if not free:
            continue
        items, want = random_step(rng, free, max_chunk), []
        for s, c, flush in items:
            kinds.add(("flush with frames" if c else "flush alone") if flush else ("frames" if c else "zero frames"))
            history[s].append(c)
            sched = convnext.schedule(history[s], R)
            k = sched[len(history[s]) - 1][1] - sched[len(history[s]) - 1][0]
            if flush:
                k += sched[-1][1] - sched[-1][0]
                done[s] = True
            want.append(k)
        before = (list(cn.received), list(cn.emitted), list(cn.flushed))
        rc, got_c = c_plan(R, S, max_chunk, cn, items)
        got_py = cn.plan(items)
        assert (list(cn.received), list(cn.emitted), list(cn.flushed)) == before          # a plan changes nothing
        assert got_py == want and got_c == want and rc == max(want), (step, items, want, got_py, got_c, rc)
        assert all(0 <= k <= cn.max_frames for k in want)
        cn.commit(items, got_py)
    assert kinds == {"reset", "flush with frames", "flush alone", "frames", "zero frames"}


def test_each_refusal_of_the_plan_has_its_status_and_changes_nothing():
    R, S, max_chunk = 12, 4, 8
    cn = ConvNeXtPoolCounters(R, S, max_chunk)
    cn.step([(1, 8, False), (2, 3, True)])
    state = (list(cn.received), list(cn.emitted), list(cn.flushed))
    L = _lib.lib()
    cases = [
        ([(0, 1, False), (4, 1, False)], _lib.FV_ERR_INVALID, ValueError, ("item 1", "session 4")),
        ([(0, 1, False), (-1, 1, False)], _lib.FV_ERR_INVALID, ValueError, ("item 1", "session -1")),
        ([(3, 1, False), (0, 2, False), (3, 0, True)], _lib.FV_ERR_INVALID, ValueError, ("duplicate session 3", "item 2")),
        ([(0, 9, False)], _lib.FV_ERR_INVALID, ValueError, ("item 0", "session 0", "9 frames", "max_chunk = 8")),
        ([(0, -1, False)], _lib.FV_ERR_INVALID, ValueError, ("item 0", "session 0", "-1 frames")),
        ([(0, 1, False), (2, 0, False)], _lib.FV_ERR_STATE, PoolStateError, ("session 2", "item 1", "flushed")),
    ]
    for items, status, exc, words in cases:
        rc, counts = c_plan(R, S, max_chunk, cn, items)
        msg = L.fv_last_error().decode()
        assert rc == status and msg.startswith("fv_cnxpool_plan:"), (items, rc, msg)
        assert all(w in msg for w in words), (msg, words)
        with pytest.raises(exc) as e:
            cn.plan(items)
        assert all(w in str(e.value) for w in words), (str(e.value), words)
        assert (list(cn.received), list(cn.emitted), list(cn.flushed)) == state
    cn.received[0], cn.emitted[0] = (1 << 30) - 4, (1 << 30) - 4 - R
    assert cn.plan([(0, 4, False)]) == [4] and c_plan(R, S, max_chunk, cn, [(0, 4, False)]) == (4, [4])       # up to 2^30 exactly
    rc, _ = c_plan(R, S, max_chunk, cn, [(3, 1, False), (0, 5, False)])
    assert rc == _lib.FV_ERR_INVALID and "2^30 frames" in L.fv_last_error().decode() and "item 1" in L.fv_last_error().decode()
    with pytest.raises(ValueError, match="2\\^30 frames"):
        cn.plan([(3, 1, False), (0, 5, False)])
    # the plan's own arguments
    assert c_plan(-1, S, max_chunk, cn, [])[0] == _lib.FV_ERR_INVALID and "reach" in L.fv_last_error().decode()
    assert c_plan(R, S, (1 << 20) + 1, cn, [])[0] == _lib.FV_ERR_INVALID and "2^20" in L.fv_last_error().decode()
    one = (ctypes.c_int64 * 1)(0)
    assert L.fv_cnxpool_plan(R, 0, max_chunk, one, one, None, None, 0, None) == _lib.FV_ERR_INVALID and "65535" in L.fv_last_error().decode()
    assert L.fv_cnxpool_plan(R, S, max_chunk, None, None, None, None, 0, None) == _lib.FV_ERR_INVALID and "null" in L.fv_last_error().decode()
    cn = ConvNeXtPoolCounters(R, 2, 8)
    assert cn.plan([(0, 0, True)]) == [0] and c_plan(R, 2, 8, cn, [(0, 0, True)]) == (0, [0])              # a flush at 0 frames emits nothing


def test_pool_ring_cap():
    for levels in (1, 2, 9, 16):
        R = 3 * (levels + 1)
        for max_chunk in (1, 2, 7, 8, 64, 100, 1000):
            cap = convnext.pool_ring_cap(max_chunk, levels)
            assert cap & (cap - 1) == 0 and cap >= 6 + max_chunk + R > cap // 2
            assert cap >= convnext.ring_cap(max_chunk, levels)
    assert convnext.pool_ring_cap(1, 1) == 16


def test_ring_simulation_of_slots_at_their_own_pace():
    """Frame by frame for S slots that advance at random paces, flushing alone and with frames, with rings of ``pool_ring_cap`` that keep
    the last utterance's frames across a reset: every ring read hits the frame asked for, no slot is read in the launch that writes it,
    every chunk frame is filed once, every output column is computed once from frames that exist, and the packed offsets are the prefix
    sums of the per-level column counts and never overlap."""
    rng = random.Random(5)
    flushed_with_frames = 0
    for trial in range(60):
        depths = [rng.randint(1, 4) for _ in range(rng.randint(1, 3))]
        L, S = sum(depths), rng.randint(1, 5)
        max_chunk = rng.randint(1, 12) if trial % 3 else rng.randint(1, 90)
        R, cap = convnext.lookahead(depths), convnext.pool_ring_cap(max_chunk, L)
        assert cap >= 6 + max_chunk + R and cap & (cap - 1) == 0
        # rings[l][s]: slot s's row of the input ring (l = 0) and of block l's ring; a slot holds (utterance, frame)
        rings = [[[("stale", i) for i in range(cap)] for _ in range(S)] for _ in range(L + 1)]
        N, E, done, utt, over = [0] * S, [0] * S, [[0] * (L + 1) for _ in range(S)], [0] * S, [False] * S
        for step in range(60):
            for s in range(S):
                if over[s] and rng.random() < 0.4:          # reset: the counters go to 0, the rings keep their frames
                    N[s] = E[s] = 0
                    done[s], utt[s], over[s] = [0] * (L + 1), utt[s] + 1, False
            free = [s for s in range(S) if not over[s]]
            if not free:
                continue
            items = random_step(rng, free, max_chunk, 0.1)
            flushed_with_frames += sum(1 for _, c, f in items if f and c)
            longest = max(c for _, c, _ in items)
            Wmax = 6 + longest
            # the stem's window: row i = [N0 - 6, N1) then zeros to Wmax
            for i, (s, c, flush) in enumerate(items):
                N0, N1, ring = N[s], N[s] + c, rings[0][s]
                out0, out1 = convnext.front(N0, 0), convnext.front(N1, 0, flush)
                assert out0 == done[s][0]
                read = {f & (cap - 1) for f in range(max(N0 - 6, 0), N0)}
                for f in range(max(N0 - 6, 0), N0):
                    assert ring[f & (cap - 1)] == (utt[s], f)
                assert not read & {f & (cap - 1) for f in range(N0, N1)}
                for f in range(N0, N1):
                    ring[f & (cap - 1)] = (utt[s], f)
                off = out0 - (N0 - 6)
                assert off >= 0 and off + (out1 - out0) <= 6 + c <= Wmax
                for t in range(out0, out1):
                    # the conv reads the window's columns t - 3 .. t + 3: frames that exist, or the zeros past a flushed utterance's end
                    assert t - 3 >= N0 - 6 and (t + 3 < N1 or (flush and t + 3 >= N1))
                done[s][0] = out1
            below = None                                    # the packed columns of the level below: (offset, count) per item
            for lv in range(1, L + 1):
                plans = [convnext.level_plan(N[s], N[s] + c, flush, lv) for s, c, flush in items]
                counts = [q["out1"] - q["out0"] for q in plans]
                pk = [sum(counts[:i]) for i in range(len(items))]                   # the prefix sums, as the engine forms them
                P = sum(counts)
                owner = [None] * P
                for i, ((s, c, flush), q) in enumerate(zip(items, plans)):
                    N1, ring = N[s] + c, rings[lv][s]
                    assert q["out0"] == done[s][lv] and q["in1"] == done[s][lv - 1]
                    assert q["in1"] - q["in0"] <= max_chunk + R and counts[i] <= max_chunk + R
                    if below is not None:
                        assert below[i][1] == q["in1"] - q["in0"]                  # the chunk is what the level below packed for this item
                    if q["tiles"] == 0:
                        assert q["in1"] == q["in0"] and counts[i] == 0
                        continue
                    read, written = set(), set()
                    filed, cols = [0] * (q["in1"] - q["in0"]), [0] * counts[i]
                    for j in range(q["tiles"]):
                        t0 = q["out0"] + 32 * j
                        for f in range(t0 - 3, t0 + 35):
                            if f < 0 or f >= q["in1"]:
                                continue                               # zero by predicate: no slot is read
                            if f < q["in0"]:
                                assert f >= q["in0"] - 6 and ring[f & (cap - 1)] == (utt[s], f), (lv, s, f)
                                read.add(f & (cap - 1))
                            elif f >= q["file_from"](j):
                                filed[f - q["in0"]] += 1
                                written.add(f & (cap - 1))
                        for t in range(t0, min(t0 + 32, q["out1"])):
                            cols[t - q["out0"]] += 1
                            assert all(t + d < q["in1"] or (flush and t + d >= N1) for d in range(-3, 4))
                            assert owner[pk[i] + t - q["out0"]] is None
                            owner[pk[i] + t - q["out0"]] = i
                    assert all(v == 1 for v in filed) and all(v == 1 for v in cols) and not read & written
                    for f in range(q["in0"], q["in1"]):
                        ring[f & (cap - 1)] = (utt[s], f)
                    done[s][lv] = q["out1"]
                assert all(o is not None for o in owner)                           # the packed buffer has no gap and no overlap
                assert all(owner[pk[i]:pk[i] + counts[i]] == [i] * counts[i] for i in range(len(items)))
                below = list(zip(pk, counts))
            for s, c, flush in items:
                N1 = N[s] + c
                E1 = N1 if flush else max(E[s], N1 - R)
                assert done[s][L] == E1
                N[s], E[s], over[s] = N1, E1, flush
    assert flushed_with_frames > 50


def test_layer_pool_needs_the_device():
    m = ConvNeXtEncoder(input_channels=20, depths=(1,), dims=(32,)).eval()
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.layer_pool(3)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.train().layer_pool(3)              # the device comes first, as in forward and layer_stream


def tiny_codec(**kw):
    return codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, encoder_depths=(1,), encoder_dims=(32,),
                             decoder_depths=(1,), decoder_dims=(32,), **kw).eval()


def test_encode_pool_layers_option():
    c = tiny_codec()
    with pytest.raises(ValueError, match="encode_pool: ConvNeXtEncoder") as e:       # not batch-invariant: refused by name, with the hint
        c.encode_pool(3, layers=True)
    assert "not bit-exact" in str(e.value) and "or set encoder.batch_invariant = True" in str(e.value)
    c.encoder.batch_invariant = True
    with pytest.raises(ValueError, match="encode_pool: ConvNeXtEncoder") as e:       # without the option: as pinned
        c.encode_pool(3)
    assert "pool form is not built" in str(e.value)
    with pytest.raises(RuntimeError, match="CUDA/HIP|HIP device"):                   # past the encoder check: the device refusal
        c.encode_pool(3, layers=True)
    c.frontend = None
    with pytest.raises(ValueError, match="encode_pool: the codec has no front-end"):
        c.encode_pool(3, layers=True)
    p = tiny_codec(encoder="posterior", hidden_channels=32, posterior_layers=2)
    with pytest.raises(ValueError, match="encode_pool: layers=True needs an encoder with a layer pool") as e:
        p.encode_pool(3, layers=True)
    assert "PosteriorEncoder has no layer_pool" in str(e.value)

    class Audio:
        takes_audio = True
    from torch import nn
    c.encoder = type("AudioEncoder", (Audio, nn.Module), {})()
    with pytest.raises(ValueError, match="takes_audio"):
        c.encode_pool(3, layers=True)


def test_the_hint_names_both_settings_for_a_square_stem():
    c = codec.build_vqvae(n_fft=62, hop_length=16, win_length=62, latent_size=32, codebook_size=48, encoder_depths=(1,), encoder_dims=(32,),
                          decoder_depths=(1,), decoder_dims=(32,)).eval()
    with pytest.raises(ValueError, match="batch_invariant = True and encoder.conv_algorithm = 'direct'"):
        c.encode_pool(3, layers=True)
    c.encoder.batch_invariant = True
    with pytest.raises(ValueError, match="conv_algorithm = 'direct'"):
        c.encode_pool(3, layers=True)


def test_decode_pool_backbone_option_is_checked_on_the_host():
    c = tiny_codec()
    with pytest.raises(ValueError, match="'window' or 'layers'"):
        c.decode_pool(3, 8, backbone="rings")
    with pytest.raises(ValueError, match="two-stage"):
        codec.CodecDecodePool(c.decoder.head, c.vq, 3, 8, "layers")
    with pytest.raises(ValueError, match="two-stage"):
        type(c.decoder)(c.decoder.backbone, c.decoder.head, c.vq).decode_pool(3, 8, backbone="layers")       # UnifyGenerator: the head alone
    with pytest.raises(RuntimeError, match="CUDA/HIP"):                  # a ConvNeXt backbone: past the option's check, to the device's
        c.decode_pool(3, 8, backbone="layers")
