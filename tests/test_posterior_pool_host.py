"""Host (no GPU): the posterior encoder pool's surface (include/fishvoc.h fv_wnpool_*, PosteriorEncoder.pool, VQVAECodec.encode_pool) — the
declared entry points, the plan in C and in Python against a brute-force simulation (one ``schedule()`` per session), and the refusals a
host can see."""
import ctypes
import os
import re

import numpy as np
import pytest

from vocoder_amd import _lib, codec
from vocoder_amd.modules.encoders import posterior_encoder as pe
from vocoder_amd.sessions import PoolStateError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_wnpool_create", "fv_wnpool_plan", "fv_wnpool_step", "fv_wnpool_reset", "fv_wnpool_received", "fv_wnpool_emitted",
           "fv_wnpool_pending", "fv_wnpool_lookahead", "fv_wnpool_max_frames", "fv_wnpool_launches", "fv_wnpool_destroy")


def test_entry_points_are_declared_exported_and_present():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_wnpool_\w+)\s*\(", hdr))
    assert declared == set(ENTRIES)
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.fv_abi_version() == 5 and _lib.FV_ABI_VERSION == 5


def c_plan(R, S, max_chunk, counters, items):
    """fv_wnpool_plan on the counters' state -> (its return value, the counts per item)."""
    L = _lib.lib()
    i64 = ctypes.c_int64 * S
    arr = (_lib.WavPoolItem * max(len(items), 1))(*[_lib.WavPoolItem(s, c, int(f)) for s, c, f in items])
    out = (ctypes.c_int64 * max(len(items), 1))(*([-7] * max(len(items), 1)))
    rc = L.fv_wnpool_plan(R, S, max_chunk, i64(*counters.received), i64(*counters.emitted), (ctypes.c_int32 * S)(*map(int, counters.flushed)), arr,
                          len(items), out)
    return int(rc), [int(out[i]) for i in range(len(items))]


@pytest.mark.parametrize("R", [0, 1, 8, 32])
def test_c_plan_python_plan_and_simulation_agree(R):
    S, max_chunk = 5, 8
    rng = np.random.default_rng(100 + R)
    cn = pe.PosteriorPoolCounters(R, S, max_chunk)
    assert cn.max_frames == max_chunk + R
    history = [[] for _ in range(S)]               # the chunks of every session's utterance so far: the simulation's only state
    done = [False] * S
    kinds = set()
    for step in range(400):
        for s in range(S):                           # a finished slot is reset after a while; slot 4 stays idle for the first half
            if done[s] and rng.random() < 0.3:
                cn.reset(s)
                history[s], done[s] = [], False
                kinds.add("reset")
        free = [s for s in range(S) if not done[s] and (s != 4 or step >= 200)]
        if not free:
            continue
        chosen = rng.permutation(free)[: rng.integers(1, len(free) + 1)]
        items, want = [], []
        for s in chosen:
            c = int(rng.choice([0, 0, 1, 3, 8, int(rng.integers(0, max_chunk + 1))]))
            flush = bool(rng.random() < 0.15)
            kinds.add(("flush with frames" if c else "flush alone") if flush else ("frames" if c else "zero frames"))
            history[s].append(c)
            sched = pe.schedule(history[s], R)
            k = sched[len(history[s]) - 1][1] - sched[len(history[s]) - 1][0]
            if flush:
                k += sched[-1][1] - sched[-1][0]
                done[s] = True
            items.append((int(s), c, flush))
            want.append(k)
        before = (list(cn.received), list(cn.emitted), list(cn.flushed))
        rc, got_c = c_plan(R, S, max_chunk, cn, items)
        got_py = cn.plan(items)
        assert (list(cn.received), list(cn.emitted), list(cn.flushed)) == before          # a plan changes nothing
        assert got_py == want and got_c == want and rc == max(want), (step, items, want, got_py, got_c, rc)
        assert all(0 <= k <= cn.max_frames for k in want)
        cn.commit(items, got_py)
        for s, _, _ in items:
            assert cn.received[s] == sum(history[s]) and cn.pending(s) == cn.received[s] - cn.emitted[s]
            assert cn.emitted[s] == (cn.received[s] if done[s] else max(0, cn.received[s] - R)) and cn.flushed[s] == done[s]
    assert kinds == {"reset", "flush with frames", "flush alone", "frames", "zero frames"}


def test_flush_at_zero_frames_emits_nothing():
    cn = pe.PosteriorPoolCounters(8, 2, 8)
    assert cn.plan([(0, 0, True)]) == [0]
    assert c_plan(8, 2, 8, cn, [(0, 0, True)]) == (0, [0])


def test_each_refusal_has_its_status_and_names_the_item_and_session():
    R, S, max_chunk = 8, 4, 8
    cn = pe.PosteriorPoolCounters(R, S, max_chunk)
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
        assert rc == status and msg.startswith("fv_wnpool_plan:"), (items, rc, msg)
        assert all(w in msg for w in words), (msg, words)
        with pytest.raises(exc) as e:
            cn.plan(items)
        assert all(w in str(e.value) for w in words), (str(e.value), words)
        assert (list(cn.received), list(cn.emitted), list(cn.flushed)) == state
    # more than 2^30 frames in one utterance
    cn.received[0], cn.emitted[0] = (1 << 30) - 4, (1 << 30) - 12
    assert cn.plan([(0, 4, False)]) == [4]                    # up to 2^30 exactly
    rc, _ = c_plan(R, S, max_chunk, cn, [(3, 1, False), (0, 5, False)])
    assert rc == _lib.FV_ERR_INVALID and "2^30 frames" in L.fv_last_error().decode() and "item 1" in L.fv_last_error().decode()
    with pytest.raises(ValueError, match="2\\^30 frames"):
        cn.plan([(3, 1, False), (0, 5, False)])
    # the plan's own arguments
    assert c_plan(-1, S, max_chunk, cn, [])[0] == _lib.FV_ERR_INVALID and "reach" in L.fv_last_error().decode()
    assert c_plan(R, S, (1 << 20) + 1, cn, [])[0] == _lib.FV_ERR_INVALID and "2^20" in L.fv_last_error().decode()
    assert L.fv_wnpool_plan(R, S, max_chunk, None, None, None, None, 0, None) == _lib.FV_ERR_INVALID and "null" in L.fv_last_error().decode()
    with pytest.raises(ValueError, match="2\\^20"):
        pe.PosteriorPoolCounters(R, S, (1 << 20) + 1)
    with pytest.raises(ValueError, match="65535"):
        pe.PosteriorPoolCounters(R, 0, 8)


def test_create_and_null_pool_refusals_name_their_cause():
    L = _lib.lib()
    p = ctypes.c_void_p()
    assert L.fv_wnpool_create(None, 1, 8, ctypes.byref(p)) == _lib.FV_ERR_INVALID
    assert L.fv_last_error().decode().startswith("fv_wnpool_create:") and "null" in L.fv_last_error().decode()
    cfg = _lib.PosteriorConfig(20, 8, 32, 5, 1, 1, 2, 0)
    h = ctypes.c_void_p()
    assert L.fv_posterior_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        assert L.fv_wnpool_create(h, 1, 8, None) == _lib.FV_ERR_INVALID and "null" in L.fv_last_error().decode()
        assert L.fv_wnpool_create(h, 1, 8, ctypes.byref(p)) == _lib.FV_ERR_STATE and not p.value
        msg = L.fv_last_error().decode()
        assert msg.startswith("fv_wnpool_create:") and "finalized" in msg, msg
    finally:
        L.fv_posterior_destroy(h)
    got = (ctypes.c_int64 * 1)(7)
    assert L.fv_wnpool_step(None, None, 0, None, 0, 0, None, None, None, 0, got, None) == _lib.FV_ERR_INVALID
    assert "fv_wnpool_step" in L.fv_last_error().decode() and got[0] == 7
    assert L.fv_wnpool_reset(None, 0) == _lib.FV_ERR_INVALID and "fv_wnpool_reset" in L.fv_last_error().decode()
    assert L.fv_wnpool_received(None, 0) == -1 and L.fv_wnpool_emitted(None, 0) == -1 and L.fv_wnpool_pending(None, 0) == -1
    assert L.fv_wnpool_lookahead(None) == -1 and L.fv_wnpool_max_frames(None) == -1 and L.fv_wnpool_launches(None) == -1
    L.fv_wnpool_destroy(None)


def test_python_pool_refusals_without_a_device():
    m = pe.PosteriorEncoder(20, 8, 32, n_layers=2).eval()
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.pool(4, 8)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.train().pool(4, 8)              # the device comes first, as in forward and stream
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.eval().stream()                 # the stream's refusal is the same one


def test_encode_pool_refuses_what_it_cannot_serve_by_name():
    from torch import nn

    class Audio:
        takes_audio = True
    c = codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, encoder_depths=(1,), encoder_dims=(32,),
                          decoder_depths=(1,), decoder_dims=(32,))
    with pytest.raises(ValueError, match="encode_pool: ConvNeXtEncoder") as e:
        c.encode_pool(3)
    assert "not bit-exact" in str(e.value)
    c.encoder = type("AudioEncoder", (Audio, nn.Module), {})()
    with pytest.raises(ValueError, match="takes_audio"):
        c.encode_pool(3)
    p = codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, encoder="posterior", hidden_channels=32,
                          posterior_layers=2, decoder_depths=(1,), decoder_dims=(32,))
    p.frontend = None
    with pytest.raises(ValueError, match="encode_pool: the codec has no front-end"):
        p.encode_pool(3)
