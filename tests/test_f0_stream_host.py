"""Host (no GPU): the streaming F0 tracker and pitch template (include/fishvoc.h fv_yin_*, fv_osc_*) — the ABI surface, the emission rule stated
three times (C: fv_yin_frames_ready; Python: vocoder_amd.f0.frames_ready; the restatement f0_stream_reference.py), the counters under random
chunkings, and the chunked restatement against the whole-row one."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import f0_reference as fref
import f0_stream_reference as sref
from vocoder_amd import _lib
from vocoder_amd import f0 as f0mod

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

YIN_API = ("fv_yin_frames_ready", "fv_yin_stream_create", "fv_yin_stream_pending_samples", "fv_yin_stream_push", "fv_yin_stream_flush",
           "fv_yin_stream_reset", "fv_yin_stream_destroy")
OSC_API = ("fv_osc_stream_create", "fv_osc_stream_pending_frames", "fv_osc_stream_push", "fv_osc_stream_flush", "fv_osc_stream_reset",
           "fv_osc_stream_destroy")
# the whole-row families, as test_f0_host.py pins them
F0_API = ("fv_f0_plan", "fv_f0_create", "fv_f0_destroy", "fv_f0_workspace_bytes", "fv_f0_forward")
TEMPLATE_API = ("fv_template_create", "fv_template_destroy", "fv_template_workspace_bytes", "fv_template_forward")

# (sr, W, hop, fmin, fmax, L): the configurations the rules were simulated on
CONFIGS = [(8000, 512, 128, 50.0, 500.0, 3001), (16000, 1024, 256, 60.0, 800.0, 2900)]


def test_entry_points_are_declared_listed_exported_and_the_abi_stays_5():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    for name in YIN_API + OSC_API:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        at = re.search(r"FV_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr).start()
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "refinegan.py:287" in comment and "hifigan.py:226" in comment, name
    assert {d for d in declared if d.startswith("fv_yin_")} == set(YIN_API)
    assert {d for d in declared if d.startswith("fv_osc_")} == set(OSC_API)
    assert {n for n in _lib.EXPORTS if n.startswith(("fv_yin_", "fv_osc_"))} == set(YIN_API + OSC_API)
    # additive: the pinned families keep their entries and the ABI its number
    assert {d for d in declared if d.startswith("fv_f0_")} == set(F0_API)
    assert {d for d in declared if d.startswith("fv_template_")} == set(TEMPLATE_API)
    assert "#define FV_ABI_VERSION 5" in hdr and _lib.FV_ABI_VERSION == 5 and L.fv_abi_version() == 5
    import vocoder_amd
    for name in ("frames_ready", "YinF0Stream", "PitchTemplateStream", "TemplateStream"):
        assert getattr(vocoder_amd, name) is getattr(f0mod, name), name
    from vocoder_amd._handle import _Handle
    assert issubclass(f0mod.YinF0Stream, _Handle) and issubclass(f0mod.PitchTemplateStream, _Handle)
    for cls in (f0mod.YinF0Stream, f0mod.PitchTemplateStream, f0mod.TemplateStream):
        assert all(hasattr(cls, m) for m in ("push", "flush", "reset", "close", "__enter__", "__exit__")), cls
    from vocoder_amd import inference
    assert inspect.signature(inference.stream_wav_synthesis).parameters["template"].default is None
    assert inspect.signature(inference.stream_synthesis).parameters["template"].default is None


def _c_ready(sr, W, hop, fmin, fmax, N):
    c = _lib.F0Config(sr, W, hop, fmin, fmax, 0.1)
    return int(_lib.lib().fv_yin_frames_ready(ctypes.byref(c), N))


def test_frames_ready_agrees_between_c_python_and_the_restatement_over_a_grid():
    grid = [(8000, 512, 128, 50.0, 500.0), (16000, 1024, 256, 60.0, 800.0), (44100, 2048, 512, 40.0, 1100.0),
            (8000, 512, 300, 50.0, 500.0), (8000, 512, 511, 50.0, 500.0),      # hop > W / 2
            (8000, 512, 512, 50.0, 500.0), (8000, 512, 1, 50.0, 500.0), (16000, 1024, 333, 60.0, 800.0)]
    checked = 0
    for sr, W, hop, fmin, fmax in grid:
        edge = hop // 2 + W // 2
        Ns = set(range(0, 40)) | set(range(edge - 3, edge + 4)) | set(range(edge + hop - 2, edge + hop + 3)) | {5 * hop, 5 * hop + 1, 11025, 99999}
        prev = 0
        for N in sorted(n for n in Ns if n >= 0):
            want = sref.frames_ready(N, W, hop)
            assert _c_ready(sr, W, hop, fmin, fmax, N) == want == f0mod.frames_ready(N, W, hop), (sr, W, hop, N)
            assert prev <= want <= N // hop
            # the rule's meaning: frame want - 1 reads nothing at or after N, frame `want` does or does not exist yet
            if want:
                assert (want - 1) * hop + hop // 2 - W // 2 + W <= N
            assert want * hop + hop // 2 - W // 2 + W > N or (want + 1) * hop > N
            prev, checked = want, checked + 1
        assert sref.frames_ready(edge - 1, W, hop) == 0
        assert sref.frames_ready(max(edge, hop), W, hop) == 1
    assert checked > 400
    # the production plan: the first frame is ready at N = 1280, and one frame of 11025 samples waits for the flush
    assert _c_ready(44100, 2048, 512, 40.0, 1100.0, 1279) == 0 and _c_ready(44100, 2048, 512, 40.0, 1100.0, 1280) == 1
    assert _c_ready(44100, 2048, 512, 40.0, 1100.0, 11025) == 20 and 11025 // 512 == 21
    # refusals: -1 with the reason
    assert _c_ready(44100, 2048, 512, 40.0, 1100.0, -1) == -1
    assert _c_ready(44100, 2047, 512, 40.0, 1100.0, 100) == -1 and "frame_length" in _lib.lib().fv_last_error().decode()
    assert _lib.lib().fv_yin_frames_ready(None, 0) == -1


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.lib()
    h = ctypes.c_void_p()
    got = ctypes.c_int64(7)
    assert L.fv_yin_stream_create(None, 1, 16, ctypes.byref(h)) == _lib.FV_ERR_INVALID and h.value is None
    assert L.fv_osc_stream_create(None, 1, 16, ctypes.byref(h)) == _lib.FV_ERR_INVALID and h.value is None
    assert L.fv_yin_stream_push(None, None, 0, 1, None, None, 0, ctypes.byref(got), None) == _lib.FV_ERR_INVALID and got.value == 0
    assert L.fv_yin_stream_flush(None, None, None, 0, ctypes.byref(got), None) == _lib.FV_ERR_INVALID
    assert L.fv_osc_stream_push(None, None, 0, 1, None, 0, ctypes.byref(got), None) == _lib.FV_ERR_INVALID
    assert L.fv_osc_stream_flush(None, None, 0, ctypes.byref(got), None) == _lib.FV_ERR_INVALID
    assert L.fv_yin_stream_reset(None) == _lib.FV_ERR_INVALID and L.fv_osc_stream_reset(None) == _lib.FV_ERR_INVALID
    assert L.fv_yin_stream_pending_samples(None) == 0 and L.fv_osc_stream_pending_frames(None) == 0
    L.fv_yin_stream_destroy(None)
    L.fv_osc_stream_destroy(None)
    # sizes are checked before anything is allocated
    t = ctypes.c_void_p()
    _lib.check(L.fv_template_create(ctypes.byref(_lib.TemplateConfig(44100, 512, 0, 1.0)), ctypes.byref(t)))
    assert L.fv_osc_stream_create(t, 1, 1 << 28, ctypes.byref(h)) == _lib.FV_ERR_INVALID and "2^30" in L.fv_last_error().decode()
    assert L.fv_osc_stream_create(t, 0, 8, ctypes.byref(h)) == _lib.FV_ERR_INVALID and h.value is None
    L.fv_template_destroy(t)


@pytest.mark.parametrize("seed", range(6))
def test_counters_under_random_chunkings(seed):
    """Host arithmetic alone: the emit counts sum to L // hop after the flush and pending stays under W (tracker), to T frames (oscillator)."""
    rng = np.random.default_rng(seed)
    for sr, W, hop in ((8000, 512, 128), (16000, 1024, 256), (44100, 2048, 512), (8000, 512, 300), (8000, 512, 512), (8000, 512, 1)):
        L = int(rng.integers(0, 6 * W))
        N = E = total = 0
        for c in sref.chunk_sizes(L, rng, 2 * W):
            N += c
            E2 = max(E, sref.frames_ready(N, W, hop))
            total, E = total + (E2 - E), E2
            assert 0 <= sref.pending_samples(N, E, W, hop) < W, (sr, W, hop, N, E)
        total += N // hop - E
        assert N == L and total == L // hop
    for W, hop in ((512, 600), (512, 513), (64, 1000)):      # hop > W: pending can pass W and stays under W / 2 + ceil(hop / 2), what the stream carries
        L = int(rng.integers(0, 8 * hop))
        N = E = total = most = 0
        for c in sref.chunk_sizes(L, rng, 2 * hop):
            N += c
            E2 = max(E, sref.frames_ready(N, W, hop))
            total, E = total + (E2 - E), E2
            most = max(most, sref.pending_samples(N, E, W, hop))
            assert sref.pending_samples(N, E, W, hop) < W // 2 + (hop + 1) // 2, (W, hop, N, E)
        assert total + N // hop - E == L // hop
    for T in (0, 1, 2, 3, 40, int(rng.integers(4, 500))):
        Tn = E = total = 0
        for c in sref.chunk_sizes(T, rng, 17):
            Tn += c
            E2 = sref.osc_emitted(Tn, E)
            total, E = total + (E2 - E), E2
            assert 0 <= Tn - E <= 1 and E == max(0, Tn - 1)
        total += sref.osc_emitted(Tn, E, flush=True) - E
        assert Tn == T and total == T


@pytest.fixture(scope="module")
def whole():
    """The whole-row restatement of both configurations, computed once."""
    out = {}
    for sr, W, hop, fmin, fmax, L in CONFIGS:
        x = fref.glide(L, sr, seed=1)[0]
        out[sr] = (x, fref.yin(x, sr, hop, W, fmin, fmax))
    return out


@pytest.mark.parametrize("sr,W,hop,fmin,fmax,L", CONFIGS)
def test_the_chunked_tracker_restatement_equals_the_whole_row_one_exactly(whole, sr, W, hop, fmin, fmax, L):
    x, ref = whole[sr]
    worst = 0
    for name, sizes in (("whole", [L]), ("hop", [hop] * (L // hop) + [L % hop]), ("37", [37] * (L // 37) + [L % 37]), ("1", [1] * L),
                        ("random", sref.chunk_sizes(L, np.random.default_rng(3), 700))):
        st = sref.YinStream(sr, hop, W, fmin, fmax)
        parts, at = [], 0
        for c in sizes:
            E = st.E
            parts.append(st.push(x[at:at + c]))
            at += c
            assert st.E - E == len(parts[-1]["f0"]) and st.E == max(E, sref.frames_ready(at, W, hop))
        parts.append(st.flush())
        assert at == L and st.E == L // hop
        for key in ("f0", "aperiodicity", "lag"):
            got = np.concatenate([p[key] for p in parts])
            assert got.shape == ref[key].shape and np.array_equal(got, ref[key]), (name, key)
        worst = max(worst, st.max_pending)
    print(f"sr = {sr}: largest pending count {worst} of W = {W}")
    assert worst <= W - 1


@pytest.mark.parametrize("sr,W,hop,fmin,fmax,L", CONFIGS)
def test_the_chunked_oscillator_restatement_equals_the_whole_row_one_exactly(whole, sr, W, hop, fmin, fmax, L):
    rng = np.random.default_rng(5)
    T = 40
    f0 = np.where(rng.random(T) < 0.3, 0.0, rng.uniform(80.0, 0.24 * sr, T))
    f0[7] = np.nan
    tracks = [f0, np.concatenate([whole[sr][1]["f0"], np.zeros(T)])[:T]]
    for track in tracks:
        phi, inc, voiced = fref.phase(track, sr, hop)
        for sizes in ([T], [1] * T, [3] * 13 + [1], [0, 2, 0, 38]):
            assert sum(sizes) == T
            st = sref.OscStream(sr, hop)
            parts, at = [], 0
            for c in sizes:
                parts.append(st.push(track[at:at + c]))
                at += c
                assert len(parts[-1][0]) % hop == 0 and st.E == max(0, at - 1)
            parts.append(st.flush())
            for i, want in enumerate((phi, inc, voiced)):
                got = np.concatenate([p[i] for p in parts])
                assert got.shape == want.shape and np.array_equal(got, want), (sizes[:4], i)


class _Fake:
    """A stream that emits what it is told: ``plan`` is the widths of the pushes' outputs, then the flush's."""

    def __init__(self, rows, plan, log=None):
        self.rows, self.plan, self.log, self.next = rows, list(plan), log, 0

    def _out(self):
        import torch
        k = self.plan.pop(0)
        out = torch.arange(self.next, self.next + k, dtype=torch.float32).expand(1, self.rows, k)
        self.next += k
        return out

    def push(self, x, template=None):
        if self.log is not None:
            self.log.append((x.clone(), template.clone()))
            return x.new_zeros((1, 1, x.shape[-1] * 4))
        return self._out()

    def flush(self):
        if self.log is not None:
            return self.plan.pop(0)
        return self._out()


def test_the_join_stage_pairs_frames_with_their_template_samples_and_names_both_totals():
    """Host: inference._TemplateJoin on streams that emit by a plan.  The mel branch runs ahead, then the template branch; the generator gets
    every frame once, in order, with its own hop samples, at most chunk_frames at a time; totals that differ raise with both named."""
    import torch
    from vocoder_amd import inference
    hop, log = 4, []
    tail = torch.full((1, 1, 5), 9.0)
    join = inference._TemplateJoin(_Fake(2, [3, 0, 2, 4, 1]), _Fake(1, [0, 4 * hop, 0, 1 * hop, 5 * hop]), _Fake(1, [tail], log), 2, hop)
    x = torch.zeros(1, 7)
    widths = [int(join.push(x).shape[-1]) for _ in range(4)]
    assert widths == [0, 4 * 3, 4 * 1, 4 * 1]         # the fake generator gives 4 columns per frame; frames pushed per call: 0, 3, 1, 1
    out = join.flush()
    assert int(out.shape[-1]) == 4 * 5 + 5 and torch.equal(out[..., -5:], tail)
    assert [int(m.shape[-1]) for m, _ in log] == [2, 1, 1, 1, 2, 2, 1] and all(t.shape[-1] == m.shape[-1] * hop for m, t in log)
    assert torch.equal(torch.cat([m for m, _ in log], dim=-1)[0, 0], torch.arange(10.0))
    assert torch.equal(torch.cat([t for _, t in log], dim=-1)[0, 0], torch.arange(10.0 * hop))
    assert join.mel_frames == join.template_frames == 10
    bad = inference._TemplateJoin(_Fake(2, [3, 2]), _Fake(1, [2 * hop, 2 * hop]), _Fake(1, [tail], []), 2, hop)
    bad.push(x)
    with pytest.raises(ValueError) as ei:
        bad.flush()
    assert "5 frames" in str(ei.value) and "4 frames" in str(ei.value)
