"""GPU: the critics (vocoder_amd/csrc/disc.hip) through the C ABI, ``vocoder_amd.modules.discriminators`` and ``vocoder_amd.scoring.
CriticDistance``.

Values are compared with the reference's goldens (every row run ALONE through the reference on the CPU) and with the float64 restatement
(disc_reference.py) at the project's parity bar, max |d| <= 1e-4 of the expected tensor's own peak; test_disc_host.py shows that float32
arithmetic alone stays a tenth of the bar on these inputs and that a dropped tap, channel quad or a row run at the batch's extent moves a map
by ten bars.  Everything else is bit-exact: a row alone / in a batch / in another order / padded / listed, NaN padding never read, exact
zeros past a row's extents.  Each parity case prints what it measured.  Nothing here reads the reference."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import disc_cases as dc
import disc_reference as dref
from vocoder_amd import _lib
from vocoder_amd.modules.discriminators import DiscriminatorP, DiscriminatorR
from vocoder_amd.scoring import CriticDistance, reference_losses

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = dc.BAR
GUARD = 1024        # floats on either side of a poisoned buffer


@functools.lru_cache(maxsize=None)
def module(kind):
    cfg, seed, _ = dc.golden(kind)
    return dc.module(kind, cfg, dc.state_dict(kind, cfg, seed)).cuda()


@functools.lru_cache(maxsize=1)
def sweep_module(name):
    kind, cfg, _ = dc.SWEEP[name]
    return dc.module(kind, cfg, dc.sweep_state_dict(name)).cuda()


def rows_of(kind):
    _, _, g = dc.golden(kind)
    lengths = [int(n) for n in g["lengths"]]
    return lengths, [torch.from_numpy(g["waves"][b, :n]).cuda() for b, n in enumerate(lengths)]


def padded(waves, T=None, fill=0.0):
    T = max(len(w) for w in waves) if T is None else T
    x = torch.full((len(waves), 1, T), fill, dtype=torch.float32, device="cuda")
    for b, w in enumerate(waves):
        x[b, 0, : len(w)] = w
    return x


def flat(result):
    """Every feature map of a forward's result as one list."""
    return [f for fm in result[1] for f in fm]


class Handle:
    """A finalized fv_disc with the calls the tests make on the C ABI; buffers are poisoned and carry a guard band."""

    def __init__(self, kind, cfg, sd):
        self.L, self.h = _lib.lib(), ctypes.c_void_p()
        c = _lib.DiscConfig()
        if kind == "mpd":
            c.kind, c.n_sub, c.n_channels, c.kernel_size, c.stride = _lib.FV_DISC_PERIOD, len(cfg["periods"]), len(cfg["channels"]), 5, 3
            for i, p in enumerate(cfg["periods"]):
                c.period[i] = p
            for i, ch in enumerate(cfg["channels"]):
                c.channels[i] = ch
        else:
            c.kind, c.n_sub = _lib.FV_DISC_RESOLUTION, len(cfg["resolutions"])
            for i, (n, hop, win) in enumerate(cfg["resolutions"]):
                c.n_fft[i], c.hop_length[i], c.win_length[i] = n, hop, win
        self.n_sub = c.n_sub
        _lib.check(self.L.fv_disc_create(ctypes.byref(c), ctypes.byref(self.h)))
        for k, v in sd.items():
            a = np.ascontiguousarray(v, np.float32)
            _lib.check(self.L.fv_disc_load_weight(self.h, k.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                  (ctypes.c_int64 * max(a.ndim, 1))(*a.shape), a.ndim))
        _lib.check(self.L.fv_disc_finalize(self.h))

    def layout(self, B, T):
        maps = (_lib.DiscMap * (self.n_sub * 6))()
        return int(self.L.fv_disc_layout(self.h, B, T, maps, len(maps), None)), list(maps)

    def forward(self, x, lengths):
        """x: (B, T) device tensor -> (the output buffer, its maps); checks the guard bands of the output and the workspace."""
        B, T = x.shape
        total, maps = self.layout(B, T)
        need = int(self.L.fv_disc_workspace_bytes(self.h, B, T))
        assert total > 0 and total % 4 == 0 and need % 256 == 0
        out = torch.full((total + 2 * GUARD,), float("nan"), device="cuda")
        ws = torch.full((need // 4 + 2 * GUARD,), float("nan"), device="cuda")
        out[:GUARD], out[GUARD + total:], ws[:GUARD], ws[GUARD + need // 4:] = 7.0, 7.0, 7.0, 7.0
        lp = None if lengths is None else (ctypes.c_int32 * B)(*lengths)
        st = self.L.fv_disc_forward(self.h, x.data_ptr(), T, lp, B, out[GUARD:].data_ptr(), total, ws[GUARD:].data_ptr(), need,
                                    int(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        _lib.check(st)
        for buf, n in ((out, total), (ws, need // 4)):
            assert bool((buf[:GUARD] == 7.0).all()) and bool((buf[GUARD + n:] == 7.0).all())
        return out[GUARD: GUARD + total], maps

    def status(self, x, lengths):
        B, T = x.shape
        out, ws = torch.zeros(max(self.layout(B, T)[0], 4), device="cuda"), torch.zeros(1 << 20, device="cuda")
        lp = None if lengths is None else (ctypes.c_int32 * B)(*lengths)
        st = self.L.fv_disc_forward(self.h, x.data_ptr(), T, lp, B, out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel() * 4, None)
        torch.cuda.synchronize()
        return st, self.L.fv_last_error().decode()

    def close(self):
        torch.cuda.synchronize()
        self.L.fv_disc_destroy(self.h)


@pytest.mark.parametrize("kind", dc.KINDS)
def test_goldens_through_the_modules(kind):
    cfg, _, g = dc.golden(kind)
    m = module(kind)
    lengths, waves = rows_of(kind)
    listed = m.forward_list(waves)
    for b, n in enumerate(lengths):
        alone = m(waves[b][None, None])
        scores = alone[0] if kind == "mpd" else [alone[0]]
        if kind == "mpd":
            for i in range(len(cfg["periods"])):
                dc.parity(f"golden disc_mpd row {b} score {i}", scores[i][0].cpu().numpy(), g[f"score_{b}_{i}"])
        else:
            dc.parity(f"golden disc_mrd row {b} scores", alone[0][0].cpu().numpy(), g[f"score_{b}"])
        for i, fm in enumerate(alone[1]):
            assert len(fm) == 6
            for l, f in enumerate(fm):
                want = g[f"fmap_{b}_{i}_{l}"]
                assert f.shape == (1,) + want.shape
                dc.parity(f"golden disc_{kind} row {b} sub {i} layer {l} alone", f[0].cpu().numpy(), want)
                dc.parity(f"golden disc_{kind} row {b} sub {i} layer {l} in the ragged batch", listed[b][1][i][l][0].cpu().numpy(), want)
    # the single discriminators are the same kernels under the list's first prefix
    sd = {k[len("discriminators.0."):]: v for k, v in m.state_dict().items() if k.startswith("discriminators.0.")}
    single = DiscriminatorP(period=cfg["periods"][0], channels=cfg["channels"]) if kind == "mpd" else DiscriminatorR(
        n_fft=cfg["resolutions"][0][0], hop_length=cfg["resolutions"][0][1], win_length=cfg["resolutions"][0][2])
    single.load_state_dict(sd, strict=True)
    score, fmap = single.cuda()(waves[0][None, None])
    assert all(dc.same(a, b) for a, b in zip(fmap, m(waves[0][None, None])[1][0])) and score.shape == (1, fmap[-1].numel())


@pytest.mark.parametrize("kind", dc.KINDS)
def test_goldens_through_the_c_abi_with_poisoned_buffers(kind):
    cfg, seed, g = dc.golden(kind)
    lengths, waves = rows_of(kind)
    h = Handle(kind, cfg, dc.state_dict(kind, cfg, seed))
    try:
        x = padded(waves, fill=float("nan"))[:, 0].contiguous()
        out, maps = h.forward(x, lengths)
        out = out.cpu().numpy()
        for m in maps:          # (up to three floats between two maps round an offset up to 16 bytes; they belong to no map and stay poisoned)
            batch = out[m.offset: m.offset + len(lengths) * m.H * m.W * m.C].reshape(len(lengths), m.H, m.W, m.C)
            for b, n in enumerate(lengths):
                want = g[f"fmap_{b}_{m.sub}_{m.layer}"]
                C, H, W = want.shape
                assert C == m.C and H <= m.H and W <= m.W
                dc.parity(f"golden disc_{kind} row {b} sub {m.sub} layer {m.layer} (C ABI)", batch[b, :H, :W].transpose(2, 0, 1), want)
                rest = batch[b].copy()
                rest[:H, :W] = 0
                assert not dc.bits(rest).any()              # exact zeros past the row's own extent
        alone, amaps = h.forward(waves[1][None].contiguous(), None)
        for m, am in zip(maps, amaps):
            a = alone[am.offset: am.offset + am.H * am.W * am.C].view(am.H, am.W, am.C)
            b = torch.from_numpy(out[m.offset: m.offset + len(lengths) * m.H * m.W * m.C]).view(len(lengths), m.H, m.W, m.C)[1, : am.H, : am.W]
            assert dc.same(a, b)
    finally:
        h.close()


@pytest.mark.parametrize("kind", dc.KINDS)
def test_a_row_has_the_same_bits_alone_batched_reordered_padded_and_listed(kind):
    m = module(kind)
    lengths, waves = rows_of(kind)
    alone = [flat(m(w[None, None])) for w in waves]
    ext = [[hw for sub in m.extents(n) for hw in sub] for n in lengths]
    order = list(reversed(range(len(waves))))
    runs = {
        "batched": (flat(m(padded(waves), lengths=lengths)), list(range(len(waves)))),
        "reordered": (flat(m(padded([waves[b] for b in order]), lengths=[lengths[b] for b in order])), order),
        "padded to a longer T with NaN": (flat(m(padded(waves, T=max(lengths) + 333, fill=float("nan")), lengths=lengths)), list(range(len(waves)))),
    }
    for what, (maps, rows) in runs.items():
        for slot, b in enumerate(rows):
            for j, f in enumerate(maps):
                h, w = ext[b][j]
                assert dc.same(f[slot, :, :h, :w], alone[b][j][0]), (what, b, j)
                rest = f[slot].clone()
                rest[:, :h, :w] = 0
                assert not dc.bits(rest).any(), (what, b, j)
    for b, res in enumerate(m.forward_list(waves)):
        assert all(dc.same(f, a) for f, a in zip(flat(res), alone[b])), b


@pytest.mark.parametrize("name,L", dc.SWEEP_CASES)
def test_shape_sweep_against_the_float64_restatement(name, L):
    kind, cfg, _ = dc.SWEEP[name]
    m = sweep_module(name)
    x = torch.from_numpy(dc.sweep_wave(name, L)).cuda()[None, None]
    scores, fmaps = m(x)
    want = dc.sweep_restated(name, L)
    assert len(fmaps) == 1 and len(fmaps[0]) == 6
    for l, (f, w) in enumerate(zip(fmaps[0], want)):
        dc.parity(f"{name} L = {L} layer {l}", f[0].cpu().numpy(), w)
    score = scores[0] if kind == "mpd" else scores
    dc.parity(f"{name} L = {L} score", score[0].cpu().numpy(), want[-1].reshape(-1))


@pytest.mark.parametrize("kind", dc.KINDS)
def test_critic_distance_on_ragged_pairs(kind):
    cfg, seed, g = dc.golden(kind)
    m = module(kind)
    extra = 57 if kind == "mpd" else 40
    rng = np.random.default_rng(seed + 7)
    reals = [g["pair_real"][0], g["pair_real"][1], rng.standard_normal(extra).astype(np.float32)]
    fakes = [g["pair_fake"][0], g["pair_fake"][1], rng.standard_normal(extra + 3).astype(np.float32)]     # cropped to the shorter
    cd = CriticDistance(**{kind: m})
    res = cd.forward_list([torch.from_numpy(r).cuda() for r in reals], [torch.from_numpy(f).cuda() for f in fakes])
    assert list(res) == [kind]
    sums = res[kind]["sums"].cpu().numpy()
    sd = dc.state_dict(kind, cfg, seed)
    assert sums.shape == (3, len(dc.subs(kind, cfg)), 6, 5) and sums.dtype == np.float64
    for i, sub in enumerate(dc.subs(kind, cfg)):
        layers = dref.folded_layers(sd, i, 5)
        for b in range(3):
            n = min(len(reals[b]), len(fakes[b]))
            want = dref.distance_sums(dc.restate(kind, sub, layers, reals[b][:n]), dc.restate(kind, sub, layers, fakes[b][:n]))
            err = np.abs(sums[b, i] - want) / np.abs(want)
            print(f"disc_{kind} pair {b} sub {i}: sums against the restatement, worst relative {err.max():.2e}")
            assert np.array_equal(sums[b, i, :, 4], want[:, 4]) and err.max() <= BAR
    for b in range(3):          # bit-identical alone or in the batch
        one = cd.forward_list([torch.from_numpy(reals[b]).cuda()], [torch.from_numpy(fakes[b]).cuda()])[kind]
        assert one["sums"].cpu().numpy().tobytes() == sums[b: b + 1].tobytes()
        for key in ("adv_fake", "adv_real", "fm"):
            assert one[key].cpu().numpy().tobytes() == res[kind][key][b: b + 1].cpu().numpy().tobytes()
    fm = (sums[..., 0] / sums[..., 4]).sum((1, 2))
    assert np.allclose(res[kind]["fm"].cpu().numpy(), fm, rtol=1e-12) and res[kind]["adv_fake"].shape == (3,)
    got = reference_losses(sums[:2], kind)
    equal = cd(torch.from_numpy(g["pair_real"]).cuda(), torch.from_numpy(g["pair_fake"]).cuda()).reference_losses(kind)
    for j, name in enumerate(("adv", "fm", "disc")):
        err = abs(got[name] - g["pair_losses"][j]) / abs(g["pair_losses"][j])
        print(f"disc_{kind} {name}: {got[name]:.8g} against the reference's {g['pair_losses'][j]:.8g}, relative {err:.2e}")
        assert err <= BAR and equal[name] == got[name]


def test_forward_refuses_rows_it_cannot_run_by_row_and_minimum():
    cfg, seed, _ = dc.golden("mrd")
    h = Handle("mrd", cfg, dc.state_dict("mrd", cfg, seed))
    try:
        x = torch.zeros((3, 64), device="cuda")
        st, msg = h.status(x, [64, 13, 64])         # (32, 6, 20): reflect padding 13, so 14 samples at least
        assert st == _lib.FV_ERR_INVALID and "host_lengths[1] = 13" in msg and "minimum length 14" in msg and "discriminator 0" in msg
        st, msg = h.status(x, [64, 64, 0])
        assert st == _lib.FV_ERR_INVALID and "host_lengths[2] = 0" in msg and "0 samples" in msg
        st, msg = h.status(x, [64, 65, 64])
        assert st == _lib.FV_ERR_INVALID and "host_lengths[1] = 65" in msg
        st, msg = h.status(x, [64, 14, 64])         # (32, 5, 24): reflect padding 14
        assert st == _lib.FV_ERR_INVALID and "host_lengths[1] = 14" in msg and "minimum length 15" in msg and "discriminator 1" in msg
        st, msg = h.status(x[:, :14].contiguous(), None)
        assert st == _lib.FV_ERR_INVALID and "T = 14" in msg and "minimum length 15" in msg
        st, msg = h.status(x[:, :15].contiguous(), None)
        assert st == 0, msg
    finally:
        h.close()
    m = module("mpd")
    with pytest.raises(_lib.FishVocError, match="0 samples"):
        m(torch.zeros((2, 1, 8), device="cuda"), lengths=[8, 0])
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train()(torch.zeros((1, 1, 8), device="cuda"))
    m.eval()


def test_eval_cli_adds_the_critics_numbers_only_with_the_flag(tmp_path):
    from vocoder_amd import eval as ev
    from vocoder_amd import synthetic as syn
    from vocoder_amd.inference import write_wav
    rng = np.random.default_rng(9)
    src, gen = tmp_path / "src", tmp_path / "gen"
    for name, n in (("a.wav", 3000), ("b.wav", 2500)):
        a = (0.2 * rng.normal(size=(n, 1))).astype(np.float32)
        write_wav(src / name, a, 24000), write_wav(gen / name, a + (0.05 * rng.normal(size=(n, 1))).astype(np.float32), 24000)
    state = {"generator.conv_pre.bias": torch.zeros(4)}
    state.update({"discriminators.mpd." + k: v for k, v in dc.tensors(syn.mpd_state_dict([2], seed=3)).items()})
    state.update({"discriminators.mrd." + k: v for k, v in dc.tensors(syn.mrd_state_dict([(32, 6, 20)], seed=4)).items()})
    torch.save({"state_dict": state}, tmp_path / "gan.ckpt")
    out = tmp_path / "scores.json"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "vocoder_amd.eval", str(src), str(gen), "--no-stft", "--json", str(out),
                        "--critics", str(tmp_path / "gan.ckpt"), "--periods", "2", "--resolutions", "32,6,20"],
                       capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    j = json.loads(out.read_text())
    assert sorted(j["files"]) == ["a.wav", "b.wav"]
    for k in ev.CRITIC_METRICS:
        assert f"    {k}: " in r.stdout and np.isfinite(j["mean"][k]) and j["mean"][k] > 0
        assert abs(j["mean"][k] - np.mean([j["files"][n][k] for n in j["files"]])) <= 1e-12
    plain = tmp_path / "plain.json"
    assert ev.main([str(src), str(gen), "--no-stft", "--json", str(plain)]) == 0
    p = json.loads(plain.read_text())
    assert set(p["mean"]) == {"spec_diff"} and all(set(v) == {"spec_diff"} for v in p["files"].values())
    assert all(p["files"][n]["spec_diff"] == j["files"][n]["spec_diff"] for n in p["files"])
