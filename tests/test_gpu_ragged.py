"""GPU: ragged batches (fv_ragged_*, Engine.forward_ragged) — every clip against itself alone and the oracle, window identity against
Engine.forward on the plan's windows, dead padding, the reference's own capture, the full-size seeded set, isolation, refusals, the CLI."""
import random

import numpy as np
import pytest

from conftest import load_golden
from oracle import oracle as orc
from test_gpu_stream import BB, HEAD, MODELS, TINY
from vocoder_amd import ragged
from vocoder_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(model):
    """(make engine, input channels, oracle(mel (1, C, T), template or None) -> (1, C_out, T * hop), has template) — the tiny configs of the
    stream tests, with their weights."""
    from vocoder_amd import _lib
    from vocoder_amd.engine import Engine, convnext_config, istft_head_config, upsampler_config
    if model.startswith(("hifigan", "bigvgan")):
        cfg = dict(TINY, use_template=model.endswith("template"))
        big = model.startswith("bigvgan")
        sd = (syn.bigvgan_state_dict if big else syn.hifigan_state_dict)(cfg, seed=6 if big else 5)
        kind = _lib.FV_MODEL_BIGVGAN if big else _lib.FV_MODEL_HIFIGAN
        fwd = orc.bigvgan_forward if big else orc.hifigan_forward
        return (lambda: Engine(kind, ups=upsampler_config(**cfg), state_dict=sd)), 20, (lambda m, t: fwd(sd, cfg, m, template=t)), cfg["use_template"]
    if model == "vocos":
        cfg = dict(backbone=BB, head=HEAD)
        sd = syn.vocos_state_dict(cfg, seed=7)
        mk = lambda: Engine(_lib.FV_MODEL_VOCOS, backbone=convnext_config(**BB), head=istft_head_config(**HEAD), state_dict=sd)   # noqa: E731
        return mk, 20, (lambda m, t: orc.vocos_forward(sd, cfg, m).reshape(m.shape[0], 1, -1)), False
    if model == "firefly":
        cfg = dict(backbone=BB, head=dict(TINY, num_mels=64))
        sd = syn.firefly_state_dict(cfg, seed=8)
        mk = lambda: Engine(_lib.FV_MODEL_FIREFLY, backbone=convnext_config(**BB), ups=upsampler_config(**cfg["head"]), state_dict=sd)   # noqa: E731
        return mk, 20, (lambda m, t: orc.firefly_forward(sd, cfg, m)), False
    if model == "convnext":
        sd = syn.convnext_state_dict(BB, seed=10)
        return (lambda: Engine(_lib.FV_MODEL_CONVNEXT, backbone=convnext_config(**BB), state_dict=sd)), 20, (lambda m, t: orc.convnext_forward(sd, BB, m)), False
    sd = syn.istft_head_state_dict(HEAD, seed=11)
    mk = lambda: Engine(_lib.FV_MODEL_ISTFT_HEAD, head=istft_head_config(**HEAD), state_dict=sd)   # noqa: E731
    return mk, 64, (lambda m, t: orc.istft_head_forward(sd, HEAD, m)[:, None, :]), False


def _lengths(R):
    return [1, R, 2 * R, 2 * R + 1, 3 * R, 97, 97, 389, 0, 200]


def _inputs(model, cin, lengths, hop, tmpl):
    T = max(lengths)
    if model == "istft_head":
        mel = np.random.default_rng(12).standard_normal((len(lengths), cin, T)).astype(np.float32)
    else:
        mel = syn.synthetic_mel(len(lengths), cin, T, seed=9)
    tt = syn.synthetic_template(len(lengths), T, hop, seed=3) if tmpl else None
    return mel, tt


@pytest.mark.parametrize("model", MODELS)
def test_each_clip_equals_itself_alone_and_the_oracle(model):
    mk, cin, oracle, tmpl = _model(model)
    dev = _dev()
    eng = mk()
    R, hop = eng.reach_frames, eng.output_length(1)
    assert R > 0
    lengths = _lengths(R)
    mel, tt = _inputs(model, cin, lengths, hop, tmpl)
    x = torch.from_numpy(mel).to(dev)
    t = None if tt is None else torch.from_numpy(tt).to(dev)
    y = eng.forward_ragged(x, lengths, template=t)
    assert y.shape == (len(lengths), eng.out_channels, max(lengths) * hop)
    for b, n in enumerate(lengths):
        assert bool((y[b, :, n * hop:] == 0.0).all()), (b, n)
        if n == 0:
            continue
        alone = eng(x[b:b + 1, :, :n].contiguous(), None, None if t is None else t[b:b + 1, :, :n * hop].contiguous()).cpu().numpy()
        ref = oracle(mel[b:b + 1, :, :n], None if tt is None else tt[b:b + 1, :, :n * hop])
        got = y[b:b + 1, :, :n * hop].cpu().numpy()
        peak = float(np.abs(ref).max())
        d_alone, d_ref = float(np.abs(got - alone).max()), float(np.abs(got - ref).max())
        print(f"{model} clip {b} ({n} frames): vs alone {d_alone:.3e}, vs oracle {d_ref:.3e}, peak {peak:.3e}")
        assert d_alone <= 2e-5 * max(1.0, peak), (b, n, d_alone)
        tol = min(TOL, TOL * peak) if model in ("vocos", "istft_head") else TOL
        assert d_ref <= tol, (b, n, d_ref)
    eng.close()


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("model", MODELS)
def test_every_keep_range_is_the_slice_of_a_forward_over_its_groups_windows(model, graph):
    mk, cin, _, tmpl = _model(model)
    dev = _dev()
    eng = mk()
    eng.set_graph_replay(graph)
    R, hop = eng.reach_frames, eng.output_length(1)
    lengths = _lengths(R)
    mel, tt = _inputs(model, cin, lengths, hop, tmpl)
    x = torch.from_numpy(mel).to(dev)
    t = None if tt is None else torch.from_numpy(tt).to(dev)
    y = eng.forward_ragged(x, lengths, template=t)
    windows = ragged.plan(lengths, R)
    assert eng._ragged_last.windows == windows and eng._ragged_last.groups == ragged.groups(windows)
    for g, (count, n) in enumerate(ragged.groups(windows)):
        ws = [w for w in windows if w.group == g]
        W = torch.zeros((count, cin, n), device=dev)
        WT = torch.zeros((count, 1, n * hop), device=dev) if tmpl else None
        for i, w in enumerate(ws):
            m = min(n, lengths[w.clip] - w.start)
            W[i, :, :m] = x[w.clip, :, w.start:w.start + m]
            if tmpl:
                WT[i, :, :m * hop] = t[w.clip, :, w.start * hop:(w.start + m) * hop]
        ref = eng(W, None, WT)
        for i, w in enumerate(ws):
            assert torch.equal(y[w.clip, :, w.keep_lo * hop:w.keep_hi * hop], ref[i, :, (w.keep_lo - w.start) * hop:(w.keep_hi - w.start) * hop]), (g, w)
    # equal lengths: exactly the plain forward
    xe = x[:4, :, :97].contiguous()
    te = None if t is None else t[:4, :, :97 * hop].contiguous()
    assert torch.equal(eng.forward_ragged(xe, [97] * 4, template=te), eng(xe, None, te))
    eng.close()


@pytest.mark.parametrize("model", ["hifigan_template", "vocos", "firefly"])
def test_padding_is_dead(model):
    mk, cin, _, tmpl = _model(model)
    dev = _dev()
    eng = mk()
    R, hop = eng.reach_frames, eng.output_length(1)
    lengths = _lengths(R)
    mel, tt = _inputs(model, cin, lengths, hop, tmpl)
    outs = []
    for fill in (float("nan"), 1e30, 0.0):
        x = torch.from_numpy(mel).to(dev)
        t = None if tt is None else torch.from_numpy(tt).to(dev)
        for b, n in enumerate(lengths):
            x[b, :, n:] = fill
            if t is not None:
                t[b, :, n * hop:] = fill
        outs.append(eng.forward_ragged(x, lengths, template=t).clone())
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    eng.close()


def _v1_engine(g=None):
    from vocoder_amd import _lib
    from vocoder_amd.engine import Engine, upsampler_config
    cfg = dict(syn.HIFIGAN_V1_44K) if g is None else g["cfg"]
    sd = syn.hifigan_state_dict(cfg, 0 if g is None else g["seed"])
    return Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**cfg), state_dict=sd)


def test_the_reference_capture_as_a_non_longest_and_as_the_longest_clip():
    g = load_golden("hifigan_v1_t86.npz")
    eng = _v1_engine(g)
    assert eng.reach_frames == 17
    dev = _dev()
    for lengths in ([300, 86, 41, 86, 120], [86, 50, 86]):
        mel = syn.synthetic_mel(len(lengths), 80, max(lengths), seed=21)
        for b, n in enumerate(lengths):
            if n == 86:
                mel[b, :, :86] = g["mel"][0]
        if lengths[0] == 300:   # the capture takes the body + tail route
            assert sum(1 for w in ragged.plan(lengths, 17) if w.clip == 1) == 2
        y = eng.forward_ragged(torch.from_numpy(mel).to(dev), lengths).cpu().numpy()
        for b, n in enumerate(lengths):
            if n == 86:
                err = float(np.abs(y[b:b + 1, :, :86 * 512] - g["out"]).max())
                print(f"lengths {lengths} clip {b}: vs the reference capture {err:.3e}")
                assert err <= TOL, (lengths, b, err)
                assert not y[b, :, 86 * 512:].any()
    eng.close()


def test_full_size_seeded_one_to_ten_second_set():
    eng = _v1_engine()
    dev = _dev()
    rng = random.Random(0)
    lengths = [rng.randint(86, 860) for _ in range(32)]
    x = torch.from_numpy(syn.synthetic_mel(32, 80, max(lengths), seed=1)).to(dev)
    plan = eng.ragged_plan(lengths, max(lengths))
    assert plan.groups == ragged.groups(ragged.plan(lengths, 17)) and plan.windows == ragged.plan(lengths, 17)
    y = eng.forward_ragged(x, lengths, plan=plan)
    worst = 0.0
    for b, n in enumerate(lengths):
        alone = eng(x[b:b + 1, :, :n].contiguous())
        peak = float(alone.abs().max())
        d = float((y[b:b + 1, :, :n * 512] - alone).abs().max())
        worst = max(worst, d / max(1.0, peak))
        assert d <= 2e-5 * max(1.0, peak), (b, n, d, peak)
        assert not bool(y[b, :, n * 512:].any())
    print(f"seed-0 set: {len(plan.groups)} forwards, worst |ragged - alone| / max(1, peak) = {worst:.3e}")
    plan.close()
    eng.close()


def test_isolation_graph_replay_guard_bands_and_poisoned_workspace():
    mk, cin, _, _ = _model("hifigan")
    dev = _dev()
    eng = mk()
    R, hop = eng.reach_frames, 16
    lengths = _lengths(R)
    mel, _ = _inputs("hifigan", cin, lengths, hop, False)
    x = torch.from_numpy(mel).to(dev)
    xp = x[:2, :, :120].contiguous()
    outp = torch.empty((2, 1, 120 * hop), device=dev)
    for _ in range(4):                       # eager, capture, replay
        eng(xp, outp)
    torch.cuda.synchronize()
    first = outp.clone()
    n_graphs = eng.graph_replay
    assert n_graphs
    plan = eng.ragged_plan(lengths)
    G = 4096
    n_out = len(lengths) * max(lengths) * hop
    obuf = torch.full((n_out + 2 * G,), 7.25, device=dev)
    out = obuf[G:G + n_out].view(len(lengths), 1, max(lengths) * hop)
    need = (plan.workspace_bytes + 3) // 4
    wbuf = torch.full((need + 2 * G,), -3.5, device=dev)
    plan._ws = wbuf[G:G + need]
    plan._ws.zero_()
    eng.forward_ragged(x, lengths, out=out, plan=plan)
    torch.cuda.synchronize()
    ref = out.clone()
    for _ in range(3):
        eng(xp, outp)                        # plain forward -> ragged -> plain forward
        plan._ws.fill_(float("nan"))
        out.fill_(float("nan"))
        eng.forward_ragged(x, lengths, out=out, plan=plan)
        eng(xp, outp)
        torch.cuda.synchronize()
        assert torch.equal(outp, first)
        assert torch.equal(out, ref) and bool(torch.isfinite(out).all())
    assert eng.graph_replay
    assert bool((obuf[:G] == 7.25).all()) and bool((obuf[G + n_out:] == 7.25).all()), "output guard"
    assert bool((wbuf[:G] == -3.5).all()) and bool((wbuf[G + need:] == -3.5).all()), "workspace guard"
    plan.close()
    eng.close()


def test_refusals_name_their_cause():
    import ctypes

    from vocoder_amd import _lib
    from vocoder_amd._lib import FishVocError
    from vocoder_amd.engine import Engine, istft_head_config, logmel_config, refinegan_config, upsampler_config
    dev = _dev()
    rcfg = dict(syn.REFINEGAN_44K)
    rg = Engine(_lib.FV_MODEL_REFINEGAN, refine=refinegan_config(**rcfg), state_dict=syn.refinegan_state_dict(rcfg, seed=1))
    with pytest.raises(FishVocError, match="RefineGAN"):
        rg.ragged_plan([8, 4])
    rg.close()
    lm = Engine(_lib.FV_MODEL_LOGMEL, mel=logmel_config(sample_rate=24000, n_fft=256, win_length=256, hop_length=64, n_mels=20), state_dict={})
    with pytest.raises(FishVocError, match="log-mel"):
        lm.ragged_plan([8, 4])
    lm.close()
    hc = dict(HEAD, padding="center")
    ic = Engine(_lib.FV_MODEL_ISTFT_HEAD, head=istft_head_config(**hc), state_dict=syn.istft_head_state_dict(hc, seed=11))
    with pytest.raises(FishVocError, match="center"):
        ic.ragged_plan([8, 4])
    ic.close()
    odd = dict(TINY, upsample_kernel_sizes=[7, 4, 5], resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3, 5]] * 2)
    oe = Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**odd), state_dict=syn.hifigan_state_dict(odd, seed=5))
    with pytest.raises(FishVocError, match="hop x frames"):
        oe.ragged_plan([8, 4])
    oe.close()
    mk, cin, _, _ = _model("hifigan_template")
    eng = mk()
    with pytest.raises(FishVocError, match="outside"):
        eng.ragged_plan([8, 40], t_max=30)
    with pytest.raises(FishVocError, match="outside"):
        eng.ragged_plan([8, -1], t_max=30)
    x = torch.from_numpy(syn.synthetic_mel(2, cin, 40, seed=9)).to(dev)
    with pytest.raises(FishVocError, match="needs a template"):
        eng.forward_ragged(x, [8, 40])
    plan = eng.ragged_plan([8, 40])
    tt = torch.zeros((2, 1, 40 * 16), device=dev)
    out = torch.empty((2, 1, 40 * 16), device=dev)
    st = eng._lib.fv_ragged_forward(plan._h, x.data_ptr(), tt.data_ptr(), out.data_ptr(), plan._ws.data_ptr(), plan.workspace_bytes - 256, None)
    assert st == _lib.FV_ERR_INVALID and b"workspace too small" in eng._lib.fv_last_error()
    g = ctypes.c_int32(0)
    assert eng._lib.fv_ragged_group(plan._h, 99, ctypes.byref(g), ctypes.byref(g)) == _lib.FV_ERR_INVALID
    eng.close()
    with pytest.raises(FishVocError, match="closed"):
        eng.forward_ragged(x, [8, 40], template=tt, plan=plan)
    with pytest.raises(FishVocError, match="closed"):
        eng.ragged_plan([8, 40])
    mk2, _, _, _ = _model("hifigan")
    e2 = mk2()
    with pytest.raises(FishVocError, match="use_template=False"):
        e2.forward_ragged(x, [8, 40], template=tt)
    e2.close()


def test_cli_batch_size_writes_the_wavs_of_the_one_by_one_run(tmp_path, capsys):
    from vocoder_amd import config, inference
    config.build_generator("hifigan", overrides={"num_mels": 80})
    sd = syn.hifigan_state_dict(dict(syn.HIFIGAN_V1_44K), 3)
    torch.save({"state_dict": {f"generator.{k}": torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "g.ckpt")
    (tmp_path / "in").mkdir()
    lengths = [150, 20, 34, 86, 61]
    for i, n in enumerate(lengths):
        torch.save(torch.from_numpy(syn.synthetic_mel(1, 80, n, seed=40 + i)[0]), tmp_path / "in" / f"m{i}.pt")
    args = ["--generator", "hifigan", "--num-mels", "80", "--ckpt-path", str(tmp_path / "g.ckpt"), "--input-path", str(tmp_path / "in")]
    inference.main(args + ["--output-path", str(tmp_path / "one")])
    inference.main(args + ["--output-path", str(tmp_path / "batched"), "--batch-size", "4"])
    assert "one ragged forward" in capsys.readouterr().out
    for i, n in enumerate(lengths):
        a, _ = inference.read_wav(tmp_path / "one" / f"m{i}.wav")
        b, _ = inference.read_wav(tmp_path / "batched" / f"m{i}.wav")
        assert a.shape == b.shape == (1, n * 512)
        assert np.abs(a - b).max() <= 1.0 / 32768 + 1e-9
    with pytest.raises(SystemExit):
        inference.main(args + ["--output-path", str(tmp_path / "x"), "--batch-size", "4", "--chunk-frames", "8"])
