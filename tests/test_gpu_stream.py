"""GPU: streaming synthesis (fv_stream_*, vocoder_amd.engine.Stream) — exact mode against the whole utterance and the oracle, window identity
against Engine.forward on the same frames, the reference's own capture, counters, isolation, and refusals by name."""
import random

import numpy as np
import pytest

from conftest import load_golden
from oracle import oracle as orc
from vocoder_amd import synthetic as syn
from vocoder_amd.streaming import schedule

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4
T, B = 389, 2
TINY = dict(hop_length=16, upsample_rates=[4, 2, 2], upsample_kernel_sizes=[8, 4, 4], resblock_kernel_sizes=[3, 7, 11],
            resblock_dilation_sizes=[[1, 3, 5]] * 3, num_mels=20, upsample_initial_channel=64, use_template=False,
            pre_conv_kernel_size=7, post_conv_kernel_size=7)
BB = dict(input_channels=20, depths=[1, 2], dims=[32, 64], drop_path_rate=0.0, kernel_size=7)
HEAD = dict(dim=64, n_fft=64, hop_length=16, win_length=64, padding="same")
MODELS = ["hifigan", "hifigan_template", "bigvgan", "bigvgan_template", "vocos", "firefly", "convnext", "istft_head"]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _case(model):
    """(make engine, mel (B, C_in, T), template or None, oracle output) — the tiny configs of the time-tiling test."""
    from vocoder_amd import _lib
    from vocoder_amd.engine import Engine, convnext_config, istft_head_config, upsampler_config
    tmpl = None
    if model.startswith(("hifigan", "bigvgan")):
        cfg = dict(TINY, use_template=model.endswith("template"))
        big = model.startswith("bigvgan")
        sd = (syn.bigvgan_state_dict if big else syn.hifigan_state_dict)(cfg, seed=6 if big else 5)
        kind = _lib.FV_MODEL_BIGVGAN if big else _lib.FV_MODEL_HIFIGAN
        mk = lambda: Engine(kind, ups=upsampler_config(**cfg), state_dict=sd)   # noqa: E731
        mel = syn.synthetic_mel(B, 20, T, seed=9)
        if cfg["use_template"]:
            tmpl = syn.synthetic_template(B, T, 16, seed=3)
        ref = (orc.bigvgan_forward if big else orc.hifigan_forward)(sd, cfg, mel, template=tmpl)
    elif model == "vocos":
        cfg = dict(backbone=BB, head=HEAD)
        sd = syn.vocos_state_dict(cfg, seed=7)
        mk = lambda: Engine(_lib.FV_MODEL_VOCOS, backbone=convnext_config(**BB), head=istft_head_config(**HEAD), state_dict=sd)   # noqa: E731
        mel = syn.synthetic_mel(B, 20, T, seed=9)
        ref = orc.vocos_forward(sd, cfg, mel)
    elif model == "firefly":
        cfg = dict(backbone=BB, head=dict(TINY, num_mels=64))
        sd = syn.firefly_state_dict(cfg, seed=8)
        mk = lambda: Engine(_lib.FV_MODEL_FIREFLY, backbone=convnext_config(**BB), ups=upsampler_config(**cfg["head"]), state_dict=sd)   # noqa: E731
        mel = syn.synthetic_mel(B, 20, T, seed=9)
        ref = orc.firefly_forward(sd, cfg, mel)
    elif model == "convnext":
        sd = syn.convnext_state_dict(BB, seed=10)
        mk = lambda: Engine(_lib.FV_MODEL_CONVNEXT, backbone=convnext_config(**BB), state_dict=sd)   # noqa: E731
        mel = syn.synthetic_mel(B, 20, T, seed=9)
        ref = orc.convnext_forward(sd, BB, mel)
    else:
        sd = syn.istft_head_state_dict(HEAD, seed=11)
        mk = lambda: Engine(_lib.FV_MODEL_ISTFT_HEAD, head=istft_head_config(**HEAD), state_dict=sd)   # noqa: E731
        mel = np.random.default_rng(12).standard_normal((B, 64, T)).astype(np.float32)
        ref = orc.istft_head_forward(sd, HEAD, mel)[:, None, :]
    return mk, mel, tmpl, ref


def _chunks(kind, total, seed=0, hi=40):
    if kind == "random":
        rng, out = random.Random(seed), []
        while sum(out) < total:
            out.append(min(total - sum(out), rng.randint(1, hi)))
        return out
    n = {"ones": 1, "seven": 7, "sixtyfour": 64}[kind]
    return [n] * (total // n) + ([total % n] if total % n else [])


def _run(stream, x, tt, chunks, hop):
    """Push x (B, C, T) in `chunks`, then flush; returns the list of outputs (the flush's last)."""
    outs, f = [], 0
    for n in chunks:
        outs.append(stream.push(x[:, :, f:f + n], None if tt is None else tt[:, :, f * hop:(f + n) * hop]))
        f += n
    outs.append(stream.flush())
    return outs


@pytest.mark.parametrize("model", MODELS)
def test_exact_mode_matches_the_whole_utterance_and_the_oracle(model):
    mk, mel, tmpl, ref = _case(model)
    dev = _dev()
    eng = mk()
    x = torch.from_numpy(mel).to(dev)
    tt = None if tmpl is None else torch.from_numpy(tmpl).to(dev)
    whole = eng(x, None, tt).cpu().numpy()
    assert whole.shape == ref.shape
    peak = float(np.abs(ref).max())
    tol = min(TOL, TOL * peak) if model in ("vocos", "istft_head") else TOL
    hop = eng.output_length(1)
    R = eng.reach_frames
    assert R > 0
    for kind in ("ones", "seven", "sixtyfour", "random"):
        chunks = _chunks(kind, T, seed=len(model))
        with eng.stream(B, max(chunks)) as st:
            assert (st.context_frames, st.lookahead_frames, st.reach_frames) == (R, R, R)
            y = torch.cat(_run(st, x, tt, chunks, hop), dim=2).cpu().numpy()
        assert y.shape == whole.shape, (kind, y.shape)
        d = float(np.abs(y - whole).max())
        assert d <= 2e-5 * max(1.0, peak), (kind, d)
        assert float(np.abs(y - ref).max()) <= tol, (kind, float(np.abs(y - ref).max()))
    eng.close()


@pytest.mark.parametrize("model,K,A", [("hifigan", None, None), ("hifigan_template", None, None), ("vocos", None, None),
                                       ("hifigan", 3, 5), ("firefly", 0, 2), ("vocos", 10, 0)])
@pytest.mark.parametrize("graph", [True, False])
def test_every_push_is_the_slice_of_a_forward_over_its_window(model, K, A, graph):
    mk, mel, tmpl, _ = _case(model)
    dev = _dev()
    eng = mk()
    eng.set_graph_replay(graph)
    x = torch.from_numpy(mel).to(dev)
    tt = None if tmpl is None else torch.from_numpy(tmpl).to(dev)
    hop = eng.output_length(1)
    chunks = _chunks("random", T, seed=3) + []
    st = eng.stream(B, 40, K, A)
    k, a = st.context_frames, st.lookahead_frames
    outs = _run(st, x, tt, chunks, hop)
    F = 0
    for i, ((w, e0, e1), y) in enumerate(zip(schedule(chunks, k, a), outs)):
        F = F + chunks[i] if i < len(chunks) else F
        assert y.shape == (B, eng.out_channels, (e1 - e0) * hop)
        if e1 > e0:
            ref = eng(x[:, :, w:F], None, None if tt is None else tt[:, :, w * hop:F * hop])
            assert torch.equal(y, ref[:, :, (e0 - w) * hop:(e1 - w) * hop]), (i, w, e0, e1, F)
    st.close()
    eng.close()


def test_the_reference_capture_streamed_alone_and_as_32_lockstep_copies():
    from vocoder_amd import _lib
    from vocoder_amd.engine import Engine, upsampler_config
    g = load_golden("hifigan_v1_t86.npz")
    sd = syn.hifigan_state_dict(g["cfg"], g["seed"])
    eng = Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**g["cfg"]), state_dict=sd)
    assert eng.reach_frames == 17
    dev = _dev()
    for b in (1, 32):
        x = torch.from_numpy(g["mel"]).to(dev).expand(b, -1, -1).contiguous()
        with eng.stream(b, 8) as st:
            y = torch.cat(_run(st, x, None, [8] * 10 + [6], 512), dim=2).cpu().numpy()
        assert y.shape == (b, 1, 86 * 512)
        err = float(np.abs(y - g["out"]).max())
        assert err <= TOL, (b, err)
    eng.close()


def test_counters_reset_and_short_utterances():
    mk, mel, _, _ = _case("hifigan")
    dev = _dev()
    eng = mk()
    x = torch.from_numpy(mel).to(dev)
    hop = eng.output_length(1)
    R = eng.reach_frames
    st = eng.stream(B, 8)
    # nothing comes out while F <= A
    f = 0
    while f + 4 <= R:
        assert st.push(x[:, :, f:f + 4]).shape[2] == 0
        f += 4
        assert st.received_frames == f and st.emitted_frames == 0 and st.pending_frames == f
    chunks = [4] * (f // 4) + [8] * 20
    sched = schedule(chunks, R, R)
    for n, (w, e0, e1) in zip(chunks[f // 4:], sched[f // 4:]):
        y = st.push(x[:, :, f:f + n])
        f += n
        assert y.shape[2] == (e1 - e0) * hop and st.emitted_frames == e1
        assert st.pending_frames == f - e1 <= R
    st.flush()
    assert st.pending_frames == 0 and st.emitted_frames == f
    from vocoder_amd._lib import FishVocError
    with pytest.raises(FishVocError, match="flushed"):
        st.push(x[:, :, :4])
    # reset reuses the stream; an utterance of T <= A frames comes out of the flush alone, bit-identical to the forward
    st.reset()
    assert st.received_frames == st.emitted_frames == st.pending_frames == 0
    short = x[:, :, :R]
    outs = _run(st, short, None, [8] * (R // 8) + ([R % 8] if R % 8 else []), hop)
    assert all(o.shape[2] == 0 for o in outs[:-1])
    assert torch.equal(outs[-1], eng(short))
    st.close()
    eng.close()


def test_interleaved_streams_and_forwards_are_isolated():
    mk, mel, _, _ = _case("hifigan")
    dev = _dev()
    x = torch.from_numpy(mel).to(dev)
    x2 = torch.flip(x, dims=[2]).contiguous()
    hop = 16

    def alone(eng, xx, chunks):
        with eng.stream(B, 16) as st:
            return torch.cat(_run(st, xx, None, chunks, hop), dim=2)

    c1, c2 = _chunks("random", T, seed=5, hi=16), [16] * (T // 16) + [T % 16]
    eng = mk()
    r1, r2 = alone(eng, x, c1), alone(eng, x2, c2)
    s1, s2 = eng.stream(B, 16), eng.stream(B, 16)
    o1, o2, f1, f2 = [], [], 0, 0
    for i in range(max(len(c1), len(c2))):
        if i < len(c1):
            o1.append(s1.push(x[:, :, f1:f1 + c1[i]]))
            f1 += c1[i]
        eng(x[:, :, :50])                                  # a plain forward in between
        if i < len(c2):
            o2.append(s2.push(x2[:, :, f2:f2 + c2[i]]))
            f2 += c2[i]
    o1.append(s1.flush())
    o2.append(s2.flush())
    assert torch.equal(torch.cat(o1, dim=2), r1) and torch.equal(torch.cat(o2, dim=2), r2)
    eng.set_graph_replay(False)
    assert torch.equal(alone(eng, x, c1), r1)
    eng.close()
    with pytest.raises(Exception, match="closed"):
        s1.push(x[:, :, :4])


def test_refusals_name_their_cause():
    from vocoder_amd import _lib
    from vocoder_amd._lib import FishVocError
    from vocoder_amd.engine import Engine, istft_head_config, logmel_config, refinegan_config, upsampler_config
    from vocoder_amd.modules.generators import HiFiGANGenerator
    dev = _dev()
    rcfg = dict(syn.REFINEGAN_44K)
    rg = Engine(_lib.FV_MODEL_REFINEGAN, refine=refinegan_config(**rcfg), state_dict=syn.refinegan_state_dict(rcfg, seed=1))
    with pytest.raises(FishVocError, match="RefineGAN"):
        rg.stream(1, 8)
    assert rg.reach_frames == -1
    rg.close()
    lm = Engine(_lib.FV_MODEL_LOGMEL, mel=logmel_config(sample_rate=24000, n_fft=256, win_length=256, hop_length=64, n_mels=20), state_dict={})
    with pytest.raises(FishVocError, match="log-mel"):
        lm.stream(1, 8)
    lm.close()
    hc = dict(HEAD, padding="center")
    ic = Engine(_lib.FV_MODEL_ISTFT_HEAD, head=istft_head_config(**hc), state_dict=syn.istft_head_state_dict(hc, seed=11))
    with pytest.raises(FishVocError, match="center"):
        ic.stream(1, 8)
    ic.close()
    odd = dict(TINY, upsample_kernel_sizes=[7, 4, 5], resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3, 5]] * 2)
    oe = Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**odd), state_dict=syn.hifigan_state_dict(odd, seed=5))
    with pytest.raises(FishVocError, match="hop x frames"):
        oe.stream(1, 8)
    oe.close()
    mk, mel, tmpl, _ = _case("hifigan_template")
    eng = mk()
    x = torch.from_numpy(mel).to(dev)
    st = eng.stream(B, 8)
    with pytest.raises(FishVocError, match="max_chunk_frames"):
        st.push(x[:, :, :9], torch.from_numpy(tmpl[:, :, :9 * 16]).to(dev))
    with pytest.raises(FishVocError, match="template"):
        st.push(x[:, :, :8])
    assert st.received_frames == 0 and st.pending_frames == 0
    st.close()
    eng.close()
    # a module that reloads its weights rebuilds its engine: its old streams raise a Python error that says what to do
    gen = HiFiGANGenerator(**TINY)
    sd = syn.hifigan_state_dict(TINY, seed=5)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    gen = gen.eval().to(dev)
    s = gen.stream(batch=B, max_chunk_frames=8)
    y0 = s.push(x[:, :, :8])
    assert y0.shape == (B, 1, max(0, 8 - s.lookahead_frames) * 16)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    with pytest.raises(_lib.FishVocError, match="create a new stream"):
        s.push(x[:, :, 8:16])
    with gen.stream(batch=B, max_chunk_frames=8) as s2:
        assert s2.push(x[:, :, :8]).shape[0] == B


def test_cli_chunk_frames_writes_the_whole_utterance_wav(tmp_path, capsys):
    """inference.main --chunk-frames streams each input through the generator's stream: the same 16-bit wav as the whole-utterance run
    (within 1 LSB), and it reports the time to first audio and the per-chunk p50."""
    from vocoder_amd import config, inference
    config.build_generator("hifigan", overrides={"num_mels": 80})
    sd = syn.hifigan_state_dict(dict(syn.HIFIGAN_V1_44K), 3)
    torch.save({"state_dict": {f"generator.{k}": torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "g.ckpt")
    (tmp_path / "in").mkdir()
    torch.save(torch.from_numpy(syn.synthetic_mel(1, 80, 150, seed=4)[0]), tmp_path / "in" / "m.pt")
    args = ["--generator", "hifigan", "--num-mels", "80", "--ckpt-path", str(tmp_path / "g.ckpt"), "--input-path", str(tmp_path / "in")]
    inference.main(args + ["--output-path", str(tmp_path / "whole")])
    inference.main(args + ["--output-path", str(tmp_path / "stream"), "--chunk-frames", "8"])
    assert "first audio after" in capsys.readouterr().out
    whole, _ = inference.read_wav(tmp_path / "whole" / "m.wav")
    streamed, _ = inference.read_wav(tmp_path / "stream" / "m.wav")
    assert whole.shape == streamed.shape == (1, 150 * 512)
    assert np.abs(whole - streamed).max() <= 1.0 / 32768 + 1e-9
