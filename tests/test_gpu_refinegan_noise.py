"""GPU: RefineGAN's seeded AdaIN noise (include/fishvoc.h fv_refinegan_set_noise_seed): the samples against the numpy rule
(vocoder_amd/refinegan_noise.py), the seeded forward against the explicit-noise forward bit for bit and against the CPU oracle, rows and
determinism, time tiles and the stream against the whole forward, and what stays refused."""

import numpy as np
import pytest

from conftest import load_golden
from oracle import oracle as orc
from vocoder_amd import refinegan_noise as rn, streaming, synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# TINY2: two stages at power-of-two rates.  ODD: 3 samples per frame in the first up stage, so an odd origin_frame puts a window's origin off
# the quad grid and T * 3 off a multiple of 4 (partial head and tail quads), at a rate that is no power of two.
TINY2 = dict(start_channels=4, num_mels=8, hop_length=4, downsample_rates=(2, 2), upsample_rates=(2, 2), leaky_relu_slope=0.2)
ODD = dict(TINY2, hop_length=12, downsample_rates=(4, 3), upsample_rates=(3, 4))
CFGS = {"tiny2": TINY2, "odd": ODD}
WINDOW_TOL = 2e-5      # of the output's peak: the project's bound for a window against the whole clip


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _engine(cfg, sd=None, seed=None, first_row=0):
    from vocoder_amd import _lib
    from vocoder_amd.engine import Engine, refinegan_config
    eng = Engine(_lib.FV_MODEL_REFINEGAN, refine=refinegan_config(**cfg), state_dict=sd if sd is not None else syn.refinegan_state_dict(cfg, 3))
    if seed is not None:
        eng.set_noise_seed(seed, first_row)
    return eng


def _inputs(cfg, B, T, seed=5):
    mel = syn.synthetic_mel(B, cfg["num_mels"], T, seed=seed)
    tmpl = syn.synthetic_template(B, T, cfg["hop_length"], seed=seed + 1)
    return mel, tmpl, torch.from_numpy(mel).to(_dev()), torch.from_numpy(tmpl).to(_dev())


def _flat(noise):
    return np.concatenate([n.reshape(-1) for n in noise])


@pytest.mark.parametrize("name,B,T,origin,first_row", [("tiny2", 2, 3, 0, 0), ("odd", 2, 5, 7, 3)])
def test_fill_noise_against_the_numpy_rule(name, B, T, origin, first_row):
    """|d| <= 16 * 2^-24 * max(1, rad) per sample, rad = sqrt(-2 ln u1) from the reference: OpenCL's ulp bounds for log (3), sqrt (3) and
    sincospi (4) propagated through sqrt(-2 ln u) cos(.) and doubled; at most 5.5e-6."""
    cfg, seed = CFGS[name], 2 ** 40 + 3
    eng = _engine(cfg, seed=seed, first_row=first_row)
    got = eng.fill_noise(B, T, origin).cpu().numpy()
    ref = _flat(rn.noise_for_forward(cfg, seed, first_row, B, T, origin))
    rad = _flat(rn.noise_for_forward(cfg, seed, first_row, B, T, origin, fn=rn.radius))
    assert got.shape == ref.shape == (eng.noise_elems(B, T),)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bound = 16 * 2.0 ** -24 * np.maximum(1.0, rad)
    print(f"{name}: max|d| = {err.max():.3e}, max |d| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (err.max(), (err / bound).max())
    eng.close()


def _golden_tiny():
    g = load_golden("refinegan_tiny.npz")
    return g["cfg"], syn.refinegan_state_dict(g["cfg"], g["seed"]), g["mel"], g["template"]


@pytest.mark.parametrize("replay", [True, False], ids=["replay", "eager"])
@pytest.mark.parametrize("origin", [0, 7])
@pytest.mark.parametrize("name", ["tiny2", "odd", "golden_tiny"])
def test_seeded_forward_equals_the_explicit_forward_fed_fill_noise(name, origin, replay):
    """The in-kernel draws are the draws fv_refinegan_fill_noise writes: both forwards agree bit for bit, eagerly and replayed from a captured
    graph (three calls with the same buffers: the third replays)."""
    if name == "golden_tiny":
        cfg, sd, mel, tmpl = _golden_tiny()
        B, T = mel.shape[0], mel.shape[2]
        x, t = torch.from_numpy(mel).to(_dev()), torch.from_numpy(tmpl).to(_dev())
    else:
        cfg, sd, B, T = CFGS[name], None, 2, 5
        _, _, x, t = _inputs(cfg, B, T)
    eng = _engine(cfg, sd, seed=1234, first_row=1)
    eng.set_graph_replay(replay)
    noise = eng.fill_noise(B, T, origin)
    L = eng.output_length(T)
    y_seeded = torch.empty((B, 1, L), dtype=torch.float32, device=_dev())
    y_explicit = torch.empty_like(y_seeded)
    seeded_calls, explicit_calls = [], []
    for calls, run in ((seeded_calls, lambda: eng.forward(x, y_seeded, t, origin_frame=origin)), (explicit_calls, lambda: eng.forward(x, y_explicit, t, noise))):
        for _ in range(3):      # the same call three times in a row: the second is captured, the third replays
            y_seeded.fill_(float("nan"))
            y_explicit.fill_(float("nan"))
            calls.append(run().clone())
    torch.cuda.synchronize()
    for call in range(3):
        assert bool(torch.isfinite(seeded_calls[call]).all())
        assert torch.equal(seeded_calls[call], explicit_calls[call]), (call, float((seeded_calls[call] - explicit_calls[call]).abs().max()))
        assert torch.equal(seeded_calls[call], seeded_calls[0]), call
    # the same buffers at another origin: other noise, not the captured graph's (its key holds the origin)
    moved = eng.forward(x, y_seeded, t, origin_frame=origin + 1).clone()
    assert not torch.equal(moved, seeded_calls[0])
    assert torch.equal(moved, eng.forward(x, None, t, origin_frame=origin + 1))
    eng.close()


@pytest.mark.parametrize("origin", [0, 7])
@pytest.mark.parametrize("name", ["tiny2", "odd"])
def test_seeded_forward_against_the_oracle(name, origin):
    """<= 1e-4 of the expected waveform's peak (the parity bar of test_refinegan_golden), the oracle fed the numpy rule's draws."""
    cfg, B, T, seed, first_row = CFGS[name], 2, 6, 77, 3
    mel, tmpl, x, t = _inputs(cfg, B, T)
    sd = syn.refinegan_state_dict(cfg, 3)
    ref = orc.refinegan_forward(sd, cfg, mel, tmpl, rn.noise_for_forward(cfg, seed, first_row, B, T, origin))
    eng = _engine(cfg, sd, seed=seed, first_row=first_row)
    y = eng.forward(x, None, t, origin_frame=origin).cpu().numpy()
    err, peak = float(np.abs(y - ref).max()), float(np.abs(ref).max())
    print(f"{name} origin {origin}: max|d| = {err:.3e}, peak {peak:.3f}")
    assert err <= 1e-4 * peak, (err, peak)
    eng.close()


def test_determinism_and_rows():
    """The same seed gives the same bits, another seed other audio; clip b of a batch run alone under first_row = b is row b — bit for bit under
    set_batch_invariant, within 2e-5 of the peak without it."""
    cfg, B, T = TINY2, 3, 9
    _, _, x, t = _inputs(cfg, B, T)
    eng = _engine(cfg, seed=5)
    y = eng.forward(x, None, t).clone()
    assert torch.equal(eng.forward(x, None, t), y)
    eng.set_noise_seed(6)
    assert not torch.equal(eng.forward(x, None, t), y)
    peak = float(y.abs().max())
    for invariant in (True, False):
        eng.set_batch_invariant(invariant)
        eng.set_noise_seed(5, 0)
        whole = eng.forward(x, None, t).clone()
        for b in range(B):
            eng.set_noise_seed(5, b)
            alone = eng.forward(x[b:b + 1].contiguous(), None, t[b:b + 1].contiguous())
            if invariant:
                assert torch.equal(alone[0], whole[b]), b
            else:
                err = float((alone[0] - whole[b]).abs().max())
                assert err <= WINDOW_TOL * peak, (b, err, peak)
    eng.close()


@pytest.mark.parametrize("name", ["tiny2", "odd"])
def test_time_tiles_draw_the_whole_clips_noise(name, monkeypatch):
    """FV_TILE_FRAMES = 4 R + 8 (read at fv_create: the tiled engine is a second engine with the same weights) splits a clip of 7 R + 21 frames into
    three tiles, the last one pulled back by a distance that is no multiple of the stride; B = 2.  Against the clip run whole: <= 2e-5 of the
    peak.  ODD's interpolation weights come from a local index in fp32 at a rate that is no power of two, so a tile may see weights that differ
    from the whole clip's in their last bits: still inside the window bound as measured (see profiles/LOG.md)."""
    cfg = CFGS[name]
    R = rn.refinegan_reach(cfg)
    L, stride, T, B = 4 * R + 8, 2 * R + 8, 7 * R + 21, 2
    assert 2 * stride < T - 2 * R <= 3 * stride and T - L < 2 * stride and (T - L) % stride != 0      # 3 tiles, the last pulled back
    _, _, x, t = _inputs(cfg, B, T)
    whole_eng = _engine(cfg, seed=31, first_row=2)
    assert whole_eng.reach_frames == R
    monkeypatch.setenv("FV_TILE_FRAMES", str(L))
    tiled_eng = _engine(cfg, seed=31, first_row=2)
    monkeypatch.delenv("FV_TILE_FRAMES")
    assert tiled_eng.workspace_bytes(B, T) != whole_eng.workspace_bytes(B, T)      # the tile plan is in force
    whole = whole_eng.forward(x, None, t)
    tiled = tiled_eng.forward(x, None, t)
    err, peak = float((tiled - whole).abs().max()), float(whole.abs().max())
    print(f"{name}: R = {R}, T = {T}: tiles vs whole max|d| = {err:.3e} = {err / peak:.3e} of the peak {peak:.3f}")
    assert err <= WINDOW_TOL * peak, (err, peak)
    # explicit noise has no tiled form: refused by name on the seeded engine at this length
    from vocoder_amd import _lib
    from vocoder_amd._lib import FishVocError
    with pytest.raises(FishVocError, match="RefineGAN") as ei:
        tiled_eng.forward(x, None, t, torch.zeros(tiled_eng.noise_elems(B, T), device=_dev()))
    assert ei.value.status == _lib.FV_ERR_UNSUPPORTED
    whole_eng.close()
    tiled_eng.close()


def test_stream_against_the_whole_forward_and_its_own_windows():
    """An utterance of 2 R + 37 frames pushed 1, 8, 3, 8, 8, ... frames at a time, mel and template chunk by chunk as a TemplateStream hands them
    over: the emitted frame counts are the rule's, every push is bit for bit the forward of its own window at origin_frame = w, and the
    concatenation is within 2e-5 of the peak of the whole seeded forward."""
    cfg, B = TINY2, 2
    hop = cfg["hop_length"]
    eng = _engine(cfg, seed=42, first_row=1)
    R = eng.reach_frames
    assert R == rn.refinegan_reach(cfg)
    T = 2 * R + 37
    _, _, x, t = _inputs(cfg, B, T)
    whole = eng.forward(x, None, t).clone()
    chunks, f = [], 0
    for n in [1, 8, 3] + [8] * T:
        n = min(n, T - f)
        if n == 0:
            break
        chunks.append(n)
        f += n
    sched = streaming.schedule(chunks, R, R)
    outs, F = [], 0
    with eng.stream(B, 8) as st:
        for i, n in enumerate(chunks + [0]):
            flush = i == len(chunks)
            y = st.flush() if flush else st.push(x[:, :, F:F + n].contiguous(), t[:, :, F * hop:(F + n) * hop].contiguous())
            F += n
            w, E, E2 = sched[i]
            assert y.shape == (B, 1, (E2 - E) * hop), (i, y.shape, E, E2)
            if E2 > E:
                own = eng.forward(x[:, :, w:F].contiguous(), None, t[:, :, w * hop:F * hop].contiguous(), origin_frame=w)
                assert torch.equal(y, own[:, :, (E - w) * hop:(E2 - w) * hop]), i
            outs.append(y)
        assert st.emitted_frames == T
    got = torch.cat(outs, dim=-1)
    err, peak = float((got - whole).abs().max()), float(whole.abs().max())
    print(f"stream vs whole: max|d| = {err:.3e} = {err / peak:.3e} of the peak")
    assert got.shape == whole.shape and err <= WINDOW_TOL * peak, (err, peak)
    eng.close()


def test_refusals():
    from vocoder_amd import _lib
    from vocoder_amd._lib import FishVocError
    cfg, B = TINY2, 2
    hop = cfg["hop_length"]
    eng = _engine(cfg)
    _, _, x, t = _inputs(cfg, B, 8)
    # an unseeded engine: the seeded entries are FV_ERR_STATE, and nothing else changed
    out = torch.empty((B, 1, 8 * hop), device=_dev())
    ws = torch.empty(eng.workspace_bytes(B, 8) // 4 + 1, device=_dev())
    st = eng._lib.fv_forward_refinegan_seeded(eng._h, x.data_ptr(), t.data_ptr(), out.data_ptr(), B, 8, 0, ws.data_ptr(), ws.numel() * 4, None)
    assert st == _lib.FV_ERR_STATE
    assert eng._lib.fv_refinegan_fill_noise(eng._h, ws.data_ptr(), B, 8, 0, None) == _lib.FV_ERR_STATE
    assert eng.reach_frames == -1
    with pytest.raises(FishVocError, match="RefineGAN"):
        eng.stream(B, 8)
    with pytest.raises(FishVocError):
        eng.forward(x, None, t)      # template + noise are mandatory without a seed
    # seeded: ragged batches and session pools stay refused, by name
    eng.set_noise_seed(9)
    for make in (lambda: eng.ragged_plan([5, 8]), lambda: eng.session_pool(2, 8)):
        with pytest.raises(FishVocError, match="RefineGAN") as ei:
            make()
        assert ei.value.status == _lib.FV_ERR_UNSUPPORTED and "origin" in str(ei.value)
    # a stream made under a seed refuses its pushes once the seed changed, and nothing moved
    stream = eng.stream(B, 8)
    stream.push(x[:, :, :3].contiguous(), t[:, :, :3 * hop].contiguous())
    eng.set_noise_seed(10)
    with pytest.raises(FishVocError) as ei:
        stream.push(x[:, :, 3:8].contiguous(), t[:, :, 3 * hop:8 * hop].contiguous())
    assert ei.value.status == _lib.FV_ERR_STATE
    assert (stream.received_frames, stream.emitted_frames, stream.pending_frames) == (3, 0, 3)
    with pytest.raises(FishVocError) as ei:
        stream.flush()
    assert ei.value.status == _lib.FV_ERR_STATE and stream.pending_frames == 3
    eng.set_noise_seed(9)
    assert stream.flush().shape == (B, 1, 3 * hop)      # the seed it was made under: it goes on
    stream.close()
    # without a seed again: no stream
    eng.clear_noise_seed()
    with pytest.raises(FishVocError, match="RefineGAN") as ei:
        eng.stream(B, 8)
    assert ei.value.status == _lib.FV_ERR_UNSUPPORTED
    eng.close()


def test_module_streams_once_a_seed_is_set():
    """RefineGANGenerator.set_noise_seed: forward draws no torch.randn (the same bits twice), stream() works, and stream_synthesis joins mel and
    template like a use_template HiFiGAN."""
    from vocoder_amd.inference import stream_synthesis
    from vocoder_amd.modules.generators.refinegan import RefineGANGenerator
    cfg = dict(TINY2, sampling_rate=16000)
    gen = RefineGANGenerator(**cfg).eval()
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.refinegan_state_dict(TINY2, 3).items()})
    gen = gen.to(_dev())
    R = rn.refinegan_reach(TINY2)
    _, _, x, t = _inputs(TINY2, 1, R + 20)
    assert not torch.equal(gen(x, t), gen(x, t))      # torch.randn per call, as before
    gen.set_noise_seed(11)
    y = gen(x, t)
    assert torch.equal(gen(x, t), y)
    streamed = stream_synthesis(gen, x, 8, template=t)[0]
    err, peak = float((streamed - y).abs().max()), float(y.abs().max())
    assert streamed.shape == y.shape and err <= WINDOW_TOL * peak, (err, peak)
    gen.set_noise_seed(None)
    assert not torch.equal(gen(x, t), y)


def test_cli_noise_seed_makes_whole_files_reproducible(tmp_path):
    """python -m vocoder_amd.inference --noise-seed N on a mel with its F0 sidecar: the same seed writes the same file twice, another seed
    another one."""
    import yaml
    from vocoder_amd import inference
    (tmp_path / "cfg" / "model" / "resolution").mkdir(parents=True)
    (tmp_path / "cfg" / "model" / "generator").mkdir(parents=True)
    (tmp_path / "cfg" / "model" / "resolution" / "tiny.yaml").write_text(
        yaml.safe_dump(dict(sampling_rate=16000, n_fft=16, hop_length=4, win_length=16, num_mels=8)))
    gen = dict(TINY2, sampling_rate=16000, downsample_rates=[2, 2], upsample_rates=[2, 2])
    (tmp_path / "cfg" / "model" / "generator" / "refinegan.yaml").write_text(
        yaml.safe_dump(dict(gen, _target_="vocoder_amd.modules.generators.refinegan.RefineGANGenerator")))
    sd = syn.refinegan_state_dict(TINY2, 5)
    torch.save({"state_dict": {f"generator.{k}": torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "g.ckpt")
    T = 50
    torch.save(torch.from_numpy(syn.synthetic_mel(1, 8, T, seed=2)[0]), tmp_path / "m.pt")
    np.save(tmp_path / "m.f0.npy", np.full(T, 220.0, dtype=np.float32))
    base = ["--generator", "refinegan", "--resolution", "tiny", "--config-root", str(tmp_path / "cfg"), "--ckpt-path", str(tmp_path / "g.ckpt"),
            "--input-path", str(tmp_path / "m.pt")]
    outs = []
    for name, seed in (("a", 7), ("b", 7), ("c", 8)):
        inference.main(base + ["--output-path", str(tmp_path / name), "--noise-seed", str(seed)])
        outs.append((tmp_path / name / "m.wav").read_bytes())
    assert len(outs[0]) > 44 + T * 4 and outs[0] == outs[1] and outs[0] != outs[2]
