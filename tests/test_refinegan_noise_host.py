"""Host (no GPU): RefineGAN's seeded AdaIN noise (include/fishvoc.h fv_refinegan_set_noise_seed) — the rule in numpy
(vocoder_amd/refinegan_noise.py): Philox4x32-10 against Random123's known answers, the statistics of the Box-Muller samples, that a sample is a
function of its absolute position alone, the reach walk against the CPU oracle, the ABI surface and the command line."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from vocoder_amd import _lib, refinegan_noise as rn, synthetic as syn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_API = ["fv_refinegan_set_noise_seed", "fv_refinegan_clear_noise_seed", "fv_forward_refinegan_seeded", "fv_refinegan_fill_noise"]
TINY2 = dict(start_channels=4, num_mels=8, hop_length=4, downsample_rates=(2, 2), upsample_rates=(2, 2), leaky_relu_slope=0.2)
ODD = dict(TINY2, hop_length=12, downsample_rates=(4, 3), upsample_rates=(3, 4))
TRIPLES = [(1234, 0, 0), (1234, 5, 7), (2 ** 40 + 3, 23, 100)]      # (seed, layer, row)


def test_philox_known_answers():
    """The three known-answer vectors of Random123's philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{int(w):08x}" for w in rn.philox4x32_10(ctr, key)) == want


@pytest.mark.parametrize("seed,layer,row", TRIPLES)
def test_samples_are_standard_normal(seed, layer, row):
    """Mean, variance, kurtosis and lag-1 product of 2^20 samples, each standardised by its own sampling error: a 4 sigma cap; and no sample
    beyond sqrt(48 ln 2), the largest radius 24 bits of u1 can give."""
    N = 1 << 20
    z = rn.normal(seed, row, layer, 0, 1, 0, N).astype(np.float64)
    var = z.var()
    stats = dict(mean=z.mean() * np.sqrt(N), var=(var - 1.0) * np.sqrt(N / 2), kurtosis=((z ** 4).mean() / var ** 2 - 3.0) * np.sqrt(N / 24),
                 lag1=(z[1:] * z[:-1]).mean() * np.sqrt(N))
    print(seed, layer, row, stats, "max|z| =", np.abs(z).max())
    for name, v in stats.items():
        assert abs(v) <= 4.0, (name, v)
    assert np.abs(z).max() < np.sqrt(48 * np.log(2))


def test_a_sample_depends_on_its_absolute_position_alone():
    whole = rn.normal(1234, 3, 2, 1, 8, 0, 4096)
    assert np.array_equal(rn.normal(1234, 3, 2, 1, 8, 1001, 50), whole[1001:1051])
    seqs = [rn.normal(s, r, l, 1, 8, 0, 256) for s in (1234, 1235) for r in (3, 4) for l in (2, 3)]
    for i in range(len(seqs)):
        for j in range(i):
            assert not np.array_equal(seqs[i], seqs[j]), (i, j)
    assert not np.array_equal(rn.normal(1234, 3, 2, 1, 8, 0, 256), rn.normal(1234, 3, 2, 2, 8, 0, 256))      # channels too


@pytest.mark.parametrize("cfg", [TINY2, ODD], ids=["tiny2", "odd"])
def test_reach_covers_the_oracle_and_a_quarter_of_it_does_not(cfg):
    """refinegan_reach on the CPU oracle: with mel and template replaced by other random data at every frame further than R from the middle
    frame, the middle frame's samples stay within 2e-5 of the output's peak (the project's window bound); replaced from R / 4 on they do not —
    the test can see a reach that is too short."""
    R = rn.refinegan_reach(cfg)
    hop, T = cfg["hop_length"], 2 * R + 9
    mid = T // 2
    sd = syn.refinegan_state_dict(cfg, seed=3)
    mel = syn.synthetic_mel(1, cfg["num_mels"], T, seed=5)
    tmpl = syn.synthetic_template(1, T, hop, seed=6)
    noise = rn.noise_for_forward(cfg, 99, 0, 1, T)
    ref = orc.refinegan_forward(sd, cfg, mel, tmpl, noise)
    peak = float(np.abs(ref).max())
    mel2 = syn.synthetic_mel(1, cfg["num_mels"], T, seed=15)
    tmpl2 = syn.synthetic_template(1, T, hop, seed=16)

    def middle_error(keep: int) -> float:
        far = np.abs(np.arange(T) - mid) > keep
        m = np.where(far[None, None, :], mel2, mel)
        t = np.where(np.repeat(far, hop)[None, None, :], tmpl2, tmpl)
        y = orc.refinegan_forward(sd, cfg, m, t, noise)
        return float(np.abs(y[..., mid * hop:(mid + 1) * hop] - ref[..., mid * hop:(mid + 1) * hop]).max())
    e_full, e_quarter = middle_error(R), middle_error(R // 4)
    print(f"R = {R}: |d| / peak = {e_full / peak:.3e} beyond R, {e_quarter / peak:.3e} beyond R / 4")
    assert e_full <= 2e-5 * peak, (e_full, peak)
    assert e_quarter > 2e-5 * peak, (e_quarter, peak)


def test_default_config_reach_is_near_eighty_frames():
    assert 70 <= rn.refinegan_reach(syn.REFINEGAN_44K) <= 90


def test_noise_for_forward_has_the_explicit_layout():
    got = rn.noise_for_forward(ODD, 7, 3, 2, 5, origin_frame=7)
    assert [a.shape for a in got] == [(2, c, t) for c, t in syn.refinegan_stage_shapes(ODD, 5) for _ in range(6)]
    C, spf = rn.layers(ODD)[7]
    assert np.array_equal(got[7][1, 2], rn.normal(7, 4, 7, 2, C, 7 * spf, 5 * spf))


def test_abi_exports_and_header_declare_the_noise_entries():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    for name in NOISE_API:
        assert name in _lib.EXPORTS, name
        assert name in declared, name
    assert {n for n in _lib.EXPORTS if "noise" in n or "seeded" in n} == set(NOISE_API) | {"fv_refinegan_noise_elems"}


@pytest.fixture(scope="module")
def tiny_refinegan(tmp_path_factory):
    import torch
    import yaml
    root = tmp_path_factory.mktemp("tiny_refinegan")
    (root / "cfg" / "model" / "resolution").mkdir(parents=True)
    (root / "cfg" / "model" / "generator").mkdir(parents=True)
    (root / "cfg" / "model" / "resolution" / "tiny.yaml").write_text(
        yaml.safe_dump(dict(sampling_rate=16000, n_fft=16, hop_length=4, win_length=16, num_mels=8)))
    gen = dict(TINY2, sampling_rate=16000, downsample_rates=[2, 2], upsample_rates=[2, 2])
    (root / "cfg" / "model" / "generator" / "refinegan.yaml").write_text(
        yaml.safe_dump(dict(gen, _target_="vocoder_amd.modules.generators.refinegan.RefineGANGenerator")))
    sd = syn.refinegan_state_dict(TINY2, 5)
    torch.save({"state_dict": {f"generator.{k}": torch.from_numpy(v) for k, v in sd.items()}}, root / "g.ckpt")
    torch.save(torch.zeros(8, 12), root / "m.pt")
    return root, ["--generator", "refinegan", "--resolution", "tiny", "--config-root", str(root / "cfg"), "--ckpt-path", str(root / "g.ckpt")]


def test_cli_takes_a_noise_seed_and_still_refuses_chunks_for_a_template_generator(tiny_refinegan):
    from vocoder_amd import inference
    root, base = tiny_refinegan
    io = ["--input-path", str(root / "m.pt"), "--output-path", str(root / "o")]
    with pytest.raises(ValueError, match="no streaming form yet"):
        inference.main(base + io + ["--noise-seed", "7", "--chunk-frames", "8"])
    assert not (root / "o").exists()
    with pytest.raises(SystemExit):
        inference.main(base + io + ["--noise-seed", "-1"])
    with pytest.raises(SystemExit):
        inference.main(base + io + ["--noise-seed", "seven"])
