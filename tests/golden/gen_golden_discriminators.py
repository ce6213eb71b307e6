#!/usr/bin/env python
"""Generate ``disc_{mpd,mrd}_tiny.npz`` by RUNNING THE REFERENCE's MultiPeriodDiscriminator and MultiResolutionDiscriminator on the CPU with
synthetic weights.

Like gen_golden_hubert.py this runs only where the reference checkout is (``FV_REFERENCE``); the two module files are imported by path and
need only torch.  The fixtures are plain data — config, seed, waves, lengths, the state dict's key names in order, every score and every
feature map, and the three numbers of models/gan.py:149 / 155 / 204 for one equal-length batch of two (real, generated) pairs.  Weights are
not stored: the tests regenerate them with ``vocoder_amd.synthetic.mpd_state_dict`` / ``mrd_state_dict`` (numpy PCG64).  Every row runs
ALONE and unpadded (fp32, one thread): that is what the kernels promise for a row of a ragged batch.  The archives are written with a fixed
time stamp, so two runs give the same bytes.
Usage:  python tests/golden/gen_golden_discriminators.py

The fixtures are the smallest shapes at which the kernels can go wrong:
  disc_mpd_tiny  DiscriminatorP(channels=[1, 12, 36, 68, 100, 132]): no width is a multiple of 32.  Periods 2, 3 and 37; 257 samples give the
                 H chain 129 -> 43 -> 15 -> 5 -> 2 -> 1 at p = 2, 23 < 37 one folded row that is mostly padding, 1 a single position
  disc_mrd_tiny  (32, 6, 20): win < n_fft, 17 bins; (32, 5, 24): n_fft - hop odd, so the two paddings differ.  200 samples give the W chain
                 33 -> 17 -> 9 -> 5 at hop 6; 15 is just above the padding
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from gen_golden_posterior import REFERENCE, write_npz  # noqa: E402
from vocoder_amd import synthetic as syn  # noqa: E402

MPD = dict(periods=[2, 3, 37], channels=[1, 12, 36, 68, 100, 132], seed=31, lengths=[257, 100, 23, 1], pair_length=100)
MRD = dict(resolutions=[[32, 6, 20], [32, 5, 24]], seed=32, lengths=[200, 61, 15], pair_length=61)


def disc_waves(lengths, seed: int) -> np.ndarray:
    """(B, max length) fp32, zero past each row's length; O(1) values from PCG64 (the tests draw theirs the same way)."""
    rng = np.random.default_rng(seed + 1000)
    x = np.zeros((len(lengths), max(lengths)), np.float32)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.standard_normal(n).astype(np.float32)
    return x


def load_reference(name: str):
    spec = importlib.util.spec_from_file_location(f"fv_reference_{name}", os.path.join(REFERENCE, f"fish_vocoder/modules/discriminators/{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gan_numbers(disc, real: torch.Tensor, fake: torch.Tensor) -> np.ndarray:
    """[adv (gan.py:149), fm (gan.py:155), disc (gan.py:204)] as gan.py:142-155 and :197-206 form them, iteration quirks included."""
    score_fakes, feat_fake = disc(fake)
    scores, feat_real = disc(real)
    loss_fake = sum(torch.mean((1 - s) ** 2) for s in score_fakes)
    loss_fm = sum(torch.nn.functional.l1_loss(rl, gl) for dr, dg in zip(feat_real, feat_fake) for rl, gl in zip(dr, dg))
    loss_disc = sum(torch.mean((s - 1) ** 2) + torch.mean(sf ** 2) for s, sf in zip(scores, score_fakes))
    return np.asarray([float(loss_fake), float(loss_fm), float(loss_disc)], np.float64)


def record(name: str, model, sd: dict, fx: dict, config: dict) -> None:
    res = model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(model.state_dict()) == list(sd), f"synthetic.{name}_state_dict must keep the reference's key order"
    model.eval()
    seed, lengths = fx["seed"], fx["lengths"]
    waves = disc_waves(lengths, seed)
    arrays = dict(config=np.frombuffer(json.dumps(config).encode(), dtype=np.uint8), seed=np.int64(seed), waves=waves,
                  lengths=np.asarray(lengths, np.int64), keys=np.frombuffer(json.dumps(list(model.state_dict())).encode(), dtype=np.uint8))
    with torch.no_grad():
        for b, n in enumerate(lengths):
            scores, fmaps = model(torch.from_numpy(waves[b: b + 1, None, :n]))
            if torch.is_tensor(scores):
                arrays[f"score_{b}"] = scores[0].numpy()
            for i, fm in enumerate(fmaps):
                if not torch.is_tensor(scores):
                    arrays[f"score_{b}_{i}"] = scores[i][0].numpy()
                for l, f in enumerate(fm):
                    arrays[f"fmap_{b}_{i}_{l}"] = f[0].numpy()
        pair = disc_waves([fx["pair_length"]] * 4, seed + 1)
        arrays["pair_real"], arrays["pair_fake"] = pair[:2], pair[2:]
        arrays["pair_losses"] = gan_numbers(model, torch.from_numpy(pair[:2, None]), torch.from_numpy(pair[2:, None]))
    path = os.path.join(HERE, f"disc_{name}_tiny.npz")
    write_npz(path, arrays)
    size = os.path.getsize(path)
    assert size <= 1024 * 1024, size
    print(f"wrote disc_{name}_tiny.npz: {len(arrays)} arrays, peak |fmap| "
          f"{max(float(np.abs(v).max()) for k, v in arrays.items() if k.startswith('fmap_')):.3g}, losses {arrays['pair_losses']} [{size / 1024:.1f} KiB]")


def main() -> None:
    torch.set_num_threads(1)             # one summation order, whatever the machine
    mpd = load_reference("mpd")
    model = mpd.MultiPeriodDiscriminator(periods=MPD["periods"])
    model.discriminators = torch.nn.ModuleList(mpd.DiscriminatorP(period=p, channels=MPD["channels"]) for p in MPD["periods"])
    record("mpd", model, syn.mpd_state_dict(MPD["periods"], MPD["channels"], seed=MPD["seed"]), MPD,
           dict(periods=MPD["periods"], channels=MPD["channels"], kernel_size=5, stride=3))
    mrd = load_reference("mrd")
    model = mrd.MultiResolutionDiscriminator(resolutions=MRD["resolutions"])
    record("mrd", model, syn.mrd_state_dict(MRD["resolutions"], seed=MRD["seed"]), MRD, dict(resolutions=MRD["resolutions"]))


if __name__ == "__main__":
    main()
