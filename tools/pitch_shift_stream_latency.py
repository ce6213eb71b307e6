#!/usr/bin/env python
"""Time per push of the streaming pitch shift, alone and inside the wav -> wav chain, and its latency in samples.

HiFiGAN-V1 44.1 kHz with synthetic weights, the shifter at the defaults (n_fft 2048, hop 512, n_steps 3 and -4, batch_invariant=True), B rows of
broadband noise --seconds-of-audio long, B in {1, 2}, 8 frames (8 * 512 samples) per push:

* shift          : PitchShift.stream — 4096 samples in, the samples that are final out
* chain          : inference.stream_wav_synthesis(pitch_shift=...) — shift stream -> log-mel stream -> generator stream
* chain, plain   : the same chain without the shift, same model, same build: the difference is what the shift costs per push
* whole rows     : PitchShift.forward on the whole rows, for scale
* N - E          : the most samples received and not yet emitted after any push (fv_pv_stream_pending), in samples and ms

Every time is the p50 over the pushes of one utterance, the median of --repeats utterances after one warm-up; wall-clock around synchronised
calls (a caller that waits for its chunk), not kernel times.

    python tools/pitch_shift_stream_latency.py [--seconds-of-audio 5] [--out profiles/r23_pitch_shift_stream_latency.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from vocoder_amd import inference, synthetic as syn  # noqa: E402
from vocoder_amd.data.transforms import LogMelSpectrogram  # noqa: E402
from vocoder_amd.modules.generators import HiFiGANGenerator  # noqa: E402
from vocoder_amd.pitch_shift import PitchShift  # noqa: E402

SR, HOP, FRAMES = 44100, 512, 8


def build_model() -> inference.InferenceModel:
    cfg = dict(syn.HIFIGAN_V1_44K)
    gen = HiFiGANGenerator(**cfg)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(cfg, 0).items()}, strict=True)
    mel = LogMelSpectrogram(sample_rate=SR, n_fft=2048, win_length=2048, hop_length=HOP, n_mels=cfg["num_mels"], f_min=0, f_max=SR // 2)
    return inference.InferenceModel(gen, SR, cfg["num_mels"], HOP, mel_transform=mel).eval().to("cuda")


def noise(B: int, L: int) -> torch.Tensor:
    rng = np.random.default_rng(B)
    return torch.from_numpy((0.3 * rng.uniform(-1.0, 1.0, (B, L))).astype(np.float32)).cuda()


def pushes(shift: PitchShift, x: torch.Tensor, step: int) -> tuple[float, int]:
    """(p50 seconds per push, the largest N - E after a push) of x (B, n) through shift.stream, `step` columns at a time, each push waited for."""
    lat, pending = [], 0
    with shift.stream(x.shape[0], step) as st:
        for i in range(0, x.shape[1], step):
            t0 = time.perf_counter()
            st.push(x[:, i:i + step])
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
            pending = max(pending, st.pending_samples)
        st.flush()
        torch.cuda.synchronize()
    return float(np.percentile(lat, 50)), pending


def chain(model, wave, shift) -> float:
    step = FRAMES * HOP
    _, st = inference.stream_wav_synthesis(model, (wave[:, i:i + step] for i in range(0, wave.shape[1], step)), wave.shape[1], FRAMES,
                                           sink=lambda y: None, pitch_shift=shift)
    return float(np.percentile(st["push_s"], 50))


def whole(shift, wave) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    shift(wave)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds-of-audio", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r23_pitch_shift_stream_latency.txt"))
    a = ap.parse_args()
    model = build_model()
    L = int(a.seconds_of_audio * SR) // HOP * HOP
    lines = [f"# tools/pitch_shift_stream_latency.py --seconds-of-audio {a.seconds_of_audio}: {torch.cuda.get_device_name(0)}; hifigan-v1-44k, "
             f"shift n_fft 2048 hop {HOP} batch_invariant, {L} samples per row, {FRAMES * HOP} samples per push; p50 ms per push, wall-clock "
             f"around synchronised calls, median of {a.repeats} utterances after one warm-up"]
    for B in (1, 2):
        wave = noise(B, L)
        for n_steps in (3, -4):
            shift = PitchShift(SR, n_steps, batch_invariant=True)
            pending = pushes(shift, wave, FRAMES * HOP)[1]
            cases = (("shift", lambda: pushes(shift, wave, FRAMES * HOP)[0]), ("chain", lambda: chain(model, wave, shift)),
                     ("chain, plain", lambda: chain(model, wave, None)), ("whole rows", lambda: whole(shift, wave)))
            for name, fn in cases:
                fn()
                ms = float(np.median([fn() for _ in range(a.repeats)])) * 1e3
                lines.append(f"B={B:<2d} n_steps={n_steps:<3d} {name:<13} {'per call' if name == 'whole rows' else 'per push p50'} {ms:7.3f} ms")
                print(lines[-1], flush=True)
            lines.append(f"B={B:<2d} n_steps={n_steps:<3d} N - E          at most {pending} samples = {pending / SR * 1e3:.1f} ms after a push")
            print(lines[-1], flush=True)
            shift.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
