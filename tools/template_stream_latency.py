#!/usr/bin/env python
"""Time per push of the streaming F0 tracker and pitch template, alone and inside the wav -> wav chain.

HiFiGAN-V1 44.1 kHz with use_template=True and synthetic weights, tracker at the production plan (W 2048, hop 512, 40 - 1100 Hz), B rows of
a harmonic glide --seconds-of-audio long, B in {1, 8}, n in {1, 4, 16} frames (n * 512 samples) per push:

* tracker        : YinF0.stream — n * hop samples in, the frames that are final out
* oscillator     : PitchTemplate.stream — n F0 frames in, their samples out
* template       : TemplateStream — the first into the second, audio in, template samples out
* generator      : inference.stream_synthesis over the whole mel and the whole template: the generator stream's own per-chunk time
* chain          : inference.stream_wav_synthesis(template=...) — log-mel stream + template stream -> join -> generator stream
* chain, silent  : the same generator fed by the chain without the tracker and the oscillator: the join stage is replaced by a template of
                   zeros pushed with every mel chunk, so the difference to `chain` is what the template stream costs per push

Every figure is the p50 over the pushes of one utterance, the median of --repeats utterances after one warm-up; wall-clock around
synchronised calls (a caller that waits for its chunk), not kernel times.

    python tools/template_stream_latency.py [--seconds-of-audio 5] [--out profiles/r22_template_stream_latency.txt]
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

from vocoder_amd import engine, f0 as f0mod, inference, synthetic as syn  # noqa: E402
from vocoder_amd.data.transforms import LogMelSpectrogram  # noqa: E402
from vocoder_amd.modules.generators import HiFiGANGenerator  # noqa: E402

SR, HOP, W = 44100, 512, 2048


def build_model() -> inference.InferenceModel:
    cfg = dict(syn.HIFIGAN_V1_44K, use_template=True)
    gen = HiFiGANGenerator(**cfg)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(cfg, 0).items()}, strict=True)
    mel = LogMelSpectrogram(sample_rate=SR, n_fft=2048, win_length=2048, hop_length=HOP, n_mels=cfg["num_mels"], f_min=0, f_max=SR // 2)
    return inference.InferenceModel(gen, SR, cfg["num_mels"], HOP, mel_transform=mel).eval().to("cuda")


def glide(B: int, L: int) -> torch.Tensor:
    """B rows: five harmonics of a 110 -> 220 Hz glide, each row a little higher than the one before."""
    n = np.arange(L)
    rows = []
    for b in range(B):
        f = 110.0 * (1.0 + 0.05 * b) * 2.0 ** (n / max(L, 1))
        ph = 2.0 * np.pi * np.cumsum(f) / SR
        rows.append(0.3 * sum(np.sin(h * ph) / h for h in range(1, 6)))
    return torch.from_numpy(np.stack(rows).astype(np.float32)).cuda()


def pushes(stream, x: torch.Tensor, step: int) -> float:
    """p50 seconds per push of x (B, n) through `stream`, `step` columns at a time, each push waited for."""
    lat = []
    for i in range(0, x.shape[1], step):
        t0 = time.perf_counter()
        stream.push(x[:, i:i + step])
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
    stream.flush()
    torch.cuda.synchronize()
    return float(np.percentile(lat, 50))


def chain(model, wave, n, template):
    step = n * HOP
    _, st = inference.stream_wav_synthesis(model, (wave[:, i:i + step] for i in range(0, wave.shape[1], step)), wave.shape[1], n,
                                           sink=lambda y: None, template=template)
    return float(np.percentile(st["push_s"], 50))


def chain_silent(model, wave, n):
    """The chain of a generator that takes a template, without making one: every mel chunk goes in with zeros."""
    push = engine.Stream.push

    def with_zeros(self, m, t=None):
        return push(self, m, torch.zeros((m.shape[0], 1, m.shape[-1] * HOP), dtype=torch.float32, device=m.device))
    engine.Stream.push = with_zeros
    try:
        return chain(model, wave, n, None)
    finally:
        engine.Stream.push = push


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds-of-audio", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r22_template_stream_latency.txt"))
    a = ap.parse_args()
    model = build_model()
    L = int(a.seconds_of_audio * SR) // HOP * HOP
    kw = dict(frame_length=W, fmin=40.0, fmax=1100.0)
    lines = [f"# tools/template_stream_latency.py --seconds-of-audio {a.seconds_of_audio}: {torch.cuda.get_device_name(0)}; hifigan-v1-44k "
             f"use_template, tracker W {W} hop {HOP}, {L} samples per row; p50 ms per push, wall-clock around synchronised calls, median of "
             f"{a.repeats} utterances after one warm-up"]
    for B in (1, 8):
        wave = glide(B, L)
        yin, osc = f0mod.YinF0(SR, HOP, **kw), f0mod.PitchTemplate(SR, HOP)
        f0 = yin(wave)[0]
        mel, template = model.mel_transform(wave), osc(f0)
        for n in (1, 4, 16):
            def tracker():
                with yin.stream(B, n * HOP) as st:
                    return pushes(st, wave, n * HOP)

            def oscillator():
                with osc.stream(B, n) as st:
                    return pushes(st, f0, n)

            def both():
                with f0mod.TemplateStream(SR, HOP, B, n * HOP, **kw) as st:
                    return pushes(st, wave, n * HOP)

            def generator():
                return float(np.percentile(inference.stream_synthesis(model.generator, mel, n, template=template)[2], 50))
            cases = (("tracker", tracker), ("oscillator", oscillator), ("template", both), ("generator", generator),
                     ("chain", lambda: chain(model, wave, n, dict(kw))), ("chain, silent", lambda: chain_silent(model, wave, n)))
            for name, fn in cases:
                fn()
                ms = float(np.median([fn() for _ in range(a.repeats)])) * 1e3
                lines.append(f"B={B:<2d} n={n:<3d} {name:<14} per push p50 {ms:7.3f} ms")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
