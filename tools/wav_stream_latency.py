#!/usr/bin/env python
"""Time to first audio and time per push for wav -> wav streaming, against the whole-mel-first path.

HiFiGAN-V1 44.1 kHz with synthetic weights (as bench.py) and B rows of white noise, --seconds-of-audio long, B in {1, 32}, n frames per push:

* chain      : inference.stream_wav_synthesis — log-mel stream -> generator stream, n * hop samples per push; the first audio leaves once the
               generator's lookahead has arrived.
* mel first  : what `--chunk-frames` did on a .wav before the log-mel stream existed — the whole utterance's mel in one forward, then
               inference.stream_synthesis over it; the first audio waits for the whole file's front-end.

Both are run --repeats times after one warm-up run; the median is printed.  Wall-clock times around synchronised calls (a caller that waits
for its audio), not kernel times.

    python tools/wav_stream_latency.py [--seconds-of-audio 10] [--chunk-frames 16] [--out profiles/r14_wav_stream_latency.txt]
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


def build_model() -> inference.InferenceModel:
    cfg = dict(syn.HIFIGAN_V1_44K)
    gen = HiFiGANGenerator(**cfg)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in syn.hifigan_state_dict(cfg, 0).items()}, strict=True)
    mel = LogMelSpectrogram(sample_rate=44100, n_fft=2048, win_length=2048, hop_length=cfg["hop_length"], n_mels=cfg["num_mels"], f_min=0,
                            f_max=22050)
    return inference.InferenceModel(gen, 44100, cfg["num_mels"], cfg["hop_length"], mel_transform=mel).eval().to("cuda")


def chain(model, wave, n):
    step = n * model.hop_length
    _, st = inference.stream_wav_synthesis(model, (wave[:, i:i + step] for i in range(0, wave.shape[1], step)), wave.shape[1], n,
                                           sink=lambda y: None)
    return st["first_audio_s"], float(np.percentile(st["push_s"], 50))


def mel_first(model, wave, n):
    t0 = time.perf_counter()
    mel = model.mel_transform(wave)
    torch.cuda.synchronize()
    t_mel = time.perf_counter() - t0
    _, first, lat = inference.stream_synthesis(model.generator, mel, n)
    return t_mel + first, float(np.percentile(lat, 50))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds-of-audio", type=float, default=10.0)
    ap.add_argument("--chunk-frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r14_wav_stream_latency.txt"))
    a = ap.parse_args()
    model = build_model()
    n, hop = a.chunk_frames, model.hop_length
    L = int(a.seconds_of_audio * 44100) // hop * hop
    lines = [f"# tools/wav_stream_latency.py --seconds-of-audio {a.seconds_of_audio} --chunk-frames {n}: {torch.cuda.get_device_name(0)}; "
             f"hifigan-v1-44k, {L} samples per row, wall-clock ms around synchronised calls, median of {a.repeats} runs after one warm-up"]
    for B in (1, 32):
        wave = 0.2 * torch.randn((B, L), device="cuda", generator=torch.Generator("cuda").manual_seed(B))
        for name, fn in (("chain", chain), ("mel first", mel_first)):
            fn(model, wave, n)
            runs = np.asarray([fn(model, wave, n) for _ in range(a.repeats)])
            first, push = np.median(runs[:, 0]) * 1e3, np.median(runs[:, 1]) * 1e3
            lines.append(f"B={B:<3d} n={n:<3d} {name:<10} first audio after {first:8.2f} ms | per push p50 {push:7.3f} ms")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
