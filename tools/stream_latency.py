#!/usr/bin/env python
"""Steady-state latency of a streaming push (Engine.stream) against a plain forward over the same window.

HiFiGAN-V1 44.1 kHz with synthetic weights and mel (as bench.py), B in {1, 32} x n in {4, 8, 16, 32, 86} frames per push, and Firefly-base at
B = 1, n = 16; K = A = the reach (exact mode).  Per configuration: warm-up pushes until the window length has settled (W = K + A + n) and the
captured graph replays, then pushes for >= --seconds, each bracketed by hipEvents on the launch stream and synchronised (a caller that waits
for its audio); p50 / p90 of those.  Next to it the p50 of Engine.forward on a clip of W frames, measured the same way.

    python tools/stream_latency.py [--seconds 2] [--out profiles/r07_stream_latency.txt]
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

from vocoder_amd import _lib, synthetic as syn  # noqa: E402
from vocoder_amd.engine import Engine, convnext_config, upsampler_config  # noqa: E402


def _timed(fn, seconds: float, warmup: int) -> np.ndarray:
    """ms per call by hipEvents on the current stream, one synchronised call at a time, for >= `seconds` after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(ms) < 20:
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.asarray(ms)


def measure(name, eng, B, n, seconds):
    R = eng.reach_frames
    W = 2 * R + n
    chunk = torch.from_numpy(syn.synthetic_mel(B, eng.in_channels, n, seed=n)).cuda()
    clip = torch.from_numpy(syn.synthetic_mel(B, eng.in_channels, W, seed=W)).cuda()
    with eng.stream(B, n) as st:
        # -(-2R // n) + 2 pushes reach the steady window; two more in a row capture and replay its graph
        push = _timed(lambda: st.push(chunk), seconds, warmup=-(-2 * R // n) + 6)
        assert st.pending_frames == R
    out = torch.empty((B, eng.out_channels, eng.output_length(W)), dtype=torch.float32, device="cuda")
    fwd = _timed(lambda: eng.forward(clip, out), seconds, warmup=5)
    p50, p90, f50 = np.percentile(push, 50), np.percentile(push, 90), np.percentile(fwd, 50)
    return (f"{name:<22} B={B:<3d} n={n:<3d} W={W:<4d} push p50 {p50:7.3f} ms  p90 {p90:7.3f} ms  ({len(push):5d} pushes) | "
            f"fv_forward(W) p50 {f50:7.3f} ms | gap {p50 - f50:+.3f} ms | {(2 * R + n) / n:5.2f}x frames computed per frame emitted")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r07_stream_latency.txt"))
    a = ap.parse_args()
    lines = [f"# tools/stream_latency.py --seconds {a.seconds}: {torch.cuda.get_device_name(0)}; ms per call by hipEvents, one synchronised call at a "
             "time, after warm-up (graph replay engaged); K = A = reach"]
    cfg = dict(syn.HIFIGAN_V1_44K)
    eng = Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**cfg), state_dict=syn.hifigan_state_dict(cfg, 0))
    lines.append(f"# hifigan-v1-44k: reach R = {eng.reach_frames} frames, hop 512")
    for B in (1, 32):
        for n in (4, 8, 16, 32, 86):
            lines.append(measure("hifigan-v1-44k", eng, B, n, a.seconds))
            print(lines[-1], flush=True)
    eng.close()
    cfg = dict(syn.FIREFLY_BASE_44K)
    eng = Engine(_lib.FV_MODEL_FIREFLY, backbone=convnext_config(**cfg["backbone"]), ups=upsampler_config(**cfg["head"]),
                 state_dict=syn.firefly_state_dict(cfg, 0))
    lines.append(f"# firefly-gan-base-44k: reach R = {eng.reach_frames} frames, hop 512")
    lines.append(measure("firefly-gan-base-44k", eng, 1, 16, a.seconds))
    print(lines[-1], flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
