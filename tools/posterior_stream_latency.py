#!/usr/bin/env python
"""Time per push of the posterior encoder stream against what a caller does without it.

PosteriorEncoder at the default config (syn.POSTERIOR_DEFAULT: 513 -> 192 hidden -> 512, k = 5, 16 layers, R = 32) with synthetic weights,
batch in {1, 8, 32} rows of noise, chunk in {1, 8, 32} frames per push:

* stream        : PosteriorEncoder.stream(batch, chunk).push — `chunk` new frames in, `chunk` latent frames out in the steady state; every
                  layer runs over the new columns only (fv_wnstream_push, 2 * 16 + 2 launches)
* window (a)    : PosteriorEncoder.forward on a (chunk + 2 R)-frame window — the exact hand-cut form: 2 R frames recomputed per push
* floor (b)     : PosteriorEncoder.forward on `chunk` frames alone — the same launches with no context at all (not a correct stream)

Every time is the p50 over --pushes steady-state calls after --warmup; wall-clock around synchronised calls (a caller that waits for its
latents), not kernel times.

    python tools/posterior_stream_latency.py [--pushes 200] [--out profiles/r37_posterior_stream_latency.txt]
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

from vocoder_amd import synthetic as syn  # noqa: E402
from vocoder_amd.modules.encoders import PosteriorEncoder  # noqa: E402


def build_module() -> PosteriorEncoder:
    cfg = dict(syn.POSTERIOR_DEFAULT)
    m = PosteriorEncoder(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in syn.posterior_state_dict(cfg, 0).items()}, strict=True)
    return m.eval().cuda()


def p50_ms(fn, warmup: int, n: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    lat = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
    return float(np.percentile(lat, 50)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r37_posterior_stream_latency.txt"))
    a = ap.parse_args()
    m = build_module()
    R = m.reach_frames
    lines = [f"# tools/posterior_stream_latency.py --pushes {a.pushes} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}; PosteriorEncoder "
             f"default config, R = {R}; p50 ms per call over {a.pushes} steady-state calls, wall-clock around synchronised calls",
             f"# {'batch':>5} {'chunk':>5} {'stream':>9} {'window (a)':>11} {'floor (b)':>10}   stream / (a)"]
    print("\n".join(lines), flush=True)
    with torch.no_grad():
        for B in (1, 8, 32):
            for c in (1, 8, 32):
                x = torch.from_numpy(np.random.default_rng(B * 100 + c).standard_normal((B, m.in_channels, c + 2 * R)).astype(np.float32)).cuda()
                chunk = x[:, :, :c].contiguous()
                with m.stream(B, c) as st:
                    for _ in range((R + c - 1) // c + 1):       # past the lookahead: from here every push emits c frames
                        st.push(chunk)
                    t_stream = p50_ms(lambda: st.push(chunk), a.warmup, a.pushes)
                    assert st.push(chunk).shape[2] == c
                t_window = p50_ms(lambda: m(x), a.warmup, a.pushes)
                t_floor = p50_ms(lambda: m(chunk), a.warmup, a.pushes)
                lines.append(f"  {B:>5d} {c:>5d} {t_stream:>9.3f} {t_window:>11.3f} {t_floor:>10.3f}   {t_stream / t_window:.2f}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
