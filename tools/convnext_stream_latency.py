#!/usr/bin/env python
"""Time per push of the ConvNeXt layer stream against the windowed stream and the floor.

Two shapes of the default codec (configs/model/vqvae.yaml, vocos-small-vae) with the untrained initialisation: the encoder (513 -> 512 x 6
blocks, R = 21) and the decoder's backbone (512 -> (512, 1024) x (6, 3), R = 30); batch in {1, 8, 32} rows of noise, chunk in {1, 8, 32}
frames per push:

* layers  : ConvNeXtEncoder.layer_stream(batch, chunk).push — every layer over its new columns only (fv_cnxstream_push)
* window  : ConvNeXtEncoder.stream(batch, chunk).push with K = A = the engine's reach — the backbone over K + A + chunk frames per push
* floor   : ConvNeXtEncoder.forward on `chunk` frames alone — the same layers with no context at all (not a correct stream)

and, for the backbone shape, the whole decode direction: VQVAECodec.decode_stream(batch, chunk, backbone="layers") against
backbone="window" (codes in, audio out: from_codes or the code ring, the backbone, the ISTFT head's stream).

Every time is wall-clock around one synchronised call in the steady state (a caller that waits for its frames), not a kernel time.  The
sides of a line are measured in alternating rounds — layers, window, floor, layers, ... — of --pushes calls each after a warm-up; a cell is
the median of its rounds' p50s and the spread column the widest (max - min) / median among the line's cells.

    python tools/convnext_stream_latency.py [--pushes 60] [--rounds 3] [--out profiles/r41_convnext_stream_latency.txt]
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

from vocoder_amd import codec  # noqa: E402


def p50_ms(fn, n: int) -> float:
    lat = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
    return float(np.percentile(lat, 50)) * 1e3


def measure(sides: dict, warmup: int, pushes: int, rounds: int):
    """sides: name -> callable.  -> (name -> median over rounds of the round's p50 in ms, the widest relative spread)."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            got[k].append(p50_ms(fn, pushes))
    med = {k: float(np.median(v)) for k, v in got.items()}
    return med, max((max(v) - min(v)) / med[k] for k, v in got.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r41_convnext_stream_latency.txt"))
    a = ap.parse_args()
    torch.manual_seed(0)
    model = codec.build_vqvae().eval().cuda()
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [f"# tools/convnext_stream_latency.py --pushes {a.pushes} --warmup {a.warmup} --rounds {a.rounds}: {torch.cuda.get_device_name(0)}; "
             "p50 ms per synchronised call in the steady state, median of alternating rounds; spread = widest (max - min) / median of the line"]
    print(lines[0], flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    with torch.no_grad():
        for what, m in (("encoder 513 -> 512 x 6", model.encoder), ("backbone 512 -> (512, 1024) x (6, 3)", model.decoder.backbone)):
            R, Rw = m.lookahead_frames, m.engine(dev).reach_frames
            emit(f"# {what}: layer stream R = {R}; windowed stream K = A = {Rw}")
            emit(f"# {'batch':>5} {'chunk':>5} {'layers':>9} {'window':>9} {'floor':>9}   window / layers   (n + 2 Rw) / n   spread")
            for B in (1, 8, 32):
                for c in (1, 8, 32):
                    chunk = torch.randn(B, m._cfg["input_channels"], c, device="cuda")
                    with m.layer_stream(B, c) as ls, m.stream(B, c) as ws:
                        for _ in range((Rw + c - 1) // c + 2):       # past both lookaheads: from here every push emits c frames
                            ls.push(chunk), ws.push(chunk)
                        med, spread = measure({"layers": lambda: ls.push(chunk), "window": lambda: ws.push(chunk), "floor": lambda: m(chunk)},
                                              a.warmup, a.pushes, a.rounds)
                        assert ls.push(chunk).shape[2] == c
                    emit(f"  {B:>5d} {c:>5d} {med['layers']:>9.3f} {med['window']:>9.3f} {med['floor']:>9.3f}   {med['window'] / med['layers']:>15.2f}   "
                         f"{(c + 2 * Rw) / c:>14.1f}   {spread:.2f}")
        emit("# decode_stream of the default codec (codes -> audio, hop 2048): backbone=\"layers\" against backbone=\"window\"")
        emit(f"# {'batch':>5} {'chunk':>5} {'layers':>9} {'window':>9}   window / layers   spread")
        for B in (1, 8, 32):
            for c in (1, 8, 32):
                codes = torch.randint(0, 4096, (B, c), device="cuda")
                with model.decode_stream(B, c, backbone="layers") as dl, model.decode_stream(B, c, backbone="window") as dw:
                    for _ in range((dw.lookahead_frames + c - 1) // c + 2):
                        dl.push(codes), dw.push(codes)
                    med, spread = measure({"layers": lambda: dl.push(codes), "window": lambda: dw.push(codes)}, a.warmup, a.pushes, a.rounds)
                    assert dl.push(codes).shape[2] == c * 2048
                emit(f"  {B:>5d} {c:>5d} {med['layers']:>9.3f} {med['window']:>9.3f}   {med['window'] / med['layers']:>15.2f}   {spread:.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
