#!/usr/bin/env python
"""Throughput of Engine.forward_ragged on batches of utterances of different lengths, against two yardsticks.

HiFiGAN-V1 44.1 kHz with synthetic weights and mel (as bench.py).  Sets: four seeded sets of 32 clips of 1 - 10 s (86 - 860 frames), one of
~1 s clips (60 - 130 frames), and 32 equal 86-frame clips.  Per set, interleaved round by round in ONE process (ms by hipEvents, median):
  ragged : one forward_ragged call over the padded batch (its plan made once, as a server that sees the lengths again would);
  loop   : the same clips one by one through Engine.forward — the only correct alternative without the ragged call;
  floor  : Engine.forward over an equal-length batch with the same number of useful frames (32 clips of sum(lengths) / 32 frames).
Then the plan (forwards, computed / useful frames) and the share of the three ragged launches in the profiled per-kernel table.
Engine.forward is the plain fv_forward path (FV_LIB_PATH selects another build of the library for all three columns).

    python tools/ragged_throughput.py [--rounds 20] [--out profiles/r08_ragged_throughput.txt]
"""
from __future__ import annotations

import argparse
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from vocoder_amd import _lib, ragged, synthetic as syn  # noqa: E402
from vocoder_amd.engine import Engine, upsampler_config  # noqa: E402


def _ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(name, eng, lengths, rounds):
    B, T = len(lengths), max(lengths)
    x = torch.from_numpy(syn.synthetic_mel(B, eng.in_channels, T, seed=T)).cuda()
    clips = [x[b:b + 1, :, :n].contiguous() for b, n in enumerate(lengths)]
    outs = [torch.empty((1, 1, n * 512), device="cuda") for n in lengths]
    mean = max(1, round(sum(lengths) / B))
    xf = torch.from_numpy(syn.synthetic_mel(B, eng.in_channels, mean, seed=mean)).cuda()
    of = torch.empty((B, 1, mean * 512), device="cuda")
    plan = eng.ragged_plan(lengths, T)
    out = torch.empty((B, 1, T * 512), device="cuda")

    def run_ragged():
        eng.forward_ragged(x, lengths, out=out, plan=plan)

    def run_loop():
        for c, o in zip(clips, outs):
            eng.forward(c, o)

    def run_floor():
        eng.forward(xf, of)

    fns = {"ragged": run_ragged, "loop": run_loop, "floor": run_floor}
    for _ in range(4):                      # warm-up of every shape (the plain forwards capture and replay their graphs)
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            ms[k].append(_ms(f))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float(np.percentile(v, 90) - np.percentile(v, 10)) for k, v in ms.items()}
    prof = eng.profile(x, repeats=3, lengths=lengths)
    total = sum(r["total_ms"] for r in prof)
    share = {r["kernel"]: r["total_ms"] / total for r in prof if r["kernel"].startswith("ragged_")}
    useful = sum(lengths)
    comp = sum(b * n for b, n in plan.groups)
    line = (f"{name:<14} B={B} frames {min(lengths)}-{T} useful {useful}: plan {len(plan.groups)} forwards, computed/useful {comp / useful:.3f} "
            f"(padded {B * T / useful:.3f}) | ragged {med['ragged']:.3f} ms (p10-p90 {spread['ragged']:.3f}) | loop {med['loop']:.3f} ms "
            f"(p10-p90 {spread['loop']:.3f}) = {med['loop'] / med['ragged']:.2f}x | floor {med['floor']:.3f} ms = {med['ragged'] / med['floor']:.2f}x floor | "
            + " ".join(f"{k} {100 * v:.2f}%" for k, v in sorted(share.items())))
    plan.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r08_ragged_throughput.txt"))
    a = ap.parse_args()
    cfg = dict(syn.HIFIGAN_V1_44K)
    eng = Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**cfg), state_dict=syn.hifigan_state_dict(cfg, 0))
    lines = [f"# tools/ragged_throughput.py --rounds {a.rounds}: {torch.cuda.get_device_name(0)}; HiFiGAN-V1 44.1 kHz, R = {eng.reach_frames}, "
             f"launch_frames = {ragged.LAUNCH_FRAMES}, max_groups = {ragged.MAX_GROUPS}; median ms per call by hipEvents, the three columns "
             "interleaved round by round; share = of the profiled (serialised) kernel time of one ragged call"]
    sets = []
    for s in range(4):
        rng = random.Random(s)
        sets.append((f"1-10s seed {s}", [rng.randint(86, 860) for _ in range(32)]))
    rng = random.Random(7)
    sets.append(("~1s seed 7", [rng.randint(60, 130) for _ in range(32)]))
    sets.append(("32 x 86 equal", [86] * 32))
    for name, lengths in sets:
        lines.append(measure(name, eng, lengths, a.rounds))
        print(lines[-1], flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
