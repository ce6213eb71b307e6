#!/usr/bin/env python
"""Throughput of the GPU resampler (vocoder_amd/csrc/resample.hip) at a server's batch: 44100 -> 48000 and 44100 -> 16000, B = 32 rows of 10 s.

    python tools/resample_throughput.py [--batch 32] [--seconds 10] [--iters 200] [--warmup 20]

Each rate pair is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started after
it).  The child warms the shape up, then times `--iters` back-to-back forwards between two device events and prints one row:

    ms per call | GB/s over the compulsory bytes 4 (L + M) per row | share of the 8.0 TB/s HBM peak | x real time

The compulsory bytes are what any resampler must move: each input sample read once, each output written once.  The share of peak says how far
the kernel is from being bound by memory alone; the banded FIR reads LDS twice per multiply-add (tap and sample), which is what binds it when
the share is low.  Writes the rows as JSON lines to --out when given.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12     # bytes / s, MI355X HBM3E specification
PAIRS = [(44100, 48000), (44100, 16000)]


def child(a) -> None:
    import torch
    from vocoder_amd import _lib
    from vocoder_amd.resample import Resample
    assert torch.cuda.is_available(), "resample_throughput.py needs an MI355X"
    mod = Resample(a.orig, a.new)
    L = int(a.seconds * a.orig)
    x = torch.rand((a.batch, L), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)) * 2 - 1
    y = mod(x)
    # the timed loop calls the C entry point on fixed buffers: the module's per-call host work (an allocation, shape checks) is not the kernel's
    lib, h, stream = _lib.lib(), mod._handle(x.device), int(torch.cuda.current_stream().cuda_stream)
    args = (h, x.data_ptr(), L, None, y.data_ptr(), int(y.shape[-1]), a.batch, L, stream)
    for _ in range(a.warmup):
        _lib.check(lib.fv_resample_forward(*args))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        lib.fv_resample_forward(*args)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    M = int(y.shape[-1])
    nbytes = 4.0 * (L + M) * a.batch
    row = dict(orig=a.orig, new=a.new, batch=a.batch, L=L, M=M, phases=mod.design.n, taps=mod.design.kp, iters=a.iters, ms=round(ms, 5),
               gb_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1), hbm_peak_share=round(nbytes / (ms * 1e-3) / HBM_PEAK, 4),
               x_real_time=round(a.batch * a.seconds / (ms * 1e-3), 0),
               lds_reads_per_output=2 * mod.design.kp)
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds each rate pair may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--orig", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--new", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.orig is not None:
        child(a)
        return 0
    print(f"{'rates':>16} {'ms':>9} {'GB/s':>9} {'of HBM peak':>12} {'x real time':>12}")
    for orig, new in PAIRS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--orig", str(orig), "--new", str(new),
               "--batch", str(a.batch), "--seconds", str(a.seconds), "--iters", str(a.iters), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"{orig} -> {new}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        print(f"{orig:>7} -> {new:<6} {row['ms']:>9.4f} {row['gb_per_s']:>9.1f} {100 * row['hbm_peak_share']:>11.1f}% {row['x_real_time']:>12.0f}")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
