#!/usr/bin/env python
"""Time of the GPU pitch shift (vocoder_amd/csrc/pitch_shift.hip) per stage and for the whole call: +3 semitones at 44100 Hz, B = 1 and B = 32 rows
of 1 s.

    python tools/pitch_shift_throughput.py [--n-steps 3] [--seconds 1] [--iters 100] [--warmup 10]

Each batch size is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started after
it).  The child warms the shape up, then times `--iters` back-to-back calls between two device events (hipEvents) for

    stretch    fv_pitch_shift_stretch: framing, STFT conv, polar, scan + synthesis, inverse-DFT conv, overlap-add
    resample   fv_resample_forward of the global-table resampler on the stretched rows (orig_freq -> sr)
    forward    fv_pitch_shift_forward: both, fixed to the input length

on fixed buffers through the C entry points (the module's per-call allocation is not the kernels').  The calls are driven from the host one
after the other, so a figure includes what the host spends per call (the ctypes dispatch, the launches) wherever the device is faster than that.  Prints ms per call and x real time;
writes the rows as JSON lines to --out when given.  No speed target is attached to these numbers.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

BATCHES = [1, 32]


def child(a) -> None:
    import torch
    from vocoder_amd import _lib
    from vocoder_amd.pitch_shift import KAISER_BEST_ROLLOFF, PitchShift
    from vocoder_amd.resample import Resample
    assert torch.cuda.is_available(), "pitch_shift_throughput.py needs an MI355X"
    sr, B = a.sample_rate, a.batch
    mod = PitchShift(sr, a.n_steps)
    res = Resample(mod.orig_freq, sr, resampling_method="sinc_interp_kaiser", lowpass_filter_width=64, rolloff=KAISER_BEST_ROLLOFF, table="global")
    L = int(a.seconds * sr)
    T, Tout, Ls, M = mod.lengths(L)
    x = torch.rand((B, L), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)) * 2 - 1
    st, y = mod.time_stretch(x), mod(x)
    r = res(st)
    lib, stream = _lib.lib(), int(torch.cuda.current_stream().cuda_stream)
    h = mod._handle(x.device)
    need = int(lib.fv_pitch_shift_workspace_bytes(h, B, L))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    calls = {
        "stretch": lambda: lib.fv_pitch_shift_stretch(h, x.data_ptr(), L, st.data_ptr(), Ls, B, L, ws.data_ptr(), need, stream),
        "resample": lambda: lib.fv_resample_forward(res._handle(x.device), st.data_ptr(), Ls, None, r.data_ptr(), M, B, Ls, stream),
        "forward": lambda: lib.fv_pitch_shift_forward(h, x.data_ptr(), L, y.data_ptr(), L, B, L, ws.data_ptr(), need, stream),
    }
    row = dict(sample_rate=sr, n_steps=a.n_steps, orig_freq=mod.orig_freq, batch=B, L=L, frames=T, frames_out=Tout, stretched=Ls, iters=a.iters)
    for name, call in calls.items():
        for _ in range(a.warmup):
            _lib.check(call())
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        status = 0
        for _ in range(a.iters):
            status |= call()
        e1.record()
        torch.cuda.synchronize()
        _lib.check(status)
        row[name + "_ms"] = round(e0.elapsed_time(e1) / a.iters, 5)
    row["x_real_time"] = round(B * a.seconds / (row["forward_ms"] * 1e-3), 0)
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sample-rate", type=int, default=44100)
    ap.add_argument("--n-steps", type=float, default=3.0)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds each batch size may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--batch", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.batch is not None:
        child(a)
        return 0
    print(f"{'B x s':>10} {'stretch ms':>11} {'resample ms':>12} {'forward ms':>11} {'x real time':>12}")
    for B in BATCHES:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--batch", str(B), "--sample-rate",
               str(a.sample_rate), "--n-steps", str(a.n_steps), "--seconds", str(a.seconds), "--iters", str(a.iters), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"B = {B}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        print(f"{B:>4} x {a.seconds:<4g} {row['stretch_ms']:>11.4f} {row['resample_ms']:>12.4f} {row['forward_ms']:>11.4f} {row['x_real_time']:>12.0f}")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
