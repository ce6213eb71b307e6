#!/usr/bin/env python
"""Time of the GPU F0 tracker and the pitch-template synthesiser (vocoder_amd/csrc/f0_template.hip): 32 rows of 1 s and of 10 s at 44100 Hz with
the default plan (frame 2048, hop 512, 40 - 1100 Hz).

    python tools/f0_template_throughput.py [--batch 32] [--seconds 1 10] [--iters 50] [--warmup 5]

Each row length is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started after
it).  The child warms the shape up, then times `--iters` back-to-back calls between two device events (hipEvents) for

    yin        fv_f0_forward: yin_f0_kernel, one workgroup per (row, frame)
    template   fv_template_forward: f0_increment_kernel, f0_template_sums_kernel, f0_template_kernel

on fixed buffers through the C entry points (the module's per-call allocation is not the kernels').  Beside each time it prints the kernel's
roofs computed from the plan: for yin, P = frames * (tau_max + 1) * Wi subtract-and-FMA pairs — two vector instructions each, so
2 P / (CUs * 128 lanes * 2.4 GHz) — and the LDS bytes the lag loop reads per pair (2 B in the register-tiled form: two 16-byte reads feed
sixteen pairs) over 256 B per clock and CU; for the template, the bytes written over 8 TB/s.  FV_LIB_PATH selects another build of the
library (an A/B partner).  Writes the rows as JSON lines to --out when given.  No speed target is attached to these numbers.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CLOCK_HZ, LDS_BYTES_PER_CLK, HBM_BYTES_PER_S = 2.4e9, 256, 8e12


def child(a) -> None:
    import torch
    from vocoder_amd import _lib
    from vocoder_amd.f0 import PitchTemplate, YinF0
    assert torch.cuda.is_available(), "f0_template_throughput.py needs an MI355X"
    sr, B, hop = a.sample_rate, a.batch, a.hop_length
    seconds = a.seconds[0]
    yin, osc = YinF0(sr, hop), PitchTemplate(sr, hop)
    L = int(seconds * sr)
    T = yin.frames(L)
    n = torch.arange(L, device="cuda", dtype=torch.float32)[None]
    f = 110.0 + 10.0 * torch.arange(B, device="cuda", dtype=torch.float32)[:, None]
    x = (0.3 * sum(torch.sin(2 * torch.pi * h * f * n / sr) / h for h in range(1, 6))).contiguous()      # a voiced row per pitch
    f0, ap = yin(x)
    y = osc(f0)
    lib, stream = _lib.lib(), int(torch.cuda.current_stream().cuda_stream)
    hy, ht = yin._handle(x.device), osc._handle(x.device)
    need = int(lib.fv_template_workspace_bytes(ht, B, T))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    f0, ap = f0.contiguous(), ap.contiguous()
    calls = {
        "yin": lambda: lib.fv_f0_forward(hy, x.data_ptr(), L, None, f0.data_ptr(), ap.data_ptr(), T, B, L, None, 0, stream),
        "template": lambda: lib.fv_template_forward(ht, f0.data_ptr(), T, None, y.data_ptr(), T * hop, B, T, ws.data_ptr(), need, stream),
    }
    tau_min, tau_max, Wi = yin.plan()
    pairs = B * T * (tau_max + 1) * Wi
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row = dict(sample_rate=sr, batch=B, seconds=seconds, L=L, frames=T, tau_max=tau_max, window=Wi, voiced=float((f0 > 0).float().mean()),
               iters=a.iters, lib=os.path.basename(_lib.LIB_PATH), pairs=pairs,
               yin_valu_roof_ms=round(2 * pairs / (cus * 128 * CLOCK_HZ) * 1e3, 4),
               yin_lds_roof_ms=round(2 * pairs / (cus * LDS_BYTES_PER_CLK * CLOCK_HZ) * 1e3, 4),
               yin_lds_roof_plain_ms=round(8 * pairs / (cus * LDS_BYTES_PER_CLK / 2 * CLOCK_HZ) * 1e3, 4),
               template_hbm_roof_ms=round(4 * B * T * hop / HBM_BYTES_PER_S * 1e3, 4))
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
    row["x_real_time"] = round(B * seconds / ((row["yin_ms"] + row["template_ms"]) * 1e-3), 0)
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sample-rate", type=int, default=44100)
    ap.add_argument("--hop-length", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, nargs="+", default=[1.0, 10.0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds each row length may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    print(f"{'B x s':>10} {'yin ms':>9} {'VALU roof':>10} {'LDS roof':>9} {'template ms':>12} {'HBM roof':>9} {'x real time':>12}")
    for seconds in a.seconds:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch),
               "--sample-rate", str(a.sample_rate), "--hop-length", str(a.hop_length), "--seconds", str(seconds), "--iters", str(a.iters),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"{a.batch} x {seconds} s: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        print(f"{a.batch:>4} x {seconds:<4g} {row['yin_ms']:>9.4f} {row['yin_valu_roof_ms']:>10.4f} {row['yin_lds_roof_ms']:>9.4f} "
              f"{row['template_ms']:>12.4f} {row['template_hbm_roof_ms']:>9.4f} {row['x_real_time']:>12.0f}")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
