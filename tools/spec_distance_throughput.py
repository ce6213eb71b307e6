#!/usr/bin/env python
"""Throughput of the scoring reduction (vocoder_amd/csrc/spec_distance.hip) at a server's batch: B = 32 log-mels of 128 channels, 10 s at
44100 Hz / hop 512 (861 frames), against the torch composite a user would write today on the same tensors.

    python tools/spec_distance_throughput.py [--batch 32] [--channels 128] [--seconds 10] [--ragged] [--iters 200] [--warmup 20]

Each mode (without and with the log term) is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and
nothing is started after it).  The child warms the shape up, then times `--iters` back-to-back calls between two device events and prints:

    kernel ms per call | GB/s over the compulsory bytes 2 * 4 * C * sum(frames) | share of the 8.0 TB/s HBM peak | torch composite ms | ratio

The compulsory bytes are what any such reduction must move: each operand read once.  The kernel is timed through the C entry point on fixed
buffers (its two launches; the module's per-call host work is not the kernel's).  The composite is the masked form of the same four sums,
`torch.where(mask, est - ref, 0).abs().sum((1, 2), dtype=float64)` and so on: several passes over the tensors and their temporaries.
The default shape is 28 MB per call and stays in the 256 MiB Infinity Cache between calls, so its GB/s is a cache figure; `--batch 512`
(451 MB) is the HBM figure.  `--ragged` gives row b the frames T * (b + 1) / B.  Writes the rows as JSON lines to --out when given.
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


def child(a) -> None:
    import ctypes
    import torch
    from vocoder_amd import _lib
    from vocoder_amd.scoring import spec_distance
    assert torch.cuda.is_available(), "spec_distance_throughput.py needs an MI355X"
    B, C, T = a.batch, a.channels, int(a.seconds * 44100) // 512
    g = torch.Generator(device="cuda").manual_seed(0)
    ref = torch.rand((B, C, T), device="cuda", generator=g) + 0.5
    est = ref * (1 + 0.1 * torch.rand((B, C, T), device="cuda", generator=g))
    frames = [max(1, T * (b + 1) // B) for b in range(B)] if a.ragged else [T] * B
    log_term = bool(a.log)
    want = spec_distance(est, ref, frames, log_term=log_term)

    def time_it(fn) -> float:
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    lib, stream = _lib.lib(), int(torch.cuda.current_stream().cuda_stream)
    need = int(lib.fv_spec_distance_workspace_bytes(B, T))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty((B, 4), dtype=torch.float64, device="cuda")
    arr = (ctypes.c_int32 * B)(*frames)
    args = (est.data_ptr(), ref.data_ptr(), C * T, T, C, T, arr, B, _lib.FV_SPEC_DISTANCE_LOG if log_term else 0, out.data_ptr(), ws.data_ptr(),
            need, stream)
    _lib.check(lib.fv_spec_distance(*args))
    ms = time_it(lambda: lib.fv_spec_distance(*args))
    assert out.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()

    mask = torch.arange(T, device="cuda")[None, None, :] < torch.tensor(frames, device="cuda")[:, None, None]
    zero = torch.zeros((), device="cuda")

    def composite():
        d = torch.where(mask, est - ref, zero)
        r = torch.where(mask, ref, zero)
        cols = [d.abs().sum((1, 2), dtype=torch.float64), (d * d).sum((1, 2), dtype=torch.float64), (r * r).sum((1, 2), dtype=torch.float64)]
        if log_term:
            cols.append(torch.where(mask, torch.log(ref) - torch.log(est), zero).abs().sum((1, 2), dtype=torch.float64))
        return torch.stack(cols, 1)
    got = composite()
    assert torch.allclose(got, want[:, :got.shape[1]], rtol=1e-6, atol=0)
    torch_ms = time_it(composite)
    nbytes = 2.0 * 4 * C * sum(frames)
    row = dict(batch=B, channels=C, T=T, ragged=bool(a.ragged), log_term=log_term, iters=a.iters, mbytes=round(nbytes / 1e6, 1), ms=round(ms, 5),
               gb_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1), hbm_peak_share=round(nbytes / (ms * 1e-3) / HBM_PEAK, 4),
               torch_composite_ms=round(torch_ms, 5), torch_over_kernel=round(torch_ms / ms, 2))
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds each mode may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--log", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.log is not None:
        child(a)
        return 0
    print(f"{'mode':>10} {'MB':>8} {'ms':>9} {'GB/s':>9} {'of HBM peak':>12} {'torch ms':>9} {'torch / kernel':>15}")
    for log in (0, 1):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--log", str(log), "--batch", str(a.batch),
               "--channels", str(a.channels), "--seconds", str(a.seconds), "--iters", str(a.iters), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd + (["--ragged"] if a.ragged else []), capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"log_term={log}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        print(f"{'with log' if log else 'no log':>10} {row['mbytes']:>8.1f} {row['ms']:>9.4f} {row['gb_per_s']:>9.1f} {100 * row['hbm_peak_share']:>11.1f}% "
              f"{row['torch_composite_ms']:>9.4f} {row['torch_over_kernel']:>14.1f}x")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
