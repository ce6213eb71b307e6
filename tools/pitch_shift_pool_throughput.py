#!/usr/bin/env python
"""What one step of a pitch-shift pool costs (fv_pvpool_step, vocoder_amd.pitch_shift.PitchShiftPool) beside the two forms a caller had
before it.  The shifter runs at 44100 Hz with n_fft 2048, hop 512 and n_steps = +3; every session pushes `--chunk` samples (4096) per step,
in the steady state (a push emits about as many samples as it takes).

    python tools/pitch_shift_pool_throughput.py [--sessions 1 8 32 256] [--chunk 4096] [--iters 50] [--rounds 7] [--warmup 5]

Each session count is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started
after it).  The child warms all forms up, then times `--rounds` alternating rounds of `--iters` steps of

    pool      one PitchShiftPool.step_padded for all S sessions on the caller's buffers
    streams   S PitchShiftStream(batch=1).push calls, one per session: the only way to serve S independent sessions without the pool
    lockstep  one PitchShiftStream(batch=S).push: rows that must advance together

with a host clock around work that ends in a device synchronise — the host's enqueue is part of what a server pays — and reports each
one's median and minimum round in ms per step and the ratios.  The pool's and the streams' outputs are compared bit for bit first.  FV_LIB_PATH selects another build of the library.  Writes the rows as JSON lines to --out when given.  No speed
target is attached to these numbers.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def child(a) -> None:
    import torch
    from vocoder_amd import _lib
    from vocoder_amd.pitch_shift import PitchShift
    assert torch.cuda.is_available(), "pitch_shift_pool_throughput.py needs an MI355X"
    S, c = a.sessions[0], a.chunk
    shift = PitchShift(a.sample_rate, a.n_steps, n_fft=a.n_fft, hop_length=a.hop, batch_invariant=True)
    # every session its own tone between 110 and 440 Hz (the same chunk every step: the cost does not depend on the samples)
    t = torch.arange(c, device="cuda", dtype=torch.float64)
    f = 110.0 * 4.0 ** (torch.arange(S, device="cuda", dtype=torch.float64) / max(S, 2))
    x = (0.5 * torch.sin(2 * torch.pi * f[:, None] * t[None, :] / a.sample_rate)).float().contiguous()
    pool = shift.pool(S, c)
    streams = [shift.stream(1, c) for _ in range(S)]
    lock = shift.stream(S, c)
    items = [(s, c, False) for s in range(S)]
    out = torch.empty((S, pool.max_outputs), dtype=torch.float32, device="cuda")

    def step_pool():
        return pool.step_padded(items, x, out=out)

    def step_streams():
        return [st.push(x[s:s + 1]) for s, st in enumerate(streams)]

    def step_lockstep():
        return lock.push(x)
    same = True
    for _ in range(a.warmup):
        (y, emit), ys, _ = step_pool(), step_streams(), step_lockstep()
        same = same and all(torch.equal(y[s, :emit[s]], ys[s][0]) for s in range(S))
    torch.cuda.synchronize()
    forms = {"pool": step_pool, "streams": step_streams, "lockstep": step_lockstep}
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, call in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                call()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.iters * 1e3)
    row = dict(sessions=S, chunk=c, sample_rate=a.sample_rate, n_steps=a.n_steps, n_fft=a.n_fft, hop=a.hop, outputs_per_item=emit[0],
               iters=a.iters, rounds=a.rounds,
               bit_identical=bool(same), lib=os.path.basename(_lib.LIB_PATH))
    for name, ts in times.items():
        row[name + "_ms"] = round(statistics.median(ts), 4)
        row[name + "_min_ms"] = round(min(ts), 4)
    row["pool_us_per_item"] = round(row["pool_ms"] / S * 1e3, 2)
    row["streams_over_pool"] = round(row["streams_ms"] / row["pool_ms"], 2)
    row["pool_over_lockstep"] = round(row["pool_ms"] / row["lockstep_ms"], 2)
    for st in streams + [lock]:
        st.close()
    pool.close()
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 8, 32, 256])
    ap.add_argument("--chunk", type=int, default=4096, help="samples every session pushes per step")
    ap.add_argument("--sample-rate", type=int, default=44100)
    ap.add_argument("--n-fft", type=int, default=2048)
    ap.add_argument("--n-steps", type=float, default=3.0)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds each session count may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    print(f"{'S':>4} {'outputs':>7} {'pool ms':>9} {'(min)':>8} {'streams ms':>11} {'(min)':>8} {'lockstep ms':>12} {'(min)':>8} {'us / item':>10} "
          f"{'streams / pool':>15} {'pool / lockstep':>16} {'same bits':>10}")
    for S in a.sessions:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--sessions", str(S), "--chunk",
               str(a.chunk), "--sample-rate", str(a.sample_rate), "--n-fft", str(a.n_fft), "--n-steps", str(a.n_steps), "--hop", str(a.hop),
               "--iters", str(a.iters), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"S = {S}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        print(f"{S:>4} {row['outputs_per_item']:>7} {row['pool_ms']:>9.4f} {row['pool_min_ms']:>8.4f} {row['streams_ms']:>11.4f} "
              f"{row['streams_min_ms']:>8.4f} {row['lockstep_ms']:>12.4f} {row['lockstep_min_ms']:>8.4f} {row['pool_us_per_item']:>10.2f} "
              f"{row['streams_over_pool']:>15.2f} {row['pool_over_lockstep']:>16.2f} {str(row['bit_identical']):>10}")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
