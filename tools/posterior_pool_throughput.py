#!/usr/bin/env python
"""What one step of a posterior encoder pool costs (fv_wnpool_step, PosteriorEncoder.pool) beside the two forms a caller had before it.
The encoder is the default config (synthetic.POSTERIOR_DEFAULT: 16 layers, 192 channels, k = 5, R = 32); every session pushes `--chunk`
frames (8) per step, in the steady state (every push emits).

    python tools/posterior_pool_throughput.py [--sessions 1 8 32 256] [--chunk 8] [--iters 50] [--rounds 7] [--warmup 6]

Each session count is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started
after it).  The child warms all forms up, then times `--rounds` alternating rounds of

    pool      one PosteriorPool.step_padded for all S sessions on the caller's buffers
    streams   S PosteriorStream(batch=1).push calls, one per session: the only way to serve S independent sessions without the pool
    lockstep  one PosteriorStream(batch=S).push: rows that must advance together, the floor no pool can beat

with a host clock around work that ends in a device synchronise — all forms are launch-bound at these sizes, so the host's enqueue is part of
what a server pays — and reports each one's median and minimum round in ms per step, the ratios and the pool's launches per step.  A round is
`--iters` steps; the streams form, whose step is S pushes, runs fewer (at least 2) so that a round stays near `--iters` pushes of 8 sessions.
The pool's and the streams' outputs are compared bit for bit first.  FV_LIB_PATH selects another build of the library.  Writes the rows as
JSON lines to --out when given.  No speed target is attached to these numbers.
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
    import numpy as np
    import torch
    from vocoder_amd import _lib
    from vocoder_amd import synthetic as syn
    from vocoder_amd.modules.encoders import PosteriorEncoder
    assert torch.cuda.is_available(), "posterior_pool_throughput.py needs an MI355X"
    S, c = a.sessions[0], a.chunk
    cfg = dict(syn.POSTERIOR_DEFAULT)
    mod = PosteriorEncoder(**cfg)
    mod.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in syn.posterior_state_dict(cfg, 11).items()}, strict=True)
    mod = mod.eval().cuda()
    gen = torch.Generator(device="cuda").manual_seed(S)
    x = torch.randn((S, cfg["in_channels"], c), generator=gen, device="cuda")
    pool = mod.pool(S, c)
    streams = [mod.stream(1, c) for _ in range(S)]
    lock = mod.stream(S, c)
    items = [(s, c, False) for s in range(S)]
    vae = cfg["mode"] != "vqvae"
    new = lambda: torch.empty((S, cfg["out_channels"], pool.max_frames), dtype=torch.float32, device="cuda")      # noqa: E731
    out = (new(), new(), new()) if vae else new()

    def step_pool():
        return pool.step_padded(items, x, out=out)

    def step_streams():
        return [st.push(x[s:s + 1]) for s, st in enumerate(streams)]

    def step_lockstep():
        return lock.push(x)
    first = lambda r: r[0] if isinstance(r, tuple) else r      # noqa: E731
    same = True
    for _ in range(max(a.warmup, mod.reach_frames // c + 2)):          # past the lookahead: every push emits from here on
        (y, emit), ys, _ = step_pool(), step_streams(), step_lockstep()
        same = same and all(torch.equal(first(y)[s, :, :emit[s]], first(ys[s])[0]) for s in range(S))
    torch.cuda.synchronize()
    assert emit[0] == c, emit[0]
    forms = {"pool": (step_pool, a.iters), "streams": (step_streams, max(2, min(a.iters, 8 * a.iters // S))), "lockstep": (step_lockstep, a.iters)}
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, (call, iters) in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                call()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / iters * 1e3)
    row = dict(sessions=S, chunk=c, frames_per_item=emit[0], launches_per_step=pool.last_step_launches, iters=a.iters, rounds=a.rounds,
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
    ap.add_argument("--chunk", type=int, default=8, help="frames every session pushes per step")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds each session count may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    print(f"{'S':>4} {'frames':>6} {'launches':>8} {'pool ms':>9} {'(min)':>8} {'streams ms':>11} {'(min)':>9} {'lockstep ms':>12} {'(min)':>8} "
          f"{'us / item':>10} {'streams / pool':>15} {'pool / lockstep':>16} {'same bits':>10}")
    for S in a.sessions:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--sessions", str(S), "--chunk",
               str(a.chunk), "--iters", str(a.iters), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"S = {S}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        print(f"{S:>4} {row['frames_per_item']:>6} {row['launches_per_step']:>8} {row['pool_ms']:>9.4f} {row['pool_min_ms']:>8.4f} "
              f"{row['streams_ms']:>11.4f} {row['streams_min_ms']:>9.4f} {row['lockstep_ms']:>12.4f} {row['lockstep_min_ms']:>8.4f} "
              f"{row['pool_us_per_item']:>10.2f} {row['streams_over_pool']:>15.2f} {row['pool_over_lockstep']:>16.2f} "
              f"{str(row['bit_identical']):>10}", flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
