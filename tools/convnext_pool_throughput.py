#!/usr/bin/env python
"""What one step of a ConvNeXt layer pool costs (fv_cnxpool_step, ConvNeXtEncoder.layer_pool) beside the forms a caller had before it, in
the default codec (codec.build_vqvae(): encoder 513 -> (512,) x 6, R = 21; decoder backbone 512 -> (512, 1024), depths (6, 3), R = 30,
and the ISTFT head, n_fft 3072, hop 2048).  Every session pushes `--chunk` frames (8) per step, in the steady state (every push emits).

    python tools/convnext_pool_throughput.py [--tables layers decode encode] [--sessions 1 8 32 256] [--chunk 8] [--iters 30] [--rounds 7]

Three tables; every (table, model, S) is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and
nothing is started after it).  The child warms all forms up, then times `--rounds` alternating rounds of

  layers   pool      one ConvNeXtPool.step_padded for all S sessions on the caller's buffers            (for the encoder and the backbone)
           streams   S ConvNeXtStream(batch=1).push calls, one per session: what served S independent sessions by layers before the pool
           lockstep  one ConvNeXtStream(batch=S).push: rows that must advance together
  decode   layers    CodecDecodePool(backbone="layers").step_padded: from_codes -> the backbone's layer pool -> the head's session pool
                     (from_codes makes its one host check of the codes, a synchronisation, in every step)
           window    CodecDecodePool(backbone="window").step_padded: the path of the commit before, the code rings in front of a backbone
                     whose whole window is recomputed for every session in every step; it remains the baseline (no check of the codes)
           checked   the same after the one host check CodecDecodePool.step makes by default (a synchronisation)
  encode   layers    CodecEncodePool(layers=True).step_padded: wav pool -> the encoder's layer pool -> vq.encode (there is no other pool form
                     of the default encoder to put beside it)

with a host clock around work that ends in a device synchronise — every form is enqueued launch by launch, so the host's enqueue is part of
what a server pays — and reports each one's median (p50) and minimum round in ms per step, the ratios and the layer pool's launches per
step.  A round is `--iters` steps; the streams form, whose step is S pushes, runs fewer (at least 2).  The pool's and the streams' outputs
are compared bit for bit first.  FV_LIB_PATH selects another build of the library.  Writes the rows as JSON lines to --out when given.  No
speed target is attached to these numbers.
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

MODELS = {"encoder": dict(input_channels=513, depths=[6], dims=[512], kernel_size=7),
          "backbone": dict(input_channels=512, depths=[6, 3], dims=[512, 1024], kernel_size=7)}
HOP = 2048


def time_forms(a, forms: dict) -> dict:
    """forms: name -> (call, iters).  Alternating rounds; -> {name_ms: p50, name_min_ms: min}."""
    import torch
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, (call, iters) in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                call()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / iters * 1e3)
    row = {}
    for name, ts in times.items():
        row[name + "_ms"] = round(statistics.median(ts), 4)
        row[name + "_min_ms"] = round(min(ts), 4)
    return row


def child_layers(a, S: int, c: int) -> dict:
    import numpy as np
    import torch
    from vocoder_amd import synthetic as syn
    from vocoder_amd.modules.encoders import ConvNeXtEncoder
    cfg = MODELS[a.model]
    mod = ConvNeXtEncoder(**cfg)
    mod.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in syn.convnext_state_dict(cfg, 11).items()}, strict=True)
    mod = mod.eval().cuda()
    x = torch.randn((S, cfg["input_channels"], c), generator=torch.Generator(device="cuda").manual_seed(S), device="cuda")
    pool = mod.layer_pool(S, c)
    streams = [mod.layer_stream(1, c) for _ in range(S)]
    lock = mod.layer_stream(S, c)
    items = [(s, c, False) for s in range(S)]
    out = torch.empty((S, pool.out_channels, pool.max_frames), dtype=torch.float32, device="cuda")

    def step_pool():
        return pool.step_padded(items, x, out=out)

    def step_streams():
        return [st.push(x[s:s + 1]) for s, st in enumerate(streams)]

    def step_lockstep():
        return lock.push(x)
    same = True
    for _ in range(max(a.warmup, pool.lookahead_frames // c + 2)):          # past the lookahead: every push emits from here on
        (y, emit), ys, yl = step_pool(), step_streams(), step_lockstep()
        same = same and all(torch.equal(y[s, :, :emit[s]], ys[s][0]) for s in range(S)) and torch.equal(y[:, :, :emit[0]], yl)
    torch.cuda.synchronize()
    assert emit[0] == c, emit[0]
    row = dict(table="layers", model=a.model, sessions=S, chunk=c, launches_per_step=pool.last_step_launches, bit_identical=bool(same),
               state_bytes=pool.state_bytes)
    row.update(time_forms(a, {"pool": (step_pool, a.iters), "streams": (step_streams, max(2, min(a.iters, 8 * a.iters // S))),
                              "lockstep": (step_lockstep, a.iters)}))
    row["streams_over_pool"] = round(row["streams_ms"] / row["pool_ms"], 2)
    row["pool_over_lockstep"] = round(row["pool_ms"] / row["lockstep_ms"], 2)
    for st in streams + [lock]:
        st.close()
    pool.close()
    return row


def child_decode(a, S: int, c: int) -> dict:
    import torch
    from vocoder_amd import codec
    from vocoder_amd.engine import _validate_codes
    torch.manual_seed(11)
    m = codec.build_vqvae().eval().cuda()
    codes = torch.randint(0, 4096, (1, S, c), generator=torch.Generator(device="cuda").manual_seed(S), device="cuda", dtype=torch.int32)
    lay, win = m.decode_pool(S, c, backbone="layers"), m.decode_pool(S, c, backbone="window")
    items = [(s, c, False) for s in range(S)]

    def step_layers():
        return lay.step_padded(items, codes)

    def step_window():
        return win.step_padded(items, codes)

    def step_checked():
        _validate_codes(codes, 4096, "convnext_pool_throughput")
        return win.step_padded(items, codes)
    for _ in range(max(a.warmup, lay.lookahead_frames // c + 2, win.lookahead_frames // c + 2)):          # past both lookaheads
        (_, emit), (_, emit2) = step_layers(), step_window()
    torch.cuda.synchronize()
    assert emit[0] == c and emit2[0] == c, (emit[0], emit2[0])
    row = dict(table="decode", sessions=S, chunk=c, launches_per_step=lay.codes.pool.last_step_launches, lookahead_layers=lay.lookahead_frames,
               lookahead_window=win.lookahead_frames, ring_bytes_layers=lay.ring_bytes, ring_bytes_window=win.ring_bytes)
    row.update(time_forms(a, {"layers": (step_layers, a.iters), "window": (step_window, a.iters), "checked": (step_checked, a.iters)}))
    row["window_over_layers"] = round(row["window_ms"] / row["layers_ms"], 3)
    row["checked_over_layers"] = round(row["checked_ms"] / row["layers_ms"], 3)
    lay.close(), win.close()
    return row


def child_encode(a, S: int, c: int) -> dict:
    import torch
    from vocoder_amd import codec
    torch.manual_seed(11)
    m = codec.build_vqvae().eval().cuda()
    m.encoder.batch_invariant = m.frontend.batch_invariant = True
    n = c * HOP
    wave = 0.1 * torch.randn((S, n), generator=torch.Generator(device="cuda").manual_seed(S), device="cuda")
    pool = m.encode_pool(S, n, layers=True)
    items = [(s, n, False) for s in range(S)]

    def step():
        return pool.step_padded(items, wave)
    for _ in range(max(a.warmup, pool.enc_pool.lookahead_frames // c + 3)):
        _, emit = step()
    torch.cuda.synchronize()
    row = dict(table="encode", sessions=S, chunk=c, samples_per_item=n, frames_per_item=emit[0], launches_per_step=pool.enc_pool.last_step_launches)
    row.update(time_forms(a, {"layers": (step, a.iters)}))
    row["us_per_item"] = round(row["layers_ms"] / S * 1e3, 2)
    pool.close()
    return row


def child(a) -> None:
    import torch
    from vocoder_amd import _lib
    assert torch.cuda.is_available(), "convnext_pool_throughput.py needs an MI355X"
    row = {"layers": child_layers, "decode": child_decode, "encode": child_encode}[a.tables[0]](a, a.sessions[0], a.chunk)
    row.update(iters=a.iters, rounds=a.rounds, lib=os.path.basename(_lib.LIB_PATH))
    print("RESULT " + json.dumps(row), flush=True)


HEADS = {
    "layers": ("model", "sessions", "launches_per_step", "pool_ms", "pool_min_ms", "streams_ms", "streams_min_ms", "lockstep_ms",
               "lockstep_min_ms", "streams_over_pool", "pool_over_lockstep", "bit_identical"),
    "decode": ("sessions", "launches_per_step", "layers_ms", "layers_min_ms", "window_ms", "window_min_ms", "checked_ms", "checked_min_ms",
               "window_over_layers", "checked_over_layers"),
    "encode": ("sessions", "frames_per_item", "launches_per_step", "layers_ms", "layers_min_ms", "us_per_item"),
}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tables", nargs="+", default=["layers", "decode", "encode"], choices=list(HEADS))
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 8, 32, 256])
    ap.add_argument("--chunk", type=int, default=8, help="frames every session pushes per step")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds each (table, model, S) may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--model", default="encoder", choices=list(MODELS), help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    for table in a.tables:
        head = HEADS[table]
        print(f"-- {table} --")
        print(" ".join(f"{h:>18}" for h in head))
        for model in (list(MODELS) if table == "layers" else ["encoder"]):
            for S in a.sessions:
                cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--tables", table,
                       "--model", model, "--sessions", str(S), "--chunk", str(a.chunk), "--iters", str(a.iters), "--rounds", str(a.rounds),
                       "--warmup", str(a.warmup)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    print(f"{table}, {model}, S = {S}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
                    return r.returncode
                row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
                print(" ".join(f"{row[h]:>18.4g}" if isinstance(row[h], float) else f"{str(row[h]):>18}" for h in head), flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
