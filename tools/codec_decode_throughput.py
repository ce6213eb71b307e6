#!/usr/bin/env python
"""What one step of a code session pool costs (fv_codepool_step, CodeSessionPool) beside the chain a caller had before it, and what its
rings cost.  The decoder stage is the backbone of the default VQ-VAE config (configs/model/vqvae.yaml: ConvNeXt depths (6, 3), dims
(512, 1024) on D = 512 latent channels, 4096 codes; R = 32) — the engine the codes enter; the ISTFT head behind it is the same in every
form.  Every session pushes `--chunk` frames (8) per step, in the steady state (every push emits).

    python tools/codec_decode_throughput.py [--sessions 1 8 32 256] [--quantizers 1 8] [--chunk 8] [--iters 50] [--rounds 7]

Each (n_q, S) is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started after
it).  The child warms all forms up, then times `--rounds` alternating rounds of

    pool      one CodeSessionPool.step_padded for all S sessions on the caller's int32 codes (no host check of the codes)
    checked   the same after the one host check CodeSessionPool.step makes (a synchronisation: every code in [-1, K))
    chain     vq.from_codes (fv_vq_decode and its host check) + SessionPool.step_padded: the unfused chain of the commit before
    streams   S CodeStream(batch=1).push calls, one per session

with a host clock around work that ends in a device synchronise, and reports each one's median (p50) and minimum round in ms per step, the
ratios, and the bytes of the code pool's rings beside the float pool's.  The pool's and the chain's outputs are compared bit for bit first.
FV_LIB_PATH selects another build of the library.  Writes the rows as JSON lines to --out when given.  No speed target is attached to these
numbers; the derived gain is memory, D / n_q on the mel ring.
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

BACKBONE = dict(input_channels=512, depths=[6, 3], dims=[512, 1024], kernel_size=7)
CODEBOOK = 4096


def child(a) -> None:
    import numpy as np
    import torch
    from vocoder_amd import _lib
    from vocoder_amd import synthetic as syn
    from vocoder_amd.engine import _validate_codes
    from vocoder_amd.modules.encoders import ConvNeXtEncoder
    from vocoder_amd.modules.quantizers import ResidualVectorQuantization, VectorQuantization
    assert torch.cuda.is_available(), "codec_decode_throughput.py needs an MI355X"
    S, c, nq, D = a.sessions[0], a.chunk, a.quantizers[0], BACKBONE["input_channels"]
    mod = ConvNeXtEncoder(**BACKBONE)
    mod.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in syn.convnext_state_dict(BACKBONE, 11).items()}, strict=True)
    mod = mod.eval().cuda()
    torch.manual_seed(nq)
    vq = (ResidualVectorQuantization(num_quantizers=nq, dim=D, codebook_size=CODEBOOK, kmeans_init=False) if nq > 1 else
          VectorQuantization(dim=D, codebook_size=CODEBOOK, kmeans_init=False)).eval().cuda()
    gen = torch.Generator(device="cuda").manual_seed(S)
    codes = torch.randint(0, CODEBOOK, (nq, S, c), generator=gen, device="cuda", dtype=torch.int32)
    cp, fp = mod.code_pool(vq, S, c), mod.session_pool(S, c)
    streams = [mod.code_stream(vq, 1, c) for _ in range(S)]
    items = [(s, c, False) for s in range(S)]
    out = torch.empty((S, cp.out_channels, c * cp.hop), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(out)

    def step_pool():
        return cp.step_padded(items, codes, out=out)

    def step_checked():
        _validate_codes(codes, CODEBOOK, "codec_decode_throughput")
        return cp.step_padded(items, codes, out=out)

    def step_chain():
        return fp.step_padded(items, vq.from_codes(codes)[0], out=out2)

    def step_streams():
        return [st.push(codes[:, s:s + 1], validate=False) for s, st in enumerate(streams)]
    same = True
    for _ in range(max(a.warmup, cp.lookahead_frames // c + 2)):          # past the lookahead: every push emits from here on
        (y, emit), (y2, _) = step_pool(), step_chain()
        same = same and torch.equal(y, y2)
        step_streams()
    torch.cuda.synchronize()
    assert emit[0] == c, emit[0]
    forms = {"pool": (step_pool, a.iters), "checked": (step_checked, a.iters), "chain": (step_chain, a.iters),
             "streams": (step_streams, max(2, min(a.iters, 8 * a.iters // S)))}
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, (call, iters) in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                call()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / iters * 1e3)
    row = dict(quantizers=nq, sessions=S, chunk=c, dim=D, iters=a.iters, rounds=a.rounds, bit_identical=bool(same),
               code_ring_bytes=cp.ring_bytes, float_ring_bytes=fp.ring_bytes, lib=os.path.basename(_lib.LIB_PATH))
    for name, ts in times.items():
        row[name + "_ms"] = round(statistics.median(ts), 4)
        row[name + "_min_ms"] = round(min(ts), 4)
    row["chain_over_pool"] = round(row["chain_ms"] / row["pool_ms"], 3)
    row["chain_over_checked"] = round(row["chain_ms"] / row["checked_ms"], 3)
    row["streams_over_pool"] = round(row["streams_ms"] / row["pool_ms"], 2)
    row["ring_ratio"] = round(row["float_ring_bytes"] / row["code_ring_bytes"], 1)
    for st in streams:
        st.close()
    cp.close(), fp.close()
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 8, 32, 256])
    ap.add_argument("--quantizers", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--chunk", type=int, default=8, help="frames every session pushes per step")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds each (n_q, S) may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    print(f"{'n_q':>3} {'S':>4} {'pool ms':>9} {'(min)':>8} {'checked ms':>11} {'(min)':>8} {'chain ms':>9} {'(min)':>8} {'streams ms':>11} "
          f"{'chain / pool':>13} {'chain / checked':>16} {'code ring B':>12} {'float ring B':>13} {'ratio':>6} {'same bits':>10}")
    for nq in a.quantizers:
        for S in a.sessions:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--sessions", str(S),
                   "--quantizers", str(nq), "--chunk", str(a.chunk), "--iters", str(a.iters), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                print(f"n_q = {nq}, S = {S}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
                return r.returncode
            row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
            print(f"{nq:>3} {S:>4} {row['pool_ms']:>9.4f} {row['pool_min_ms']:>8.4f} {row['checked_ms']:>11.4f} {row['checked_min_ms']:>8.4f} "
                  f"{row['chain_ms']:>9.4f} {row['chain_min_ms']:>8.4f} {row['streams_ms']:>11.4f} {row['chain_over_pool']:>13.3f} "
                  f"{row['chain_over_checked']:>16.3f} {row['code_ring_bytes']:>12} {row['float_ring_bytes']:>13} {row['ring_ratio']:>6.1f} "
                  f"{str(row['bit_identical']):>10}", flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
