#!/usr/bin/env python
"""Time of the GPU quantiser's encode (vocoder_amd/csrc/vq.hip) next to a PyTorch-ROCm formulation of the same arithmetic on the same device:
the codec's own shape (D 512, K 4096, 32 clips x 12 frames) and 4096 frames (32 x 128), at n_q in {1, 8}.

    python tools/vq_throughput.py [--dim 512] [--codebook-size 4096] [--layouts 32x12 32x128] [--num-quantizers 1 8] [--iters 50] [--warmup 5]

Each (layout, n_q) is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started
after it).  The child warms the shape up, then times `--iters` back-to-back calls between two device events (hipEvents) for

    fused   fv_vq_encode on fixed buffers through the C entry point: vq_search_kernel + vq_select_kernel per layer, 2 n_q launches
    torch   per layer: s = frames @ embed.T - h (matmul), argmax, index_select, subtract, add into z - the N x K matrix is written and read

and reports on how many frames the two pick other codes (fp32 near-ties).  Beside each time: the matrix roof of the search,
2 N K D n_q flops over CUs * 256 flops per clock (v_mfma_f32_32x32x2_f32) at 2.4 GHz.  FV_LIB_PATH selects another build of the library.
Writes the rows as JSON lines to --out when given.  No speed target is attached to these numbers.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CLOCK_HZ, MFMA_F32_FLOPS_PER_CLK_CU = 2.4e9, 256


def child(a) -> None:
    import torch
    from vocoder_amd import _lib
    from vocoder_amd.modules.quantizers import ResidualVectorQuantization
    assert torch.cuda.is_available(), "vq_throughput.py needs an MI355X"
    D, K, nq = a.dim, a.codebook_size, a.num_quantizers[0]
    B, T = (int(v) for v in a.layouts[0].split("x"))
    g = torch.Generator().manual_seed(0)
    vq = ResidualVectorQuantization(num_quantizers=nq, dim=D, codebook_size=K, kmeans_init=False)
    vq.load_state_dict({**vq.state_dict(), **{f"layers.{q}._codebook.embed": 0.8 * 0.6 ** q * torch.randn(K, D, generator=g) for q in range(nq)}})
    vq = vq.eval().cuda()
    x = torch.randn(B, D, T, generator=g).cuda()
    z, codes, _ = vq(x)
    lib, stream = _lib.lib(), int(torch.cuda.current_stream().cuda_stream)
    h = vq.engine(x.device).handle
    need = int(lib.fv_vq_workspace_bytes(h, B, T))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    c32 = torch.empty((nq, B, T), dtype=torch.int32, device="cuda")

    embeds = [layer._codebook.embed for layer in vq.layers]
    halves = [(0.5 * (e.double() ** 2).sum(1)).float() for e in embeds]

    def torch_encode():
        r = x.transpose(1, 2).reshape(B * T, D)
        zt, out = None, []
        for e, hh in zip(embeds, halves):
            c = torch.argmax(r @ e.T - hh, dim=1)
            q = e.index_select(0, c)
            r = r - q
            zt = q if zt is None else zt + q
            out.append(c)
        return torch.stack(out), zt

    calls = {"fused": lambda: lib.fv_vq_encode(h, x.data_ptr(), T, None, c32.data_ptr(), z.data_ptr(), B, T, ws.data_ptr(), need, stream),
             "torch": lambda: torch_encode() and 0}
    tc = torch_encode()[0].reshape(nq, B, T)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row = dict(dim=D, codebook_size=K, num_quantizers=nq, batch=B, T=T, frames=B * T, iters=a.iters, lib=os.path.basename(_lib.LIB_PATH),
               search_kernel=_lib.last_kernel(), frames_with_other_codes=int((tc != codes).any(0).sum()),
               mfma_roof_ms=round(2.0 * B * T * K * D * nq / (cus * MFMA_F32_FLOPS_PER_CLK_CU * CLOCK_HZ) * 1e3, 5))
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
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--codebook-size", type=int, default=4096)
    ap.add_argument("--layouts", nargs="+", default=["32x12", "32x128"], help="clips x frames")
    ap.add_argument("--num-quantizers", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds each shape may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    print(f"{'B x T':>9} {'n_q':>4} {'fused ms':>10} {'torch ms':>10} {'MFMA roof':>10} {'other codes':>12}")
    for layout in a.layouts:
        for nq in a.num_quantizers:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--dim", str(a.dim),
                   "--codebook-size", str(a.codebook_size), "--layouts", layout, "--num-quantizers", str(nq), "--iters", str(a.iters),
                   "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                print(f"{layout} n_q {nq}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
                return r.returncode
            row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
            print(f"{layout:>9} {nq:>4} {row['fused_ms']:>10.4f} {row['torch_ms']:>10.4f} {row['mfma_roof_ms']:>10.4f} "
                  f"{row['frames_with_other_codes']:>12}")
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
