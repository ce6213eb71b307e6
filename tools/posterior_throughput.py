#!/usr/bin/env python
"""Time of the GPU posterior encoder's forward (vocoder_amd/csrc/wavenet.hip) next to PyTorch-ROCm eager running the same arithmetic on the
same tensors: the default config (513 -> 192 -> 512, k 5, 16 layers, vqvae) at (B, T) = (1, 12), (32, 12), (32, 86) and (1, 4096).

    python tools/posterior_throughput.py [--layouts 1x12 32x12 32x86 1x4096] [--iters 50] [--warmup 5] [--out rows.jsonl]

Each layout is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started after
it).  The child warms the shape up, then times `--iters` back-to-back calls between two device events (hipEvents) for

    fused   fv_posterior_forward on fixed buffers through the C entry point: pre, (gate, res_skip) x n_layers, proj = 2 n_layers + 2 launches
    torch   the formulas of include/fishvoc.h written out in torch.nn.functional with folded weights: F.conv1d and the elementwise steps of
            posterior_encoder.py:57-80,133-160 — pre and its mask, zeros_like, per layer two convs, tanh, sigmoid, mul and the add / mask / add
            of res and skip (one add in the last layer), mask, proj, mask: 8 n_layers + 4 torch calls, each at least one launch (marked *);
            --count-launches counts the device kernels with torch.profiler instead

and reports max |fused - torch| over the peak.  Beside each time: the matrix roof, 2 B T (C in + n_layers 2C C k + (2 n_layers - 1) C C +
out C) flops over CUs * 256 flops per clock (v_mfma_f32_32x32x2_f32) at 2.4 GHz.  FV_LIB_PATH selects another build of the library.  No
speed target is attached to these numbers.
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
    import numpy as np
    import torch
    import torch.nn.functional as F
    from vocoder_amd import _lib
    from vocoder_amd import synthetic as syn
    from vocoder_amd.modules.encoders import PosteriorEncoder
    assert torch.cuda.is_available(), "posterior_throughput.py needs an MI355X"
    cfg = dict(syn.POSTERIOR_DEFAULT)
    B, T = (int(v) for v in a.layouts[0].split("x"))
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in syn.posterior_state_dict(cfg, 0).items()}
    m = PosteriorEncoder(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.eval().cuda()
    C, nl, k, O = cfg["hidden_channels"], cfg["n_layers"], cfg["kernel_size"], cfg["out_channels"]
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, cfg["in_channels"], T)).astype(np.float32)).cuda()
    y = m(x)
    lib, stream = _lib.lib(), int(torch.cuda.current_stream().cuda_stream)
    h = m.engine(x.device).handle
    need = int(lib.fv_posterior_workspace_bytes(h, B, T))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")

    def fold(prefix):
        g, v = sd[f"{prefix}.weight_g"].double(), sd[f"{prefix}.weight_v"].double()
        return (g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)).float().cuda()

    w_in = [(fold(f"enc.in_layers.{i}"), sd[f"enc.in_layers.{i}.bias"].cuda()) for i in range(nl)]
    w_rs = [(fold(f"enc.res_skip_layers.{i}"), sd[f"enc.res_skip_layers.{i}.bias"].cuda()) for i in range(nl)]
    pre_w, pre_b, proj_w, proj_b = (sd[n].cuda() for n in ("pre.weight", "pre.bias", "proj.weight", "proj.bias"))
    mask = torch.ones(B, 1, T, device="cuda")

    def torch_forward():
        hh = F.conv1d(x, pre_w, pre_b) * mask
        out = torch.zeros_like(hh)
        for i in range(nl):
            aa = F.conv1d(hh, w_in[i][0], w_in[i][1], padding=(k - 1) // 2)
            g = torch.tanh(aa[:, :C]) * torch.sigmoid(aa[:, C:])
            r = F.conv1d(g, w_rs[i][0], w_rs[i][1])
            if i < nl - 1:
                hh = (hh + r[:, :C]) * mask
                out = out + r[:, C:]
            else:
                out = out + r
        return F.conv1d(out * mask, proj_w, proj_b) * mask

    yt = torch_forward()
    torch_launches = None
    if a.count_launches:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            torch_forward()
            torch.cuda.synchronize()
        torch_launches = sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "Memcpy" not in e.key
                             and str(e.device_type).endswith("CUDA"))
    calls = {"fused": lambda: lib.fv_posterior_forward(h, x.data_ptr(), T, None, y.data_ptr(), None, None, B, T, ws.data_ptr(), need, stream),
             "torch": lambda: torch_forward() is None}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    flops = 2.0 * B * T * (C * cfg["in_channels"] + nl * 2 * C * C * k + (2 * nl - 1) * C * C + O * C)
    row = dict(batch=B, T=T, iters=a.iters, lib=os.path.basename(_lib.LIB_PATH), kernel=_lib.last_kernel(), fused_launches=2 * nl + 2,
               torch_launches=torch_launches if torch_launches is not None else 8 * nl + 4,
               torch_launches_counted=torch_launches is not None,
               max_rel_diff=float((y - yt).abs().max() / yt.abs().max()),
               mfma_roof_ms=round(flops / (cus * MFMA_F32_FLOPS_PER_CLK_CU * CLOCK_HZ) * 1e3, 5))
    for name, call in calls.items():
        for _ in range(a.warmup):
            _lib.check(int(call()))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        status = 0
        for _ in range(a.iters):
            status |= int(call())
        e1.record()
        torch.cuda.synchronize()
        _lib.check(status)
        row[name + "_ms"] = round(e0.elapsed_time(e1) / a.iters, 5)
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layouts", nargs="+", default=["1x12", "32x12", "32x86", "1x4096"], help="rows x frames")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds each layout may take")
    ap.add_argument("--count-launches", action="store_true", help="count the eager side's kernel launches with torch.profiler")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    print(f"{'B x T':>9} {'fused ms':>10} {'torch ms':>10} {'MFMA roof':>10} {'launches':>9} {'torch':>6} {'max rel diff':>13}")
    for layout in a.layouts:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--layouts", layout,
               "--iters", str(a.iters), "--warmup", str(a.warmup)] + (["--count-launches"] if a.count_launches else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"{layout}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        print(f"{layout:>9} {row['fused_ms']:>10.4f} {row['torch_ms']:>10.4f} {row['mfma_roof_ms']:>10.4f} {row['fused_launches']:>9} "
              f"{row['torch_launches']:>6}{'' if row['torch_launches_counted'] else '*'} {row['max_rel_diff']:>13.2e}")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
