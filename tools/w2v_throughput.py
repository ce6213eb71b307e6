#!/usr/bin/env python
"""Time of the GPU wav2vec2 / HuBERT backbone (vocoder_amd/csrc/w2v.hip) next to HF's ``HubertModel`` on PyTorch-ROCm with the same synthetic
weights: the large config (hidden 1024, 24 layers, 16 heads, the seven default conv layers at 512 channels) on 1 x 1 s, 8 x 10 s and 1 x 30 s
of 16 kHz audio, fp32.

    python tools/w2v_throughput.py [--layouts 1x1 8x10 1x30] [--iters 10] [--warmup 3] [--out rows.jsonl]

Each layout is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started after
it).  The child warms the shape up, then takes the median of `--iters` calls, each between two device events (hipEvents), for

    ours    fv_w2v_forward with post_channels = 0 (last_hidden_state) on fixed buffers through the C entry point
    hf      HubertModel(HubertConfig(...)) in eval mode under torch.no_grad, fp32, its default attention — only where `transformers` imports;
            otherwise there is no comparison and the row says so.  Nothing is downloaded (HF_HUB_OFFLINE, a config built in place).

and reports max |ours - hf| over the peak.  One more call of ours runs under torch.profiler, which gives every kernel's share of the forward
and, with the algorithmic flops of the launches behind each name, the fraction of the fp32 MFMA peak (CUs * 256 flops per clock of
v_mfma_f32_32x32x2_f32 at 2.4 GHz) that each GEMM instance and the attention reach.  No speed target is attached to these numbers.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CLOCK_HZ, MFMA_F32_FLOPS_PER_CLK_CU, RATE = 2.4e9, 256, 16000
LARGE = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, conv_dim=[512] * 7,
             conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
             feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, feat_proj_layer_norm=True)
# w2v_gemm_kernel's epilogue instances (the template argument in the kernel's name)
EPI = {0: "conv, projection, q|k|v", 1: "FFN in + GELU", 2: "post + SiLU", 3: "out_proj, FFN out + residual", 4: "pos conv + GELU + residual", 5: "post, channel major"}


def gemm_flops(cfg, B, frames):
    """Algorithmic flops behind each kernel name of one backbone forward; frames[l + 1] after conv layer l."""
    H, I, nl, F = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], frames[-1]
    conv = sum(2.0 * B * frames[l + 1] * c * k * (cfg["conv_dim"][l - 1] if l else 1)
               for l, (c, k) in enumerate(zip(cfg["conv_dim"], cfg["conv_kernel"])))
    bias = conv + 2.0 * B * F * H * cfg["conv_dim"][-1] + nl * 2.0 * B * F * 3 * H * H
    return {"gemm<0>": bias, "gemm<1>": nl * 2.0 * B * F * I * H, "gemm<3>": nl * 2.0 * B * F * (H * H + H * I),
            "gemm<4>": 2.0 * B * F * H * (H // cfg["num_conv_pos_embedding_groups"]) * cfg["num_conv_pos_embeddings"],
            "attn": nl * 4.0 * B * F * F * H}


def child(a) -> None:
    import numpy as np
    import torch
    from torch.profiler import ProfilerActivity, profile

    from vocoder_amd import _lib
    from vocoder_amd import synthetic as syn
    assert torch.cuda.is_available(), "w2v_throughput.py needs an MI355X"
    B, secs = (int(v) for v in a.layouts[0].split("x"))
    T = secs * RATE
    cfg = dict(LARGE, output_size=4)
    sd = syn.hubert_state_dict(cfg, 0)
    frames = [T]
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        frames.append((frames[-1] - k) // s + 1)
    F, H = frames[-1], cfg["hidden_size"]

    # ours, the backbone alone, through the C entry point
    lib = _lib.lib()
    import ctypes
    arr = ctypes.c_int32 * _lib.W2V_MAX_CONV
    c = _lib.W2VConfig(H, cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["intermediate_size"], 7, arr(*cfg["conv_dim"], 0),
                       arr(*cfg["conv_kernel"], 0), arr(*cfg["conv_stride"], 0), cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"], 0)
    h = ctypes.c_void_p()
    _lib.check(lib.fv_w2v_create(ctypes.byref(c), ctypes.byref(h)))
    for k, v in sd.items():
        if k.startswith("post."):
            continue
        arr = np.ascontiguousarray(v, np.float32)
        _lib.check(lib.fv_w2v_load_weight(h, k.encode(), arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), (ctypes.c_int64 * max(arr.ndim, 1))(*arr.shape), arr.ndim))
    _lib.check(lib.fv_w2v_finalize(h))
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, T)).astype(np.float32)).cuda()
    y = torch.empty((B, F, H), device="cuda")
    need = int(lib.fv_w2v_workspace_bytes(h, B, T))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)
    calls = {"ours": lambda: _lib.check(lib.fv_w2v_forward(h, x.data_ptr(), T, None, B, y.data_ptr(), None, ws.data_ptr(), need, stream))}

    hf, hf_note = None, None
    try:
        from transformers import HubertConfig, HubertModel
        hf = HubertModel(HubertConfig(**LARGE))
        res = hf.load_state_dict({k[len("model."):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items() if k.startswith("model.")}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        hf = hf.eval().cuda()
        yh = [None]

        def hf_call():
            with torch.no_grad():
                yh[0] = hf(x).last_hidden_state
        calls["hf"] = hf_call
    except ImportError as exc:
        hf_note = f"transformers does not import here ({exc}): ours is timed against nothing"

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    peak = cus * MFMA_F32_FLOPS_PER_CLK_CU * CLOCK_HZ
    row = dict(batch=B, seconds=secs, frames=F, iters=a.iters, lib=os.path.basename(_lib.LIB_PATH), hf=hf_note or "HubertModel, fp32, default attention")
    for name, call in calls.items():
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        row[name + "_ms"] = round(statistics.median(times), 4)
        row[name + "_ms_min_max"] = [round(min(times), 4), round(max(times), 4)]
    if hf is not None:
        row["max_rel_diff"] = float((y - yh[0]).abs().max() / yh[0].abs().max())

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        calls["ours"]()
        torch.cuda.synchronize()
    flops = gemm_flops(cfg, B, frames)
    total_flops = sum(flops.values())
    row["mfma_roof_ms"] = round(total_flops / peak * 1e3, 4)
    shares, total_us = {}, 0.0
    for e in prof.key_averages():
        if "w2v_" not in e.key:
            continue
        key = e.key.split("w2v_")[1].split("(")[0]
        epi = re.match(r"gemm_kernel<(\d+)", key)
        key = f"gemm<{epi.group(1)}>" if epi else key
        key = "attn" if key.startswith("attn") else "ln" if key.startswith("ln") else key
        us = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
        ent = shares.setdefault(key, dict(us=0.0, launches=0))
        ent["us"] += us
        ent["launches"] += e.count
        total_us += us
    for key, ent in shares.items():
        ent["share"] = round(ent["us"] / max(total_us, 1e-9), 4)
        ent["us"] = round(ent["us"], 1)
        if key in flops and ent["us"] > 0:
            ent["mfma_peak_fraction"] = round(flops[key] / (ent["us"] * 1e-6) / peak, 4)
    row["kernels"] = shares
    lib.fv_w2v_destroy(h)
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layouts", nargs="+", default=["1x1", "8x10", "1x30"], help="rows x seconds of 16 kHz audio")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=280, help="seconds each layout may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    print(f"{'B x s':>7} {'frames':>7} {'ours ms':>10} {'hf ms':>10} {'MFMA roof':>10} {'max rel diff':>13}")
    for layout in a.layouts:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--layouts", layout,
               "--iters", str(a.iters), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            print(f"{layout}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        hf_ms = f"{row['hf_ms']:>10.3f}" if "hf_ms" in row else f"{'-':>10}"
        diff = f"{row['max_rel_diff']:>13.2e}" if "max_rel_diff" in row else f"{'-':>13}"
        print(f"{layout:>7} {row['frames']:>7} {row['ours_ms']:>10.3f} {hf_ms} {row['mfma_roof_ms']:>10.3f} {diff}")
        for key, ent in sorted(row["kernels"].items(), key=lambda kv: -kv[1]["us"]):
            what = EPI.get(int(key[5]), "") if key.startswith("gemm<") else ""
            frac = f"  {100 * ent['mfma_peak_fraction']:.1f} % of the fp32 MFMA peak" if "mfma_peak_fraction" in ent else ""
            print(f"          {key:<10} {100 * ent['share']:5.1f} %  {ent['us'] / 1e3:9.3f} ms  {ent['launches']:4d} launches{frac}  {what}")
        if "hf_ms" not in row:
            print(f"          {row['hf']}")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
