#!/usr/bin/env python
"""Time of MMSEncoder's two kernels (vocoder_amd/csrc/mms_front.hip) and of the whole chain, next to the same chain with the two steps done
in torch eager on the device: mms-300m's shape (hidden 1024, 24 layers, 16 heads, the seven default conv layers at 512 channels), synthetic
weights, 44100 Hz in, hop 512, on 1 x 1 s, 8 x 10 s and 1 x 30 s of audio, fp32.

    python tools/mms_throughput.py [--layouts 1x1 8x10 1x30] [--iters 10] [--warmup 3] [--out rows.jsonl]

Each layout is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started after
it).  The child warms every call up, then takes the median of `--iters` windows, each between two device events (hipEvents); a window
of one of the two small kernels holds `--reps` calls, so that it is not the events that are timed.

    normalize      fv_mms_normalize on the resampled batch (B, M)             eager: (x - mean) / sqrt(var + 1e-7) per row, torch ops
    interpolate    fv_mms_interpolate, (B, F, 1024) -> (B, 1024, N)            eager: F.interpolate(h.transpose(1, 2), size=N, mode="nearest")
    backbone       fv_w2v_forward alone (post_channels = 0), for its share of the chain
    chain          MMSEncoder.forward: Resample -> normalize -> backbone -> interpolate, all on the library
    chain_eager    the same resampler and backbone with the two steps in torch eager between and after them

Bytes per call are the compulsory ones (normalize: the rows read twice and written once; interpolate: every source frame read once, every
output written once) and give the GB/s beside each kernel time.  The eager and library results are compared: the interpolation bit for bit,
the normalisation and the chain by max |d| over the peak.  No speed target is attached to these numbers.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

RATE_IN, HOP = 44100, 512
LARGE = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, conv_dim=[512] * 7,
             conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
             feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, feat_proj_layer_norm=True)


def child(a) -> None:
    import ctypes

    import numpy as np
    import torch

    from vocoder_amd import _lib
    from vocoder_amd import synthetic as syn
    from vocoder_amd.modules.encoders import MMSEncoder
    assert torch.cuda.is_available(), "mms_throughput.py needs an MI355X"
    B, secs = (int(v) for v in a.layouts[0].split("x"))
    L = secs * RATE_IN
    m = MMSEncoder(sampling_rate=RATE_IN, hop_length=HOP, config=LARGE)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in syn.mms_state_dict(LARGE, 0).items()}, strict=True)
    m = m.eval().cuda()
    H, N, F = LARGE["hidden_size"], m.frames(L), m.backbone_frames(L)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, L)).astype(np.float32)).cuda()
    lib, stream = _lib.lib(), int(torch.cuda.current_stream().cuda_stream)
    wave = m.resample(x)
    M = int(wave.shape[1])
    eng = m.engine(x.device)

    values, hidden, out = torch.empty_like(wave), torch.empty((B, F, H), device="cuda"), torch.empty((B, H, N), device="cuda")
    nws = torch.empty(max(int(lib.fv_mms_normalize_workspace_bytes(B, M)), 16), dtype=torch.uint8, device="cuda")
    need = int(lib.fv_w2v_workspace_bytes(eng.handle, B, M))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def normalize():
        _lib.check(lib.fv_mms_normalize(wave.data_ptr(), M, None, B, values.data_ptr(), nws.data_ptr(), nws.numel(), stream))

    def backbone(src=None):
        src = values if src is None else src
        _lib.check(lib.fv_w2v_forward(eng.handle, src.data_ptr(), M, None, B, hidden.data_ptr(), None, ws.data_ptr(), need, stream))

    def interpolate():
        _lib.check(lib.fv_mms_interpolate(hidden.data_ptr(), F, H, None, None, B, out.data_ptr(), N, stream))

    def normalize_eager(w=None):
        w = wave if w is None else w
        return (w - w.mean(1, keepdim=True)) / torch.sqrt(w.var(1, unbiased=False, keepdim=True) + 1e-7)

    def interpolate_eager():
        return torch.nn.functional.interpolate(hidden.transpose(1, 2), size=N, mode="nearest")

    def chain():
        return m(x)

    def chain_eager():
        backbone(normalize_eager(m.resample(x)).contiguous())
        return interpolate_eager()

    def timed(call, reps):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / reps)
        return dict(ms=round(statistics.median(times), 5), ms_min_max=[round(min(times), 5), round(max(times), 5)])

    with torch.no_grad():
        normalize()
        backbone()
        interpolate()
        torch.cuda.synchronize()
        ne, ie = normalize_eager(), interpolate_eager()
        ce, co = chain_eager(), chain()
        row = dict(batch=B, seconds=secs, samples=L, samples_16k=M, frames=F, out_frames=N, iters=a.iters, reps=a.reps,
                   lib=os.path.basename(_lib.LIB_PATH),
                   normalize_max_rel_diff=float((values - ne).abs().max() / ne.abs().max()),
                   interpolate_bit_equal=bool(torch.equal(out.view(torch.int32), ie.contiguous().view(torch.int32))),
                   chain_max_rel_diff=float((co - ce).abs().max() / ce.abs().max()))
        for name, call, reps in (("normalize", normalize, a.reps), ("normalize_eager", normalize_eager, a.reps),
                                 ("interpolate", interpolate, a.reps), ("interpolate_eager", interpolate_eager, a.reps),
                                 ("backbone", backbone, 1), ("chain", chain, 1), ("chain_eager", chain_eager, 1)):
            row[name] = timed(call, reps)
    row["normalize"]["bytes"] = 3 * B * M * 4
    row["interpolate"]["bytes"] = (B * F * H + B * H * N) * 4
    for key in ("normalize", "interpolate"):
        row[key]["gbytes_per_s"] = round(row[key]["bytes"] / (row[key]["ms"] * 1e-3) / 1e9, 1)
    row["backbone_share_of_chain"] = round(row["backbone"]["ms"] / row["chain"]["ms"], 4)
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layouts", nargs="+", default=["1x1", "8x10", "1x30"], help="rows x seconds of 44.1 kHz audio")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="calls of a small kernel per timed window")
    ap.add_argument("--step-timeout", type=int, default=280, help="seconds each layout may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    print(f"{'B x s':>6} {'F':>5} {'N':>5} | {'normalize':>10} {'eager':>9} {'GB/s':>7} | {'interp':>9} {'eager':>9} {'GB/s':>7} | "
          f"{'chain':>9} {'eager':>9} {'backbone':>9} {'share':>6}   (ms)")
    for layout in a.layouts:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--layouts", layout,
               "--iters", str(a.iters), "--warmup", str(a.warmup), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            print(f"{layout}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        t = lambda k: row[k]["ms"]      # noqa: E731
        print(f"{layout:>6} {row['frames']:>5} {row['out_frames']:>5} | {t('normalize'):>10.4f} {t('normalize_eager'):>9.4f} "
              f"{row['normalize']['gbytes_per_s']:>7.1f} | {t('interpolate'):>9.4f} {t('interpolate_eager'):>9.4f} "
              f"{row['interpolate']['gbytes_per_s']:>7.1f} | {t('chain'):>9.3f} {t('chain_eager'):>9.3f} {t('backbone'):>9.3f} "
              f"{100 * row['backbone_share_of_chain']:>5.1f}%")
        print(f"       normalize vs eager max |d| / peak = {row['normalize_max_rel_diff']:.2e}; interpolate bit-equal to eager: "
              f"{row['interpolate_bit_equal']}; chain vs eager chain max |d| / peak = {row['chain_max_rel_diff']:.2e}")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
