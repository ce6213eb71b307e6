#!/usr/bin/env python
"""What RefineGAN's AdaIN noise costs in its two forms (vocoder_amd/csrc/small_kernels.hip adain_kernel / adain_seeded_kernel): the default
config (synthetic.REFINEGAN_44K) on 32 clips x 86 frames and on 1 x 86.

    python tools/refinegan_noise_throughput.py [--batch 32 1] [--frames 86] [--iters 20] [--rounds 5] [--warmup 3]

Each batch size is timed in a child process of its own under `timeout` (a fault or a hang in one ends that step, and nothing is started after
it).  The child warms every shape up, then times, between two device events (hipEvents), `--rounds` alternating rounds of `--iters` calls of

    explicit   torch.randn(noise_elems) + the explicit-noise forward (fv_forward_refinegan): what RefineGANGenerator.forward costs without a seed
    seeded     the seeded forward (fv_forward_refinegan_seeded): no noise tensor

and reports each one's median and minimum round, and the peak device memory torch allocated for it (inputs and the engine's workspace
included).  Then, from the engine's per-launch profile (hipEvents around every launch, one stream), the AdaIN launches alone in both forms:
`adain` (12 / 16 bytes per element) and `adain_seeded` (8 / 12 bytes per element, plus one Philox4x32-10 and two Box-Muller pairs per four
elements), beside the time their bytes would take at 8 TB/s.  Last, a steady-state seeded stream push of `--chunk` frames (the window is
context + lookahead + chunk frames; the push runs eagerly: its window's origin is a kernel scalar, so no captured graph fits the next push).
FV_LIB_PATH selects another build of the library.  Writes the rows as JSON lines to --out when given.  No speed target is attached to these
numbers.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HBM_BYTES_PER_S = 8e12


def _profile(eng, run, repeats: int) -> dict:
    from vocoder_amd._lib import check
    import torch
    check(eng._lib.fv_profile_begin(eng._h))
    for _ in range(repeats):
        run()
    torch.cuda.synchronize()
    need = ctypes.c_size_t(0)
    buf = ctypes.create_string_buffer(1 << 20)
    check(eng._lib.fv_profile_end(eng._h, buf, len(buf), ctypes.byref(need)))
    return {r["kernel"]: r for r in json.loads(buf.value.decode())}


def child(a) -> None:
    import torch
    from vocoder_amd import _lib, synthetic as syn
    from vocoder_amd.engine import Engine, refinegan_config
    assert torch.cuda.is_available(), "refinegan_noise_throughput.py needs an MI355X"
    cfg, B, T = dict(syn.REFINEGAN_44K), a.batch[0], a.frames
    dev = torch.device("cuda:0")
    eng = Engine(_lib.FV_MODEL_REFINEGAN, refine=refinegan_config(**cfg), state_dict=syn.refinegan_state_dict(cfg, 1))
    mel = torch.from_numpy(syn.synthetic_mel(B, cfg["num_mels"], T, seed=2)).to(dev)
    tmpl = torch.from_numpy(syn.synthetic_template(B, T, cfg["hop_length"], seed=3)).to(dev)
    out = torch.empty((B, 1, eng.output_length(T)), dtype=torch.float32, device=dev)
    n_noise = eng.noise_elems(B, T)
    eng.set_noise_seed(1234)

    def explicit():
        eng.forward(mel, out, tmpl, torch.randn(n_noise, dtype=torch.float32, device=dev))

    def seeded():
        eng.forward(mel, out, tmpl)
    forms = {"explicit": explicit, "seeded": seeded}
    row = dict(batch=B, frames=T, noise_elems=n_noise, noise_bytes=4 * n_noise, reach_frames=eng.reach_frames, iters=a.iters, rounds=a.rounds,
               lib=os.path.basename(_lib.LIB_PATH))
    base = torch.cuda.memory_allocated(dev)
    for name, call in forms.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        row[name + "_peak_bytes"] = int(torch.cuda.max_memory_allocated(dev))
    row["resident_before_bytes"] = int(base)
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, call in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                call()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    for name, ts in times.items():
        row[name + "_ms"] = round(statistics.median(ts), 4)
        row[name + "_min_ms"] = round(min(ts), 4)
    # the AdaIN launches alone, per forward, from the per-launch profile
    noise = torch.randn(n_noise, dtype=torch.float32, device=dev)
    for label, run in (("adain", lambda: eng.forward(mel, out, tmpl, noise)), ("adain_seeded", seeded)):
        p = _profile(eng, run, a.profile_repeats)[label]
        row[label + "_ms_per_forward"] = round(p["total_ms"] / a.profile_repeats, 4)
        row[label + "_launches_per_forward"] = p["launches"] // a.profile_repeats
        row[label + "_hbm_roof_ms_per_forward"] = round(p["bytes_per_launch"] * p["launches"] / a.profile_repeats / HBM_BYTES_PER_S * 1e3, 4)
    del noise
    # a steady-state seeded stream push
    n = a.chunk
    st = eng.stream(B, n)
    chunk_mel, chunk_tmpl = mel[:, :, :n].contiguous(), tmpl[:, :, :n * st.hop].contiguous()
    fill = (st.context_frames + st.lookahead_frames) // n + 2 + a.warmup      # pushes until the window has its steady length
    for _ in range(fill):
        st.push(chunk_mel, chunk_tmpl)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            st.push(chunk_mel, chunk_tmpl)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / a.iters)
    row.update(push_chunk_frames=n, push_window_frames=st.context_frames + st.lookahead_frames + n, push_ms=round(statistics.median(ts), 4),
               push_min_ms=round(min(ts), 4))
    st.close()
    eng.close()
    print("RESULT " + json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 1])
    ap.add_argument("--frames", type=int, default=86)
    ap.add_argument("--chunk", type=int, default=8, help="frames per stream push")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-repeats", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each batch size may take")
    ap.add_argument("--out", default=None, help="append the rows as JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    print(f"{'B x T':>8} {'explicit ms':>12} {'seeded ms':>10} {'peak MB':>16} {'adain ms':>9} {'seeded ms':>10} {'roofs ms':>14} {'push ms':>8}")
    for batch in a.batch:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--batch", str(batch),
               "--frames", str(a.frames), "--chunk", str(a.chunk), "--iters", str(a.iters), "--rounds", str(a.rounds), "--warmup", str(a.warmup),
               "--profile-repeats", str(a.profile_repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"{batch} x {a.frames}: the step ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        row = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        print(f"{batch:>3} x {a.frames:<3} {row['explicit_ms']:>12.4f} {row['seeded_ms']:>10.4f} "
              f"{row['explicit_peak_bytes'] / 1e6:>7.1f} /{row['seeded_peak_bytes'] / 1e6:>7.1f} {row['adain_ms_per_forward']:>9.4f} "
              f"{row['adain_seeded_ms_per_forward']:>10.4f} {row['adain_hbm_roof_ms_per_forward']:>6.4f} /{row['adain_seeded_hbm_roof_ms_per_forward']:>6.4f} "
              f"{row['push_ms']:>8.4f}")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
