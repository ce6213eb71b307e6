#!/usr/bin/env python
"""What a session pool (Engine.session_pool) costs in lockstep, and what it saves when sessions advance independently.

HiFiGAN-V1 44.1 kHz with synthetic weights and mel (as bench.py), n = 8 frames per chunk, K = A = the reach.  ms by hipEvents on the launch
stream, one synchronised call at a time; both sides of every comparison run interleaved in ONE process, after a warm-up in which every side
has reached its steady window and captured its graph.

(a) Lockstep overhead, S in {1, 32}: a pool step in which every session gets n frames (SessionPool.step_padded, and the bare fv_pool_step
    call under it) against Stream.push at batch S and Engine.forward over the same (S, C, K + A + n) window.
(b) Independent sessions, S in {8, 32}: utterances of 1 - 10 s (86 - 860 frames, drawn as tools/ragged_throughput.py draws them) whose
    starts are spread over one window cycle (the ceil((K + A + n) / n) steps a window takes to settle), every live session receiving n
    frames per step and flushing with its last chunk.  One pool serves them all, against a loop over S Stream(batch=1) objects — the only
    way to serve them without the pool.  Audio-seconds per wall-second, p50 / p90 per step.

    python tools/pool_throughput.py [--rounds 3] [--seconds 1.5] [--out profiles/r11_pool_throughput.txt]
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from vocoder_amd import _lib, synthetic as syn  # noqa: E402
from vocoder_amd.engine import Engine, upsampler_config  # noqa: E402

N = 8
HOP, SR = 512, 44100


def _ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def lockstep(eng, S, seconds):
    R = eng.reach_frames
    W = 2 * R + N
    chunk = torch.from_numpy(syn.synthetic_mel(S, eng.in_channels, N, seed=N)).cuda()
    clip = torch.from_numpy(syn.synthetic_mel(S, eng.in_channels, W, seed=W)).cuda()
    out_f = torch.empty((S, 1, W * HOP), device="cuda")
    out_p = torch.empty((S, 1, N * HOP), device="cuda")
    out_r = torch.empty((S, 1, N * HOP), device="cuda")
    items = [(s, N, False) for s in range(S)]
    arr = (_lib.PoolItem * S)(*[_lib.PoolItem(s, N, 0) for s in range(S)])
    st, pool, raw = eng.stream(S, N), eng.session_pool(S, N), eng.session_pool(S, N)
    L = eng._lib

    def run_raw():
        _lib.check(L.fv_pool_step(raw._h, arr, S, chunk.data_ptr(), None, N, out_r.data_ptr(), N, None, raw._ws.data_ptr(), raw._ws.numel() * 4, None))

    fns = {"forward": lambda: eng.forward(clip, out_f), "push": lambda: st.push(chunk), "step": lambda: pool.step_padded(items, chunk, None, out_p),
           "fv_pool_step": run_raw}
    for f in fns.values():                  # each side on its own until its window has settled and its graph replays
        for _ in range(-(-2 * R // N) + 6):
            f()
    torch.cuda.synchronize()
    assert st.pending_frames == R == pool.pending_frames(0) == raw.pending_frames(S - 1)
    ms = {k: [] for k in fns}
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(ms["step"]) < 50:
        for k, f in fns.items():
            ms[k].append(_ms(f))
    assert eng.graph_replay
    for h in (st, pool, raw):
        h.close()
    p = {k: (float(np.percentile(v, 50)), float(np.percentile(v, 90))) for k, v in ms.items()}
    return (f"lockstep S={S:<3d} n={N} W={W}: forward p50 {p['forward'][0]:.3f} ms | Stream.push p50 {p['push'][0]:.3f} p90 {p['push'][1]:.3f} "
            f"(gap {p['push'][0] - p['forward'][0]:+.3f}) | pool step p50 {p['step'][0]:.3f} p90 {p['step'][1]:.3f} (gap {p['step'][0] - p['forward'][0]:+.3f} "
            f"over forward, {p['step'][0] - p['push'][0]:+.3f} over push) | bare fv_pool_step p50 {p['fv_pool_step'][0]:.3f} "
            f"(gap {p['fv_pool_step'][0] - p['forward'][0]:+.3f} over forward) | {len(ms['step'])} rounds")


def independent(eng, S, seed, rounds):
    R = eng.reach_frames
    cycle = -(-(2 * R + N) // N)
    rng = random.Random(seed)
    lengths = [rng.randint(86, 860) for _ in range(S)]
    starts = [s * cycle // S for s in range(S)]
    mel = torch.from_numpy(syn.synthetic_mel(S, eng.in_channels, max(lengths), seed=seed)).cuda()
    # per step: the live sessions, their chunk sizes, and the chunks as they would arrive — one padded buffer for the pool, one (1, C, n) each
    # for the streams — staged before the clock starts
    steps = []
    t = 0
    while True:
        live = [(s, (t - starts[s]) * N) for s in range(S) if t >= starts[s] and (t - starts[s]) * N < lengths[s]]
        if not live and t > max(starts):
            break
        items = [(s, min(N, lengths[s] - f), f + N >= lengths[s]) for s, f in live]
        pad = torch.zeros((len(items), eng.in_channels, N), device="cuda")
        singles = []
        for i, ((s, f), (_, n, _)) in enumerate(zip(live, items)):
            pad[i, :, :n] = mel[s, :, f:f + n]
            singles.append(mel[s:s + 1, :, f:f + n].contiguous())
        steps.append((items, pad, singles))
        t += 1
    audio = sum(lengths) * HOP / SR
    out = torch.empty((S, 1, (N + R) * HOP), device="cuda")     # a last chunk emits its n frames and the A = R pending ones

    def serve_pool():
        ms = []
        with eng.session_pool(S, N) as pool:
            t0 = time.perf_counter()
            for items, pad, _ in steps:
                if items:
                    ms.append(_ms(lambda: pool.step_padded(items, pad, None, out[:len(items)])))
            torch.cuda.synchronize()
            return time.perf_counter() - t0, ms

    def serve_streams():
        ms = []
        sts = [eng.stream(1, N) for _ in range(S)]
        t0 = time.perf_counter()
        for items, _, singles in steps:
            if not items:
                continue

            def one_step():
                for (s, n, fl), c in zip(items, singles):
                    sts[s].push(c)
                    if fl:
                        sts[s].flush()
            ms.append(_ms(one_step))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        for st in sts:
            st.close()
        return wall, ms

    serve_pool(), serve_streams()            # warm-up of every window length either side forms
    res = {"pool": [], "streams": []}
    for _ in range(rounds):
        res["pool"].append(serve_pool())
        res["streams"].append(serve_streams())
    line = f"independent S={S:<3d} n={N} seed {seed}: {sum(lengths)} frames = {audio:.1f} s of audio in {sum(1 for s in steps if s[0])} steps"
    med = {}
    for k, v in res.items():
        wall = float(np.median([w for w, _ in v]))
        ms = np.concatenate([m for _, m in v])
        med[k] = wall
        line += f" | {k}: {audio / wall:7.1f} audio-s per wall-s (wall {wall * 1e3:.1f} ms), step p50 {np.percentile(ms, 50):.3f} p90 {np.percentile(ms, 90):.3f} ms"
    return line + f" | pool {med['streams'] / med['pool']:.2f}x the loop of streams"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r11_pool_throughput.txt"))
    a = ap.parse_args()
    cfg = dict(syn.HIFIGAN_V1_44K)
    eng = Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**cfg), state_dict=syn.hifigan_state_dict(cfg, 0))
    lines = [f"# tools/pool_throughput.py --rounds {a.rounds} --seconds {a.seconds}: {torch.cuda.get_device_name(0)}; HiFiGAN-V1 44.1 kHz, "
             f"R = K = A = {eng.reach_frames} frames, n = {N}; ms per call by hipEvents, one synchronised call at a time, the sides of each line "
             "interleaved in one process after a warm-up (windows settled, graphs replaying)"]
    for S in (1, 32):
        lines.append(lockstep(eng, S, a.seconds))
        print(lines[-1], flush=True)
    for S in (8, 32):
        lines.append(independent(eng, S, 0, a.rounds))
        print(lines[-1], flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
