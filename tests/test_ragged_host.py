"""CPU: the plan of a ragged batch (vocoder_amd.ragged) — coverage, the reach rule at every window edge, grouping, optimality of the
dynamic programme against brute force, the frame-count conditions of the seeded 1 - 10 s sets, and refusals."""
import itertools
import random

import pytest

from vocoder_amd import ragged
from vocoder_amd.ragged import Window, body_runs, computed_frames, groups, plan, run_cost


def _check_plan(lengths, R, windows):
    by_clip = {}
    for w in windows:
        by_clip.setdefault(w.clip, []).append(w)
    frames_of_group = {}
    for w in windows:
        assert frames_of_group.setdefault(w.group, w.frames) == w.frames          # one length per group
    for b, T in enumerate(lengths):
        ws = by_clip.get(b, [])
        if T == 0:
            assert ws == []
            continue
        kept = [0] * T
        for w in ws:
            a, n, lo, hi = w.start, w.frames, w.keep_lo, w.keep_hi
            assert 0 <= a and n >= 1 and a < T
            right = min(a + n, T)                     # the zero fill past T inside a longer window is not the clip's end ...
            assert a <= lo < hi <= right              # keep lies inside the window (and inside the clip)
            if a > 0:
                assert lo - a >= R                    # left edge is not the clip's own
            if not (a + n == T):                      # ... so only a window that ends exactly at T has the clip's own right edge
                assert right - hi >= R
            for f in range(lo, hi):
                kept[f] += 1
        assert kept == [1] * T, (b, T, ws)            # every frame kept by exactly one window


@pytest.mark.parametrize("seed", range(240))
def test_plan_properties_over_random_length_sets(seed):
    rng = random.Random(5000 + seed)
    R = rng.choice([1, 17, 115])
    B = rng.randint(1, 64)
    hi = rng.choice([3 * R + 5, 300, 900])
    lengths = [rng.choice([0, rng.randint(0, hi), rng.randint(0, 900), 2 * R, 2 * R + 1]) for _ in range(B)]
    lf = rng.choice([0, 1, 64, 192, 1000])
    mg = rng.choice([0, 1, 2, 8, 64])
    windows = plan(lengths, R, lf, mg)
    _check_plan(lengths, R, windows)
    g = groups(windows)
    assert [w.group for w in windows] == sorted(w.group for w in windows)
    assert [n for _, n in g] == sorted({w.frames for w in windows}, reverse=True)      # numbered by descending length, lengths distinct
    assert sum(1 for _, n in g if n > 2 * R) <= (mg if mg > 0 else ragged.MAX_GROUPS)
    assert sum(b for b, _ in g) == len(windows)
    assert plan(lengths, R, lf, mg) == windows                                          # deterministic


@pytest.mark.parametrize("R", [1, 17, 115])
@pytest.mark.parametrize("T", [1, 16, 34, 35, 86, 230, 231, 860])
def test_equal_lengths_plan_to_one_plain_forward(R, T):
    for B in (1, 5, 32):
        windows = plan([T] * B, R)
        assert windows == [Window(b, 0, T, 0, T, 0) for b in range(B)]
        assert groups(windows) == [(B, T)] and computed_frames(windows) == B * T


def test_window_kinds_of_one_mixed_batch():
    R = 17
    lengths = [1, R, 2 * R, 2 * R + 1, 3 * R, 97, 97, 389, 0, 200]
    windows = plan(lengths, R, launch_frames=1, max_groups=8)       # cheap launches: every long length its own body group
    assert [w for w in windows if w.clip == 8] == []
    for b in (0, 1, 2):
        assert [w[:5] for w in windows if w.clip == b] == [(b, 0, lengths[b], 0, lengths[b])]
    assert {w.frames for w in windows if lengths[w.clip] > 2 * R} == {35, 51, 97, 389, 200}
    merged = plan(lengths, R, launch_frames=10 ** 6, max_groups=8)  # dear launches: one body group of the longest clip + the tails
    body = [w for w in merged if w.frames == 389]
    assert sorted(w.clip for w in body) == [3, 4, 5, 6, 7, 9]
    for w in body:
        T = lengths[w.clip]
        assert (w.start, w.keep_lo, w.keep_hi) == (0, 0, T if T == 389 else T - R)
    tails = [w for w in merged if w.frames == 2 * R]
    assert sorted(w.clip for w in tails) == [2, 3, 4, 5, 6, 9]      # the 2R-frame clip shares the tails' group
    assert len({w.group for w in tails}) == 1
    for w in tails:
        T = lengths[w.clip]
        assert w[:5] == ((w.clip, 0, T, 0, T) if T == 2 * R else (w.clip, T - 2 * R, 2 * R, T - R, T))


def _brute_force(L, R, lf, mg):
    m = len(L)
    best = None
    for k in range(1, min(mg, m) + 1):
        for cuts in itertools.combinations(range(1, m), k - 1):
            edges = (0,) + cuts + (m,)
            c = sum(run_cost(L, edges[t], edges[t + 1], R, lf) for t in range(k))
            best = c if best is None else min(best, c)
    return best


@pytest.mark.parametrize("seed", range(120))
def test_dynamic_programme_equals_brute_force_over_all_contiguous_partitions(seed):
    rng = random.Random(9000 + seed)
    R = rng.choice([1, 17, 115])
    m = rng.randint(1, 9)
    L = sorted(rng.choice([rng.randint(2 * R + 1, 2 * R + 40), rng.randint(2 * R + 1, 900 + 2 * R)]) for _ in range(m))
    lf = rng.choice([1, 10, 192, 2000])
    mg = rng.choice([1, 2, 3, 8])
    runs = body_runs(L, R, lf, mg)
    assert runs[0][0] == 0 and runs[-1][1] == m and all(a[1] == b[0] for a, b in zip(runs, runs[1:])) and len(runs) <= mg
    cost = sum(run_cost(L, i, j, R, lf) for i, j in runs)
    assert cost == _brute_force(L, R, lf, mg), (L, R, lf, mg, runs)
    # the same through plan(): the body groups it forms have that cost
    windows = plan(L, R, lf, mg)
    got = 0
    for k, (b, n) in enumerate(groups(windows)):
        if n > 2 * R:
            got += b * n + 2 * R * sum(1 for w in windows if w.group == k and L[w.clip] < n) + lf
    assert got == cost


@pytest.mark.parametrize("seed,forwards,ratio", [(0, 9, 1.106), (1, 8, 1.131), (2, 9, 1.112), (3, 9, 1.086)])
def test_seeded_one_to_ten_second_sets_meet_the_frame_count_conditions(seed, forwards, ratio):
    """32 clips of 1 - 10 s at 44.1 kHz / hop 512 (HiFiGAN-V1: R = 17): at most 9 forwards over at most 1.20 x the useful frames, where one
    padded forward would run over at least 1.6 x."""
    rng = random.Random(seed)                       # ONE generator per set (a fresh Random(seed) per draw would give 32 equal clips)
    lengths = [rng.randint(86, 860) for _ in range(32)]
    windows = plan(lengths, 17, 192, 8)
    _check_plan(lengths, 17, windows)
    useful = sum(lengths)
    r = computed_frames(windows) / useful
    print(f"seed {seed}: {len(groups(windows))} forwards, computed / useful {r:.3f}, padded {32 * max(lengths) / useful:.3f}")
    assert len(groups(windows)) <= 9 and r <= 1.20
    assert 32 * max(lengths) / useful >= 1.6
    assert len(groups(windows)) == forwards and abs(r - ratio) < 5e-4


def test_one_second_clips_and_the_large_reach_limit():
    rng = random.Random(7)
    lengths = [rng.randint(60, 130) for _ in range(32)]
    w = plan(lengths, 17)
    _check_plan(lengths, 17, w)
    assert len(groups(w)) <= 9 and computed_frames(w) / sum(lengths) <= 1.45        # the 2R-frame tails are a third of a 1 s clip
    assert computed_frames(w) <= 32 * max(lengths)


def test_bad_arguments_are_refused_by_name():
    with pytest.raises(ValueError, match="negative length"):
        plan([5, -1, 7], 17)
    with pytest.raises(ValueError, match="empty batch"):
        plan([], 17)
    with pytest.raises(ValueError, match="reach"):
        plan([5], 0)
    assert plan([0, 0], 17) == []
    assert plan([100], 17, launch_frames=0, max_groups=-3) == plan([100], 17, ragged.LAUNCH_FRAMES, ragged.MAX_GROUPS)


# ---- the C ABI: declarations, the ctypes mirror, and the C planner against the Python plan ----
import ctypes  # noqa: E402
import os  # noqa: E402
import re  # noqa: E402

from vocoder_amd import _lib  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RAGGED_API = ("fv_ragged_plan", "fv_ragged_create", "fv_ragged_workspace_bytes", "fv_ragged_num_groups", "fv_ragged_group",
              "fv_ragged_windows", "fv_ragged_forward", "fv_ragged_destroy")


def test_ragged_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    assert {n for n in declared if n.startswith("fv_ragged")} == set(RAGGED_API)
    for name in RAGGED_API:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert "#define FV_ABI_VERSION 5" in hdr


def test_ragged_window_mirror_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    body = re.search(r"typedef struct fv_ragged_window \{(.*?)\} fv_ragged_window;", hdr, re.S).group(1)
    fields = [f.strip() for f in re.search(r"int32_t\s+([\w\s,]+);", body).group(1).split(",")]
    assert fields == [f for f, _ in _lib.RaggedWindow._fields_] == list(Window._fields)
    assert ctypes.sizeof(_lib.RaggedWindow) == 4 * len(fields) == 24


def _c_plan(lengths, R, lf=0, mg=0, cap=None):
    L = _lib.lib()
    arr = (ctypes.c_int32 * max(len(lengths), 1))(*lengths)
    n = L.fv_ragged_plan(R, arr, len(lengths), lf, mg, None, 0)
    if n < 0:
        return n, []
    cap = n if cap is None else cap
    buf = (_lib.RaggedWindow * max(cap, 1))()
    n2 = L.fv_ragged_plan(R, arr, len(lengths), lf, mg, buf, cap)
    return n2, [Window(w.clip, w.start, w.frames, w.keep_lo, w.keep_hi, w.group) for w in buf[:min(cap, n2)]]


@pytest.mark.parametrize("seed", range(240))
def test_c_planner_returns_the_python_plan_window_for_window(seed):
    rng = random.Random(5000 + seed)                    # the sets of test_plan_properties_over_random_length_sets
    R = rng.choice([1, 17, 115])
    B = rng.randint(1, 64)
    hi = rng.choice([3 * R + 5, 300, 900])
    lengths = [rng.choice([0, rng.randint(0, hi), rng.randint(0, 900), 2 * R, 2 * R + 1]) for _ in range(B)]
    lf = rng.choice([0, 1, 64, 192, 1000])
    mg = rng.choice([0, 1, 2, 8, 64])
    n, got = _c_plan(lengths, R, lf, mg)
    assert got == plan(lengths, R, lf, mg) and n == len(got)


def test_c_planner_on_the_seeded_sets_and_a_known_tie():
    for seed in range(4):
        rng = random.Random(seed)
        lengths = [rng.randint(86, 860) for _ in range(32)]
        assert _c_plan(lengths, 17)[1] == plan(lengths, 17)
    # a tie by construction, R = 1: [10, 20] as one run costs 2 * 20 + 2 + lf, as two runs 10 + 20 + 2 lf — equal at lf = 12: the fewest runs win
    for planner in (lambda l, lf: plan(l, 1, lf, 8), lambda l, lf: _c_plan(l, 1, lf, 8)[1]):
        assert [g for g in groups(planner([10, 20], 12))] == [(2, 20), (1, 2)]
        assert [g for g in groups(planner([10, 20], 11))] == [(1, 20), (1, 10)]
        # three runs' worth of ties further back: [10, 20, 30] at lf = 12 — {10,20,30}: 90+4+12 = 106; {10,20},{30}: 54+30+12 = 96;
        # {10},{20,30}: 22+60+2+12 = 96; {10},{20},{30}: 96 -> two runs win over three, and of the two the LAST run that starts earliest: {20, 30}
        w = planner([10, 20, 30], 12)
        assert groups(w) == [(2, 30), (1, 10), (1, 2)]
        assert sorted(x.clip for x in w if x.frames == 30) == [1, 2]


def test_c_planner_refuses_bad_arguments_by_name():
    L = _lib.lib()
    n, _ = _c_plan([5, -1, 7], 17)
    assert n == _lib.FV_ERR_INVALID and b"negative length" in L.fv_last_error()
    n, _ = _c_plan([], 17)
    assert n == _lib.FV_ERR_INVALID and b"batch" in L.fv_last_error()
    n, _ = _c_plan([5], 0)
    assert n == _lib.FV_ERR_INVALID and b"reach" in L.fv_last_error()
    lengths = [100, 40, 3]
    full = plan(lengths, 17)
    n, got = _c_plan(lengths, 17, cap=2)                # cap too small: the needed count comes back, the first cap windows are written
    assert n == len(full) == 4 and got == full[:2]


def test_shard_lengths_follows_shard_slice():
    from vocoder_amd.sharding import shard_lengths, shard_slice
    lengths = list(range(100, 137))
    parts = [shard_lengths(lengths, 8, r) for r in range(8)]
    assert sum(parts, []) == lengths and [len(p) for p in parts] == [5, 5, 5, 5, 5, 4, 4, 4]
    assert parts[3] == lengths[shard_slice(37, 8, 3)]
