"""CPU: the session pool's C declarations and exports, the ctypes mirrors of its three structs, the plan of a step stated twice (fv_pool_plan
in C, vocoder_amd.sessions.plan_step in Python) over random session histories, the plan's properties, and its refusals by name."""
import ctypes
import os
import random
import re

import pytest

from vocoder_amd import _lib, sessions, streaming

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
POOL_API = ("fv_pool_plan", "fv_pool_create", "fv_pool_workspace_bytes", "fv_pool_pending_frames", "fv_pool_step", "fv_pool_reset",
            "fv_pool_destroy")
C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}


def _header():
    return open(os.path.join(REPO, "include", "fishvoc.h")).read()


def test_pool_entry_points_are_declared_listed_and_exported():
    hdr = _header()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_\w+)\s*\(", hdr))
    L = _lib.lib()
    assert {n for n in declared if n.startswith("fv_pool_")} == set(POOL_API)
    assert {n for n in _lib.EXPORTS if n.startswith("fv_pool_")} == set(POOL_API)
    for name in POOL_API:
        assert hasattr(L, name), name
    assert re.search(r"^#define FV_ABI_VERSION 5$", hdr, re.M)
    assert _lib.FV_ABI_VERSION == 5 == L.fv_abi_version()


@pytest.mark.parametrize("name,mirror,size", [("fv_pool_config", _lib.PoolConfig, 16), ("fv_pool_item", _lib.PoolItem, 12),
                                              ("fv_pool_row", _lib.PoolRow, 40)])
def test_pool_struct_mirrors_match_the_header(name, mirror, size):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|int64_t)\s+([\w\s,]+);", body):
        fields += [(n.strip(), C_TYPES[ctype]) for n in names.split(",")]
    assert fields == list(mirror._fields_)
    assert ctypes.sizeof(mirror) == size


# ---- the plan, twice ------------------------------------------------------------------------------------------------------
def _c_plan(S, max_chunk, K, A, F, E, flushed, items, in_frames=-1, out_frames=-1):
    """fv_pool_plan -> (rows as sessions.Row, groups as (rows, frames)); raises FishVocError on a refusal."""
    L = _lib.lib()
    cfg = _lib.PoolConfig(S, max_chunk, K, A)
    n = len(items)
    arr = (_lib.PoolItem * max(n, 1))(*[_lib.PoolItem(int(s), int(f), int(bool(fl))) for s, f, fl in items])
    i64 = ctypes.c_int64 * S
    rows = (_lib.PoolRow * max(n, 1))()
    gr, gf = (ctypes.c_int32 * max(n, 1))(), (ctypes.c_int32 * max(n, 1))()
    ng = ctypes.c_int32(-1)
    r = L.fv_pool_plan(ctypes.byref(cfg), i64(*F), i64(*E), (ctypes.c_int32 * S)(*[int(x) for x in flushed]), arr, n, in_frames, out_frames,
                       rows, n, gr, gf, n, ctypes.byref(ng))
    if r < 0:
        _lib.check(r)
    assert r <= n and 0 <= ng.value <= n
    return ([sessions.Row(x.item, x.group, x.col0, x.frames, x.w, x.emit_lo, x.emit_hi) for x in rows[:r]],
            [(gr[g], gf[g]) for g in range(ng.value)])


def _history(seed):
    """One seeded random history of a pool: (S, max_chunk, K, A, lengths per utterance served, steps), a step being a list of
    (session, n, flush) items with resets listed as ("reset", session).  Utterances start staggered, receive chunks of 0 ... max_chunk
    frames (0 included), end with a push + flush item or a bare flush, and a freed slot is reset and serves another utterance."""
    rng = random.Random(7000 + seed)
    S = rng.randint(1, 12)
    K, A = rng.randint(0, 40), rng.randint(0, 40)
    max_chunk = rng.randint(1, 70)
    start = [rng.randint(0, 6) for _ in range(S)]
    left = [rng.choice([0, 1, 2, 5, 17, 40, 61, 150, 389]) for _ in range(S)]     # frames still to come in the slot's current utterance
    served = [1] * S
    total = [[t] for t in left]
    live = [True] * S
    steps = []
    step = 0
    while any(live) and step < 400:
        items, resets = [], []
        order = list(range(S))
        rng.shuffle(order)
        for s in order:
            if not live[s] or step < start[s] or rng.random() < 0.2:
                continue
            n = min(left[s], rng.randint(0, max_chunk))
            left[s] -= n
            flush = left[s] == 0 and rng.random() < 0.7
            items.append((s, n, flush))
            if flush:
                if served[s] < 3 and rng.random() < 0.6:
                    resets.append(s)
                else:
                    live[s] = False
        steps.append(items)
        for s in resets:
            steps.append(("reset", s))
            served[s] += 1
            left[s] = rng.choice([0, 3, 9, 30, 77, 200])
            total[s].append(left[s])
            start[s] = step + rng.randint(1, 4)
        step += 1
    return S, max_chunk, K, A, total, steps


@pytest.mark.parametrize("seed", range(240))
def test_the_c_plan_and_the_python_plan_agree_and_hold_their_properties(seed):
    S, max_chunk, K, A, total, steps = _history(seed)
    st = sessions.PoolState(S, max_chunk, K, A)
    cap = K + A + max_chunk
    assert st.cap == cap
    emitted_next = [0] * S          # per session: the emitted ranges tile [0, T) in order
    done = [[] for _ in range(S)]   # per session: the lengths of the utterances it finished
    for items in steps:
        if items and items[0] == "reset":
            s = items[1]
            assert st.flushed[s]
            st.reset(s)
            emitted_next[s] = 0
            continue
        before = (list(st.received), list(st.emitted), list(st.flushed))
        py = st.plan(items)
        c_rows, c_groups = _c_plan(S, max_chunk, K, A, st.received, st.emitted, st.flushed, items)
        assert (list(st.received), list(st.emitted), list(st.flushed)) == before      # planning moves nothing
        assert c_rows == py.rows, (seed, items)
        assert c_groups == py.groups, (seed, items)
        # -- properties --
        assert sorted(r.item for r in py.rows) == [i for i, (s, n, fl) in enumerate(items) if py.emitted[i] > st.emitted[s]]
        assert [r.group for r in py.rows] == sorted(r.group for r in py.rows)
        for g, (cnt, frames) in enumerate(py.groups):
            mine = [r for r in py.rows if r.group == g]
            assert len(mine) == cnt >= 1 and [r.item for r in mine] == sorted(r.item for r in mine)
            assert 1 <= frames <= cap
            if g > 0:
                assert frames < py.groups[g - 1][1]
        for r in py.rows:
            s, n, fl = items[r.item]
            F, E = st.received[s], st.emitted[s]
            F2, w, E2 = streaming.step(F, E, n, K, A)
            if fl:
                E2 = F2
            glen = py.groups[r.group][1]
            assert (r.w, r.frames, r.emit_lo, r.emit_hi) == (w, F2 - w, E, E2)
            assert r.frames <= cap and 0 <= r.col0 and r.col0 + r.frames <= glen
            assert r.emit_lo == emitted_next[s]
            if r.w == 0:
                assert r.col0 == 0                                   # a left-owning row starts at the tensor's left edge
            else:
                assert r.emit_lo - r.w >= K                          # K frames of context inside an edge it does not own
            if fl:
                assert r.col0 + r.frames == glen                     # a flushing row ends at its group's last column
            else:
                assert r.w + r.frames - r.emit_hi >= A               # A frames of lookahead inside an edge it does not own
            if r.w == 0 and fl:
                assert r.frames == glen                              # a whole utterance runs at its own length
            if r.group > 0:
                assert r.w == 0 and fl and r.col0 == 0
        assert py.groups == [] or py.groups[0][1] == max(r.frames for r in py.rows)
        st.apply(items, py)
        for i, (s, n, fl) in enumerate(items):
            emitted_next[s] = st.emitted[s]
            assert st.received[s] - st.emitted[s] <= A
            if fl:
                assert st.emitted[s] == st.received[s] and st.flushed[s]
                done[s].append(st.received[s])
    for s in range(S):
        assert done[s] == total[s][:len(done[s])]                    # every finished utterance came out whole: [0, T) tiled in order


@pytest.mark.parametrize("seed", range(30))
def test_lockstep_items_plan_to_one_group_at_column_zero_with_the_streams_counters(seed):
    rng = random.Random(seed)
    S, K, A, max_chunk = rng.randint(1, 12), rng.randint(0, 40), rng.randint(0, 40), rng.randint(1, 70)
    st = sessions.PoolState(S, max_chunk, K, A)
    F = E = 0
    chunks = [rng.randint(0, max_chunk) for _ in range(rng.randint(1, 30))]
    for k, n in enumerate(chunks + [0]):
        flush = k == len(chunks)
        items = [(s, n, flush) for s in range(S)]
        F2, w, E2 = streaming.step(F, E, n, K, A, flush)
        p = st.plan(items)
        c_rows, c_groups = _c_plan(S, max_chunk, K, A, st.received, st.emitted, st.flushed, items)
        assert c_rows == p.rows and c_groups == p.groups
        if E2 > E:
            assert p.groups == [(S, F2 - w)]
            assert p.rows == [sessions.Row(i, 0, 0, F2 - w, w, E, E2) for i in range(S)]
        else:
            assert p.rows == [] and p.groups == []
        assert p.received == [F2] * S and p.emitted == [E2] * S
        st.apply(items, p)
        F, E = F2, E2


# ---- refusals -------------------------------------------------------------------------------------------------------------
REFUSALS = [
    ("duplicate session", [(1, 4, False), (2, 4, False), (1, 0, True)], {}, _lib.FV_ERR_INVALID),
    ("outside", [(0, 4, False), (4, 4, False)], {}, _lib.FV_ERR_INVALID),
    ("outside", [(-1, 4, False)], {}, _lib.FV_ERR_INVALID),
    ("max_chunk_frames", [(0, 4, False), (1, 9, False)], {}, _lib.FV_ERR_INVALID),
    ("max_chunk_frames", [(0, -1, False)], {}, _lib.FV_ERR_INVALID),
    ("in_frames", [(0, 4, False), (1, 7, False)], dict(in_frames=6), _lib.FV_ERR_INVALID),
    ("out_frames", [(0, 8, False), (1, 2, True)], dict(out_frames=7), _lib.FV_ERR_INVALID),
    ("flushed", [(0, 4, False), (3, 1, False)], {}, _lib.FV_ERR_STATE),
    ("flushed", [(3, 0, True)], {}, _lib.FV_ERR_STATE),
]


@pytest.mark.parametrize("name,items,buffers,status", REFUSALS)
def test_a_refused_plan_names_its_cause_and_moves_no_counter(name, items, buffers, status):
    S, max_chunk, K, A = 4, 8, 3, 2
    st = sessions.PoolState(S, max_chunk, K, A)
    st.step([(0, 8, False), (1, 5, False), (3, 6, True)])           # session 0: F = 8, E = 6; session 3 is flushed
    before = (list(st.received), list(st.emitted), list(st.flushed))
    assert before == ([8, 5, 0, 6], [6, 3, 0, 6], [False, False, False, True])
    with pytest.raises(sessions.PoolStateError if status == _lib.FV_ERR_STATE else ValueError, match=name):
        st.step(items, **buffers)
    assert (st.received, st.emitted, st.flushed) == before
    F, E, fl = (list(x) for x in before)
    with pytest.raises(_lib.FishVocError, match=name) as ei:
        _c_plan(S, max_chunk, K, A, F, E, fl, items, buffers.get("in_frames", -1), buffers.get("out_frames", -1))
    assert ei.value.status == status
    assert (F, E, fl) == before
    # the same items without the offending part plan fine, in both statements
    ok = [(0, 4, False), (1, 7, False)]
    assert _c_plan(S, max_chunk, K, A, F, E, fl, ok, 7, 7)[0] == st.plan(ok, 7, 7).rows != []
    st.reset(3)
    assert st.plan([(3, 1, False)]).received == [1]
