"""GPU: the session pool (fv_pool_*, vocoder_amd.engine.SessionPool) — lockstep against a Stream, independent sessions against each
utterance alone and the oracle, every row against Engine.forward over its group's tensor, isolation and dead padding, refusals by name, CLI."""
import random

import numpy as np
import pytest

from test_gpu_ragged import _dev, _model
from test_gpu_stream import HEAD, MODELS, TINY
from vocoder_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-4
LENGTHS = [389, 150, 61, 9, 77]      # the fifth is served by the slot the 9-frame utterance frees
STARTS = [0, 3, 3, 10]
MAX_CHUNK = 16


def _utterances(model, cin, hop, tmpl):
    """Five utterances (mel (C_in, T_u), template (1, T_u * hop) or None), each its own data."""
    T = max(LENGTHS)
    if model == "istft_head":
        mel = np.random.default_rng(12).standard_normal((len(LENGTHS), cin, T)).astype(np.float32)
    else:
        mel = syn.synthetic_mel(len(LENGTHS), cin, T, seed=9)
    tt = syn.synthetic_template(len(LENGTHS), T, hop, seed=3) if tmpl else None
    return [(np.ascontiguousarray(mel[u, :, :n]), None if tt is None else np.ascontiguousarray(tt[u, :, :n * hop])) for u, n in enumerate(LENGTHS)]


def _schedule(seed):
    """The steps of the independent-sessions case: a list of ("step", [(slot, utterance, first frame, n, flush)]) and ("reset", slot).
    Slot u serves utterance u from step STARTS[u]; chunk sizes are seeded random in 0 ... MAX_CHUNK; an utterance flushes at its own end,
    with its last chunk or with a bare flush item one step later; slot 3 is then reset and serves utterance 4."""
    rng = random.Random(seed)
    utt = [0, 1, 2, 3]
    pos = [0, 0, 0, 0]
    start = list(STARTS)
    live = [True] * 4
    out, step = [], 0
    while any(live):
        items = []
        for s in range(4):
            if not live[s] or step < start[s]:
                continue
            T = LENGTHS[utt[s]]
            n = T - pos[s] if T <= 9 else min(T - pos[s], rng.randint(0, MAX_CHUNK))   # (the 9-frame utterance arrives in one chunk)
            flush = pos[s] + n == T and (n == 0 or rng.random() < 0.5)
            items.append((s, utt[s], pos[s], n, flush))
            pos[s] += n
        out.append(("step", items))
        for s, u, _, _, flush in items:
            if flush:
                if s == 3 and u == 3:
                    out.append(("reset", 3))
                    utt[3], pos[3], start[3] = 4, 0, step + 2
                else:
                    live[s] = False
        step += 1
    return out


def _serve(pool, eng, utts, sched, in_frames=MAX_CHUNK, poison=(), out_buf=None, record=None):
    """Runs `sched` through pool.step_padded; returns the concatenated output per utterance.  `poison`: utterances whose whole data is NaN;
    with any, the chunk buffers' columns >= n are NaN too.  `record`: a list that receives (plan, items, group tensors, rows' outputs)."""
    dev = _dev()
    hop = pool.hop
    cin = pool.in_channels
    has_t = utts[0][1] is not None
    outs = [[] for _ in utts]
    for kind, what in sched:
        if kind == "reset":
            pool.reset(what)
            continue
        count = len(what)
        fill = float("nan") if poison else 0.0
        chunks = np.full((count, cin, in_frames), fill, np.float32)
        tmpl = np.full((count, 1, in_frames * hop), fill, np.float32) if has_t else None
        for i, (s, u, f0, n, _) in enumerate(what):
            chunks[i, :, :n] = np.nan if u in poison else utts[u][0][:, f0:f0 + n]
            if has_t:
                tmpl[i, :, :n * hop] = np.nan if u in poison else utts[u][1][:, f0 * hop:(f0 + n) * hop]
        items = [(s, n, fl) for s, _, _, n, fl in what]
        plan = pool.state.plan(items)
        before = [(pool.received_frames(s), pool.emitted_frames(s)) for s, _, _ in items]
        emit_want = plan.emit_frames
        out = None
        if out_buf is not None:
            of = max(emit_want, default=0)
            out = out_buf[:count * pool.out_channels * of * hop].view(count, pool.out_channels, of * hop)
            out.fill_(float("nan"))
        y, emit = pool.step_padded(items, torch.from_numpy(chunks).to(dev) if count else None,
                                   None if tmpl is None or not count else torch.from_numpy(tmpl).to(dev), out)
        assert emit == emit_want
        for i, (s, u, f0, n, fl) in enumerate(what):
            assert pool.received_frames(s) == before[i][0] + n == f0 + n
            assert pool.emitted_frames(s) == before[i][1] + emit[i]
            assert pool.pending_frames(s) == pool.received_frames(s) - pool.emitted_frames(s)
            assert bool((y[i, :, emit[i] * hop:] == 0.0).all()), "tails and non-emitting rows are exactly 0.0f"
            if emit[i]:
                outs[u].append(y[i, :, :emit[i] * hop].clone())
        if record is not None:
            record.append((plan, what, y.clone()))
    return [torch.cat(o, dim=1) if o else torch.empty((pool.out_channels, 0), device=dev) for o in outs]


def _tol(model, peak):
    return min(TOL, TOL * peak) if model in ("vocos", "istft_head") else TOL


@pytest.mark.parametrize("model", ["hifigan", "hifigan_template", "vocos"])
def test_lockstep_steps_are_the_streams_pushes_bit_for_bit(model):
    mk, cin, _, tmpl = _model(model)
    dev = _dev()
    eng = mk()
    hop, B, T = eng.output_length(1), 2, 389
    mel = syn.synthetic_mel(B, cin, T, seed=9)
    tt = syn.synthetic_template(B, T, hop, seed=3) if tmpl else None
    x = torch.from_numpy(mel).to(dev)
    t = None if tt is None else torch.from_numpy(tt).to(dev)
    rng = random.Random(4)
    chunks = [8] * 30                                  # a steady state: the window settles and the captured graph replays
    while sum(chunks) < T:
        chunks.append(min(T - sum(chunks), rng.randint(0, MAX_CHUNK)))
    want, f = [], 0
    with eng.stream(B, MAX_CHUNK) as st:
        for n in chunks:
            want.append(st.push(x[:, :, f:f + n], None if t is None else t[:, :, f * hop:(f + n) * hop]).clone())
            f += n
        want.append(st.flush().clone())
    assert eng.graph_replay
    with eng.session_pool(B, MAX_CHUNK) as pool:
        assert (pool.context_frames, pool.lookahead_frames) == (eng.reach_frames, eng.reach_frames)
        f = 0
        for k, n in enumerate(chunks + [0]):
            flush = k == len(chunks)
            pad = torch.full((B, cin, MAX_CHUNK), float("nan"), device=dev)
            pad[:, :, :n] = x[:, :, f:f + n]
            tp = None
            if t is not None:
                tp = torch.full((B, 1, MAX_CHUNK * hop), float("nan"), device=dev)
                tp[:, :, :n * hop] = t[:, :, f * hop:(f + n) * hop]
            plan = pool.state.plan([(b, n, flush) for b in range(B)])
            assert len(plan.groups) <= 1 and all(r.col0 == 0 for r in plan.rows)
            y, emit = pool.step_padded([(b, n, flush) for b in range(B)], pad, tp)
            f += n
            assert emit == [want[k].shape[2] // hop] * B
            assert torch.equal(y, want[k]), (k, n)
    assert eng.graph_replay
    eng.close()


def test_lockstep_past_one_launchs_table_entries():
    """34 sessions on the smallest engine, more than the 32 entries one launch carries: a step in which no session has its lookahead yet
    (34 ring-only gather entries, 34 zero crop rows), a step in which all 34 emit (34 rows), a flush.  Every step is the push of a Stream of
    34 rows bit for bit; sessions 0, 31, 32 and 33 — either side of the edge between the first and the second launch — are named."""
    mk, cin, _, _ = _model("istft_head")
    dev = _dev()
    eng = mk()
    hop, S, R = eng.output_length(1), 34, eng.reach_frames
    sizes = [R - 1, MAX_CHUNK]
    assert 1 <= sizes[0] < R < sum(sizes)
    x = torch.from_numpy(np.random.default_rng(12).standard_normal((S, cin, sum(sizes))).astype(np.float32)).to(dev)
    with eng.stream(S, MAX_CHUNK) as st:
        want = [st.push(x[:, :, :sizes[0]]).clone(), st.push(x[:, :, sizes[0]:]).clone(), st.flush().clone()]
    assert want[0].shape[2] == 0 and want[1].shape[2] > 0 and sum(w.shape[2] for w in want) == sum(sizes) * hop
    with eng.session_pool(S, MAX_CHUNK) as pool:
        f = 0
        for k, n in enumerate(sizes + [0]):
            items = [(s, n, k == 2) for s in range(S)]
            pad = torch.full((S, cin, MAX_CHUNK), float("nan"), device=dev)
            pad[:, :, :n] = x[:, :, f:f + n]
            plan = pool.state.plan(items)
            assert len(plan.rows) == (0 if k == 0 else S) and len(plan.groups) == min(k, 1)
            out = torch.full((S, pool.out_channels, MAX_CHUNK * hop), float("nan"), device=dev)      # (an output with columns: step 0 crops too)
            y, emit = pool.step_padded(items, pad, None, out)
            f += n
            cols = want[k].shape[2]
            assert emit == [cols // hop] * S
            for s in (0, 31, 32, 33):
                assert torch.equal(y[s, :, :cols], want[k][s]) and bool((y[s, :, cols:] == 0.0).all()), (k, s)
            assert torch.equal(y[:, :, :cols], want[k]) and bool((y[:, :, cols:] == 0.0).all()), k
    assert not torch.equal(want[1][32], want[1][0]) and not torch.equal(want[1][33], want[1][1])      # every session has its own data
    eng.close()


@pytest.mark.parametrize("model", MODELS)
def test_independent_sessions_equal_each_utterance_alone_and_the_oracle(model):
    mk, cin, oracle, tmpl = _model(model)
    dev = _dev()
    eng = mk()
    R, hop = eng.reach_frames, eng.output_length(1)
    utts = _utterances(model, cin, hop, tmpl)
    sched = _schedule(seed=len(model))
    record = []
    with eng.session_pool(4, MAX_CHUNK) as pool:
        got = _serve(pool, eng, utts, sched, record=record)
    if LENGTHS[3] <= R:   # the 9-frame utterance is a single window owning both edges: a group of its own beside the running sessions
        plan, what, _ = next(r for r in record if any(u == 3 and fl for _, u, _, _, fl in r[1]))
        row = next(r for r in plan.rows if what[r.item][1] == 3)
        assert (row.w, row.frames, row.emit_lo, row.emit_hi, row.col0) == (0, 9, 0, 9, 0)
        if len(plan.rows) > 1:
            assert row.group > 0 and plan.groups[row.group] == (1, 9) and plan.groups[0][1] > 9
    assert any(r.col0 > 0 for p, _, _ in record for r in p.rows), "some row is right-aligned inside a longer group"
    for u, (mel, tt) in enumerate(utts):
        n = LENGTHS[u]
        assert got[u].shape == (eng.out_channels, n * hop), (u, got[u].shape)
        x = torch.from_numpy(mel[None]).to(dev)
        t = None if tt is None else torch.from_numpy(tt[None]).to(dev)
        alone = eng(x, None, t).cpu().numpy()[0]
        ref = oracle(mel[None], None if tt is None else tt[None])[0]
        y = got[u].cpu().numpy()
        peak = float(np.abs(ref).max())
        d_alone, d_ref = float(np.abs(y - alone).max()), float(np.abs(y - ref).max())
        print(f"{model} utterance {u} ({n} frames): vs alone {d_alone:.3e}, vs oracle {d_ref:.3e}, peak {peak:.3e}")
        assert d_alone <= 2e-5 * max(1.0, peak), (u, n, d_alone)
        assert d_ref <= _tol(model, peak), (u, n, d_ref)
    eng.close()


@pytest.mark.parametrize("model,K,A", [("hifigan", None, None), ("hifigan_template", None, None), ("vocos", None, None), ("bigvgan", None, None),
                                       ("hifigan", 3, 5)])
@pytest.mark.parametrize("graph", [True, False])
def test_every_row_is_the_slice_of_a_forward_over_its_groups_tensor(model, K, A, graph):
    mk, cin, _, tmpl = _model(model)
    dev = _dev()
    eng = mk()
    eng.set_graph_replay(graph)
    hop = eng.output_length(1)
    utts = _utterances(model, cin, hop, tmpl)
    record = []
    with eng.session_pool(4, MAX_CHUNK, K, A) as pool:
        if K is not None:
            assert K < eng.reach_frames and A < eng.reach_frames
        _serve(pool, eng, utts, _schedule(seed=11), record=record)
    checked = 0
    for plan, what, y in record:
        for g, (cnt, Wg) in enumerate(plan.groups):
            rows = [r for r in plan.rows if r.group == g]
            xin = np.zeros((cnt, cin, Wg), np.float32)
            tin = np.zeros((cnt, 1, Wg * hop), np.float32) if tmpl else None
            for k, r in enumerate(rows):
                u = what[r.item][1]
                xin[k, :, r.col0:r.col0 + r.frames] = utts[u][0][:, r.w:r.w + r.frames]
                if tmpl:
                    tin[k, :, r.col0 * hop:(r.col0 + r.frames) * hop] = utts[u][1][:, r.w * hop:(r.w + r.frames) * hop]
            ref = eng(torch.from_numpy(xin).to(dev), None, None if tin is None else torch.from_numpy(tin).to(dev))
            for k, r in enumerate(rows):
                lo, hi = (r.col0 + r.emit_lo - r.w) * hop, (r.col0 + r.emit_hi - r.w) * hop
                assert torch.equal(y[r.item, :, :hi - lo], ref[k, :, lo:hi]), (g, k, r)
                checked += 1
    assert checked > 50
    eng.close()


@pytest.mark.parametrize("model", ["hifigan_template", "vocos"])
def test_isolation_dead_padding_zero_tails_and_guard_bands(model):
    mk, cin, _, tmpl = _model(model)
    dev = _dev()
    eng = mk()
    hop = eng.output_length(1)
    utts = _utterances(model, cin, hop, tmpl)
    sched = _schedule(seed=5)
    with eng.session_pool(4, MAX_CHUNK) as pool:
        clean = _serve(pool, eng, utts, sched)
    G = 4096
    pool = eng.session_pool(4, MAX_CHUNK)
    n_out = 4 * eng.out_channels * max(MAX_CHUNK, pool.lookahead_frames) * hop     # a step emits at most max_chunk frames, a flush at most A
    obuf = torch.full((n_out + 2 * G,), 7.25, device=dev)
    need = (pool.workspace_bytes + 3) // 4
    wbuf = torch.full((need + 2 * G,), -3.5, device=dev)
    pool._ws = wbuf[G:G + need]
    pool._ws.fill_(float("nan"))
    # utterance 1 is NaN throughout, and so is every chunk column >= n of every item (the chunk buffers are wider than any chunk)
    got = _serve(pool, eng, utts, sched, in_frames=MAX_CHUNK + 5, poison={1}, out_buf=obuf[G:G + n_out])
    torch.cuda.synchronize()
    for u in (0, 2, 3, 4):
        assert torch.equal(got[u], clean[u]), u
        assert bool(torch.isfinite(got[u]).all())
    assert got[1].shape == clean[1].shape
    assert bool((obuf[:G] == 7.25).all()) and bool((obuf[G + n_out:] == 7.25).all()), "output guard"
    assert bool((wbuf[:G] == -3.5).all()) and bool((wbuf[G + need:] == -3.5).all()), "workspace guard"
    pool.close()
    eng.close()


def test_refusals_name_their_cause_and_a_refused_step_changes_nothing():
    from vocoder_amd import _lib
    from vocoder_amd._lib import FishVocError
    from vocoder_amd.engine import Engine, istft_head_config, logmel_config, refinegan_config
    dev = _dev()
    rcfg = dict(syn.REFINEGAN_44K)
    rg = Engine(_lib.FV_MODEL_REFINEGAN, refine=refinegan_config(**rcfg), state_dict=syn.refinegan_state_dict(rcfg, seed=1))
    with pytest.raises(FishVocError, match="RefineGAN") as ei:
        rg.session_pool(2, 8)
    assert ei.value.status == _lib.FV_ERR_UNSUPPORTED
    rg.close()
    lm = Engine(_lib.FV_MODEL_LOGMEL, mel=logmel_config(sample_rate=24000, n_fft=256, win_length=256, hop_length=64, n_mels=20), state_dict={})
    with pytest.raises(FishVocError, match="log-mel") as ei:
        lm.session_pool(2, 8)
    assert ei.value.status == _lib.FV_ERR_UNSUPPORTED
    lm.close()
    hc = dict(HEAD, padding="center")
    ic = Engine(_lib.FV_MODEL_ISTFT_HEAD, head=istft_head_config(**hc), state_dict=syn.istft_head_state_dict(hc, seed=11))
    with pytest.raises(FishVocError, match="center") as ei:
        ic.session_pool(2, 8)
    assert ei.value.status == _lib.FV_ERR_UNSUPPORTED
    ic.close()

    mk, cin, _, _ = _model("hifigan_template")
    eng = mk()
    hop = 16
    x = torch.from_numpy(syn.synthetic_mel(3, cin, 120, seed=9)).to(dev)
    tt = torch.from_numpy(syn.synthetic_template(3, 120, hop, seed=3)).to(dev)
    with pytest.raises(FishVocError, match="sessions"):
        eng.session_pool(0, 8)

    def run(with_refusals):
        pool = eng.session_pool(3, 8, 6, 4)
        L = eng._lib
        outs = []

        def step(f, n, flush2=False):
            items = [(0, n, False), (1, n, False), (2, n, flush2)]
            y, emit = pool.step_padded(items, x[:, :, f:f + n].contiguous(), tt[:, :, f * hop:(f + n) * hop].contiguous())
            outs.append((y.clone(), emit))

        def raw(items, chunks, tmpl, in_frames, out_frames, ws_bytes=None):
            arr = (_lib.PoolItem * len(items))(*[_lib.PoolItem(*it) for it in items])
            out = torch.empty((len(items), 1, max(out_frames, 1) * hop), device=dev)
            return L.fv_pool_step(pool._h, arr, len(items), chunks.data_ptr(), None if tmpl is None else tmpl.data_ptr(), in_frames, out.data_ptr(),
                                  out_frames, None, pool._ws.data_ptr(), pool.workspace_bytes if ws_bytes is None else ws_bytes, None)

        step(0, 8)
        step(8, 8, flush2=True)
        if with_refusals:
            counters = [(pool.received_frames(s), pool.emitted_frames(s), pool.pending_frames(s)) for s in range(3)]
            c8, t8 = x[:, :, 16:24].contiguous(), tt[:, :, 16 * hop:24 * hop].contiguous()
            c9, t9 = x[:, :, 16:25].contiguous(), tt[:, :, 16 * hop:25 * hop].contiguous()
            cases = [
                ("duplicate session", _lib.FV_ERR_INVALID, lambda: raw([(0, 8, 0), (0, 8, 0)], c8, t8, 8, 8)),
                ("outside", _lib.FV_ERR_INVALID, lambda: raw([(0, 8, 0), (3, 8, 0)], c8, t8, 8, 8)),
                ("max_chunk_frames", _lib.FV_ERR_INVALID, lambda: raw([(0, 8, 0), (1, 9, 0)], c9, t9, 9, 9)),
                ("in_frames", _lib.FV_ERR_INVALID, lambda: raw([(0, 8, 0), (1, 8, 0)], c8, t8, 7, 8)),
                ("out_frames", _lib.FV_ERR_INVALID, lambda: raw([(0, 8, 0), (1, 8, 0)], c8, t8, 8, 7)),
                ("template", _lib.FV_ERR_INVALID, lambda: raw([(0, 8, 0), (1, 8, 0)], c8, None, 8, 8)),
                ("workspace too small", _lib.FV_ERR_INVALID, lambda: raw([(0, 8, 0), (1, 8, 0)], c8, t8, 8, 8, pool.workspace_bytes - 256)),
                ("flushed", _lib.FV_ERR_STATE, lambda: raw([(0, 8, 0), (2, 8, 0)], c8, t8, 8, 8)),
            ]
            for name, status, call in cases:
                assert call() == status, name
                assert name.encode() in L.fv_last_error(), (name, L.fv_last_error())
                assert [(pool.received_frames(s), pool.emitted_frames(s), pool.pending_frames(s)) for s in range(3)] == counters, name
            with pytest.raises(ValueError, match="duplicate session"):       # the Python plan refuses first, by the same name
                pool.step_padded([(0, 8, False), (0, 8, False)], c8[:2].contiguous(), t8[:2].contiguous())
        pool.reset(2)
        step(16, 8)
        step(24, 5, flush2=True)
        pool.close()
        return outs

    a, b = run(False), run(True)
    assert len(a) == len(b) == 4
    for (ya, ea), (yb, eb) in zip(a, b):
        assert ea == eb and torch.equal(ya, yb)
    e2 = _model("hifigan")[0]()
    p2 = e2.session_pool(2, 8)
    arr = (_lib.PoolItem * 1)(_lib.PoolItem(0, 8, 0))
    out = torch.empty((1, 1, 8 * hop), device=dev)
    st = e2._lib.fv_pool_step(p2._h, arr, 1, x[:1, :, :8].contiguous().data_ptr(), tt.data_ptr(), 8, out.data_ptr(), 8, None, p2._ws.data_ptr(),
                              p2.workspace_bytes, None)
    assert st == _lib.FV_ERR_INVALID and b"use_template=False" in e2._lib.fv_last_error()
    assert p2.pending_frames(0) == 0
    e2.close()
    with pytest.raises(FishVocError, match="closed"):
        p2.step([(0, x[0, :, :8], False)])
    eng.close()


def test_module_session_pool_and_the_list_form_of_step():
    from vocoder_amd.modules.generators import HiFiGANGenerator
    dev = _dev()
    gen = HiFiGANGenerator(**TINY)
    sd = syn.hifigan_state_dict(TINY, seed=5)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    gen = gen.eval().to(dev)
    mel = torch.from_numpy(syn.synthetic_mel(2, 20, 100, seed=9)).to(dev)
    with torch.no_grad():
        whole = gen(mel)
    with gen.session_pool(sessions=2, max_chunk_frames=16) as pool:
        outs = [[], []]
        pos = [0, 0]
        ends = [100, 40]
        sizes = [16, 7]
        while pos[0] < ends[0] or pos[1] < ends[1]:
            items = []
            for s in range(2):
                if pos[s] < ends[s]:
                    n = min(sizes[s], ends[s] - pos[s])
                    items.append((s, mel[s, :, pos[s]:pos[s] + n], pos[s] + n == ends[s]))
                    pos[s] += n
            for (s, _, _), y in zip(items, pool.step(items)):
                outs[s].append(y.clone())
        y0, y1 = torch.cat(outs[0], dim=1), torch.cat(outs[1], dim=1)
    assert y0.shape == (1, 100 * 16) and y1.shape == (1, 40 * 16)
    assert float((y0 - whole[0]).abs().max()) <= 2e-5 * max(1.0, float(whole[0].abs().max()))
    with torch.no_grad():
        short = gen(mel[1:2, :, :40].contiguous())
    assert float((y1 - short[0]).abs().max()) <= 2e-5 * max(1.0, float(short.abs().max()))


def test_cli_sessions_writes_the_wavs_of_the_one_by_one_run(tmp_path, capsys):
    from vocoder_amd import config, inference
    config.build_generator("hifigan", overrides={"num_mels": 80})
    sd = syn.hifigan_state_dict(dict(syn.HIFIGAN_V1_44K), 3)
    torch.save({"state_dict": {f"generator.{k}": torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "g.ckpt")
    (tmp_path / "in").mkdir()
    lengths = [150, 20, 34, 86, 61]
    for i, n in enumerate(lengths):
        torch.save(torch.from_numpy(syn.synthetic_mel(1, 80, n, seed=40 + i)[0]), tmp_path / "in" / f"m{i}.pt")
    args = ["--generator", "hifigan", "--num-mels", "80", "--ckpt-path", str(tmp_path / "g.ckpt"), "--input-path", str(tmp_path / "in")]
    inference.main(args + ["--output-path", str(tmp_path / "one")])
    inference.main(args + ["--output-path", str(tmp_path / "pool"), "--chunk-frames", "8", "--sessions", "3"])
    assert "3 sessions in one pool" in capsys.readouterr().out
    for i, n in enumerate(lengths):
        a, _ = inference.read_wav(tmp_path / "one" / f"m{i}.wav")
        b, _ = inference.read_wav(tmp_path / "pool" / f"m{i}.wav")
        assert a.shape == b.shape == (1, n * 512)
        assert np.abs(a - b).max() <= 1.0 / 32768 + 1e-9
    with pytest.raises(SystemExit):
        inference.main(args + ["--output-path", str(tmp_path / "x"), "--sessions", "3"])
    with pytest.raises(SystemExit):
        inference.main(args + ["--output-path", str(tmp_path / "x"), "--batch-size", "4", "--chunk-frames", "8"])
