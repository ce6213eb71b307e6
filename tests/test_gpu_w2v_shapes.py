"""GPU: the wav2vec2 kernels (vocoder_amd/csrc/w2v.hip: w2v_gemm_kernel, w2v_ln_kernel, w2v_attn_kernel) at the real widths, at widths that are
no multiple of a tile, over more rows than one launch table holds and beside rows without frames — the paths that the two fixture networks of
test_gpu_w2v.py never take.

The configs here (w2v_cases.SWEEP) have no golden from the reference: every expected value rests on the float64 restatement
(w2v_reference.py) ALONE, which the host suite pins to the reference's goldens at the fixture configs.  The bar is the project's, max |d| <=
1e-4 of the expected tensor's own peak; test_w2v_host.py shows for every config here that float32 arithmetic alone stays a factor of 10 under
it and that a dropped K tail, tap or LayerNorm quad lies a factor of 10 above it.  Everything that is not a parity check is bit-exact.  Each
parity case prints what it measured (profiles/LOG.md, R33.1).  Nothing here reads the reference or imports ``transformers``.

Path -> the test that fails if it is wrong:
  LayerNorm slots 1-3 (C in (256, 1024]), all full at C = 1024 / 768 / 512   test_sweep_against_the_restatement[large-37], [base-37], [ln1024-*]
  the ``q < nq`` guard of a partly filled slot (C = 260, 516, 1020)          test_sweep_against_the_restatement[odd-*], [ln516-*], [ln1020-*]
  N / Ng no multiple of 32: the ``n >= nend`` guard, the ``min(n, nend - 1)``
    weight-row clamp and the accumulator's channel map at a ragged edge        64 x 64: test_sweep_against_the_restatement[odd-*] (N = 36, 260, 100, 68),
                                                                               [depthwise-*] (Ng = 1), [cg2-*] (Ng = 2), [k12-*], [k4-*] (N = 4, 12);
                                                                               128 x 128 and 64 x 128: test_the_wide_gemm_tiles_at_odd_widths
                                                                               (a single row runs 64 x 64 tiles but for [depthwise-131], whose
                                                                               positional conv is 2 x 128 groups = 256 workgroups of 128 x 128)
  a K tail on the 16-byte path (``kin``, ``kc = min(k, K - 4)``, the partial
    last stage) and K below one stage                                          test_sweep_against_the_restatement[odd-*] (K = 108, 260, 100, 204, 68),
                                                                               [k12-*] (K = 12), [k4-*] (K = 4); wide tiles: ..._at_odd_widths
  a grouped conv on the single-float path (Cg = 1, 2, 3)                      test_sweep_against_the_restatement[depthwise-*], [cg2-*], [odd-*]
  a group wider than one column tile (groups = 1, Ng = 192)                   test_sweep_against_the_restatement[onegroup-*]
  a positional conv of one and of two taps                                    test_sweep_against_the_restatement[posk1-*], [posk2-*]
  the first conv at K = 32 (the limit) and 17, stride above the kernel,
    kernel = stride = 64 (the limits)                                          test_sweep_against_the_restatement[first32-*], [first17-*], [k1s3-*], [k64s64-*]
  the real widths on every tile                                               64 x 64: test_sweep_against_the_restatement[large-37], [base-37];
                                                                               128 x 128 and 64 x 128: test_the_wide_gemm_tiles_at_the_real_widths
  the backbone alone (post_channels = 0) at an odd and a real width           test_sweep_backbone_only_through_the_c_abi
  row0 > 0 in every kernel, the hidden-state plane offset across tables       test_more_rows_than_one_launch_table, ..._through_the_c_abi
  rows with no frames (0 samples; shorter than the first kernel; one or two
    frames after layer 0 and none after layer 1) beside rows with some         test_rows_without_frames, test_only_rows_without_frames
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import w2v_cases as wc
import w2v_reference as wref
from vocoder_amd import synthetic as syn
from vocoder_amd.modules.encoders import HubertEncoder
from w2v_cases import Handle, bits, mask_of, parity, same

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def build(cfg, sd):
    m = HubertEncoder(config={k: v for k, v in cfg.items() if k != "output_size"}, output_size=cfg["output_size"])
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().cuda()


@functools.lru_cache(maxsize=2)
def sweep_module(name, layers=None):
    cfg = wc.SWEEP[name][0]
    return build(cfg if layers is None else wc.with_layers(cfg, layers), wc.sweep_state_dict(name, layers))


@functools.lru_cache(maxsize=None)
def tiny():
    """hubert_tiny: (config, weights, module)."""
    g = np.load(os.path.join(GOLDEN, "hubert_tiny.npz"))
    cfg = json.loads(bytes(g["config"]).decode())
    sd = syn.hubert_state_dict(cfg, int(g["seed"]))
    return cfg, sd, build(cfg, sd)


def padded(waves):
    """A list of 1-d arrays -> ((B, T) device tensor, zero padded; lengths)."""
    lengths = [len(w) for w in waves]
    x = np.zeros((len(waves), max(lengths)), np.float32)
    for b, w in enumerate(waves):
        x[b, : len(w)] = w
    return torch.from_numpy(x).cuda(), lengths


# -- 1. the config sweep: one row, every hidden state and the output -------------------------------------------------------------------------
@pytest.mark.parametrize("name,F", wc.SWEEP_CASES)
def test_sweep_against_the_restatement(name, F):
    cfg = wc.SWEEP[name][0]
    m, wave, want = sweep_module(name), wc.sweep_wave(name, F), wc.sweep_restated(name, F)
    assert m.frames(len(wave), backbone=True) == F and m.frames(len(wave) - 1, backbone=True) == F - 1
    out, hs = m(torch.from_numpy(wave)[None].cuda(), output_hidden_states=True)
    assert hs.shape == (cfg["num_hidden_layers"] + 1, 1, F, cfg["hidden_size"])
    for layer in range(cfg["num_hidden_layers"] + 1):
        parity(f"sweep {name} {F} frames hidden state {layer}", hs[layer, 0].cpu().numpy(), want["hidden_states"][layer])
    parity(f"sweep {name} {F} frames out", out[0].cpu().numpy(), want["out"])


@pytest.mark.parametrize("name,F", wc.BACKBONE_ONLY)
def test_sweep_backbone_only_through_the_c_abi(name, F):
    cfg = wc.SWEEP[name][0]
    wave, want = wc.sweep_wave(name, F), wc.sweep_restated(name, F)
    x = torch.from_numpy(wave)[None].cuda()
    h = Handle(cfg, wc.sweep_state_dict(name), 0)
    try:
        last, hs, _ = h.run(x, None, hidden=True)
    finally:
        h.close()
    assert last.shape == (1, F, cfg["hidden_size"])
    for layer in range(cfg["num_hidden_layers"] + 1):
        parity(f"sweep {name} {F} frames backbone only hidden state {layer}", hs[layer, 0].cpu().numpy(), want["hidden_states"][layer])
    parity(f"sweep {name} {F} frames backbone only last_hidden_state", last[0].cpu().numpy(), want["last_hidden_state"])
    assert same(hs, sweep_module(name)(x, output_hidden_states=True)[1])          # the post stack changes nothing before it


# -- 2. the wide tiles -----------------------------------------------------------------------------------------------------------------------
def wide_case(tag, m, cfg, sd, B, F, seed):
    """B ragged rows of up to F backbone frames (three lengths, ragged inside the wide tiles): rows 0, 1, 2 and the last have the bits of the
    row alone (64 x 64 tiles), zeros past their frames, and the shortest of the three lengths (row 2) the restatement's values."""
    rng = np.random.default_rng(seed)
    xd, lengths = padded([rng.standard_normal(wc.samples_for(cfg, F - (b % 3) * (F // 7))).astype(np.float32) for b in range(B)])
    assert m.frames(xd.shape[1], backbone=True) == F
    out, hs = m(xd, mask_of(lengths, xd.shape[1]), output_hidden_states=True)
    for b in (0, 1, 2, B - 1):
        n = lengths[b]
        Fb, F2 = m.frames(n, backbone=True), m.frames(n)
        alone, alone_hs = m(xd[b:b + 1, :n], output_hidden_states=True)
        assert same(alone[0], out[b, :, :F2]) and same(alone_hs[:, 0], hs[:, b, :Fb]), b
        assert not bits(out[b, :, F2:]).any() and not bits(hs[:, b, Fb:]).any()
    want = wref.forward(sd, cfg, xd[2, : lengths[2]].cpu().numpy())
    Fb, F2 = want["hidden_states"].shape[1], want["out"].shape[1]
    for layer in range(cfg["num_hidden_layers"] + 1):
        parity(f"{tag}: row 2 hidden state {layer}", hs[layer, 2, :Fb].cpu().numpy(), want["hidden_states"][layer])
    parity(f"{tag}: row 2 out", out[2, :, :F2].cpu().numpy(), want["out"])


@pytest.mark.parametrize("F", (257, 200))
def test_the_wide_gemm_tiles_at_odd_widths(F):
    """The `odd` config, 128 rows.  The launcher takes 128 x 128 tiles (BK = 16) where ceil(Fout / 128) x groups x ceil(Ng / 128) x rows >= the
    256 compute units, else 64 x 128 (BK = 32) where ceil(Fout / 64) x groups x ceil(Ng / 128) x rows >= 256, else 64 x 64.  With 128 rows a
    product is on 128 x 128 as soon as Fout > 128.
    F = 257 (515 frames after conv 0, 129 after post's stride): every product on 128 x 128 — conv 0 (N = 36, K = 7, single floats),
    conv 1 (N = 260 = 2 x 128 + 4, K = 108 = 6 x 16 + 12), projection (N = 192, K = 260 = 16 x 16 + 4), positional conv (64 groups of Ng = 3,
    K = 15, single floats), q|k|v (N = 576), out_proj, FFN in (N = 100 = 3 x 32 + 4), FFN out (K = 100 = 6 x 16 + 4), post 0 (N = 68 = 2 x 32 + 4,
    K = 576), post 1 (N = 68, K = 204 = 12 x 16 + 12, Fout = 129: 2 x 1 x 128 = 256 workgroups), post 2 (N = 68, K = 68 = 4 x 16 + 4).
    F = 200 (401 and 100): the same on 128 x 128 but post 1 and post 2, whose Fout = 100 gives 128 workgroups of 128 x 128 and 256 of
    64 x 128: N = 68 and K = 204 = 6 x 32 + 12, K = 68 = 2 x 32 + 4 on the 64 x 128 tile.
    So both wide tiles see a ragged N tail inside a 32-wide sub-tile and a K tail on the 16-byte path; the row alone is on 64 x 64."""
    cfg = wc.SWEEP["odd"][0]
    wide_case(f"odd, 128 rows of up to {F} frames", sweep_module("odd"), cfg, wc.sweep_state_dict("odd"), 128, F, 7000 + F)


@pytest.mark.parametrize("B,F", ((16, 129), (10, 127)))
def test_the_wide_gemm_tiles_at_the_real_widths(B, F):
    """The `large` config with one transformer layer; 256 compute units, the rule of the test above.
    16 rows of up to 129 frames (259 after conv 0, 65 after post's stride): conv 0 (N = 512, K = 10, single floats) 3 x 4 x 16 = 192 then
    5 x 4 x 16 = 320: 64 x 128; conv 1 (K = 1536) 128 then 192: 64 x 64; projection (N = 1024, K = 512) 2 x 8 x 16 = 256: 128 x 128; positional
    conv (16 groups of Ng = 64, K = 8192, half of every tile past the group's end) 2 x 16 x 16: 128 x 128; q|k|v (N = 3072), out_proj,
    FFN in (N = 4096) and FFN out (K = 4096): 128 x 128; the post convs (N = 512): 64 x 64.
    10 rows of up to 127 frames (255 and 64): q|k|v 24 x 10 = 240 then 480: 64 x 128; positional conv 160 then 320: 64 x 128; FFN in
    32 x 10 = 320: 128 x 128; everything else (at most 8 column tiles: 80 then 160 workgroups) 64 x 64."""
    cfg = wc.with_layers(wc.SWEEP["large"][0], 1)
    wide_case(f"large with one layer, {B} rows of up to {F} frames", sweep_module("large", 1), cfg, wc.sweep_state_dict("large", 1), B, F, 8000 + F)


# -- 3. more rows than one launch table --------------------------------------------------------------------------------------------------------
def many_rows(B):
    """B waves of hubert_tiny of 1 to 40 frames (10 F + 10 samples give F), a one-frame row at index 128."""
    rng = np.random.default_rng(3300 + B)
    frames = rng.integers(1, 41, B)
    frames[128] = 1
    return [rng.standard_normal(10 * int(F) + 10).astype(np.float32) for F in frames], frames.tolist()


@pytest.mark.parametrize("B", (130, 257))
def test_more_rows_than_one_launch_table(B):
    cfg, sd, m = tiny()
    waves, frames = many_rows(B)
    xd, lengths = padded(waves)
    out, hs = m(xd, mask_of(lengths, xd.shape[1]), output_hidden_states=True)
    assert out.shape[0] == B and hs.shape[1] == B and max(frames) == hs.shape[2]
    listed = m.forward_list([xd[b, :n] for b, n in enumerate(lengths)])
    for b in range(128, B):         # the second and third launch tables: row0 = 128, 256
        F, F2 = frames[b], (frames[b] - 1) // 2 + 1
        alone, alone_hs = m(xd[b:b + 1, : lengths[b]], output_hidden_states=True)
        assert alone_hs.shape[2] == F and alone.shape[2] == F2
        assert same(alone[0], out[b, :, :F2]) and same(alone_hs[:, 0], hs[:, b, :F]), b
        assert not bits(out[b, :, F2:]).any() and not bits(hs[:, b, F:]).any(), b
    for b in range(B):
        F2 = (frames[b] - 1) // 2 + 1
        assert listed[b].shape == (out.shape[1], F2) and same(listed[b], out[b, :, :F2]), b
    for b in (0, 127, 128, B - 1):
        want = wref.forward(sd, cfg, waves[b])
        for layer in range(cfg["num_hidden_layers"] + 1):
            parity(f"{B} rows: row {b} ({frames[b]} frames) hidden state {layer}", hs[layer, b, : frames[b]].cpu().numpy(), want["hidden_states"][layer])
        parity(f"{B} rows: row {b} ({frames[b]} frames) out", out[b, :, : want["out"].shape[1]].cpu().numpy(), want["out"])


def test_more_rows_than_one_launch_table_through_the_c_abi():
    cfg, sd, m = tiny()
    waves, _ = many_rows(130)
    xd, lengths = padded(waves)
    h = Handle(cfg, sd, cfg["output_size"])
    try:
        guard = 1 << 16
        out, hs, ws = h.run(xd, lengths, hidden=True, guard=guard)
    finally:
        h.close()
    assert bool((ws[-guard:] == 0xA5).all())                      # nothing was written past the bytes it asked for
    assert not torch.isnan(out).any() and not torch.isnan(hs).any()         # every element of both outputs was written, in both tables
    m_out, m_hs = m(xd, mask_of(lengths, xd.shape[1]), output_hidden_states=True)
    assert same(out, m_out) and same(hs, m_hs)


# -- 4. rows without frames --------------------------------------------------------------------------------------------------------------------
# hubert_tiny (k = 10, s = 5, then k = 3, s = 2): 0 and 9 samples give no frame after layer 0; 10 and 14 give one there and none after layer 1;
# 15 gives two there and still none after layer 1 (its k = 3 needs three); 20 is the shortest row that keeps a frame
FRAMELESS = (0, 9, 10, 14, 15)


def frameless_batch():
    rng = np.random.default_rng(44)
    return padded([rng.standard_normal(n).astype(np.float32) for n in FRAMELESS + (20, 1300)])


def test_rows_without_frames():
    cfg, sd, m = tiny()
    xd, lengths = frameless_batch()
    T, nf = xd.shape[1], len(FRAMELESS)
    assert [m.frames(n, backbone=True) for n in lengths] == [0] * nf + [1, 129]
    out, hs = m(xd, mask_of(lengths, T), output_hidden_states=True)
    assert out.shape == (nf + 2, cfg["output_size"], 65) and hs.shape[2] == 129
    assert not bits(out[:nf]).any() and not bits(hs[:, :nf]).any()          # exact zeros, not even a negative one
    for b in (nf, nf + 1):
        F, F2 = m.frames(lengths[b], backbone=True), m.frames(lengths[b])
        alone, alone_hs = m(xd[b:b + 1, : lengths[b]], output_hidden_states=True)
        assert same(alone[0], out[b, :, :F2]) and same(alone_hs[:, 0], hs[:, b, :F])
        assert not bits(out[b, :, F2:]).any() and not bits(hs[:, b, F:]).any()
        want = wref.forward(sd, cfg, xd[b, : lengths[b]].cpu().numpy())
        parity(f"beside frameless rows: row {b} ({F} frames) last hidden state", hs[-1, b, :F].cpu().numpy(), want["hidden_states"][-1])
        parity(f"beside frameless rows: row {b} ({F} frames) out", out[b, :, :F2].cpu().numpy(), want["out"])
    # NaN in the padding and in the WHOLE of the frameless rows, the samples they do have included
    poisoned = xd.clone()
    for b, n in enumerate(lengths):
        poisoned[b, 0 if b < nf else n:] = float("nan")
    assert torch.isnan(poisoned[:nf]).all()
    pout, phs = m(poisoned, mask_of(lengths, T), output_hidden_states=True)
    assert same(out, pout) and same(hs, phs)
    h = Handle(cfg, sd, cfg["output_size"])
    try:
        for x in (xd, poisoned):
            c_out, c_hs, _ = h.run(x, lengths, hidden=True)
            assert same(c_out, out) and same(c_hs, hs)
    finally:
        h.close()


def test_only_rows_without_frames():
    """Every row is frameless, but T still gives frames: zeros everywhere and no error."""
    cfg, sd, m = tiny()
    xd, lengths = frameless_batch()
    T, nf = xd.shape[1], len(FRAMELESS)
    x = xd[:nf].contiguous()
    x[:] = float("nan")
    out, hs = m(x, mask_of(lengths[:nf], T), output_hidden_states=True)
    assert out.shape == (nf, cfg["output_size"], 65) and hs.shape == (cfg["num_hidden_layers"] + 1, nf, 129, cfg["hidden_size"])
    assert not bits(out).any() and not bits(hs).any()
    h = Handle(cfg, sd, cfg["output_size"])
    try:
        c_out, c_hs, _ = h.run(x, lengths[:nf], hidden=True)        # out and hs start as NaN: every element was written
    finally:
        h.close()
    assert not bits(c_out).any() and not bits(c_hs).any()
