"""GPU: the wav2vec2 / HuBERT encoder (vocoder_amd/csrc/w2v.hip) through the C ABI and ``vocoder_amd.modules.encoders.HubertEncoder``.

Values are compared with the reference's goldens (every row run ALONE through the reference on the CPU) and with the float64 restatement
(w2v_reference.py) at the project's parity bar, max |d| <= 1e-4 of the expected tensor's own peak; the reference's own fp32 sits near 2e-6 of
its fp64 on these shapes, so the bar does not hide a wrong tap, a swapped head or a key too many.  Everything else is bit-exact: a row alone /
in a batch / in another order / padded / through forward_list, NaN padding against zero padding, exact zeros past a row's frames.  Each
parity case prints what it measured.  Nothing here reads the reference or imports ``transformers``."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import w2v_reference as wref
from vocoder_amd import _lib
from vocoder_amd import synthetic as syn
from vocoder_amd.modules.encoders import HubertEncoder
from w2v_cases import BAR, Handle, bits, mask_of, parity, same     # noqa: F401  (shared with test_gpu_w2v_shapes.py)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("tiny", "shape")
EDGE_FRAMES = (1, 31, 32, 33, 127, 128, 129)       # around the attention's key tile (32) and query block (128)


@functools.lru_cache(maxsize=None)
def golden(name):
    g = np.load(os.path.join(GOLDEN, f"hubert_{name}.npz"))
    cfg = json.loads(bytes(g["config"]).decode())
    return cfg, syn.hubert_state_dict(cfg, int(g["seed"])), {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def module(name):
    cfg, sd, _ = golden(name)
    m = HubertEncoder(config={k: v for k, v in cfg.items() if k != "output_size"}, output_size=cfg["output_size"])
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().cuda()


@functools.lru_cache(maxsize=None)
def restated(name, row):
    cfg, sd, g = golden(name)
    return wref.forward(sd, cfg, g["waves"][row, : int(g["lengths"][row])])


@pytest.mark.parametrize("name", FIXTURES)
def test_goldens_through_the_module(name):
    cfg, _, g = golden(name)
    m, lengths, waves = module(name), g["lengths"].tolist(), torch.from_numpy(g["waves"]).cuda()
    batch = m(waves, mask_of(lengths, waves.shape[1])).cpu().numpy()
    assert batch.shape == (len(lengths), cfg["output_size"], m.frames(waves.shape[1]))
    for b, n in enumerate(lengths):
        want = g[f"out_{b}"]
        alone = m(waves[b:b + 1, :n]).cpu().numpy()
        parity(f"golden hubert_{name} row {b} alone (module)", alone[0], want)
        parity(f"golden hubert_{name} row {b} in the ragged batch (module)", batch[b, :, : want.shape[1]], want)
        assert not bits(batch[b, :, want.shape[1]:]).any()
    # (B, 1, T) with a (B, 1, T) mask is the same call
    assert same(m(waves[:, None], mask_of(lengths, waves.shape[1])[:, None]), batch)


@pytest.mark.parametrize("name", FIXTURES)
def test_goldens_through_the_c_abi(name):
    cfg, sd, g = golden(name)
    lengths, waves = g["lengths"].tolist(), torch.from_numpy(g["waves"]).cuda()
    for post, key in ((cfg["output_size"], "out"), (0, "last_hidden_state")):
        h = Handle(cfg, sd, post)
        try:
            batch = h.run(waves, lengths)[0].cpu().numpy()
            for b, n in enumerate(lengths):
                want = g[f"{key}_{b}"]
                alone = h.run(waves[b:b + 1, :n].contiguous(), None)[0].cpu().numpy()[0]
                row = batch[b]
                if post:
                    valid, rest = row[:, : want.shape[1]], row[:, want.shape[1]:]
                else:
                    valid, rest = row[: want.shape[0]], row[want.shape[0]:]
                parity(f"golden hubert_{name} {key} row {b} alone (C ABI)", alone, want)
                parity(f"golden hubert_{name} {key} row {b} in the ragged batch (C ABI)", valid, want)
                assert same(alone, valid) and not bits(rest).any()
        finally:
            h.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_every_hidden_state_against_the_restatement(name):
    cfg, _, g = golden(name)
    m, lengths, waves = module(name), g["lengths"].tolist(), torch.from_numpy(g["waves"]).cuda()
    out, hs = m(waves, mask_of(lengths, waves.shape[1]), output_hidden_states=True)
    hs = hs.cpu().numpy()
    nl = cfg["num_hidden_layers"]
    assert hs.shape == (nl + 1, len(lengths), m.frames(waves.shape[1], backbone=True), cfg["hidden_size"])
    assert same(out, m(waves, mask_of(lengths, waves.shape[1])))
    for b in range(len(lengths)):
        want = restated(name, b)["hidden_states"]
        F = want.shape[1]
        for layer in range(nl + 1):
            parity(f"hubert_{name} row {b} hidden state {layer}", hs[layer, b, :F], want[layer])
        assert not bits(hs[:, b, F:]).any()                                       # exact zeros past the row's frames, in every hidden state
    b = int(g["hidden_row"])
    parity(f"golden hubert_{name} hidden states of row {b}", hs[:-1, b, : g["hidden_states"].shape[1]], g["hidden_states"])


@pytest.mark.parametrize("name", FIXTURES)
def test_a_row_has_the_same_bits_alone_batched_reordered_padded_and_listed(name):
    _, _, g = golden(name)
    m, lengths, waves = module(name), g["lengths"].tolist(), torch.from_numpy(g["waves"]).cuda()
    B, T = waves.shape
    out, hs = m(waves, mask_of(lengths, T), output_hidden_states=True)
    order = list(range(B))[::-1]
    rev, rev_hs = m(waves[order].contiguous(), mask_of([lengths[i] for i in order], T), output_hidden_states=True)
    wide = torch.zeros(B, T + 777, device="cuda")
    wide[:, :T] = waves
    pad, pad_hs = m(wide, mask_of(lengths, T + 777), output_hidden_states=True)
    listed = m.forward_list([waves[b, :n] for b, n in enumerate(lengths)])
    for b, n in enumerate(lengths):
        F, F2 = m.frames(n, backbone=True), m.frames(n)
        alone, alone_hs = m(waves[b:b + 1, :n], output_hidden_states=True)
        assert alone.shape[2] == F2 and alone_hs.shape[2] == F
        assert same(alone[0], out[b, :, :F2]) and same(alone_hs[:, 0], hs[:, b, :F])
        assert same(rev[order.index(b)], out[b]) and same(rev_hs[:, order.index(b)], hs[:, b])
        assert same(pad[b, :, :F2], out[b, :, :F2]) and same(pad_hs[:, b, :F], hs[:, b, :F])
        assert not bits(pad[b, :, F2:]).any() and not bits(pad_hs[:, b, F:]).any() and not bits(out[b, :, F2:]).any()
        assert listed[b].shape == (out.shape[1], F2) and same(listed[b], out[b, :, :F2])


@pytest.mark.parametrize("name", FIXTURES)
def test_poisoned_padding_is_never_read(name):
    _, _, g = golden(name)
    m, lengths, waves = module(name), g["lengths"].tolist(), torch.from_numpy(g["waves"]).cuda()
    T = waves.shape[1]
    poisoned = waves.clone()
    for b, n in enumerate(lengths):
        poisoned[b, n:] = float("nan")
    assert torch.isnan(poisoned).any()
    out, hs = m(waves, mask_of(lengths, T), output_hidden_states=True)
    pout, phs = m(poisoned, mask_of(lengths, T), output_hidden_states=True)
    assert same(out, pout) and same(hs, phs)


def edge_wave(F, seed=5):
    """A wave that hubert_tiny's two conv layers turn into exactly F frames: 2 F + 1 after layer 0, so 10 F + 10 samples."""
    return np.random.default_rng(seed * 1000 + F).standard_normal(10 * F + 10).astype(np.float32)


@pytest.mark.parametrize("F", EDGE_FRAMES)
def test_attention_edges_against_the_restatement(F):
    cfg, sd, _ = golden("tiny")
    m, wave = module("tiny"), edge_wave(F)
    assert m.frames(len(wave), backbone=True) == F
    want = wref.forward(sd, cfg, wave)
    out, hs = m(torch.from_numpy(wave)[None].cuda(), output_hidden_states=True)
    for layer in range(cfg["num_hidden_layers"] + 1):
        parity(f"hubert_tiny {F} frames hidden state {layer}", hs[layer, 0].cpu().numpy(), want["hidden_states"][layer])
    parity(f"hubert_tiny {F} frames out", out[0].cpu().numpy(), want["out"])


def test_a_one_frame_row_beside_a_long_one():
    cfg, sd, _ = golden("tiny")
    m = module("tiny")
    short, long = edge_wave(1), edge_wave(129)
    x = torch.zeros(2, len(long), device="cuda")
    x[0, : len(short)] = torch.from_numpy(short).cuda()
    x[1] = torch.from_numpy(long).cuda()
    out, hs = m(x, mask_of([len(short), len(long)], len(long)), output_hidden_states=True)
    for b, wave in enumerate((short, long)):
        want = wref.forward(sd, cfg, wave)
        F, F2 = want["hidden_states"].shape[1], want["out"].shape[1]
        parity(f"one frame beside 129: row {b} last hidden state", hs[-1, b, :F].cpu().numpy(), want["hidden_states"][-1])
        parity(f"one frame beside 129: row {b} out", out[b, :, :F2].cpu().numpy(), want["out"])
        assert not bits(out[b, :, F2:]).any() and not bits(hs[:, b, F:]).any()
        alone = m(torch.from_numpy(wave)[None].cuda())
        assert same(alone[0], out[b, :, :F2])


@pytest.mark.parametrize("F", (257, 100, 50))
def test_the_wide_gemm_tiles_give_the_bits_of_the_narrow_one(F):
    """The GEMM takes 128 x 128 tiles where those give every compute unit a workgroup, 64 x 128 or 64 x 64 where they do not; the tests above
    are too small for anything but 64 x 64.  128 rows of F = 257 frames put every product of the network on 128 x 128 tiles; F = 100 puts
    layer 0 on 128 x 128, the second conv and the transformer on 64 x 128 and the strided post conv on 64 x 64; F = 50 puts layer 0, the one
    product that loads single floats, on 64 x 128.  A row's bits are those of the row run alone (64 x 64 tiles), and its values are the
    restatement's."""
    cfg, sd, _ = golden("tiny")
    m, B = module("tiny"), 128
    lengths = [10 * (F - (b % 3) * (F // 7)) + 10 for b in range(B)]      # three lengths, ragged inside the wide tiles
    rng = np.random.default_rng(9000 + F)
    x = np.zeros((B, max(lengths)), np.float32)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.standard_normal(n).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    out, hs = m(xd, mask_of(lengths, x.shape[1]), output_hidden_states=True)
    for b in (0, 1, 2, B - 1):
        n = lengths[b]
        Fb, F2 = m.frames(n, backbone=True), m.frames(n)
        alone, alone_hs = m(xd[b:b + 1, :n], output_hidden_states=True)
        assert same(alone[0], out[b, :, :F2]) and same(alone_hs[:, 0], hs[:, b, :Fb])
        assert not bits(out[b, :, F2:]).any() and not bits(hs[:, b, Fb:]).any()
    want = wref.forward(sd, cfg, x[1, : lengths[1]])
    parity(f"128 rows of up to {F} frames: row 1 last hidden state", hs[-1, 1, : want["hidden_states"].shape[1]].cpu().numpy(), want["hidden_states"][-1])
    parity(f"128 rows of up to {F} frames: row 1 out", out[1, :, : want["out"].shape[1]].cpu().numpy(), want["out"])


@pytest.mark.parametrize("name", FIXTURES)
def test_the_workspace_it_asks_for_is_enough(name):
    cfg, sd, g = golden(name)
    lengths, waves = g["lengths"].tolist(), torch.from_numpy(g["waves"]).cuda()
    h = Handle(cfg, sd, cfg["output_size"])
    try:
        guard = 1 << 16
        out, hs, ws = h.run(waves, lengths, hidden=True, guard=guard)
        assert bool((ws[-guard:] == 0xA5).all())                      # nothing was written past the bytes it asked for
        assert not torch.isnan(out).any() and not torch.isnan(hs).any()         # every element of both outputs was written
        m_out, m_hs = module(name)(waves, mask_of(lengths, waves.shape[1]), output_hidden_states=True)
        assert same(out, m_out) and same(hs, m_hs)
        need = int(h.L.fv_w2v_workspace_bytes(h.h, *waves.shape))
        st = h.L.fv_w2v_forward(h.h, waves.data_ptr(), waves.shape[1], None, waves.shape[0], out.data_ptr(), None, ws.data_ptr(), need - 4, None)
        assert st == _lib.FV_ERR_INVALID and "workspace" in h.L.fv_last_error().decode()
        B, T = waves.shape
        st = h.L.fv_w2v_forward(h.h, waves.data_ptr(), T, (ctypes.c_int32 * B)(*([1] * (B - 1) + [T + 1])), B, out.data_ptr(), None, ws.data_ptr(), need, None)
        assert st == _lib.FV_ERR_INVALID and f"host_lengths[{B - 1}]" in h.L.fv_last_error().decode()
    finally:
        h.close()
