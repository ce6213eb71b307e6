"""GPU: the posterior encoder (vocoder_amd/csrc/wavenet.hip) through the C ABI, ``vocoder_amd.modules.encoders.PosteriorEncoder`` and
``vocoder_amd.codec``.

Values are compared with the reference's goldens and with the float64 restatement (posterior_reference.py) at the project's parity bar,
max |d| <= 1e-4 of the expected tensor's own peak; the reference's own fp32 sits within 1e-6 of its fp64 on these shapes, so the bar does not
hide a wrong tap or a swapped half.  Everything else is bit-exact: a row alone / in a batch / padded, NaN padding against zero padding, the
reach.  Each parity case prints what it measured."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import posterior_reference as pref
from vocoder_amd import _lib
from vocoder_amd import synthetic as syn
from vocoder_amd.modules.encoders import PosteriorEncoder

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("vqvae", "vae", "bnvae")
BAR = 1e-4
NAMES = {"vqvae": ("y",), "vae": ("z", "mean", "logvar"), "bnvae": ("z", "mean", "logvar")}


def bits(a) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b) -> bool:
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_cfg(C, k, rate, cycle, nl, cin, out, mode):
    return dict(in_channels=cin, out_channels=out, hidden_channels=C, kernel_size=k, dilation_rate=rate, dilation_cycle=cycle, n_layers=nl, mode=mode)


def make_module(cfg, sd):
    m = PosteriorEncoder(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().cuda()


def make_input(cfg, B, T, seed):
    return np.random.default_rng(seed).standard_normal((B, cfg["in_channels"], T)).astype(np.float32)


def as_dict(mode, res):
    return {"y": res} if mode == "vqvae" else dict(zip(("z", "mean", "logvar", "mask"), res))


class Handle:
    """A finalized fv_posterior with the calls the tests make on the C ABI."""

    def __init__(self, cfg, sd):
        self.cfg, self.L, self.h = cfg, _lib.lib(), ctypes.c_void_p()
        c = _lib.PosteriorConfig(cfg["in_channels"], cfg["out_channels"], cfg["hidden_channels"], cfg["kernel_size"], cfg["dilation_rate"],
                                 cfg["dilation_cycle"], cfg["n_layers"], _lib.POSTERIOR_MODES[cfg["mode"]])
        _lib.check(self.L.fv_posterior_create(ctypes.byref(c), ctypes.byref(self.h)))
        for k, v in sd.items():
            a = np.ascontiguousarray(v, np.float32)
            _lib.check(self.L.fv_posterior_load_weight(self.h, k.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                       (ctypes.c_int64 * max(a.ndim, 1))(*a.shape), a.ndim))
        _lib.check(self.L.fv_posterior_finalize(self.h))

    def need(self, B, T):
        return int(self.L.fv_posterior_workspace_bytes(self.h, B, T))

    def forward(self, x, lengths, z, mean, logvar, ws_ptr, ws_bytes, stride=None):
        B, _, T = x.shape
        lp = None if lengths is None else (ctypes.c_int32 * B)(*lengths)
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        return self.L.fv_posterior_forward(self.h, x.data_ptr(), x.stride(1) if stride is None else stride, lp, ptr(z), ptr(mean), ptr(logvar), B, T,
                                           ws_ptr, ws_bytes, int(torch.cuda.current_stream().cuda_stream))

    def close(self):
        torch.cuda.synchronize()
        self.L.fv_posterior_destroy(self.h)


@functools.lru_cache(maxsize=None)
def golden(mode):
    g = np.load(os.path.join(GOLDEN, f"posterior_{mode}.npz"))
    cfg = json.loads(bytes(g["config"]).decode())
    return cfg, syn.posterior_state_dict(cfg, int(g["seed"])), {k: g[k] for k in g.files}


def check_parity(tag, mode, got, want, lengths, T):
    """got: device tensors by name; want: arrays by name.  The bar on every tensor; exact zeros past each length in y, z and logvar."""
    pad = np.arange(T)[None, :] >= np.asarray(lengths)[:, None]
    for k in NAMES[mode]:
        a, w = got[k].cpu().numpy(), np.asarray(want[k])
        err = np.abs(a - w).max() / max(np.abs(w).max(), 1e-30)
        print(f"{tag} {k}: max |d| / peak = {err:.2e} (peak {np.abs(w).max():.3g})")
        assert a.shape == w.shape and np.isfinite(a).all() and err <= BAR, (tag, k, err)
        if k != "mean":
            assert not bits(a.transpose(0, 2, 1)[pad]).any(), (tag, k)
    if mode != "vqvae":
        m = got["mask"].cpu().numpy()
        assert m.shape == (len(lengths), 1, T) and m.dtype == np.float32 and np.array_equal(m[:, 0] == 0, pad) and np.array_equal(m[:, 0] == 1, ~pad)


@pytest.mark.parametrize("mode", MODES)
def test_goldens_through_the_c_abi_and_the_module(mode):
    cfg, sd, g = golden(mode)
    lengths, (B, _, T) = g["lengths"].tolist(), g["x"].shape
    x = torch.from_numpy(g["x"]).cuda()
    got = as_dict(mode, make_module(cfg, sd)(x, torch.tensor(lengths)))
    check_parity(f"golden {mode} (module)", mode, got, g, lengths, T)
    if mode == "bnvae":      # the mean of a padded frame is BN(0), what the reference returns there
        pad = np.arange(T)[None, :] >= np.asarray(lengths)[:, None]
        d = np.abs(got["mean"].cpu().numpy() - g["mean"]).transpose(0, 2, 1)[pad].max()
        assert d <= BAR * np.abs(g["mean"]).max() and np.abs(g["mean"].transpose(0, 2, 1)[pad]).min() > 0
    h = Handle(cfg, sd)
    try:
        O = cfg["out_channels"]
        outs = {k: torch.full((B, O, T), 7.5, device="cuda") for k in NAMES[mode]}
        ws = torch.empty(h.need(B, T), dtype=torch.uint8, device="cuda")
        assert h.forward(x, lengths, outs.get("z", outs.get("y")), outs.get("mean"), outs.get("logvar"), ws.data_ptr(), ws.numel()) == 0, h.L.fv_last_error()
        torch.cuda.synchronize()
        for k in NAMES[mode]:
            assert same(outs[k], got[k]), k             # the module is the C ABI
        if mode != "vqvae":                             # each of mean / logvar may be left out
            z2 = torch.empty_like(outs["z"])
            assert h.forward(x, lengths, z2, None, None, ws.data_ptr(), ws.numel()) == 0
            assert same(z2, outs["z"])
    finally:
        h.close()


# (C, k, rate, cycle, n_layers, T, in_channels, out_channels, mode, lengths or batch)
CASES = [
    (32, 5, 1, 1, 2, 31, 20, 8, "vqvae", 2),
    (48, 5, 1, 1, 2, 129, 20, 8, "vae", [129, 64]),
    (192, 5, 1, 1, 1, 31, 20, 16, "vqvae", [31, 5]),
    (8, 5, 1, 1, 2, 300, 1, 3, "bnvae", [300, 129, 128]),
    (32, 1, 1, 1, 2, 2, 20, 8, "vae", [2, 1]),
    (32, 3, 2, 3, 4, 129, 20, 8, "vqvae", [129, 1]),
    (48, 7, 3, 2, 4, 300, 20, 8, "bnvae", [300, 200]),
    (32, 7, 1, 1, 1, 1, 20, 8, "vae", 1),
    (48, 3, 3, 2, 2, 31, 513, 40, "vqvae", [31, 30]),
    (192, 3, 2, 3, 4, 129, 20, 70, "vae", [100, 129]),
    (8, 7, 2, 3, 4, 31, 20, 8, "bnvae", [31, 0, 2]),
    (32, 5, 2, 3, 4, 300, 1, 8, "vqvae", 1),
    (48, 1, 1, 1, 1, 129, 20, 8, "bnvae", [129, 77]),
    (8, 3, 1, 1, 1, 2, 513, 8, "vae", [2, 2]),
    (192, 7, 3, 2, 2, 129, 20, 8, "vqvae", [129, 128]),
    (32, 5, 3, 2, 2, 64, 20, 8, "vae", [64, 33]),         # the widest T of the 32-column tile ...
    (32, 5, 3, 2, 2, 65, 20, 8, "vae", [65, 33]),         # ... and the narrowest of the 128-column one
    (48, 5, 1, 1, 4, 1, 20, 8, "bnvae", 2),
    (8, 1, 1, 1, 2, 31, 1, 1, "vqvae", [31, 3]),
    (192, 5, 1, 1, 4, 300, 513, 32, "vae", [300, 1]),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "C{}-k{}-r{}c{}-n{}-T{}-in{}-out{}-{}".format(*c[:9]))
def test_against_the_float64_restatement(case):
    C, k, rate, cycle, nl, T, cin, out, mode, rows = case
    cfg = make_cfg(C, k, rate, cycle, nl, cin, out, mode)
    lengths = rows if isinstance(rows, list) else None
    B = len(rows) if lengths else rows
    sd = syn.posterior_state_dict(cfg, seed=C + k)
    x = make_input(cfg, B, T, seed=T)
    want = pref.forward(cfg, sd, x, lengths)
    got = as_dict(mode, make_module(cfg, sd)(torch.from_numpy(x).cuda(), lengths))
    check_parity("C {} k {} rate {} cycle {} layers {} T {} in {} out {} {}".format(*case[:9]), mode, got, want, lengths or [T] * B, T)


def test_the_clamp_of_logvar():
    cfg = make_cfg(32, 3, 1, 1, 2, 20, 8, "vae")
    sd = syn.posterior_state_dict(cfg, 3)
    sd["proj.weight"] = sd["proj.weight"] * 60.0
    x = make_input(cfg, 2, 31, 5)
    want = pref.forward(cfg, sd, x, [31, 20])
    assert (want["logvar"] == 20.0).any() and (want["logvar"] == -30.0).any()
    got = as_dict("vae", make_module(cfg, sd)(torch.from_numpy(x).cuda(), [31, 20]))
    check_parity("clamp", "vae", got, want, [31, 20], 31)
    lv = got["logvar"].cpu().numpy()
    assert lv.max() == 20.0 and lv.min() == -30.0


@pytest.mark.parametrize("mode,T", [("vae", 131), ("bnvae", 40)])
def test_padding_is_never_read(mode, T):
    cfg = make_cfg(48, 5, 2, 3, 3, 20, 8, mode)
    m = make_module(cfg, syn.posterior_state_dict(cfg, 1))
    lengths = [T, T // 2, 1]
    x = make_input(cfg, 3, T, 2)
    outs = []
    for fill in (float("nan"), 0.0):
        buf = torch.full((3, 20, T + 5), fill, device="cuda")      # slack beyond T, reached only through x_row_stride
        for b, n in enumerate(lengths):
            buf[b, :, :n] = torch.from_numpy(x[b, :, :n])
        view = buf[:, :, :T]
        assert view.stride(1) == T + 5
        outs.append(m(view, lengths))
    for a, z in zip(outs[0][:3], outs[1][:3]):
        assert torch.isfinite(a).all() and same(a, z)


@pytest.mark.parametrize("mode", ["vqvae", "bnvae"])
def test_a_row_has_the_same_bits_alone_in_a_batch_and_padded(mode):
    T = 70
    cfg = make_cfg(48, 5, 2, 2, 3, 20, 8, mode)
    sd = syn.posterior_state_dict(cfg, 4)
    m = make_module(cfg, sd)
    lengths = [T, 7, 0, T - 1]
    x = torch.from_numpy(make_input(cfg, 4, T, 6)).cuda()
    full = as_dict(mode, m(x, lengths))
    for b, n in enumerate(lengths):
        padded = as_dict(mode, m(x[b:b + 1], [n]))                  # a batch of one, padded to T
        for k in NAMES[mode]:
            assert same(padded[k], full[k][b:b + 1]), (b, k)
        if n:
            alone = as_dict(mode, m(x[b:b + 1, :, :n]))             # the row alone at T = lengths[b]: the 32-column tile for 7 frames
            for k in NAMES[mode]:
                assert same(alone[k], full[k][b:b + 1, :, :n]), (b, k)
    for k in NAMES[mode]:      # the length-0 row
        if k == "mean" and mode == "bnvae":
            row = full[k][2].cpu().numpy()
            want = pref.forward(cfg, sd, np.zeros((1, 20, T), np.float32), [0])["mean"][0]
            assert np.array_equal(row, np.broadcast_to(row[:, :1], row.shape)) and np.abs(row - want).max() <= BAR * np.abs(want).max()
        else:
            assert not bits(full[k][2]).any()


def test_more_rows_than_one_launch_table():
    """256 lengths travel with a launch: 258 rows cross the table's edge."""
    B, T = 258, 3
    cfg = make_cfg(8, 3, 1, 1, 2, 5, 4, "bnvae")
    sd = syn.posterior_state_dict(cfg, 8)
    m = make_module(cfg, sd)
    lengths = np.random.default_rng(1).integers(0, T + 1, B).tolist()
    lengths[255], lengths[256], lengths[257] = 3, 2, 3
    xn = make_input(cfg, B, T, 9)
    x = torch.from_numpy(xn).cuda()
    full = as_dict("bnvae", m(x, lengths))
    check_parity("258 rows", "bnvae", full, pref.forward(cfg, sd, xn, lengths), lengths, T)
    for lo, hi in ((0, 256), (256, 258), (255, 257)):
        part = as_dict("bnvae", m(x[lo:hi], lengths[lo:hi]))
        for k in NAMES["bnvae"]:
            assert same(part[k], full[k][lo:hi]), (lo, k)


def test_reach():
    cfg = make_cfg(32, 3, 2, 2, 3, 20, 8, "vqvae")          # dilations 1, 2, 1
    m = make_module(cfg, syn.posterior_state_dict(cfg, 2))
    R, T, t = m.reach_frames, 40, 20
    assert R == 4
    xn = make_input(cfg, 1, T, 3)
    far = np.abs(np.arange(T) - t) > R
    other = xn.copy()
    other[:, :, far] = make_input(cfg, 1, T, 4)[:, :, far]
    y = m(torch.from_numpy(xn).cuda())
    assert same(m(torch.from_numpy(other).cuda())[:, :, t], y[:, :, t])
    for edge in (t - R, t + R):
        moved = xn.copy()
        moved[:, :, edge] += 1.0
        assert not same(m(torch.from_numpy(moved).cuda())[:, :, t], y[:, :, t])


def test_workspace_and_refusals_enqueue_nothing():
    cfg = make_cfg(32, 5, 1, 1, 2, 20, 8, "vae")
    sd = syn.posterior_state_dict(cfg, 5)
    B, T, lengths = 2, 33, [33, 10]
    x = torch.from_numpy(make_input(cfg, B, T, 1)).cuda()
    h = Handle(cfg, sd)
    try:
        need = h.need(B, T)
        assert need == 3 * B * 32 * T * 4
        guard = 256
        buf = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
        z, mean, logvar = (torch.full((B, 8, T), 3.5, device="cuda") for _ in range(3))
        L = h.L
        for kw, word in ((dict(ws_bytes=need - 1), "workspace"), (dict(stride=T - 1), "x_row_stride"), (dict(lengths=[3, T + 1]), "host_lengths[1]"),
                         (dict(lengths=[-1, 2]), "host_lengths[0]")):
            args = dict(lengths=lengths, ws_bytes=need, stride=None)
            args.update(kw)
            st = h.forward(x, args["lengths"], z, mean, logvar, buf.data_ptr() + guard, args["ws_bytes"], stride=args["stride"])
            assert st == _lib.FV_ERR_INVALID and word in L.fv_last_error().decode(), (kw, L.fv_last_error())
            torch.cuda.synchronize()
            assert (z == 3.5).all() and (mean == 3.5).all() and (logvar == 3.5).all() and (buf == 0xA5).all()         # nothing was written
        assert h.forward(x, lengths, z, mean, logvar, buf.data_ptr() + guard, need) == 0, L.fv_last_error()
        torch.cuda.synchronize()
        assert (buf[:guard] == 0xA5).all() and (buf[-guard:] == 0xA5).all()                 # the workspace's exact size is all it touches
        want = pref.forward(cfg, sd, x.cpu().numpy(), lengths)
        check_parity("workspace", "vae", dict(z=z, mean=mean, logvar=logvar, mask=torch.from_numpy(want["mask"].astype(np.float32))), want, lengths, T)
        # batch = 0 and T = 0 do nothing
        assert h.forward(x[:0], None, None, None, None, None, 0) == 0 and h.forward(x[:, :, :0], None, None, None, None, None, 0) == 0
    finally:
        h.close()
    hq = Handle(make_cfg(32, 5, 1, 1, 2, 20, 8, "vqvae"), syn.posterior_state_dict(make_cfg(32, 5, 1, 1, 2, 20, 8, "vqvae"), 5))
    try:
        z = torch.full((B, 8, T), 3.5, device="cuda")
        ws = torch.empty(hq.need(B, T), dtype=torch.uint8, device="cuda")
        assert hq.forward(x, None, z, z, None, ws.data_ptr(), ws.numel()) == _lib.FV_ERR_INVALID and "d_mean" in hq.L.fv_last_error().decode()
        torch.cuda.synchronize()
        assert (z == 3.5).all()
    finally:
        hq.close()


def test_codec_with_the_posterior_encoder():
    from vocoder_amd import codec
    torch.manual_seed(0)
    m = codec.build_vqvae(n_fft=64, hop_length=16, win_length=64, latent_size=32, codebook_size=48, decoder_depths=(1, 1), decoder_dims=(32, 64),
                          encoder="posterior", hidden_channels=24, posterior_layers=3, posterior_kernel_size=3)
    assert isinstance(m.encoder, PosteriorEncoder) and m.encoder.mode == "vqvae" and m.encoder.out_channels == 32 and m.encoder.in_channels == 33
    m = m.eval().cuda()
    T, lengths = 11, [11, 4, 0]
    spec = torch.from_numpy(np.abs(np.random.default_rng(0).standard_normal((3, 33, T))).astype(np.float32)).cuda()
    codes = m.encode(spec, lengths)
    assert codes.dtype == torch.int64 and codes.shape == (3, T)
    for b, n in enumerate(lengths):
        assert (codes[b, n:] == -1).all()
        if n:       # the latent of a row is bit-identical to the row's alone, so the codes are too
            assert torch.equal(m.encode(spec[b:b + 1, :, :n])[0], codes[b, :n])
    audio = (0.1 * torch.randn(2, 1, 16 * 9, generator=torch.Generator().manual_seed(1))).cuda()
    y = m.decode(m.encode(audio))
    assert y.shape == (2, 1, 16 * 9) and torch.isfinite(y).all()
    fake, aux = m(audio)
    assert fake.shape == audio.shape and aux == 0 and same(fake, y)


def test_module_behaviour():
    cfg = make_cfg(32, 3, 1, 1, 2, 20, 8, "vae")
    sd = syn.posterior_state_dict(cfg, 6)
    m = make_module(cfg, sd)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m(torch.zeros(1, 20, 4))
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train()(torch.zeros(1, 20, 4, device="cuda"))
    m.eval()
    with pytest.raises(ValueError, match="x_lengths"):
        m(torch.zeros(2, 20, 4, device="cuda"), [1, 5])
    xs = [torch.from_numpy(make_input(cfg, 1, n, n)[0]).cuda() for n in (9, 1, 40)]
    padded = torch.zeros(3, 20, 40, device="cuda")
    for b, x in enumerate(xs):
        padded[b, :, : x.shape[1]] = x
    z = m(padded, [9, 1, 40])[0]
    for b, (x, row) in enumerate(zip(xs, m.forward_list(xs))):
        assert row.shape == (8, x.shape[1]) and same(row, z[b, :, : x.shape[1]])
    assert m.forward_list([]) == []
    # the handle follows the weights
    before = m(padded)[0]
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in syn.posterior_state_dict(cfg, 7).items()}, strict=True)
    after = m(padded)[0]
    want = pref.forward(cfg, syn.posterior_state_dict(cfg, 7), padded.cpu().numpy())["z"]
    assert not same(before, after) and np.abs(after.cpu().numpy() - want).max() <= BAR * np.abs(want).max()
