"""Host (no GPU): the critics' surface (include/fishvoc.h fv_disc_*, vocoder_amd/modules/discriminators, vocoder_amd/scoring.py) — the declared
entry points and the config mirror, the state dict's keys against the reference's recorded ones, the refusals that name their field, the
extents formula, and the float64 restatement (disc_reference.py) against the reference's goldens, loss numbers included.
For the configs of the shape sweep (disc_cases.py, run on the GPU by test_gpu_disc.py), which have no golden: float32 arithmetic alone stays
a factor of 10 under the parity bar, and the faults the sweep is there to catch move the restatement a factor of 10 above it."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import disc_cases as dc
import disc_reference as dref
from vocoder_amd import _lib
from vocoder_amd import synthetic as syn
from vocoder_amd.modules.discriminators import DiscriminatorP, DiscriminatorR, MultiPeriodDiscriminator, MultiResolutionDiscriminator
from vocoder_amd.scoring import CriticDistance, reference_losses

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_disc_create", "fv_disc_load_weight", "fv_disc_finalize", "fv_disc_destroy", "fv_disc_layout", "fv_disc_workspace_bytes",
           "fv_disc_forward", "fv_disc_distance")
BAR = dc.BAR
G, V = "parametrizations.weight.original0", "parametrizations.weight.original1"


def period_config(periods=(2, 3), widths=(1, 12, 36), **over):
    """``over``: field = value, or field = (index, value) for an array's element."""
    c = _lib.DiscConfig()
    c.kind, c.n_sub, c.n_channels, c.kernel_size, c.stride = _lib.FV_DISC_PERIOD, len(periods), len(widths), 5, 3
    for i, p in enumerate(periods):
        c.period[i] = p
    for i, ch in enumerate(widths):
        c.channels[i] = ch
    return apply(c, over)


def resolution_config(resolutions=((32, 6, 20), (32, 5, 24)), **over):
    c = _lib.DiscConfig()
    c.kind, c.n_sub = _lib.FV_DISC_RESOLUTION, len(resolutions)
    for i, (n, h, w) in enumerate(resolutions):
        c.n_fft[i], c.hop_length[i], c.win_length[i] = n, h, w
    return apply(c, over)


def apply(c, over):
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


def create(cfg):
    L, h = _lib.lib(), ctypes.c_void_p()
    st = L.fv_disc_create(ctypes.byref(cfg), ctypes.byref(h))
    return st, h, L.fv_last_error().decode()


def load(h, name, arr):
    arr = np.ascontiguousarray(arr, np.float32)
    shape = (ctypes.c_int64 * max(arr.ndim, 1))(*arr.shape)
    return _lib.lib().fv_disc_load_weight(h, name.encode(), arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), shape, arr.ndim)


def test_entry_points_are_declared_exported_and_present():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_disc_\w+)\s*\(", hdr))
    assert declared == set(ENTRIES)
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    assert L.fv_abi_version() == 5 and _lib.FV_ABI_VERSION == 5
    for name in ENTRIES:        # each cites the reference lines it replaces
        comment = hdr[: hdr.index(f" {name}(")].rsplit("/*", 1)[1]
        assert re.search(r"(mpd|mrd|gan)\.py:\d+", comment), name


def test_config_mirror_matches_the_header_field_for_field():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    for struct, mirror, total in (("fv_disc_config", _lib.DiscConfig, 4 * (2 + 4 * 8 + 1 + 8 + 2)), ("fv_disc_map", _lib.DiscMap, 8 + 5 * 4 + 4)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        fields = []
        for ctype, names in re.findall(r"^\s*(int32_t|int64_t)\s+([^;]+);", body, re.M):
            for name in names.split(","):
                m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", name)
                fields.append((ctype, m.group(1), int(m.group(2) or 1)))
        assert [n for _, n, _ in fields] == [n for n, _ in mirror._fields_], struct
        for (ctype, name, dim), (_, mtype) in zip(fields, mirror._fields_):
            assert ctypes.sizeof(mtype) == (8 if ctype == "int64_t" else 4) * dim, (struct, name)
        assert ctypes.sizeof(mirror) == total, struct
    assert (_lib.FV_DISC_PERIOD, _lib.FV_DISC_RESOLUTION) == (0, 1) and "#define FV_DISC_RESOLUTION 1" in hdr


def test_constructor_signatures_defaults_and_aliases():
    from vocoder_amd import config
    sig = inspect.signature(DiscriminatorP.__init__)
    assert list(sig.parameters)[1:] == ["period", "kernel_size", "stride", "use_spectral_norm", "channels"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[1:])
    assert [p.default for p in list(sig.parameters.values())[2:]] == [5, 3, False, None]
    sig = inspect.signature(DiscriminatorR.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [("n_fft", 1024), ("hop_length", 120), ("win_length", 600),
                                                                             ("use_spectral_norm", False)]
    assert inspect.signature(MultiPeriodDiscriminator.__init__).parameters["periods"].default is None
    assert inspect.signature(MultiResolutionDiscriminator.__init__).parameters["resolutions"].default is inspect.Parameter.empty
    assert MultiPeriodDiscriminator().periods == [2, 3, 5, 7, 11] and DiscriminatorP(period=2).channels == [1, 64, 128, 256, 512, 1024]
    assert config.locate("fish_vocoder.modules.discriminators.mpd.MultiPeriodDiscriminator") is MultiPeriodDiscriminator
    assert config.locate("fish_vocoder.modules.discriminators.mpd.DiscriminatorP") is DiscriminatorP
    assert config.locate("fish_vocoder.modules.discriminators.mrd.DiscriminatorR") is DiscriminatorR
    m = config.instantiate({"_target_": "fish_vocoder.modules.discriminators.mrd.MultiResolutionDiscriminator", "resolutions": [[32, 6, 20]]})
    assert isinstance(m, MultiResolutionDiscriminator) and not m.training and not any(p.requires_grad for p in m.parameters())


@pytest.mark.parametrize("kind", dc.KINDS)
def test_state_dict_keys_are_the_references_and_load_strictly(kind):
    cfg, seed, g = dc.golden(kind)
    keys = json.loads(bytes(g["keys"]).decode())
    m = dc.module(kind, cfg)
    assert list(m.state_dict()) == keys
    sd = dc.state_dict(kind, cfg, seed)
    assert list(sd) == keys
    res = m.load_state_dict(dc.tensors(sd), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in sd.items():
        assert np.array_equal(m.state_dict()[k].numpy(), v), k
    missing = dict(dc.tensors(sd))
    del missing["discriminators.1.convs.2.bias"]
    with pytest.raises(RuntimeError, match=r"discriminators\.1\.convs\.2\.bias"):
        dc.module(kind, cfg).load_state_dict(missing, strict=True)
    with pytest.raises(RuntimeError, match=r"discriminators\.0\.conv_extra"):
        dc.module(kind, cfg).load_state_dict(dict(dc.tensors(sd), **{"discriminators.0.conv_extra.bias": torch.zeros(1)}), strict=True)
    # the single discriminators carry the same keys without the list's prefix
    single = DiscriminatorP(period=2, channels=cfg["channels"]) if kind == "mpd" else DiscriminatorR(n_fft=32, hop_length=6, win_length=20)
    assert ["discriminators.0." + k for k in single.state_dict()] == [k for k in keys if k.startswith("discriminators.0.")]


@pytest.mark.parametrize("kind", dc.KINDS)
def test_legacy_weight_norm_names_load(kind):
    cfg, seed, _ = dc.golden(kind)
    sd = dc.tensors(dc.state_dict(kind, cfg, seed))
    legacy = {k.replace(G, "weight_g").replace(V, "weight_v"): v for k, v in sd.items()}
    assert "discriminators.0.conv_post.weight_g" in legacy and not any("parametrizations" in k for k in legacy)
    m = dc.module(kind, cfg)
    res = m.load_state_dict(legacy, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())


@pytest.mark.parametrize("kind", dc.KINDS)
def test_synthetic_weights_are_what_the_issue_asks_for(kind):
    cfg, seed, g = dc.golden(kind)
    sd = dc.state_dict(kind, cfg, seed)
    for k in sd:
        if k.endswith(G):
            v = sd[k.replace(G, V)].astype(np.float64)
            ratio = sd[k].reshape(-1) / np.sqrt((v ** 2).sum((1, 2, 3)))
            assert sd[k].shape == (v.shape[0], 1, 1, 1) and np.abs(ratio - 1).min() > 0 and np.abs(ratio - 1).max() > 0.2, k
    assert all(np.abs(sd[k]).min() >= 0.02 for k in sd if k.endswith(".bias"))
    assert all(np.array_equal(a, sd[k]) for k, a in dc.state_dict(kind, cfg, seed).items())
    for i in range(len(dc.subs(kind, cfg))):        # O(1) activations through every layer
        assert all(0.05 < np.sqrt((f ** 2).mean()) < 20 for f in dc.golden_restated(kind, i, 0))


def test_load_weight_and_finalize_name_what_is_wrong():
    L = _lib.lib()
    cfg, seed, _ = dc.golden("mpd")
    sd = dc.state_dict("mpd", cfg, seed)
    st, h, msg = create(period_config(cfg["periods"], cfg["channels"]))
    assert st == 0, msg
    try:
        assert load(h, "discriminators.0.convs.9.bias", np.zeros(3)) == _lib.FV_ERR_INVALID and "discriminators.0.convs.9.bias" in L.fv_last_error().decode()
        assert load(h, "discriminators.1.convs.1." + V, np.zeros((36, 12, 3, 1))) == -4
        msg = L.fv_last_error().decode()
        assert "discriminators.1.convs.1." + V in msg and "(36, 12, 3, 1)" in msg and "(36, 12, 5, 1)" in msg
        assert load(h, "discriminators.2.conv_post.weight_g", np.zeros((2, 1, 1, 1))) == -4 and "(1, 1, 1, 1)" in L.fv_last_error().decode()
        skip = ("discriminators.2.convs.4.bias", "discriminators.0.convs.0." + G)
        for k, v in sd.items():
            if k not in skip:
                assert load(h, k, v) == 0, (k, L.fv_last_error())
        assert load(h, "discriminators.0.convs.0.weight_g", sd[skip[1]]) == 0        # the legacy name fills original0
        assert L.fv_disc_finalize(h) == -3 and skip[0] in L.fv_last_error().decode()   # before any device work
        assert L.fv_disc_forward(h, None, 100, None, 1, None, 0, None, 0, None) == _lib.FV_ERR_STATE
        assert L.fv_disc_workspace_bytes(h, -1, 5) == 0 and "batch" in L.fv_last_error().decode()
        assert L.fv_disc_layout(h, 1, (1 << 26) + 1, None, 0, None) == -1 and "T =" in L.fv_last_error().decode()
    finally:
        L.fv_disc_destroy(h)


@pytest.mark.parametrize("cfg,field", [
    (period_config(kind=2), "kind"), (period_config(n_sub=0), "n_sub"), (period_config(n_sub=9), "n_sub"),
    (period_config(n_channels=1), "n_channels"), (period_config(n_channels=9), "n_channels"),
    (period_config(kernel_size=0), "kernel_size"), (period_config(kernel_size=16), "kernel_size"),
    (period_config(stride=0), "stride"), (period_config(stride=17), "stride"),
    (period_config(channels=(0, 2)), "channels[0]"), (period_config(channels=(1, 0)), "channels[1]"), (period_config(channels=(2, 1028)), "channels[2]"),
    (period_config(channels=(1, 14)), "channels[1]"),
    (period_config(period=(0, 0)), "period[0]"), (period_config(period=(1, 4097)), "period[1]"),
    (resolution_config(n_fft=(0, 0)), "n_fft[0]"), (resolution_config(n_fft=(1, 4100)), "n_fft[1]"), (resolution_config(n_fft=(1, 30)), "n_fft[1]"),
    (resolution_config(hop_length=(0, 0)), "hop_length[0]"), (resolution_config(hop_length=(1, 33)), "hop_length[1]"),
    (resolution_config(win_length=(0, 0)), "win_length[0]"), (resolution_config(win_length=(1, 33)), "win_length[1]"),
])
def test_create_refuses_each_limit_by_name(cfg, field):
    st, h, msg = create(cfg)
    assert st == _lib.FV_ERR_INVALID and not h.value
    assert msg.startswith("fv_disc_create:") and f"{field} =" in msg, msg


def test_create_takes_the_default_critics_and_layout_gives_their_maps():
    L = _lib.lib()
    st, h, msg = create(period_config((3, 5, 7, 11, 17, 23, 37), dref.DEFAULT_CHANNELS))
    assert st == 0, msg
    n, maps = ctypes.c_int32(), (_lib.DiscMap * 42)()
    total = L.fv_disc_layout(h, 2, 44100, maps, 42, ctypes.byref(n))
    assert n.value == 42 and total > 0
    assert L.fv_disc_layout(h, 2, 44100, maps, 41, None) == -1 and "capacity" in L.fv_last_error().decode()
    offset = 0
    for i, p in enumerate((3, 5, 7, 11, 17, 23, 37)):
        for l, (hh, ww) in enumerate(dref.period_extents(44100, p)):
            m = maps[i * 6 + l]
            assert (m.sub, m.layer, m.H, m.W, m.C, m.offset) == (i, l, hh, ww, (list(dref.DEFAULT_CHANNELS) + [1])[l + 1], offset) and offset % 4 == 0
            offset += (2 * hh * ww * m.C + 3) // 4 * 4
    assert total == offset and L.fv_disc_workspace_bytes(h, 2, 44100) % 256 == 0
    L.fv_disc_destroy(h)
    st, h, msg = create(resolution_config(((2048, 512, 2048), (1024, 120, 600), (2048, 240, 1200))))
    assert st == 0, msg
    maps = (_lib.DiscMap * 18)()
    assert L.fv_disc_layout(h, 1, 44100, maps, 18, ctypes.byref(n)) > 0 and n.value == 18
    assert [(maps[6 + l].H, maps[6 + l].W) for l in range(6)] == dref.resolution_extents(44100, 1024, 120)
    assert L.fv_disc_workspace_bytes(h, 1, 44100) >= 4 * (44100 + 2048 + 2 * 86 * 2050)
    L.fv_disc_destroy(h)


def test_python_refusals():
    with pytest.raises(ValueError, match="use_spectral_norm"):
        DiscriminatorP(period=3, use_spectral_norm=True)
    with pytest.raises(ValueError, match="use_spectral_norm"):
        DiscriminatorR(use_spectral_norm=True)
    with pytest.raises(ValueError, match=r"channels\[1\] = 6"):
        DiscriminatorP(period=3, channels=[1, 6, 8])
    with pytest.raises(ValueError, match=r"period\[0\] = 0"):
        MultiPeriodDiscriminator([0, 2])
    with pytest.raises(ValueError, match=r"n_fft\[0\] = 30"):
        MultiResolutionDiscriminator([(30, 6, 20)])
    with pytest.raises(ValueError, match="1 to 8"):
        MultiPeriodDiscriminator(list(range(2, 11)))
    m = MultiResolutionDiscriminator([(32, 6, 20)])
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m(torch.zeros(1, 1, 100))
    with pytest.raises(ValueError, match="fp32 only"):
        m.precision = "f16x3"
    assert m.precision == "f32" and m.min_length() == 14
    with pytest.raises(ValueError, match="no critic"):
        CriticDistance()
    with pytest.raises(ValueError, match="key = 'msd'"):
        reference_losses(np.ones((1, 1, 6, 5)), "msd")


@pytest.mark.parametrize("kind", dc.KINDS)
def test_extents_equal_the_goldens_shapes(kind):
    cfg, _, g = dc.golden(kind)
    m = dc.module(kind, cfg)
    for b, n in enumerate(g["lengths"]):
        ext = m.extents(int(n))
        for i, sub in enumerate(dc.subs(kind, cfg)):
            shapes = [tuple(g[f"fmap_{b}_{i}_{l}"].shape[1:]) for l in range(6)]
            assert ext[i] == shapes == dc.extents(kind, sub, int(n)), (b, i)
    if kind == "mpd":
        assert [h for h, _ in m.extents(257)[0]] == [43, 15, 5, 2, 1, 1] and m.extents(23)[2][0] == (1, 37) and m.extents(1)[0][-1] == (1, 2)
        assert m.discriminators[0].extents(257) == m.extents(257)[0]
    else:
        assert [w for _, w in m.extents(200)[0]] == [33, 17, 9, 5, 5, 5] and m.extents(15)[0][0] == (17, 2)


def test_extents_equal_the_brute_force_rule():
    for p in (1, 2, 3, 11, 37):
        m = DiscriminatorP(period=p, channels=[1, 12, 36, 68, 100, 132])
        boundaries = [p * h + d for h in (1, 2, 3, 4, 6, 7, 9, 10, 27, 28, 81, 82) for d in (-1, 0, 1)]
        for n in list(range(0, 4 * p + 1)) + boundaries:
            h, want = -(-n // p), []
            for _ in range(5):
                h = dref.brute_force_extent(h, 5, 3, 2)
                want.append((h, p))
            want.append((dref.brute_force_extent(h, 3, 1, 1), p))
            assert m.extents(n) == want == dref.period_extents(n, p), (p, n)
    for n_fft, hop in ((32, 6), (32, 5), (1024, 120)):
        m = DiscriminatorR(n_fft=n_fft, hop_length=hop, win_length=n_fft // 2)
        for n in list(range(0, 4 * hop + 1)) + [hop * f + d for f in (2, 3, 4, 5, 8, 9, 16, 17, 33) for d in (-1, 0, 1)]:
            w, want = n // hop, []
            for kw, sw, pw in ((9, 1, 4), (9, 2, 4), (9, 2, 4), (9, 2, 4), (3, 1, 1), (3, 1, 1)):
                w = dref.brute_force_extent(w, kw, sw, pw) if w else 0
                want.append((n_fft // 2 + 1, w))
            assert m.extents(n) == want == dref.resolution_extents(n, n_fft, hop), (n_fft, hop, n)


@pytest.mark.parametrize("kind", dc.KINDS)
def test_restatement_against_the_references_goldens(kind):
    """Pins disc_reference to the real reference: every stored tensor."""
    cfg, _, g = dc.golden(kind)
    for b in range(len(g["lengths"])):
        scores = []
        for i in range(len(dc.subs(kind, cfg))):
            fm = dc.golden_restated(kind, i, b)
            for l, f in enumerate(fm):
                dc.parity(f"disc_{kind} row {b} sub {i} layer {l}", f, g[f"fmap_{b}_{i}_{l}"])
            scores.append(fm[-1].reshape(-1))
            if kind == "mpd":
                dc.parity(f"disc_mpd row {b} score {i}", scores[-1], g[f"score_{b}_{i}"])
        if kind == "mrd":
            dc.parity(f"disc_mrd row {b} scores", np.concatenate(scores), g[f"score_{b}"])


@pytest.mark.parametrize("kind", dc.KINDS)
def test_reference_losses_fed_the_restatements_sums_give_the_stored_numbers(kind):
    cfg, seed, g = dc.golden(kind)
    sd = dc.state_dict(kind, cfg, seed)
    sums = np.zeros((2, len(dc.subs(kind, cfg)), 6, 5))
    for i, sub in enumerate(dc.subs(kind, cfg)):
        layers = dref.folded_layers(sd, i, 5)
        for b in range(2):
            sums[b, i] = dref.distance_sums(dc.restate(kind, sub, layers, g["pair_real"][b]), dc.restate(kind, sub, layers, g["pair_fake"][b]))
    got = reference_losses(sums, kind)
    for j, name in enumerate(("adv", "fm", "disc")):
        err = abs(got[name] - g["pair_losses"][j]) / abs(g["pair_losses"][j])
        print(f"disc_{kind} {name}: {got[name]:.8g} against the reference's {g['pair_losses'][j]:.8g}, relative {err:.2e}")
        assert err <= BAR


def test_reference_losses_iterates_mrd_scores_by_row():
    """gan.py:148 / :203 on MRD's concatenated (B, sum n) scores: a mean per ROW over all resolutions, not per resolution over the batch.
    With resolutions of 10 and 30 scores the two rules give different numbers."""
    sums = np.zeros((2, 2, 6, 5))
    sums[..., 4] = 1
    sums[:, 0, -1] = [[0, 5.0, 1.0, 2.0, 10], [0, 7.0, 3.0, 4.0, 10]]
    sums[:, 1, -1] = [[0, 6.0, 2.0, 8.0, 30], [0, 9.0, 5.0, 1.0, 30]]
    mrd, mpd = reference_losses(sums, "mrd"), reference_losses(sums, "mpd")
    assert mrd["adv"] == pytest.approx((5 + 6) / 40 + (7 + 9) / 40) and mpd["adv"] == pytest.approx((5 + 7) / 20 + (6 + 9) / 60)
    assert mrd["disc"] == pytest.approx((2 + 8 + 1 + 2) / 40 + (4 + 1 + 3 + 5) / 40)
    assert mpd["disc"] == pytest.approx((2 + 4 + 1 + 3) / 20 + (8 + 1 + 2 + 5) / 60)


# -- conditions on the GPU sweep's inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", dc.SWEEP_CASES)
def test_float32_arithmetic_alone_stays_a_tenth_of_the_bar_at_every_sweep_config(name, L):
    """The restatement evaluated in float32 lies within BAR / 10 of the float64 one's peak in every feature map and score, so a kernel in
    exact fp32 has a factor of 10 of room under the bar."""
    kind, cfg, _ = dc.SWEEP[name]
    sub = dc.subs(kind, cfg)[0]
    want = dc.sweep_restated(name, L)
    got = dc.restate(kind, sub, dref.folded_layers(dc.sweep_state_dict(name), 0, 5, np.float32), dc.sweep_wave(name, L), dtype=np.float32)
    assert [f.shape[1:] for f in want] == dc.extents(kind, sub, L)
    for l, (g, w) in enumerate(zip(got, want)):
        err = dc.moved(w, g)
        print(f"{name} L = {L} layer {l}: float32 restatement vs float64, max |d| / peak = {err:.2e}, std {w.std():.3g}")
        assert g.dtype == np.float32 and w.dtype == np.float64 and g.shape == w.shape and err <= BAR / 10, (l, err)


def reaches(n_in, k, s, pad, n_out) -> bool:
    """Does the last tap of a k-tap window touch the row's data at some output position?"""
    return any(0 <= o * s - pad + k - 1 < n_in for o in range(n_out))


@pytest.mark.parametrize("name,L", dc.LONGEST)
def test_a_dropped_tap_or_channel_quad_moves_the_next_map_ten_bars(name, L):
    """What a kernel that drops the last tap of a window (kh, and for MRD the last kw) or the last four input channels of a layer would
    compute, stated as altered folded weights of the float64 restatement: that layer's feature map moves by more than 10 BAR of its peak,
    so a sweep case that passes at the bar has excluded it.  Checked at every layer where the tap reaches the row's data at all: at the
    deepest layers of a short row the last tap lies in the zero padding for every output position, whatever the weights."""
    kind, cfg, _ = dc.SWEEP[name]
    sub = dc.subs(kind, cfg)[0]
    layers, wave, want = dc.sweep_layers(name), dc.sweep_wave(name, L), dc.sweep_restated(name, L)
    ext = dc.extents(kind, sub, L)
    h_in, w_in = ((-(-L // sub), sub) if kind == "mpd" else (sub[0] // 2 + 1, L // sub[1]))
    checked = 0
    for l, (w, b) in enumerate(layers):
        KH, KW = w.shape[2:]
        if kind == "mpd":
            s, pad = ((3, 1), (2, 0)) if l < 5 else ((1, 1), (1, 0))
        else:
            s, pad = dref.RES_STRIDES[l], dref.RES_PADS[l]
        cases = []
        if reaches(h_in, KH, s[0], pad[0], ext[l][0]):
            cases.append(("the last kh", (slice(None), slice(None), KH - 1)))
        if kind == "mrd" and reaches(w_in, KW, s[1], pad[1], ext[l][1]):
            cases.append(("the last kw", (slice(None), slice(None), slice(None), KW - 1)))
        if l >= 1:
            cases.append(("the last four input channels", (slice(None), slice(-4, None))))
        for what, index in cases:
            w2 = w.copy()
            assert np.abs(w2[index]).min() > 0
            w2[index] = 0
            got = dc.restate(kind, sub, layers[:l] + [(w2, b)], wave)[l]
            err = dc.moved(want[l], got)
            print(f"{name} L = {L}: {what} of layer {l} zeroed moves its map by {err:.2e} of its peak")
            assert err > 10 * BAR, (what, l, err)
            checked += 1
        h_in, w_in = ext[l]
    assert checked >= (9 if kind == "mpd" else 11)


@pytest.mark.parametrize("name,L", dc.LONGEST)
def test_running_a_row_at_the_batchs_extent_moves_a_later_map_ten_bars(name, L):
    """What a kernel that pads a row with the batch's zeros instead of stopping at the row's own extent would compute: the first layer's map
    then holds SiLU(bias) past the row's end, and the first later layer whose last window crosses the row's end (which layer that is depends
    on the extent modulo the strides) moves by more than 10 BAR inside the row's own extent."""
    kind, cfg, _ = dc.SWEEP[name]
    sub = dc.subs(kind, cfg)[0]
    step = sub if kind == "mpd" else sub[1]
    got = dc.restate(kind, sub, dc.sweep_layers(name), dc.sweep_wave(name, L), extent=L + 9 * step)
    want = dc.sweep_restated(name, L)
    errs = [dc.moved(w, g[:, : w.shape[1], : w.shape[2]]) for g, w in zip(got[1:], want[1:])]
    print(f"{name} L = {L}: run at the extent of {L + 9 * step} samples, layers 1.. move by {['%.2e' % e for e in errs]} of their peaks")
    assert dc.moved(want[0], got[0][:, : want[0].shape[1], : want[0].shape[2]]) == 0 and got[0].shape != want[0].shape
    assert max(errs) > 10 * BAR
