"""GPU: the direct-sum MFMA conv kernel (conv_mfma_impl.h) instance by instance.

Every (GEMM taps, dilation, tile) that launch_cfg<KS, DIL> instantiates, the split-K kernels staged through LDS and straight from global memory,
the flattened pointwise columns (" flat" / " flat2"), the three-operand SUM3 inputs of the upsamplers and the generic kernel are listed in
INSTANCES; FV_CONV_TILE forces a tile on every launch that has it instantiated, and every case asserts the instance that ran
(_lib.last_kernel(), or the labels of Engine.profile inside fv_forward).  Three arbiters:
  - impulses: a zero input with +-2^j impulses further apart than the receptive field, no bias — every output is one weight times one impulse,
    exact in fp32: the kernel must equal the float64 reference bit for bit (halo, padding crop, polyphase phases, chunk tails, batch strides);
  - float64 with a per-output bound (conv_reference.py: c 2^-24 (sqrt K + a) A with A the absolute-value conv of the same layer) on heavy-tailed
    weights and inputs of unequal channel scale, under pre- / post-activations and residuals;
  - tile invariance: a conv output's sum order does not depend on the tile (batch-invariant mode relies on it, conv_layer.hip), so every
    non-split-K tile, the flattened and the per-clip pointwise tiling, and the 256-row upsampler tiles must agree bit for bit; the split-K kernels
    sum K in another order (staged and direct agree with each other) and meet the float64 bound.
test_every_instance_ran (last in the module) prints the table and fails on any row that no case reached: run the module as a whole."""
import contextlib
import os
import re

import numpy as np
import pytest

import conv_reference as cr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILES = ["128x128", "64x256", "32x512", "128x64", "32x128", "64x128", "splitK32x64", "splitK32x32", "256x64", "256x32", "128x96"]
SPLITK = ("splitK32x64", "splitK32x32")
REGULAR = ["128x128", "64x256", "32x512", "128x64", "32x128", "64x128"]
SPEC_PAIRS = [(1, 1), (2, 1), (4, 1), (13, 1)] + [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]


def _extras(ks):
    return {1: ["256x64", "256x32"], 2: ["256x64", "128x96"]}.get(ks, [])


def _instances():
    """(family, GEMM taps, dilation, tile, tags) of every conv_mfma instance the library holds."""
    rows = []
    for ks, d in SPEC_PAIRS:
        for t in REGULAR + _extras(ks) + list(SPLITK):
            rows.append(("spec", ks, d, t, ""))
    # split-K with the B operands straight from global memory (splitk_direct_shape, fv_internal.h)
    rows += [("spec", 1, 1, t, "direct") for t in SPLITK] + [("spec", 2, 1, t, "direct") for t in SPLITK] + [("spec", 7, 1, "splitK32x32", "direct")]
    # the three-operand input (stack-mean of the ResBlock branches) of the polyphase upsamplers: inside fv_forward only
    for ks in (1, 2, 4):
        for t in REGULAR + _extras(ks) + list(SPLITK):
            rows.append(("spec", ks, 1, t, "sum3"))
    rows += [("spec", ks, 1, t, "direct sum3") for ks in (1, 2) for t in SPLITK]
    # pointwise convs over the flattened (clip, time) columns: single columns / 8-byte column pairs
    rows += [("spec", 1, 1, t, f) for t in REGULAR + _extras(1) for f in ("flat", "flat2")]
    rows.append(("generic", 5, 2, "64x128", ""))
    return rows


INSTANCES = _instances()
_SEEN = {}   # row -> number of launches that ran it


def _dev():
    assert torch.cuda.is_available(), "GPU test on a box without a GPU"
    return torch.device("cuda:0")


_NAME = re.compile(r"conv_mfma<(spec|generic) k=(\d+) d=(\d+) tile=([0-9a-zA-Z]+)>(.*)")


def _parse(label):
    """conv_mfma label (last_kernel, or a profile row 'name cin=.. cout=..<tags> grid=..') -> row key, or None for other kernels."""
    m = _NAME.match(label)
    if not m:
        return None
    fam, ks, d, tile, rest = m.group(1), int(m.group(2)), int(m.group(3)), m.group(4), m.group(5).split()
    tags = [t for t in ("direct", "sum3", "flat", "flat2") if t in rest]
    return fam, ks, d, tile, " ".join(tags)


def _record(label):
    key = _parse(label)
    if key is not None:
        _SEEN[key] = _SEEN.get(key, 0) + 1
    return key


@contextlib.contextmanager
def _knobs(**env):
    """Set FV_* variables (None = unset) and re-read the library's knobs; restore both afterwards."""
    from vocoder_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.reload_env()
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.reload_env()


def _forceable(ks, d, tile, M):
    """conv_tile_forceable (conv_layer.hip)."""
    spec = (ks, d) in SPEC_PAIRS
    m_pad = (M + 127) // 128 * 128
    if not spec:
        return False
    if tile == "256x32":
        return ks == 1 and m_pad % 256 == 0
    if tile == "256x64":
        return ks in (1, 2) and m_pad % 256 == 0
    if tile == "128x96":
        return ks == 2
    return True


def _settings():
    """(FV_CONV_TILE, FV_SPLITK_DIRECT) pairs: the shape's own choice, every tile, the split-K tiles also staged through LDS."""
    out = [(None, None)] + [(t, None) for t in TILES] + [(t, "0") for t in SPLITK]
    return out


# ---- the layers ------------------------------------------------------------------------------------------------------------------------------
# (id, c_in, c_out, k, dilation, stride, transposed, B, T): C_in with a partial last 8-channel sub-chunk and a partial 32-channel chunk (10, 40,
# 72, 100, 1), rows that are no multiple of the tile rows, GEMM columns N = 1 / -1 modulo the tile widths (513, 511, 129, 257, 255), B = 1 and 3,
# transposed-conv outputs cropped by the padding
LAYERS = [
    ("k3d1", 40, 100, 3, 1, 1, False, 3, 513), ("k3d3", 72, 64, 3, 3, 1, False, 1, 511), ("k3d5", 10, 33, 3, 5, 1, False, 3, 129),
    ("k7d1", 100, 96, 7, 1, 1, False, 1, 257), ("k7d3", 1, 40, 7, 3, 1, False, 3, 300), ("k7d5", 40, 40, 7, 5, 1, False, 3, 97),
    ("k11d1", 72, 130, 11, 1, 1, False, 1, 513), ("k11d3", 10, 64, 11, 3, 1, False, 3, 255), ("k11d5", 100, 32, 11, 5, 1, False, 1, 600),
    ("k13d1", 40, 200, 13, 1, 1, False, 3, 129), ("k2d1", 10, 20, 2, 1, 1, False, 3, 130), ("k4d1", 72, 24, 4, 1, 1, False, 1, 300),
    ("k5d2_generic", 10, 24, 5, 2, 1, False, 3, 100),
    # polyphase ConvTranspose1d: (k, stride) = (16, 8) and (4, 2) -> 2 GEMM taps, (8, 2) -> 4, (2, 2) -> 1, (7, 3) -> 3 (k % stride != 0)
    ("convT16x8", 100, 32, 16, 1, 8, True, 1, 65), ("convT16x8_m320", 72, 40, 16, 1, 8, True, 3, 97),
    ("convT4x2", 40, 100, 4, 1, 2, True, 3, 255), ("convT8x2", 100, 50, 8, 1, 2, True, 1, 129),
    ("convT2x2", 72, 128, 2, 1, 2, True, 3, 511), ("convT7x3", 10, 12, 7, 1, 3, True, 3, 97),
    # pointwise: even T (flattened column pairs), odd T (single columns), a single clip (per-clip tiles)
    ("pw_even", 100, 130, 1, 1, 1, False, 3, 512), ("pw_odd", 40, 256, 1, 1, 1, False, 3, 129), ("pw_b1", 72, 64, 1, 1, 1, False, 1, 257),
]
LAYER_IDS = [row[0] for row in LAYERS]


def _geo(k, d, u, tr):
    if tr:
        return dict(transposed=True, stride=u, padding=(k - u) // 2)
    return dict(transposed=False, padding=(k - 1) * d // 2, dilation=d)


def _gemm(cin, cout, k, d, u, tr):
    """(GEMM taps, GEMM rows) of the layer (conv_layer_create)."""
    return ((k + u - 1) // u, cout * u) if tr else (k, cout)


def _make(w, b, k, d, u, tr, pre, post, slope):
    from vocoder_amd import _lib
    from vocoder_amd.engine import FusedConv
    acts = {"none": _lib.FV_ACT_NONE, "silu": _lib.FV_ACT_SILU, "leaky": _lib.FV_ACT_LEAKY_RELU, "tanh": _lib.FV_ACT_TANH, "gelu": _lib.FV_ACT_GELU}
    geo = _geo(k, d, u, tr)
    kw = dict(transposed=True, stride=u, padding=geo["padding"]) if tr else dict(dilation=d, padding=geo["padding"])
    conv = FusedConv(w, b, pre_act=acts[pre], post_act=acts[post], act_slope=slope, **kw)
    return conv.set_algorithm("direct")   # the Winograd kernels must not take the k = 3 / 7 / 11 layers


def _run_all(conv, xd, ks, d, M, B, flat_ok, res=None, alias=False):
    """The layer under every setting: {(tile knob, splitk knob): (output, kernel name)}, each name checked against the knobs."""
    from vocoder_amd import _lib
    outs = {}
    for tile, skd in _settings():
        with _knobs(FV_CONV_TILE=tile, FV_SPLITK_DIRECT=skd):
            if alias:
                buf = res.clone()
                y = conv(xd, buf, out=buf)
            else:
                y = conv(xd, res)
            torch.cuda.synchronize()
            name = _lib.last_kernel()
        key = _record(name)
        assert key is not None, name
        fam, kk, dd, got, tags = key
        assert (kk, dd) == (ks, d), name
        if tile is not None and _forceable(ks, d, tile, M):
            assert fam == "spec" and got == tile, (tile, name)
            if flat_ok:
                assert ("flat" in tags.split() or "flat2" in tags.split()) == (tile not in SPLITK), (tile, name)
        if fam == "generic":
            assert (ks, d) not in SPEC_PAIRS, name
        if skd == "0":
            assert "direct" not in tags.split(), name
        outs[(tile, skd)] = (y.cpu().numpy(), name)
    return outs


def _flat_ok(k, tr, B):
    return k == 1 and not tr and B > 1


# ---- impulses: indexing, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lid,cin,cout,k,d,u,tr,B,T", LAYERS, ids=LAYER_IDS)
def test_impulses_are_exact_on_every_tile(lid, cin, cout, k, d, u, tr, B, T):
    """Every output receives at most one product w * act(x) with x = +-2^j: exact in fp32, so the kernel must equal the float64 reference bit
    for bit on every tile — a wrong halo offset, padding crop, polyphase phase, chunk tail or batch stride moves or drops a weight."""
    rng = np.random.default_rng(sum(map(ord, lid)))
    ks, M = _gemm(cin, cout, k, d, u, tr)
    w = (rng.normal(size=(cin, cout, k) if tr else (cout, cin, k)) * 0.5).astype(np.float32)
    pre = "leaky" if (k == 1 or LAYER_IDS.index(lid) % 2) else "none"
    # impulse positions (input samples): both ends, both sides of every tile column boundary (GEMM column n reads inputs n - pad_l ... n)
    bounds = [m * c for c in (32, 64, 96, 128, 256, 512) for m in range(1, 4)]
    pad_l = ks - 1 if tr else _geo(k, d, u, tr)["padding"]
    pos = [0, T - 1, 1, T - 2] + [n - pad_l + e for n in bounds for e in (-1, 0)]
    gap = (ks if tr else (k - 1) * d) + 1
    chans = sorted({c for c in (0, 7, 8, 31, 32, cin - 1) if c < cin})
    x, placed = cr.impulse_input(B, cin, T, pos, chans, gap, seed=len(lid))
    B = x.shape[0]
    geo = _geo(k, d, u, tr)
    ref = cr.conv64(cr.act64(x, pre, 0.25), w, **geo)
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref), "the reference itself is not exact in fp32"
    assert len(placed) >= 4
    conv = _make(w, None, k, d, u, tr, pre, "none", 0.25)
    xd = torch.from_numpy(x).to(_dev())
    outs = _run_all(conv, xd, ks, d, M, B, _flat_ok(k, tr, B))
    for key, (y, name) in outs.items():
        if not np.array_equal(y, ref32):
            bad = np.argwhere(y != ref32)
            raise AssertionError(f"{lid} {key} {name}: {len(bad)} outputs differ, first at {tuple(bad[0])}: {y[tuple(bad[0])]} vs {ref32[tuple(bad[0])]}")
    if k == 1 and not tr and B > 1:   # the per-clip tiling (single clips) of the same outputs
        for bi in range(B):
            with _knobs(FV_CONV_TILE="128x64"):
                y1 = conv(xd[bi:bi + 1]).cpu().numpy()
            _record(_lib_last())
            assert np.array_equal(y1[0], ref32[bi]), (lid, bi)


def _lib_last():
    from vocoder_amd import _lib
    return _lib.last_kernel()


# ---- float64 with a per-output bound, and tile invariance ------------------------------------------------------------------------------------
# (pre-activation, post-activation, residual: None / "res" / "alias" = the residual is the output tensor itself), cycled over the layers
ACTS = [("silu", "none", "res"), ("leaky", "tanh", None), ("none", "gelu", "res"), ("silu", "none", "alias"), ("leaky", "none", None)]
_RATIOS = {}   # family -> largest error ratio measured


@pytest.mark.parametrize("lid,cin,cout,k,d,u,tr,B,T", LAYERS, ids=LAYER_IDS)
def test_float64_bound_and_tile_invariance(lid, cin, cout, k, d, u, tr, B, T):
    """Heavy-tailed weights, unequal channel scales, bias, activations and residuals against float64 torch on the CPU, per output, on every
    tile; all non-split-K tiles bit-identical, split-K staged == split-K direct; pointwise: flattened column pairs == single columns (a 4-byte
    offset input) == per-clip tiles."""
    rng = np.random.default_rng(7 + sum(map(ord, lid)))
    ks, M = _gemm(cin, cout, k, d, u, tr)
    pre, post, rmode = ACTS[LAYER_IDS.index(lid) % len(ACTS)]
    if k == 1 and pre == "none":
        pre = "leaky"   # (no pre-activation: the pointwise GEMM kernel, gemm_pw.hip, would take the layer)
    w = cr.heavy_tailed_weight(rng, cout, cin, k, transposed=tr)
    b = rng.normal(size=cout).astype(np.float32)
    x = cr.unequal_channels(rng, B, cin, T)
    geo = _geo(k, d, u, tr)
    tout = (T - 1) * u - 2 * geo["padding"] + k if tr else T + 2 * geo["padding"] - d * (k - 1)
    res = None if rmode is None else rng.normal(size=(B, cout, tout)).astype(np.float32)
    ref, _, A = cr.layer_ref(x, w, b, geo, pre=pre, post=post, slope=0.2, res=res)
    K = cr.terms(cin, k, tr, u)
    conv = _make(w, b, k, d, u, tr, pre, post, 0.2)
    xd = torch.from_numpy(x).to(_dev())
    rd = None if res is None else torch.from_numpy(res).to(_dev())
    outs = _run_all(conv, xd, ks, d, M, B, _flat_ok(k, tr, B), res=rd, alias=rmode == "alias")
    worst = 0.0
    for key, (y, name) in outs.items():
        r = cr.error_ratio(y, ref, A, K, post)
        fam, _, _, tl, tags = _parse(name)
        fam = fam if fam == "generic" else ("splitK " + ("direct" if "direct" in tags else "staged")) if tl in SPLITK else "tiled"
        _RATIOS[fam] = max(_RATIOS.get(fam, 0.0), r)
        worst = max(worst, r)
        cr.check_per_output(y, ref, A, K, post, what=f"{lid} {key} {name}")
    print(f"{lid}: pre {pre} post {post} res {rmode}: K = {K}, largest error ratio {worst:.3f}")
    non_split = {key: v for key, v in outs.items() if "splitK" not in v[1]}
    first = next(iter(non_split.values()))
    for key, (y, name) in non_split.items():
        assert np.array_equal(y, first[0]), (lid, key, name, first[1], float(np.abs(y - first[0]).max()))
    for t in SPLITK:
        if (t, None) in outs and "splitK" in outs[(t, None)][1]:
            assert np.array_equal(outs[(t, None)][0], outs[(t, "0")][0]), (lid, t, outs[(t, None)][1], outs[(t, "0")][1])
    if rmode == "alias":   # the residual read from the output tensor itself, element by element before its store
        y = conv(xd, rd).cpu().numpy()
        assert np.array_equal(y, outs[(None, None)][0]), lid
    if k == 1 and not tr and B > 1:
        # single columns: the same input at a 4-byte offset (no 8-byte column pairs) -> p.flat = 1; per clip: B = 1 launches
        base = torch.empty(x.size + 1, device=_dev())
        xo = base[1:].view(*x.shape)
        xo.copy_(xd)
        for tile in REGULAR + _extras(1):
            if not _forceable(1, 1, tile, M):
                continue
            with _knobs(FV_CONV_TILE=tile):
                y1 = conv(xo, rd).cpu().numpy()
                name = _lib_last()
            _record(name)
            assert name.endswith(" flat"), name
            assert np.array_equal(y1, first[0]), (lid, tile, name)
        for bi in range(B):
            with _knobs(FV_CONV_TILE="128x128"):
                yb = conv(xd[bi:bi + 1], None if rd is None else rd[bi:bi + 1]).cpu().numpy()
                name = _lib_last()
            _record(name)
            assert "flat" not in name, name
            assert np.array_equal(yb[0], first[0][bi]), (lid, bi, name)


# ---- the three-operand upsampler input through the engine ------------------------------------------------------------------------------------
def _k1_sum3_model():
    """A generator whose second upsampler is a (2, 2) ConvTranspose1d with 256 GEMM rows: the 256-row SUM3 tiles of the one-tap kernels
    (HiFiGAN-V1-44k's one-tap upsamplers have 64 and 32 rows)."""
    return dict(hop_length=8, upsample_rates=[2, 2, 2], upsample_kernel_sizes=[4, 2, 8], resblock_kernel_sizes=[3, 7, 11],
                resblock_dilation_sizes=[[1, 3, 5]] * 3, num_mels=80, upsample_initial_channel=512, use_template=False,
                pre_conv_kernel_size=7, post_conv_kernel_size=7)


def _models():
    from vocoder_amd import synthetic as syn
    return {"hifigan_v1_44k": ("hifigan", dict(syn.HIFIGAN_V1_44K), 5), "bigvgan_24k": ("bigvgan", dict(syn.BIGVGAN_24K), 5),
            "hifigan_k1_256rows": ("hifigan", _k1_sum3_model(), 24)}


@pytest.mark.parametrize("model", ["hifigan_v1_44k", "bigvgan_24k", "hifigan_k1_256rows"])
def test_sum3_upsamplers_through_the_engine_on_every_tile(model):
    """fv_forward at B = 1, 3 and 32 with graph replay off, under every FV_CONV_TILE and FV_NO_SUM3 on / off (and the split-K tiles staged):
    every run within 1e-4 of the CPU oracle, every run whose conv_mfma launches are all non-split-K bit-identical to the others.  The instances
    are read from the engine's per-launch profile labels."""
    from oracle import oracle as orc
    from vocoder_amd import _lib
    from vocoder_amd import synthetic as syn
    from vocoder_amd.engine import Engine, upsampler_config
    kind, cfg, frames = _models()[model]
    sd = (syn.hifigan_state_dict if kind == "hifigan" else syn.bigvgan_state_dict)(cfg, seed=3)
    mel = syn.synthetic_mel(32, cfg["num_mels"], frames, seed=4)
    items = [0, 1, 2, 31]
    fwd = orc.hifigan_forward if kind == "hifigan" else orc.bigvgan_forward
    ref = fwd(sd, cfg, mel[items])
    eng = Engine(_lib.FV_MODEL_HIFIGAN if kind == "hifigan" else _lib.FV_MODEL_BIGVGAN, ups=upsampler_config(**cfg), state_dict=sd)
    eng.set_graph_replay(False)
    assert not eng.graph_replay
    for B in (1, 3, 32):
        xd = torch.from_numpy(np.ascontiguousarray(mel[:B])).to(_dev())
        sel = [i for i, it in enumerate(items) if it < B]
        bit_groups = {}
        n_sum3 = 0
        for tile, skd in _settings():
            for no_sum3 in (None, "1"):
                with _knobs(FV_CONV_TILE=tile, FV_SPLITK_DIRECT=skd, FV_NO_SUM3=no_sum3):
                    y = eng(xd)
                    torch.cuda.synchronize()
                    y = y.cpu().numpy()
                    labels = [row["kernel"] for row in eng.profile(xd, repeats=1)]
                keys = [k for k in (_record(lab) for lab in labels) if k is not None]
                assert keys, labels
                n_sum3 += sum("sum3" in k[4] for k in keys)
                assert all("sum3" not in k[4] for k in keys) if no_sum3 else True, (tile, labels)
                err = float(np.abs(y[[items[i] for i in sel]] - ref[sel]).max())
                assert err <= 1e-4, (model, B, tile, skd, no_sum3, err)
                split = any("splitK" in k[3] for k in keys)
                bit_groups.setdefault("split" if split else "non_split", []).append(((tile, skd, no_sum3), y))
        assert n_sum3 > 0, (model, B)
        group = bit_groups.get("non_split", [])
        assert len(group) >= 8, (model, B, [g[0] for g in group])
        for key, y in group:
            assert np.array_equal(y, group[0][1]), (model, B, key, group[0][0], float(np.abs(y - group[0][1]).max()))
    eng.close()


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------------
def test_every_instance_ran():
    """Every row of INSTANCES ran at least once in this module (the other tests record what they launched)."""
    missing = [row for row in INSTANCES if _SEEN.get(row, 0) == 0]
    print(f"\n{'family':8s} {'k':>3s} {'d':>2s} {'tile':12s} {'tags':12s} launches")
    for row in INSTANCES:
        fam, ks, d, tile, tags = row
        print(f"{fam:8s} {ks:3d} {d:2d} {tile:12s} {tags:12s} {_SEEN.get(row, 0):6d}{'' if _SEEN.get(row, 0) else '   NOT RUN'}")
    extra = sorted(k for k in _SEEN if k not in INSTANCES)
    print("largest per-output error ratio by family: " + ", ".join(f"{f} {r:.3f}" for f, r in sorted(_RATIOS.items())))
    assert not extra, f"launched instances missing from the table: {extra}"
    assert not missing, f"{len(missing)} instances never ran: {missing}"
