"""GPU: the fused ResBlock pair kernels y = x + c2(silu(c1(silu x))) behind conv_pair_run (conv_pair.hip), instance by instance.

Five kernel families — the direct fp32 sums (resblock_pair.hip), F(2,3) and F(4,4) Winograd tap groups (pair_wino_impl.h, pair_wino44_impl.h), the
split-fp16 pairs (pair_f16x3_impl.h) and their C = 16 layout (pair16_f16x3.hip) — are listed per (C, k, dilation) in INSTANCES; every case selects
its family (set_algorithm / FV_PAIR_WINO44 / set_precision) and asserts the instance that ran (_lib.last_kernel(), or the labels of Engine.profile
inside fv_forward).  Lengths come from each family's own tile width TT (mirrored from conv_pair.hip): 1, 2, TT - 1, TT, TT + 1, TT + (k - 1) / 2 (the
clip ends inside the c2 halo of the last tile) and 2 TT + 3, the ones around TT with three batch items.  Arbiters, per instance:
  - float64 with the family's per-output bound (conv_reference.py pair_bound) on heavy-tailed weights, inputs of unequal channel scale, biases;
  - x and y embedded in NaN-filled buffers: the guard floats around y stay NaN (no write outside the output, 8-byte stores included), every output is
    finite (a halo read outside the item's [0, T) that is not masked would poison one) — with both tensors 8-byte aligned and 4 bytes off;
  - a clip alone equals the clip in a batch, bit for bit;
  - pair16_f16x3 falls back to the fp32 pair kernel on an odd T or a 4-byte-offset tensor; |activation| >= 65504 gives non-finite outputs, never
    finite wrong ones.
The accumulate epilogues (OUT_ACCUM, out_scale = 1/3), which only the engine reaches, run through two small HiFiGAN generators: the chain form of
the branch mean against the tree form, bit for bit, per family.  test_every_pair_instance_ran (last in the module) prints the table and fails on any
row that no case reached: run the module as a whole."""
import contextlib
import os
import re

import numpy as np
import pytest

import conv_reference as cr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KS, DS = (3, 7, 11), (1, 3, 5)
NO_F16_PAIRS = bool(os.environ.get("FV_NO_F16X3_PAIRS"))   # the diagnostic switch turns the f16x3 pair kernels off (test_gpu_f16x3.py)


def _fp32_shapes():
    """pair_supported (resblock_pair.hip) == pair_wino_supported (conv_pair.hip): every (k, d) at C = 16 / 32, k = 3 at C = 64 / 128."""
    return [(C, k, d) for C in (16, 32) for k in KS for d in DS] + [(C, 3, d) for C in (64, 128) for d in DS]


def _instances():
    """(family, C, k, d) of every pair kernel instance the library holds; "pair_f16x3_c16" is pair16_f16x3.hip (same kernel name, C = 16)."""
    rows = [("resblock_pair", C, k, d) for C, k, d in _fp32_shapes()]
    rows += [("pair_wino", C, k, d) for C, k, d in _fp32_shapes()]
    rows += [("pair_wino44", C, k, d) for C in (16, 32) for k in (7, 11) for d in DS]
    rows += [("pair_f16x3", C, k, d) for C in (32, 64, 128, 256) for k in KS for d in DS]
    rows += [("pair_f16x3_c16", 16, k, d) for k in KS for d in DS]
    return rows


INSTANCES = _instances()
IDS = [f"{f}-C{C}-k{k}-d{d}" for f, C, k, d in INSTANCES]
BOUND_OF = {"resblock_pair": "direct", "pair_wino": "wino23", "pair_wino44": "wino44", "pair_f16x3": "f16x3", "pair_f16x3_c16": "f16x3"}
_SEEN = {}     # row -> number of launches that ran it
_RATIOS = {}   # family -> largest |y - ref| / unit measured (conv_reference.py: the multiplier's unit; direct: the bound itself)


def _dev():
    assert torch.cuda.is_available(), "GPU test on a box without a GPU"
    return torch.device("cuda:0")


_NAME = re.compile(r"(resblock_pair|pair_wino44|pair_wino|pair_f16x3)<k=(\d+) d=(\d+) C=(\d+)>")


def _parse(label):
    """Pair label (last_kernel, or a profile row '<family><k=.. d=.. C=..> grid=..') -> row key, or None for other kernels."""
    m = _NAME.match(label)
    if not m:
        return None
    fam, k, d, C = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
    if fam == "pair_f16x3" and C == 16:
        fam = "pair_f16x3_c16"
    return fam, C, k, d


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


def _tt(fam, C, k, d):
    """Final output columns per workgroup, mirrored from the host side."""
    if fam == "resblock_pair":      # conv_pair.hip conv_pair_run: tt = max(128, kPairCols / C) - (k - 1), kPairCols = 2048 (PairGeom::TT)
        return max(128, 2048 // C) - (k - 1)
    if fam == "pair_wino":          # conv_pair.hip conv_pair_run: nbp = C == 128 ? 32 : 64; tt = 2 * (nbp / d * d) - (k - 1) (PWGeom / PW32Geom::TT)
        nbp = 32 if C == 128 else 64
        return 2 * (nbp // d * d) - (k - 1)
    if fam == "pair_wino44":        # conv_pair.hip conv_pair_run: nbq = 16 * (4 / (C / 16)); tt = 4 * (nbq / d * d) - (k - 1) (PQGeom::TT)
        nbq = 16 * (4 // (C // 16))
        return 4 * (nbq // d * d) - (k - 1)
    if fam == "pair_f16x3":         # conv_pair.hip conv_pair_run_f16x3: (C == 32 ? kPairF16ColsC32 = 384 : C == 64 ? 128 : 96) - (k - 1)
        return {32: 384, 64: 128}.get(C, 96) - (k - 1)
    assert fam == "pair_f16x3_c16"  # pair16_f16x3.hip pair16_f16x3_tile: 2 d * (256 / d) - (k - 1)
    return 2 * d * (256 // d) - (k - 1)


def _lengths(fam, C, k, d):
    """[(B, T)]: three items around the tile width, one otherwise; pair16_f16x3 takes even lengths only (the nearest even one above)."""
    tt = _tt(fam, C, k, d)
    out = []
    for T in (1, 2, tt - 1, tt, tt + 1, tt + (k - 1) // 2, 2 * tt + 3):
        B = 3 if tt - 1 <= T <= tt + (k - 1) // 2 else 1
        if fam == "pair_f16x3_c16" and T % 2:
            T += 1
        if (B, T) not in out:
            out.append((B, T))
    return out


def test_the_mirrored_tile_widths():
    """The extremes the module's docstring and the lengths rely on: 86 (wide f16x3, k = 11) ... 510 (pair16_f16x3, k = 3, d = 1 / 5)."""
    tts = {row: _tt(*row) for row in INSTANCES}
    assert min(tts.values()) == 2 * 30 - 2 == tts[("pair_wino", 128, 3, 5)]
    assert tts[("pair_f16x3", 256, 11, 1)] == 86 and tts[("pair_f16x3_c16", 16, 3, 1)] == 510 == max(tts.values())
    assert all(t % 2 == 0 for row, t in tts.items() if row[0] == "pair_f16x3_c16")
    assert len(INSTANCES) == 24 + 24 + 12 + 36 + 9


# ---- one launch, embedded in NaN ----------------------------------------------------------------------------------------------------------------
GUARD = 512   # floats before and after the tensor


def _embedded(n, off4):
    """A NaN-filled flat buffer and the start of an n-float window inside it that is 8-byte aligned (off4: 4 bytes past an 8-byte boundary)."""
    buf = torch.full((n + 2 * GUARD + 2,), float("nan"), device=_dev())
    start = GUARD
    if ((buf.data_ptr() + 4 * start) % 8 == 4) != off4:
        start += 1
    assert (buf.data_ptr() + 4 * start) % 8 == (4 if off4 else 0)
    return buf, start


def _launch(c1, c2, xd, off4):
    """The pair on copies of xd inside NaN-filled buffers -> (y on the host, kernel name); nothing outside y written, x untouched."""
    from vocoder_amd import _lib
    n = xd.numel()
    xbuf, xs = _embedded(n, off4)
    ybuf, ys = _embedded(n, off4)
    xv = xbuf[xs:xs + n].view(xd.shape)
    yv = ybuf[ys:ys + n].view(xd.shape)
    xv.copy_(xd)
    got = c1.pair(c2, xv, out=yv)
    torch.cuda.synchronize()
    name = _lib.last_kernel()
    assert got.data_ptr() == yv.data_ptr()
    assert bool(torch.isnan(ybuf[:ys]).all()) and bool(torch.isnan(ybuf[ys + n:]).all()), f"{name}: a write outside the output {tuple(xd.shape)}"
    assert bool(torch.isnan(xbuf[:xs]).all()) and bool(torch.isnan(xbuf[xs + n:]).all()) and torch.equal(xv, xd), f"{name}: the input was written"
    return yv.cpu().numpy(), name


def _layers(rng, C, k, d, precision="f32", algo="auto"):
    from vocoder_amd.engine import FusedConv
    w1 = cr.heavy_tailed_weight(rng, C, C, k)
    w2 = cr.heavy_tailed_weight(rng, C, C, k)
    b1 = rng.normal(size=C).astype(np.float32)
    b2 = rng.normal(size=C).astype(np.float32)
    c1 = FusedConv(w1, b1, dilation=d, padding=(k - 1) * d // 2).set_precision(precision).set_algorithm(algo)
    c2 = FusedConv(w2, b2, padding=(k - 1) // 2).set_precision(precision)
    return (w1, b1, w2, b2), c1, c2


def _select(fam, C, k):
    """(knobs, precision, algorithm) that make conv_pair_run take the family."""
    if fam == "resblock_pair":
        return {}, "f32", "direct"
    if fam == "pair_wino":
        return ({"FV_PAIR_WINO44": "0"} if k >= 7 else {}), "f32", "auto"
    if fam == "pair_wino44":
        return {}, "f32", "auto"
    return {}, "f16x3", "auto"


def _fp32_default(C, k):
    """The fp32 pair kernel of the shape under the default knobs (what pair16_f16x3 falls back to)."""
    return "pair_wino44" if (C <= 32 and k >= 7) else "pair_wino"


def _judge(y, name, want, row, x, wts, k, d, what, parts=None):
    """Name, coverage, ratio (kept for the table), bound.  parts: the (reference, bound) of this x per family, computed once."""
    key = _record(name)
    assert key == (want,) + row[1:], (what, name, want)
    fam = BOUND_OF[want]
    parts = {} if parts is None else parts
    if fam not in parts:
        parts[fam] = cr.pair_bound_parts(fam, x, *wts, k, d)
    ref, fixed, unit = parts[fam]
    assert np.isfinite(y).all(), f"{what} {name}: non-finite outputs (an unmasked read outside the item?)"
    r = cr.pair_ratio(y, ref, unit)
    tag = want if want != "pair_f16x3_c16" else "pair_f16x3 C=16"
    _RATIOS[tag] = max(_RATIOS.get(tag, 0.0), r)
    cr.check_pair_per_output(y, ref, fixed + cr.pair_multiplier(fam) * unit, what=f"{what} {name}")
    return r


@pytest.mark.parametrize("fam,C,k,d", INSTANCES, ids=IDS)
def test_pair_instance_against_float64(fam, C, k, d):
    row = (fam, C, k, d)
    if NO_F16_PAIRS and fam.startswith("pair_f16x3"):
        pytest.skip("the diagnostic switch FV_NO_F16X3_PAIRS turns these kernels off")
    rng = np.random.default_rng(1000 * C + 10 * k + d + sum(map(ord, fam)))
    env, precision, algo = _select(fam, C, k)
    worst = 0.0
    with _knobs(FV_PAIR_WINO44=env.get("FV_PAIR_WINO44"), FV_PAIR_WINO=None):
        wts, c1, c2 = _layers(rng, C, k, d, precision, algo)
        for B, T in _lengths(fam, C, k, d):
            x = cr.unequal_channels(rng, B, C, T)
            xd = torch.from_numpy(x).to(_dev())
            outs, parts = {}, {}
            for off4 in (False, True):
                y, name = _launch(c1, c2, xd, off4)
                want = fam
                if fam == "pair_f16x3_c16" and off4:   # pair16_f16x3 needs 8-byte aligned tensors: the exact-fp32 pair kernel takes the call
                    want = _fp32_default(C, k)
                r = _judge(y, name, want, row, x, wts, k, d, f"B={B} T={T} off4={off4}", parts)
                worst = max(worst, r) if want == fam else worst
                outs[off4] = y
            if fam == "pair_wino44" and T % 2 == 0:
                # the suite's claim (test_winograd_pair_reads_its_residual_from_a_4_byte_aligned_input): an x that starts 4 bytes off an 8-byte
                # boundary changes the residual's load width only — same bits
                xbuf, xs = _embedded(xd.numel(), True)
                xm = xbuf[xs:xs + xd.numel()].view(xd.shape)
                xm.copy_(xd)
                ym = c1.pair(c2, xm)
                torch.cuda.synchronize()
                _record(_last())
                assert np.array_equal(ym.cpu().numpy(), outs[False]), (row, B, T)
            if B > 1:   # one workgroup never spans items: the clip alone (C T is even: the same alignment as inside the batch)
                bi = T % B
                y1, name = _launch(c1, c2, xd[bi:bi + 1].contiguous(), False)
                assert _record(name) == row, name
                assert np.array_equal(y1[0], outs[False][bi]), (row, B, T, bi, float(np.abs(y1[0] - outs[False][bi]).max()))
        if fam == "pair_f16x3_c16":   # an odd T: the exact-fp32 pair kernel, at its own bound
            tt = _tt(fam, C, k, d)
            for B, T in ((1, 1), (3, tt + 1), (1, 2 * tt + 3)):
                x = cr.unequal_channels(rng, B, C, T)
                y, name = _launch(c1, c2, torch.from_numpy(x).to(_dev()), False)
                _judge(y, name, _fp32_default(C, k), row, x, wts, k, d, f"odd T={T}")
    print(f"{fam} C={C} k={k} d={d}: TT = {_tt(fam, C, k, d)}, largest |y - ref| / unit {worst:.3f}")


def _last():
    from vocoder_amd import _lib
    return _lib.last_kernel()


def test_pair_out_argument_must_not_alias_the_input():
    rng = np.random.default_rng(1)
    _, c1, c2 = _layers(rng, 16, 3, 1)
    x = torch.zeros(1, 16, 40, device=_dev())
    with pytest.raises(ValueError, match="alias"):
        c1.pair(c2, x, out=x)
    flat = torch.zeros(2 * x.numel(), device=_dev())
    with pytest.raises(ValueError, match="alias"):
        c1.pair(c2, flat[:x.numel()].view(x.shape), out=flat[8:8 + x.numel()].view(x.shape))
    with pytest.raises(ValueError, match="shape"):
        c1.pair(c2, x, out=torch.zeros(1, 16, 41, device=_dev()))


@pytest.mark.parametrize("fam,C,k,d", [("pair_f16x3", 64, 7, 3), ("pair_f16x3_c16", 16, 7, 3)])
def test_f16x3_pair_range_contract_is_loud(fam, C, k, d):
    """|activation| >= 65504 is outside the f16x3 contract (include/fishvoc.h fv_precision): the fp16 high plane becomes inf, and the outputs it
    reaches are non-finite — never finite wrong numbers: every finite output still meets the bound, and the non-finite ones lie inside the
    neighbourhood that the two convs' taps span."""
    if NO_F16_PAIRS:
        pytest.skip("the diagnostic switch FV_NO_F16X3_PAIRS turns these kernels off")
    rng = np.random.default_rng(77 + C)
    wts, c1, c2 = _layers(rng, C, k, d, "f16x3")
    B, T = 2, _tt(fam, C, k, d) + 40
    t0, ch = _tt(fam, C, k, d) - 2, 5          # near the first tile seam
    x = cr.unequal_channels(rng, B, C, T)
    x[0, ch, t0] = 1.0e5
    y, name = _launch(c1, c2, torch.from_numpy(x).to(_dev()), False)
    assert _record(name) == (fam, C, k, d), name
    reach = (k - 1) * d // 2 + (k - 1) // 2
    if fam == "pair_f16x3_c16":
        # pair16_f16x3 carries two output times per MFMA row pair over k + 1 combined taps: each row multiplies one tap past its own k by a
        # structural zero weight, and 0 * inf is NaN — the neighbourhood is one dilation step (c1) and one sample (c2) wider
        reach += d + 1
    bad = ~np.isfinite(y)
    assert bad[0, :, t0].all(), "the outputs under the centre taps of both convs must be non-finite"
    where = np.argwhere(bad)
    assert (where[:, 0] == 0).all() and (np.abs(where[:, 2] - t0) <= reach).all(), where[:5]
    with np.errstate(over="ignore"):   # (exp(1e5) inside the float64 SiLU of the outlier's neighbours: inf, and x / inf = -0 is the right value)
        ref, fixed, unit = cr.pair_bound_parts("f16x3", x, *wts, k, d)
    err = np.where(bad, 0.0, np.abs(np.where(bad, 0.0, y).astype(np.float64) - ref))
    bnd = fixed + cr.pair_multiplier("f16x3") * unit
    assert (err <= bnd).all(), (float((err / bnd).max()), np.unravel_index(int(np.argmax(err / bnd)), err.shape))


# ---- the accumulate epilogues, through the engine -----------------------------------------------------------------------------------------------
def _cfg(width, rates):
    return dict(hop_length=int(np.prod(rates)), upsample_rates=list(rates), upsample_kernel_sizes=[4] * len(rates), resblock_kernel_sizes=[3, 7, 11],
                resblock_dilation_sizes=[[1, 3, 5]] * 3, num_mels=20, upsample_initial_channel=width, use_template=False,
                pre_conv_kernel_size=7, post_conv_kernel_size=7)


# (config, mel frames): every stage longer than the widest tile of its width — 64 / 32 / 16 channels at 200 / 400 / 800 samples (TT <= 128 / 384 /
# 510), 256 / 128 channels at 100 / 200 samples (TT <= 96 / 126)
ENGINE_MODELS = {"c64_32_16": (_cfg(128, (2, 2, 2)), 100), "c256_128": (_cfg(512, (2, 2)), 50)}
ENGINE_SETTINGS = {"default": ({}, "f32"), "direct": ({"FV_PAIR_WINO": "0"}, "f32"), "f23": ({"FV_PAIR_WINO44": "0"}, "f32"), "f16x3": ({}, "f16x3")}
_ORACLE = {}


def _oracle(model):
    """(state dict, mel, CPU oracle waveform) of a model: computed once, shared by its four settings."""
    if model not in _ORACLE:
        from oracle import oracle as orc
        from vocoder_amd import synthetic as syn
        cfg, frames = ENGINE_MODELS[model]
        sd = syn.hifigan_state_dict(cfg, seed=9)
        mel = syn.synthetic_mel(2, cfg["num_mels"], frames, seed=10)
        _ORACLE[model] = (sd, mel, orc.hifigan_forward(sd, cfg, mel))
    return _ORACLE[model]


def _expected_pairs(setting, widths):
    """The pair instances a forward of the model launches under the setting (batch-invariant mode: plan_branch_form, engine_forward.hip)."""
    rows = set()
    for C in widths:
        for k in KS:
            for d in DS:
                if setting == "f16x3":
                    rows.add(("pair_f16x3_c16" if C == 16 else "pair_f16x3", C, k, d))
                elif (C, k, d) in _fp32_shapes():
                    fam = "resblock_pair" if setting == "direct" else "pair_wino44" if (C <= 32 and k >= 7 and setting != "f23") else "pair_wino"
                    rows.add((fam, C, k, d))
    return rows


@pytest.mark.parametrize("setting", list(ENGINE_SETTINGS))
@pytest.mark.parametrize("model", list(ENGINE_MODELS))
def test_chain_and_tree_branch_means_agree_bit_for_bit(model, setting):
    """FV_BRANCH_MEAN=chain forms the stack mean in the branches' last epilogues (OUT_SET, OUT_ACCUM, OUT_ACCUM with out_scale = 1/3); the tree
    form keeps three outputs (OUT_SET) and the consumer adds them.  DESIGN §3: the same additions in the same order — the waveforms must agree to
    the last bit under every pair family, both within 1e-4 of the CPU oracle, with the intended pair kernels in every stage (batch-invariant mode:
    the C = 64 / 128 k = 3 pairs fuse whatever the launch size).  Graph replay off."""
    if NO_F16_PAIRS and setting == "f16x3":
        pytest.skip("the diagnostic switch FV_NO_F16X3_PAIRS turns these kernels off")
    from vocoder_amd import _lib
    from vocoder_amd.engine import Engine, upsampler_config
    cfg, _ = ENGINE_MODELS[model]
    env, precision = ENGINE_SETTINGS[setting]
    sd, mel, ref = _oracle(model)
    x = torch.from_numpy(mel).to(_dev())
    widths = [cfg["upsample_initial_channel"] >> (i + 1) for i in range(len(cfg["upsample_rates"]))]
    outs = {}
    with _knobs(FV_PAIR_WINO=env.get("FV_PAIR_WINO"), FV_PAIR_WINO44=env.get("FV_PAIR_WINO44"), FV_CHAIN_MAX_C=None, FV_BRANCH_MEAN=None,
                FV_SINGLE_STREAM=None):
        eng = Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**cfg), state_dict=sd, precision=precision)
        try:
            eng.set_graph_replay(False)
            eng.set_batch_invariant(True)
            assert not eng.graph_replay
            for form in ("tree", "chain"):
                with _knobs(FV_BRANCH_MEAN="chain" if form == "chain" else None):
                    y = eng(x).clone()
                    torch.cuda.synchronize()
                    labels = [r["kernel"] for r in eng.profile(x, repeats=1)]
                pairs = {key for key in (_record(lab) for lab in labels) if key is not None}
                assert pairs == _expected_pairs(setting, widths), (form, sorted(pairs ^ _expected_pairs(setting, widths)))
                consumers = [lab for lab in labels if "sum3" in lab or "mean_of_three" in lab]
                assert bool(consumers) == (form == "tree"), (form, consumers)   # tree: the consumers add three tensors; chain: the epilogues did
                outs[form] = y.cpu().numpy()
                err = float(np.abs(outs[form] - ref).max())
                print(f"{model} {setting} {form}: max|d| vs the oracle {err:.3e}")
                assert err <= 1e-4, (model, setting, form, err)
        finally:
            eng.close()
    assert np.array_equal(outs["tree"], outs["chain"]), (model, setting, float(np.abs(outs["tree"] - outs["chain"]).max()))


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_pair_instance_ran():
    """Every row of INSTANCES ran at least once in this module (the other tests record what they launched)."""
    rows = [row for row in INSTANCES if not (NO_F16_PAIRS and row[0].startswith("pair_f16x3"))]
    missing = [row for row in rows if _SEEN.get(row, 0) == 0]
    print(f"\n{'family':16s} {'C':>3s} {'k':>3s} {'d':>2s} {'TT':>4s} launches")
    for row in rows:
        fam, C, k, d = row
        print(f"{fam:16s} {C:3d} {k:3d} {d:2d} {_tt(*row):4d} {_SEEN.get(row, 0):6d}{'' if _SEEN.get(row, 0) else '   NOT RUN'}")
    extra = sorted(key for key in _SEEN if key not in INSTANCES)
    print("largest |y - ref| / unit by family (the multiplier's unit, conv_reference.py; resblock_pair: of the bound itself): "
          + ", ".join(f"{f} {r:.3f}" for f, r in sorted(_RATIOS.items())))
    print(f"multipliers: C_F16 {cr.C_F16}, M_WINO23 {cr.M_WINO23}, M_WINO44 {cr.M_WINO44}")
    assert not extra, f"launched instances missing from the table: {extra}"
    assert not missing, f"{len(missing)} instances never ran: {missing}"
