"""GPU: the fused wide k = 3 ResBlock pairs on one Winograd F(4,3) tap group (pair_wino4_impl.h; C = 64 / 128, dilation 1 / 3 / 5), instance by
instance under FV_PAIR_WINO4=2, which makes conv_pair_run take the family at any size.  Lengths come from the kernel's own tile width TT
(fv_pair_wino4_tile): 1, 2, TT - 1, TT, TT + 1 (three items each), 2 TT + 3 (T % 4 = 3) and 2 TT + 4 (T % 4 = 0).  Arbiters, per instance:
  - float64 per output: conv_reference.pair_bound_parts("wino44", ...) — its span of 4 d is the quad lattice's — at the project's own multiplier
    pair_multiplier("wino44"), on heavy-tailed weights and inputs of unequal channel scale; the largest measured ratio is printed;
  - x and y embedded in NaN-filled buffers, 8-byte aligned and 4 bytes off: every output finite, nothing outside y written, x unchanged;
  - a clip alone equals the same clip inside a batch of three, bit for bit;
  - _lib.last_kernel() names pair_wino4<k=3 d C>.
With the knob unset the same calls report pair_wino<...>.  Engine level: a small HiFiGAN generator with a C = 128 and a C = 64 stage, B = 2, 9 mel
frames — knob 2 against the CPU oracle (1e-4) and against the knob-0 output (below 1e-4 of full scale, printed), six profile rows of the new family,
none in batch-invariant mode."""
import contextlib
import os
import re

import numpy as np
import pytest

import conv_reference as cr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INSTANCES = [(C, d) for C in (64, 128) for d in (1, 3, 5)]
IDS = [f"C{C}-d{d}" for C, d in INSTANCES]
K = 3
GUARD = 512   # floats before and after the tensor


def _dev():
    assert torch.cuda.is_available(), "GPU test on a box without a GPU"
    return torch.device("cuda:0")


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


def _tt(C, d):
    from vocoder_amd import _lib
    return int(_lib.lib().fv_pair_wino4_tile(C, d))


def _lengths(C, d):
    tt = _tt(C, d)
    cases = [(1, 1), (1, 2), (3, tt - 1), (3, tt), (3, tt + 1), (1, 2 * tt + 3), (1, 2 * tt + 4)]
    assert (2 * tt + 3) % 4 != 0 and (2 * tt + 4) % 4 == 0
    return cases


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


def _layers(rng, C, d):
    from vocoder_amd.engine import FusedConv
    w1 = cr.heavy_tailed_weight(rng, C, C, K)
    w2 = cr.heavy_tailed_weight(rng, C, C, K)
    b1 = rng.normal(size=C).astype(np.float32)
    b2 = rng.normal(size=C).astype(np.float32)
    c1 = FusedConv(w1, b1, dilation=d, padding=(K - 1) * d // 2)
    c2 = FusedConv(w2, b2, padding=(K - 1) // 2)
    return (w1, b1, w2, b2), c1, c2


@pytest.mark.parametrize("C,d", INSTANCES, ids=IDS)
def test_wide_quad_pair_instance(C, d):
    rng = np.random.default_rng(2600 + 10 * C + d)
    want = f"pair_wino4<k={K} d={d} C={C}>"
    mult = cr.pair_multiplier("wino44")
    worst = 0.0
    with _knobs(FV_PAIR_WINO4="2", FV_PAIR_WINO=None):
        wts, c1, c2 = _layers(rng, C, d)
        for B, T in _lengths(C, d):
            x = cr.unequal_channels(rng, B, C, T)
            xd = torch.from_numpy(x).to(_dev())
            ref, fixed, unit = cr.pair_bound_parts("wino44", x, *wts, K, d)
            outs = {}
            for off4 in (False, True):
                y, name = _launch(c1, c2, xd, off4)
                what = f"{want} B={B} T={T} off4={off4}"
                assert name == want, (what, name)
                assert np.isfinite(y).all(), f"{what}: non-finite outputs (an unmasked read outside the item?)"
                r = cr.pair_ratio(y, ref, unit)
                worst = max(worst, r)
                cr.check_pair_per_output(y, ref, fixed + mult * unit, what=what)
                outs[off4] = y
            if B > 1:   # one workgroup never spans items: the clip alone, same alignment as inside the batch (C T is even)
                bi = T % B
                y1, name = _launch(c1, c2, xd[bi:bi + 1].contiguous(), False)
                assert name == want, name
                assert np.array_equal(y1[0], outs[False][bi]), (want, B, T, bi, float(np.abs(y1[0] - outs[False][bi]).max()))
    print(f"{want}: TT = {_tt(C, d)}, largest |y - ref| / unit {worst:.3f} (multiplier {mult}, half of it {mult / 2})"
          f"{'  ABOVE HALF THE MULTIPLIER' if worst > mult / 2 else ''}")


@pytest.mark.parametrize("C,d", INSTANCES, ids=IDS)
def test_default_knobs_keep_f23(C, d):
    """With FV_PAIR_WINO4 unset a direct conv_pair_run keeps pair_wino<...> at every size: only the engine's pair branches ask for the new family."""
    rng = np.random.default_rng(2700 + 10 * C + d)
    with _knobs(FV_PAIR_WINO4=None, FV_PAIR_WINO=None):
        _, c1, c2 = _layers(rng, C, d)
        for B, T in ((1, 1), (3, _tt(C, d) + 1)):
            xd = torch.from_numpy(cr.unequal_channels(rng, B, C, T)).to(_dev())
            _, name = _launch(c1, c2, xd, False)
            assert name == f"pair_wino<k={K} d={d} C={C}>", name


# ---- through the engine ---------------------------------------------------------------------------------------------------------------------------
CFG = dict(hop_length=4, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], resblock_kernel_sizes=[3, 7, 11],
           resblock_dilation_sizes=[[1, 3, 5]] * 3, num_mels=20, upsample_initial_channel=256, use_template=False,
           pre_conv_kernel_size=7, post_conv_kernel_size=7)
_NEW = re.compile(r"pair_wino4<k=3 d=(\d+) C=(\d+)>")


def test_engine_takes_the_family_under_the_knob_only():
    from oracle import oracle as orc
    from vocoder_amd import _lib
    from vocoder_amd import synthetic as syn
    from vocoder_amd.engine import Engine, upsampler_config
    sd = syn.hifigan_state_dict(CFG, seed=26)
    mel = syn.synthetic_mel(2, CFG["num_mels"], 9, seed=27)
    ref = orc.hifigan_forward(sd, CFG, mel)
    x = torch.from_numpy(mel).to(_dev())
    outs, rows = {}, {}
    for knob in ("2", "0"):
        with _knobs(FV_PAIR_WINO4=knob, FV_PAIR_WINO=None, FV_BRANCH_MEAN=None, FV_SINGLE_STREAM=None):
            eng = Engine(_lib.FV_MODEL_HIFIGAN, ups=upsampler_config(**CFG), state_dict=sd)
            try:
                eng.set_graph_replay(False)
                outs[knob] = eng(x).clone().cpu().numpy()
                rows[knob] = [r["kernel"] for r in eng.profile(x, repeats=1)]
                if knob == "2":
                    eng.set_batch_invariant(True)
                    inv = [r["kernel"] for r in eng.profile(x, repeats=1)]
                    assert not [lab for lab in inv if _NEW.match(lab)], inv
                    assert len([lab for lab in inv if lab.startswith("pair_wino<k=3")]) == 6, inv   # the stages still fuse, on F(2,3)
            finally:
                eng.close()
    new = sorted((int(m.group(2)), int(m.group(1))) for m in (_NEW.match(lab) for lab in rows["2"]) if m)
    assert new == [(64, 1), (64, 3), (64, 5), (128, 1), (128, 3), (128, 5)], rows["2"]
    assert not [lab for lab in rows["0"] if _NEW.match(lab)], rows["0"]
    err = float(np.abs(outs["2"] - ref).max())
    diff = float(np.abs(outs["2"] - outs["0"]).max())   # the waveform is a tanh: full scale is 1
    print(f"knob 2 vs the oracle: max|d| {err:.3e}; knob 2 vs knob 0: {diff:.3e} of full scale")
    assert err <= 1e-4, err
    assert diff < 1e-4, diff
