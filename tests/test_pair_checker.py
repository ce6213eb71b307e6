"""CPU: the arbiter of the fused-pair instance tests (conv_reference.py pair_ref / pair_bound) has teeth.  Float32 "mutants" of the float64
pair y = x + c2(silu(c1(silu x))) — the errors a fused pair kernel makes when its two-level halo, its in-tile zero padding, a seam, a batch
stride or a split-fp16 plane is off — must fail the per-output check of EVERY kernel family's bound (direct, f16x3, F(2,3), F(4,4)), each at a
shape where it is at least 10 x past the loosest of them; the correctly rounded reference passes all four; pair_ref equals the pair written
out as loops; and the Winograd bound's A_W is never below A."""
import numpy as np
import pytest

import conv_reference as cr

pytest.importorskip("torch")


def _pair(seed, C, k, d, B=2, T=60):
    rng = np.random.default_rng(seed)
    w1 = cr.heavy_tailed_weight(rng, C, C, k)
    w2 = cr.heavy_tailed_weight(rng, C, C, k)
    b1 = rng.normal(size=C).astype(np.float32)
    b2 = rng.normal(size=C).astype(np.float32)
    x = cr.unequal_channels(rng, B, C, T)
    return x, w1, b1, w2, b2


def _bounds(x, w1, b1, w2, b2, k, d):
    return {f: cr.pair_bound(f, x, w1, b1, w2, b2, k, d) for f in cr.PAIR_FAMILIES}


def _caught_by_every_family(y, ref, bounds, what):
    """Fails every family's check, and is >= 10 x past the loosest bound somewhere."""
    y = y.astype(np.float32)
    for fam, bnd in bounds.items():
        with pytest.raises(AssertionError):
            cr.check_pair_per_output(y, ref, bnd, what=f"{what} [{fam}]")
    loosest = np.maximum.reduce(list(bounds.values()))
    past = float((np.abs(y.astype(np.float64) - ref) / loosest).max())
    print(f"{what}: {past:.1f} x past the loosest family bound")
    assert past >= 10.0, (what, past)


def _h64(x, w1, b1, k, d):
    return cr.conv64(cr.act64(x, "silu"), w1, padding=(k - 1) * d // 2, dilation=d) + np.asarray(b1, dtype=np.float64)[None, :, None]


def _c2(h, w2, b2, k, padding=None):
    return cr.conv64(cr.act64(h, "silu"), w2, padding=(k - 1) // 2 if padding is None else padding) + np.asarray(b2, dtype=np.float64)[None, :, None]


@pytest.mark.parametrize("C,k,d", [(16, 3, 1), (16, 11, 5), (32, 7, 3), (64, 3, 5), (128, 3, 1)])
def test_the_rounded_reference_passes_every_family(C, k, d):
    x, w1, b1, w2, b2 = _pair(C + k + d, C, k, d, B=2, T=90)
    ref, A1, A2, K = cr.pair_ref(x, w1, b1, w2, b2, k, d)
    assert K == C * k
    for fam, bnd in _bounds(x, w1, b1, w2, b2, k, d).items():
        cr.check_pair_per_output(ref.astype(np.float32), ref, bnd, what=f"rounded [{fam}]")


def test_the_fp32_torch_pair_stays_inside_the_direct_bound():
    """An honest fp32 evaluation (torch conv1d in float32, its own summation order) is well inside the direct family's bound."""
    import torch
    import torch.nn.functional as F
    for C, k, d in ((16, 11, 5), (32, 7, 3), (128, 3, 1)):
        x, w1, b1, w2, b2 = _pair(3 * C + k, C, k, d, B=2, T=150)
        xt = torch.from_numpy(x)
        h = F.conv1d(F.silu(xt), torch.from_numpy(w1), torch.from_numpy(b1), padding=(k - 1) * d // 2, dilation=d)
        y = (xt + F.conv1d(F.silu(h), torch.from_numpy(w2), torch.from_numpy(b2), padding=(k - 1) // 2)).numpy()
        ref, fixed, unit = cr.pair_bound_parts("direct", x, w1, b1, w2, b2, k, d)
        assert cr.pair_ratio(y, ref, unit) <= 0.5, (C, k, d, cr.pair_ratio(y, ref, unit))
        cr.check_pair_per_output(y, ref, fixed, what="fp32 torch")


def test_pair_ref_equals_the_loop_definition():
    rng = np.random.default_rng(21)
    for C, k, d, T in ((3, 3, 1, 9), (4, 3, 3, 14), (2, 7, 5, 40), (3, 11, 1, 8), (2, 3, 5, 1)):
        x = rng.normal(size=(2, C, T))
        w1, w2 = rng.normal(size=(C, C, k)), rng.normal(size=(C, C, k))
        b1, b2 = rng.normal(size=C), rng.normal(size=C)
        ref, A1, A2, K = cr.pair_ref(x, w1, b1, w2, b2, k, d)
        silu = lambda v: v / (1.0 + np.exp(-v))   # noqa: E731
        h = cr.conv1d_loops(silu(x), w1, b1, d, (k - 1) * d // 2)
        want = x + cr.conv1d_loops(silu(h), w2, b2, 1, (k - 1) // 2)
        assert np.allclose(ref, want, rtol=1e-12, atol=1e-12), (C, k, d, T)
        assert (np.abs(ref) <= A2 * (1 + 1e-12)).all() and (np.abs(h) <= A1 * (1 + 1e-12)).all()


@pytest.mark.parametrize("C,k,d", [(16, 3, 1), (16, 11, 5), (32, 7, 3), (64, 3, 5)])
def test_the_winograd_neighbourhood_sum_is_never_below_A(C, k, d):
    x, w1, b1, w2, b2 = _pair(5 * C + k + d, C, k, d, B=2, T=70)
    ref, A1, A2, K = cr.pair_ref(x, w1, b1, w2, b2, k, d)
    a1 = cr.act64(x, "silu")
    a2 = cr.act64(_h64(x, w1, b1, k, d), "silu")
    for span in (2, 4):
        AW1 = cr.wino_A(a1, w1, b1, span * d + (k - 1) * d // 2)
        AW2 = cr.wino_A(a2, w2, b2, span + (k - 1) // 2, res=x.astype(np.float64))
        assert (AW1 >= A1 * (1 - 1e-12)).all() and (AW2 >= A2 * (1 - 1e-12)).all()
        assert AW1.shape == A1.shape and AW2.shape == A2.shape
    # a window of zero is A itself
    assert np.allclose(cr.wino_A(a1, w1[:, :, :1], b1, 0), cr.layer_ref(x, w1[:, :, :1], b1, dict(transposed=False, padding=0, dilation=1), pre="silu")[2])


# ---- the mutants ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,k,d", [(16, 11, 5), (32, 7, 3), (64, 3, 1)])
def test_an_intermediate_not_zeroed_outside_the_clip_is_caught(C, k, d):
    """c2's zero padding applies to silu(h) outside [0, T); a kernel that computes h there from the zero-padded x sees silu(b1 + ...) instead."""
    x, w1, b1, w2, b2 = _pair(31 + C, C, k, d)
    ref = cr.pair_ref(x, w1, b1, w2, b2, k, d)[0]
    H2 = (k - 1) // 2
    xe = np.pad(x, ((0, 0), (0, 0), (H2, H2)))
    bad = x + _c2(_h64(xe, w1, b1, k, d), w2, b2, k, padding=0)
    assert bad.shape == ref.shape
    assert np.allclose(bad[:, :, H2:ref.shape[2] - H2], ref[:, :, H2:ref.shape[2] - H2], rtol=1e-12, atol=1e-12)   # only the clip's ends differ
    _caught_by_every_family(bad, ref, _bounds(x, w1, b1, w2, b2, k, d), "h not zeroed outside [0, T)")


@pytest.mark.parametrize("C,k,d", [(16, 7, 1), (32, 11, 3), (128, 3, 5)])
def test_a_c2_tap_dropped_left_of_a_tile_seam_is_caught(C, k, d):
    x, w1, b1, w2, b2 = _pair(41 + C, C, k, d, B=2, T=80)
    ref = cr.pair_ref(x, w1, b1, w2, b2, k, d)[0]
    w2m = w2.copy()
    w2m[:, :, k - 1] = 0.0          # the tap that reaches furthest right: into the next tile's intermediate
    seam = 48
    y = ref.copy()
    y[:, :, seam - 1] = (x + _c2(_h64(x, w1, b1, k, d), w2m, b2, k))[:, :, seam - 1]
    _caught_by_every_family(y, ref, _bounds(x, w1, b1, w2, b2, k, d), "c2 tap dropped at a seam")


@pytest.mark.parametrize("C,k,d", [(16, 3, 3), (64, 3, 1)])
def test_the_residual_of_the_neighbouring_item_on_the_last_tile_is_caught(C, k, d):
    x, w1, b1, w2, b2 = _pair(51 + C, C, k, d, B=3, T=70)
    ref = cr.pair_ref(x, w1, b1, w2, b2, k, d)[0]
    y = ref.copy()
    t0 = 48
    y[:, :, t0:] += np.roll(x, -1, axis=0)[:, :, t0:].astype(np.float64) - x[:, :, t0:]
    _caught_by_every_family(y, ref, _bounds(x, w1, b1, w2, b2, k, d), "residual of the next batch item")


@pytest.mark.parametrize("C,k,d,seed", [(16, 3, 1, 3), (32, 3, 1, 4), (64, 3, 3, 8)])
def test_the_lowest_gain_row_off_by_1e_3_is_caught_where_the_global_bar_is_not(C, k, d, seed):
    """The conv part of the lowest-gain output row 1e-3 too large (a row of c2 scaled wrongly): the suite's older bar, one max-abs number, lets it
    through; every family's per-output bound does not."""
    x, w1, b1, w2, b2 = _pair(seed, C, k, d, B=2, T=200)
    b2 = np.zeros_like(b2)           # a row whose conv part is its weights' gain alone
    ref = cr.pair_ref(x, w1, b1, w2, b2, k, d)[0]
    conv_part = ref - x
    row = int(np.argmin(np.abs(conv_part).max(axis=(0, 2))))
    assert np.abs(conv_part[:, row]).max() < 0.05 * np.abs(conv_part).max()
    y = ref.copy()
    y[:, row] += 1e-3 * conv_part[:, row]
    err = np.abs(y.astype(np.float32) - ref).max()
    assert err <= 1e-4 and err <= 2e-5 * max(np.abs(ref).max(), 1.0)      # the old global bar (test_gpu_f16x3.py) lets it through ...
    _caught_by_every_family(y, ref, _bounds(x, w1, b1, w2, b2, k, d), "lowest-gain row off by 1e-3")   # ... no family's bound does


@pytest.mark.parametrize("C,k,d", [(32, 3, 1), (32, 3, 5)])
def test_a_lost_low_fp16_plane_of_the_c1_weights_is_caught(C, k, d):
    """A split-fp16 kernel that drops the low plane of one operand computes with c1's weights rounded to fp16 (11 bits)."""
    x, w1, b1, w2, b2 = _pair(61 + d, C, k, d, B=2, T=120)
    ref = cr.pair_ref(x, w1, b1, w2, b2, k, d)[0]
    w1h = w1.astype(np.float16).astype(np.float32)
    assert not np.array_equal(w1h, w1)
    bad = x + _c2(_h64(x, w1h, b1, k, d), w2, b2, k)
    _caught_by_every_family(bad, ref, _bounds(x, w1, b1, w2, b2, k, d), "c1 weights rounded to fp16")
