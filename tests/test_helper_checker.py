"""CPU: the arbiter of test_gpu_helper_instances.py (helper_reference.py) has teeth.  The float64 references equal their definitions written as plain
loops, torch's float64 conv1d + layer_norm, the C oracle's Activation1d and the golden activation; the fp32 restatements sit at no more than half
of every bound on every input family the GPU tests use; every mutant is at least ten times past the bound at the smallest shape where it shows."""
import math

import numpy as np
import pytest

import helper_reference as hr
from conftest import load_golden

torch = pytest.importorskip("torch")
F32 = np.float32


# ---- the references are their definitions ------------------------------------------------------------------------------------------------------
def _snake_loops(x, al, ib, up, dn, x2=None, x3=None):
    B, C, T = x.shape
    y = np.zeros((B, C, T))
    for b in range(B):
        for c in range(C):
            xm = [float(x[b, c, t]) if x2 is None else (float(x[b, c, t]) + float(x2[b, c, t]) + float(x3[b, c, t])) / 3.0 for t in range(T)]
            a = []
            for n in range(2 * T):
                h, acc = n // 2, 0.0
                for q in range(6):
                    tap, src = (up[2 * q + 1], h + 2 - q) if n % 2 == 0 else (up[2 * q], h + 3 - q)
                    acc += 2.0 * float(tap) * xm[min(max(src, 0), T - 1)]
                a.append(acc + float(ib[c]) * math.sin(float(al[c]) * acc) ** 2)
            for t in range(T):
                y[b, c, t] = sum(float(dn[j]) * a[min(max(2 * t + j - 5, 0), 2 * T - 1)] for j in range(12))
    return y


@pytest.mark.parametrize("T", [1, 2, 5, 9])
@pytest.mark.parametrize("operands", [1, 3])
def test_snake_ref_equals_its_definition_in_plain_loops(T, operands):
    x, x2, x3, al, ib, up, dn = hr.snake_case("synthetic", T, seed=1, operands=operands)
    ref, bound = hr.snake_ref(x, al, ib, up, dn, x2, x3)
    loops = _snake_loops(x, al, ib, up, dn, x2, x3)
    assert np.abs(ref - loops).max() <= 1e-13 * max(1.0, np.abs(loops).max())
    assert (bound > 0).all() and bound.shape == ref.shape


def _dwln_loops(x, w, b, g, beta, eps):
    B, C, T = x.shape
    k = 1 if w is None else w.shape[1]
    pad = (k - 1) // 2
    y = np.zeros((B, C, T))
    for bi in range(B):
        for t in range(T):
            h = []
            for c in range(C):
                if w is None:
                    h.append(float(x[bi, c, t]))
                    continue
                acc = 0.0 if b is None else float(b[c])
                for j in range(k):
                    tt = t + j - pad
                    if 0 <= tt < T:
                        acc += float(w[c, j]) * float(x[bi, c, tt])
                h.append(acc)
            mu = sum(h) / C
            var = sum((v - mu) ** 2 for v in h) / C
            for c in range(C):
                y[bi, c, t] = (h[c] - mu) / math.sqrt(var + float(F32(eps))) * float(g[c]) + float(beta[c])
    return y


@pytest.mark.parametrize("k", [0, 1, 3, 7])
def test_dwln_ref_equals_its_definition_in_plain_loops(k):
    x, w, b, g, beta = hr.dwln_case("unequal", 2, 3, 5, k, seed=2)
    ref, bound = hr.dwln_ref(x, w, b, g, beta, 1e-6)
    assert np.abs(ref - _dwln_loops(x, w, b, g, beta, 1e-6)).max() <= 1e-13
    ref_nb, _ = hr.dwln_ref(x, w, None, g, beta, 1e-6)
    assert np.abs(ref_nb - _dwln_loops(x, w, None, g, beta, 1e-6)).max() <= 1e-13
    assert (bound > 0).all() and bound.shape == ref.shape


@pytest.mark.parametrize("B,C,T,k", [(3, 7, 33, 7), (2, 100, 31, 3), (1, 65, 40, 9), (2, 20, 6, 0)])
@pytest.mark.parametrize("family", hr.DWLN_FAMILIES)
def test_dwln_ref_equals_torch_float64(B, C, T, k, family):
    import torch.nn.functional as F
    x, w, b, g, beta = hr.dwln_case(family, B, C, T, k, seed=3)
    eps = float(F32(1e-6))
    ref, _ = hr.dwln_ref(x, w, b, g, beta, 1e-6)
    h = torch.from_numpy(x.astype(np.float64))
    if w is not None:
        h = F.conv1d(h, torch.from_numpy(w.astype(np.float64))[:, None, :], torch.from_numpy(b.astype(np.float64)), padding=(k - 1) // 2, groups=C)
    y = F.layer_norm(h.transpose(1, 2), (C,), torch.from_numpy(g.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)), eps).transpose(1, 2)
    assert np.abs(ref - y.numpy()).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("family,T", [("synthetic", 37), ("synthetic", 1), ("synthetic", 5), ("trained", 300), ("constant", 13)])
def test_snake_ref_agrees_with_the_c_oracle(family, T):
    """Two independent restatements: oracle.activation1d around oracle.snake (fp32, sinf(fl(u alpha))) lies within the float64 bound plus what the
    rounded phase product adds (snake_oracle_slack, twice: sinf's own ulp rides on it)."""
    from oracle import oracle as orc
    x, _, _, al, ib, up, dn = hr.snake_case(family, T, seed=4)
    beta_lin = (F32(1.0) / ib).astype(F32)                       # the oracle forms 1 / (beta + 1e-9f) in fp32: hand the reference that value
    ib32 = (F32(1.0) / (beta_lin + F32(1e-9))).astype(F32)
    y = orc.activation1d(x, lambda z: orc.snake(z, al, beta_lin, False), up, dn)
    ref, bound = hr.snake_ref(x, al, ib32, up, dn)
    tol = bound + 2.0 * hr.snake_oracle_slack(x, al, ib32, up, dn)
    err = np.abs(y.astype(np.float64) - ref)
    print(f"{family} T = {T}: oracle vs float64 max |d| = {err.max():.3e}, largest ratio to bound + slack {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), float((err / tol).max())
    assert err.max() <= 1e-4 * max(1.0, np.abs(ref).max())     # (the class itself: nowhere near a structural difference)


def test_snake_ref_reproduces_the_golden_activation():
    g = load_golden("activation1d.npz")
    al = np.exp(g["alpha"].astype(np.float64)).astype(F32)
    ib = (1.0 / (np.exp(g["beta"].astype(np.float64)) + 1e-9)).astype(F32)
    p = hr.snake_parts(g["x"], al, ib, g["taps"], g["taps"])
    Au = hr._up_fir(np.abs(g["x"].astype(np.float64)), np.abs(2.0 * g["taps"].astype(np.float64)))
    assert (np.abs(g["up"] - p["u"]) <= 8.0 * hr.U * Au + hr.U * np.abs(p["u"])).all()
    # the golden's fp32 exp(alpha) and sin(fl(x alpha)): the phase slack, and as much again for one ulp of alpha
    tol = p["bound"] + 4.0 * hr.snake_oracle_slack(g["x"], al, ib, g["taps"], g["taps"])
    err = np.abs(g["y"] - p["ref"])
    print(f"golden activation: max |d| = {err.max():.3e}, largest ratio {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    assert err.max() <= 2e-6


# ---- the fp32 restatements sit inside every bound, with room ----------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", [1, 3])
@pytest.mark.parametrize("family", hr.SNAKE_FAMILIES)
def test_snake_f32_restatement_is_within_half_of_every_bound(family, operands):
    worst = 0.0
    for T in hr.SNAKE_T:
        x, x2, x3, al, ib, up, dn = hr.snake_case(family, T, operands=operands)
        ref, bound = hr.snake_ref(x, al, ib, up, dn, x2, x3)
        worst = max(worst, hr.check_per_output(hr.snake_f32(x, al, ib, up, dn, x2, x3), ref, bound, f"snake_f32 {family} T={T} x{operands}"))
    print(f"snake fp32 restatement, {family}, {operands} operand(s), {len(hr.SNAKE_T)} lengths: largest ratio {worst:.3f}")
    assert worst <= 0.5, worst


def test_the_trained_family_reaches_hundreds_of_radians():
    x, _, _, al, ib, up, dn = hr.snake_case("trained", 4100)
    p = hr.snake_parts(x, al, ib, up, dn)
    phase = np.abs(al.astype(np.float64)[None, :, None] * p["u"]).max()
    assert phase > 200.0, phase


@pytest.mark.parametrize("k", [0, 7, 3, 9])
@pytest.mark.parametrize("family", hr.DWLN_FAMILIES)
def test_dwln_f32_restatement_is_within_half_of_every_bound(family, k):
    worst = 0.0
    for (B, C, T) in (hr.DWLN_SHAPES if k in (0, 7) else hr.DWLN_ODD_K_SHAPES):
        case = hr.dwln_case(family, B, C, T, k)
        for eps in hr.DWLN_EPS:
            ref, bound = hr.dwln_ref(*case, eps)
            worst = max(worst, hr.check_per_output(hr.dwln_f32(*case, eps), ref, bound, f"dwln_f32 {family} {(B, C, T)} k={k} eps={eps}"))
    print(f"dwln fp32 restatement, {family}, k = {k}: largest ratio {worst:.3f}")
    assert worst <= 0.5, worst


def test_the_low_variance_family_has_var_near_eps():
    x, _, _, _, _ = hr.dwln_case("lowvar", 3, 65, 94, 0)
    var = x.astype(np.float64).var(axis=1)
    assert 3e-7 < var[0].mean() < 3e-6 and 3e-8 < var[1].mean() < 3e-7, (var[0].mean(), var[1].mean())


# ---- every mutant fails, far outside ----------------------------------------------------------------------------------------------------------
# (LayerNorm over two channels is +-1 whatever the depthwise conv gave, so the conv's mutants start at three channels; the seam mutant needs a
# second 32-column tile, the padding mutant a second column)
def _must_fail(y, ref, bound, what):
    r = hr.ratio(y, ref, bound)
    print(f"{what}: {r:.3g} x the bound")
    with pytest.raises(AssertionError):
        hr.check_per_output(y, ref, bound, what)
    assert r >= 10.0, (what, r)


# (mutant, family, B, T, operands): the smallest shape where the mutant can show — a single sample has both paddings, two up taps need a row
# that is not constant, the row-indexed parameters a second batch item
@pytest.mark.parametrize("mutant,family,B,T,operands", [
    ("zero_pad_x", "synthetic", 1, 1, 1), ("zero_pad_x", "constant", 1, 1, 1), ("zero_pad_a", "synthetic", 1, 1, 1),
    ("zero_pad_a", "constant", 1, 1, 1), ("swap_up_taps", "synthetic", 1, 2, 1), ("params_by_row", "synthetic", 2, 1, 1),
    ("mean_of_two", "synthetic", 1, 1, 3), ("zero_pad_x", "trained", 1, 1, 1), ("zero_pad_a", "tiny", 1, 1, 1)])
def test_snake_mutants_are_far_outside_the_bound(mutant, family, B, T, operands):
    x, x2, x3, al, ib, up, dn = hr.snake_case(family, T, seed=5, B=B, operands=operands)
    ref, bound = hr.snake_ref(x, al, ib, up, dn, x2, x3)
    hr.check_per_output(hr.snake_f32(x, al, ib, up, dn, x2, x3), ref, bound, "unmutated")
    _must_fail(hr.snake_f32(x, al, ib, up, dn, x2, x3, mutant=mutant), ref, bound, f"snake {mutant} {family} B={B} T={T}")


def test_snake_params_by_row_needs_the_second_batch_item():
    x, _, _, al, ib, up, dn = hr.snake_case("synthetic", 5, seed=5, B=1)
    assert np.array_equal(hr.snake_f32(x, al, ib, up, dn, mutant="params_by_row"), hr.snake_f32(x, al, ib, up, dn))


@pytest.mark.parametrize("mutant,family,B,C,T,k,eps", [
    ("eps_1e-5", "lowvar", 1, 2, 1, 0, 1e-6), ("eps_1e-5", "lowvar", 2, 65, 1, 7, 1e-6),
    ("drop_last_channel", "unequal", 1, 65, 1, 0, 1e-6), ("drop_last_channel", "unequal", 1, 513, 1, 0, 1e-6),
    ("drop_last_channel", "unequal", 1, 1025, 1, 0, 1e-6), ("drop_last_channel", "offset", 1, 1025, 1, 7, 1e-6),
    ("drop_last_channel", "lowvar", 1, 1025, 1, 0, 1e-5),
    ("var_over_c_minus_1", "unequal", 1, 2, 1, 0, 1e-6), ("var_over_c_minus_1", "unequal", 1, 1025, 1, 0, 1e-6),
    ("drop_tap0_at_seams", "unequal", 1, 3, 33, 7, 1e-6), ("drop_tap0_at_seams", "lowvar", 1, 3, 33, 3, 1e-6),
    ("replicate_pad", "unequal", 1, 3, 2, 3, 1e-6), ("replicate_pad", "offset", 1, 3, 2, 7, 1e-6),
    ("no_bias", "unequal", 1, 3, 1, 3, 1e-6), ("no_bias", "lowvar", 1, 3, 1, 7, 1e-6)])
def test_dwln_mutants_are_far_outside_the_bound(mutant, family, B, C, T, k, eps):
    case = hr.dwln_case(family, B, C, T, k, seed=6)
    ref, bound = hr.dwln_ref(*case, eps)
    hr.check_per_output(hr.dwln_f32(*case, eps), ref, bound, "unmutated")
    _must_fail(hr.dwln_f32(*case, eps, mutant=mutant), ref, bound, f"dwln {mutant} {family} {(B, C, T)} k={k}")


def test_check_per_output_names_the_worst_output_and_refuses_non_finite_ones():
    ref = np.zeros((1, 2, 3))
    bound = np.full((1, 2, 3), 1e-6)
    y = np.zeros((1, 2, 3), dtype=F32)
    assert hr.check_per_output(y, ref, bound) == 0.0
    y[0, 1, 2] = 3e-6
    y[0, 0, 1] = 2e-6
    with pytest.raises(AssertionError, match=r"2 of 6 outputs.*worst at \(0, 1, 2\)"):
        hr.check_per_output(y, ref, bound, "case")
    y[0, 1, 0] = np.nan
    with pytest.raises(AssertionError, match=r"non-finite outputs, first at \(0, 1, 0\)"):
        hr.check_per_output(y, ref, bound, "case")
    assert hr.ratio(y, ref, bound) == float("inf")
