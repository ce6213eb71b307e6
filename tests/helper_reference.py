"""Float64 references, per-output error bounds, fp32 restatements with mutant switches and the input families of the two helper kernels that
sit between the convs (small_kernels.hip): the anti-aliased SnakeBeta (aa_snake_pk_kernel) and depthwise conv + LayerNorm (launch_dwconv_ln).
CPU only (numpy); test_helper_checker.py shows that the arbiter has teeth, test_gpu_helper_instances.py holds the kernels to it.

The operations (bigvgan.py:121-135 inside alias_free_torch's Activation1d; convnext.py:71-74, 126-129):
  snake   xm = x, or (x + x2 + x3) / 3
          u[2h]   = sum_q 2 up[2q+1] xm[cl(h+2-q)],  u[2h+1] = sum_q 2 up[2q] xm[cl(h+3-q)]      q = 0..5, cl = clamp to [0, T-1]
          a[n]    = u[n] + inv_beta[c] sin(alpha[c] u[n])^2
          y[t]    = sum_j down[j] a[cl2(2t+j-5)]                                                  j = 0..11, cl2 = clamp to [0, 2T-1]
  dwln    h[c,t]  = b[c] + sum_j w[c,j] x[c, t+j-(k-1)/2]   (zeros outside the row; LayerNorm alone: h = x)
          mu = mean_c h,  d = h - mu,  var = mean_c d^2,  y = d / sqrt(var + eps) * g[c] + beta[c]

The bounds.  U = 2^-24; every quantity is float64, formed from the fp32 inputs; the constants are operation counts, not fits, and change only by
derivation, never to what a GPU kernel measures (EPS_COS alone may be replaced by a figure measured for the cosine instruction by itself).
  snake   Au[n]  = sum_q |2 up| |xm|                      the absolute up-FIR of sample n: six products, six sums, the doubled tap -> 8 U Au
          du     = 8 U Au   (+ 3 U sum_q |2 up| (|x| + |x2| + |x3|) / 3 with three operands: two sums and the product with fl(1/3))
          da     = du (1 + inv_beta alpha |sin 2 alpha u|)       d/du of u + inv_beta sin^2(alpha u)
                   + 4 U (|u| + inv_beta)                        the roundings of the activation's own sums and products (sin^2 <= 1)
                   + inv_beta EPS_COS / 2                        the cosine of inv_beta / 2 (1 - cos 2 alpha u)
          bound  = sum_j |dn_j| da[cl2] + 14 U sum_j |dn_j| |a[cl2]|       twelve products, twelve sums
  dwln    Ah = |b| + sum_j |w_j| |x|,  M = mean_c Ah
          dh = (k + 2) U Ah,  dmu = (k + 2 + sqrt C + 8) U M,  dd = dh + dmu + U |d|
          dvar = 2 mean_c(|d| dd) + (sqrt C + 8) U var,  dinv = inv (dvar / (2 (var + eps)) + 3 U)
          bound = |g| (dd inv + |d| dinv) + 4 U |y - beta| + 2 U |y|
          (sums over C channels count sqrt C roundings: their signs are independent; 8 covers the partial-sum tree and the division.  eps is
          the float32 the kernel receives.  The last sum's rounding is counted twice: it is the one term that a single operation attains in
          full — half an ulp is U |y| just above a power of two — so where |g| is small and y ~ beta a faithful fp32 evaluation sits at up to
          1.0 of a bound that counts it once (measured on the CPU: 0.62 at C = 1025, low variance), and the checker's condition that the fp32
          restatement stays below half of every bound needs the factor; every other term sums several roundings that do not all attain theirs)
The fp32 restatements round every operation to float32 in a natural order (taps in ascending order, channel sums in eight groups); the snake's phase alpha * u is formed exactly and the
sine rounded once — what the kernel's compensated phase is for; sinf(fl(alpha u)) loses |alpha u| U of phase, hundreds of U at trained scale."""
import numpy as np

U = 2.0 ** -24
EPS_COS = 8e-7   # twice the 3.8e-7 small_kernels.hip records for v_cos_f32 against sin^2 in double (tools/ubench/valu_rates.hip: the instruction's)
F32 = np.float32


# ---- snake ---------------------------------------------------------------------------------------------------------------------------------
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _up_fir(xm, up2, pad_mode="edge"):
    """(B, C, T) -> (B, C, 2T): u[2h] = sum_q up2[2q+1] xm[h+2-q], u[2h+1] = sum_q up2[2q] xm[h+3-q] on the padded row (q ascending)."""
    T = xm.shape[-1]
    xp = np.pad(xm, ((0, 0), (0, 0), (3, 3)), mode=pad_mode)
    ev = np.zeros_like(xm)
    od = np.zeros_like(xm)
    for q in range(6):
        ev = ev + up2[2 * q + 1] * xp[..., 5 - q:5 - q + T]
        od = od + up2[2 * q] * xp[..., 6 - q:6 - q + T]
    u = np.empty(xm.shape[:-1] + (2 * T,), dtype=xm.dtype)
    u[..., 0::2] = ev
    u[..., 1::2] = od
    return u


def _down_fir(a, dn, pad_mode="edge"):
    """(B, C, 2T) -> (B, C, T): y[t] = sum_j dn[j] a[2t+j-5] on the padded row (j ascending)."""
    T = a.shape[-1] // 2
    ap = np.pad(a, ((0, 0), (0, 0), (5, 6)), mode=pad_mode)
    y = np.zeros(a.shape[:-1] + (T,), dtype=a.dtype)
    for j in range(12):
        y = y + dn[j] * ap[..., j:j + 2 * T:2]
    return y


def snake_parts(x, alpha_eff, inv_beta, up, down, x2=None, x3=None):
    """dict(u, a, ref, bound) in float64: the 2x-rate signal before and after the activation, the output and its per-output bound."""
    x = _f64(x)
    al = _f64(alpha_eff)[None, :, None]
    ib = _f64(inv_beta)[None, :, None]
    up2, dn = 2.0 * _f64(up), _f64(down)
    three = x2 is not None
    assert three == (x3 is not None), "x2 and x3 go together"
    xm = (x + _f64(x2) + _f64(x3)) / 3.0 if three else x
    u = _up_fir(xm, up2)
    a = u + ib * np.sin(al * u) ** 2
    ref = _down_fir(a, dn)
    du = 8.0 * U * _up_fir(np.abs(xm), np.abs(up2))
    if three:
        du = du + 3.0 * U * _up_fir((np.abs(x) + np.abs(_f64(x2)) + np.abs(_f64(x3))) / 3.0, np.abs(up2))
    da = du * (1.0 + ib * al * np.abs(np.sin(2.0 * al * u))) + 4.0 * U * (np.abs(u) + ib) + 0.5 * ib * EPS_COS
    bound = _down_fir(da, np.abs(dn)) + 14.0 * U * _down_fir(np.abs(a), np.abs(dn))
    return dict(u=u, a=a, ref=ref, bound=bound)


def snake_ref(x, alpha_eff, inv_beta, up, down, x2=None, x3=None):
    """(ref, bound) of the anti-aliased SnakeBeta in float64; alpha_eff = exp(alpha), inv_beta = 1 / (exp(beta) + 1e-9) per channel."""
    p = snake_parts(x, alpha_eff, inv_beta, up, down, x2, x3)
    return p["ref"], p["bound"]


def snake_oracle_slack(x, alpha_eff, inv_beta, up, down):
    """What sinf(fl(u alpha)) adds to the bound, per output: the phase product's rounding |alpha u| U moves inv_beta sin^2 by at most as much
    (|d sin^2 / d phase| <= 1) — the fp32 C oracle's class."""
    p = snake_parts(x, alpha_eff, inv_beta, up, down)
    al, ib = _f64(alpha_eff)[None, :, None], _f64(inv_beta)[None, :, None]
    return _down_fir(ib * np.abs(al * p["u"]) * U, np.abs(_f64(down)))


SNAKE_MUTANTS = ("zero_pad_x", "zero_pad_a", "swap_up_taps", "params_by_row", "mean_of_two")


def snake_f32(x, alpha_eff, inv_beta, up, down, x2=None, x3=None, mutant=None):
    """The snake with every operation rounded to float32 (sequential sums, tap order ascending; the phase alpha * u exact, the sine rounded once).
    mutant: None or one of SNAKE_MUTANTS —
      zero_pad_x     zeros instead of replicate padding of the up-sampler input
      zero_pad_a     zeros instead of replicate padding of the 2x-rate signal
      swap_up_taps   up[4] and up[5] trade places
      params_by_row  alpha / inv_beta read at min(b C + c, C - 1) instead of c (shows from the second batch item on)
      mean_of_two    (x + x2) / 3: the third operand never added"""
    assert mutant is None or mutant in SNAKE_MUTANTS, mutant
    x = np.asarray(x, dtype=F32)
    B, C, T = x.shape
    al, ib = np.asarray(alpha_eff, dtype=F32), np.asarray(inv_beta, dtype=F32)
    if mutant == "params_by_row":
        idx = np.minimum(np.arange(B * C), C - 1).reshape(B, C)
        al, ib = al[idx][..., None], ib[idx][..., None]
    else:
        al, ib = al[None, :, None], ib[None, :, None]
    up2 = (F32(2.0) * np.asarray(up, dtype=F32)).astype(F32)
    if mutant == "swap_up_taps":
        up2 = up2.copy()
        up2[[4, 5]] = up2[[5, 4]]
    dn = np.asarray(down, dtype=F32)
    if x2 is not None:
        s = (x + np.asarray(x2, dtype=F32)).astype(F32)
        if mutant != "mean_of_two":
            s = (s + np.asarray(x3, dtype=F32)).astype(F32)
        x = (s * F32(1.0 / 3.0)).astype(F32)
    u = _up_fir(x, up2, "constant" if mutant == "zero_pad_x" else "edge")     # float32 arrays: numpy rounds every product and sum
    assert u.dtype == F32
    s = np.sin(al.astype(np.float64) * u.astype(np.float64)).astype(F32)
    a = (u + (ib * (s * s).astype(F32)).astype(F32)).astype(F32)
    y = _down_fir(a, dn, "constant" if mutant == "zero_pad_a" else "edge")
    assert y.dtype == F32
    return y


# ---- depthwise conv + LayerNorm ----------------------------------------------------------------------------------------------------------------
def _dw(x, w, b, pad_mode="constant", drop_tap0_at_seams=False):
    """(B, C, T), (C, k) or None, (C,) or None -> b + sum_j w[:, j] x[:, t + j - pad] in x's dtype (j ascending); None weight: x itself."""
    if w is None:
        return x
    C, k = w.shape
    T = x.shape[-1]
    pad = (k - 1) // 2
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad)), mode=pad_mode)
    h = np.zeros_like(x) + (b[None, :, None] if b is not None else 0)
    for j in range(k):
        term = w[None, :, j, None] * xp[..., j:j + T]
        if drop_tap0_at_seams and j == 0:
            term = term.copy()
            term[..., 32::32] = 0
        h = h + term
    return h.astype(x.dtype)


def dwln_ref(x, dw_w, dw_b, ln_w, ln_b, eps):
    """(ref, bound) of depthwise conv ('same' zero padding; dw_w None: none) + LayerNorm over channels in float64."""
    x = _f64(x)
    B, C, T = x.shape
    w = None if dw_w is None else _f64(dw_w).reshape(C, -1)
    b = None if dw_b is None else _f64(dw_b)
    g, beta = _f64(ln_w)[None, :, None], _f64(ln_b)[None, :, None]
    k = 1 if w is None else w.shape[1]
    eps = float(F32(eps))
    h = _dw(x, w, b)
    mu = h.mean(axis=1, keepdims=True)
    d = h - mu
    var = (d * d).mean(axis=1, keepdims=True)
    inv = 1.0 / np.sqrt(var + eps)
    ref = d * inv * g + beta
    Ah = np.abs(x) if w is None else _dw(np.abs(x), np.abs(w), None if b is None else np.abs(b))
    M = Ah.mean(axis=1, keepdims=True)
    rc = np.sqrt(C)
    dh = (k + 2) * U * Ah
    dmu = (k + 2 + rc + 8) * U * M
    dd = dh + dmu + U * np.abs(d)
    dvar = 2.0 * (np.abs(d) * dd).mean(axis=1, keepdims=True) + (rc + 8) * U * var
    dinv = inv * (0.5 * dvar / (var + eps) + 3.0 * U)
    bound = np.abs(g) * (dd * inv + np.abs(d) * dinv) + 4.0 * U * np.abs(ref - beta) + 2.0 * U * np.abs(ref)
    return ref, bound


def _group_sum(v, groups=8):
    """(B, n, T) float32 -> (B, T): channel c goes to group c % 8, each group summed in ascending order, then the eight partial sums — the
    coarsest split of the channel sums among the launcher's kernels (8 groups: the generic and the 8-group tile kernels; the others 16)."""
    part = np.zeros((v.shape[0], groups, v.shape[2]), dtype=F32)
    for c in range(v.shape[1]):
        part[:, c % groups] = (part[:, c % groups] + v[:, c]).astype(F32)
    s = np.zeros((v.shape[0], v.shape[2]), dtype=F32)
    for g in range(groups):
        s = (s + part[:, g]).astype(F32)
    return s


DWLN_MUTANTS = ("eps_1e-5", "drop_last_channel", "var_over_c_minus_1", "drop_tap0_at_seams", "replicate_pad", "no_bias")


def dwln_f32(x, dw_w, dw_b, ln_w, ln_b, eps, mutant=None):
    """Depthwise conv + LayerNorm with every operation rounded to float32: taps ascending, channel sums in eight interleaved groups (_group_sum), 1 / sqrt(var + eps).
    mutant: None or one of DWLN_MUTANTS —
      eps_1e-5            eps = 1e-5 whatever was passed
      drop_last_channel   channel C - 1 left out of the sums of the mean and the variance (still divided by C)
      var_over_c_minus_1  the unbiased variance
      drop_tap0_at_seams  tap 0 (the input three columns back, in the previous 32-column tile) dropped at columns 32, 64, ...
      replicate_pad       replicate instead of zero padding of the depthwise conv
      no_bias             the depthwise bias never added"""
    assert mutant is None or mutant in DWLN_MUTANTS, mutant
    x = np.asarray(x, dtype=F32)
    B, C, T = x.shape
    w = None if dw_w is None else np.asarray(dw_w, dtype=F32).reshape(C, -1)
    b = None if (dw_b is None or mutant == "no_bias") else np.asarray(dw_b, dtype=F32)
    g, beta = np.asarray(ln_w, dtype=F32)[None, :, None], np.asarray(ln_b, dtype=F32)[None, :, None]
    eps = F32(1e-5 if mutant == "eps_1e-5" else eps)
    h = _dw(x, w, b, "edge" if mutant == "replicate_pad" else "constant", mutant == "drop_tap0_at_seams")
    assert h.dtype == F32
    n_sum = C - 1 if mutant == "drop_last_channel" else C
    mu = (_group_sum(h[:, :n_sum]) / F32(C)).astype(F32)[:, None, :]
    d = (h - mu).astype(F32)
    q = _group_sum((d[:, :n_sum] * d[:, :n_sum]).astype(F32))
    var = (q / F32(C - 1 if mutant == "var_over_c_minus_1" else C)).astype(F32)[:, None, :]
    inv = (F32(1.0) / np.sqrt((var + eps).astype(F32)).astype(F32)).astype(F32)
    y = (((d * inv).astype(F32) * g).astype(F32) + beta).astype(F32)
    return y


# ---- the arbiter -----------------------------------------------------------------------------------------------------------------------------
def ratio(y, ref, bound):
    """max |y - ref| / bound over the outputs (inf for a non-finite output)."""
    y64 = _f64(y)
    if not np.isfinite(y64).all():
        return float("inf")
    return float((np.abs(y64 - ref) / bound).max()) if y64.size else 0.0


def check_per_output(y, ref, bound, what=""):
    """Every output finite and inside its bound; the worst one is named.  Returns the largest ratio."""
    y64 = _f64(y)
    assert y64.shape == ref.shape == bound.shape, (what, y64.shape, ref.shape, bound.shape)
    if not np.isfinite(y64).all():
        i = tuple(int(v) for v in np.argwhere(~np.isfinite(y64))[0])
        raise AssertionError(f"{what}: {int((~np.isfinite(y64)).sum())} non-finite outputs, first at {i}: {y64[i]} (ref {ref[i]:.6e})")
    assert (bound > 0).all(), f"{what}: the bound is not positive everywhere"
    err = np.abs(y64 - ref)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} outputs past the per-output bound; worst at {tuple(int(v) for v in i)}: "
                             f"|d| = {err[i]:.3e}, bound {bound[i]:.3e} ({err[i] / bound[i]:.2f} x), y {y64[i]:.6e}, ref {ref[i]:.6e}")
    return float((err / bound).max()) if err.size else 0.0


# ---- the input families (shared by the CPU checker and the GPU instance tests) ----------------------------------------------------------------
SNAKE_B, SNAKE_C = 2, 3
SNAKE_T_SHORT = [1, 2, 5, 6, 7, 8, 11, 12, 13]                                       # both row ends inside one tile
SNAKE_T_SEAM = [1018, 1023, 1024, 1025, 1030, 1031, 1036, 2047, 2048, 2052]          # one and two tiles: a seam with the row end within +-12
SNAKE_T_INTERIOR = [2055, 2056, 2060]                                                # interior(1024) needs 1024 + 1030 < T: first at T = 2055
SNAKE_T_MANY = [3078, 3079, 3084, 4100]                                              # interior(2048) needs T >= 3079; four tiles and a tail
SNAKE_T = SNAKE_T_SHORT + SNAKE_T_SEAM + SNAKE_T_INTERIOR + SNAKE_T_MANY
SNAKE_FAMILIES = ("synthetic", "trained", "tiny", "constant")


def kaiser_sinc_taps():
    """alias_free_torch's kaiser_sinc_filter1d(cutoff 0.25, half-width 0.3, 12 taps) in float64, rounded to float32 (the oracle's design)."""
    ks, cutoff, half_width = 12, 0.25, 0.3
    A = 2.285 * (ks // 2 - 1) * np.pi * 4 * half_width + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50 else (0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21) if A >= 21 else 0.0)
    win = np.kaiser(ks, beta)
    t = np.arange(-(ks // 2), ks // 2) + 0.5
    f = 2 * cutoff * win * np.sinc(2 * cutoff * t)
    return (f / f.sum()).astype(F32)


def snake_params(family, C, rng):
    """(alpha_eff, inv_beta) as make_aasnake uploads them: exp(alpha), 1 / (exp(beta) + 1e-9), distinct per channel."""
    mean, std = (2.5, 0.5) if family == "trained" else (0.0, 0.3)
    la, lb = rng.normal(mean, std, size=C).astype(F32), rng.normal(mean, std, size=C).astype(F32)
    alpha = np.exp(la.astype(np.float64)).astype(F32)
    inv_beta = (1.0 / (np.exp(lb.astype(np.float64)) + 1e-9)).astype(F32)
    return alpha, inv_beta


def snake_input(family, B, C, T, rng):
    """synthetic: |x| ~ 1; trained: |x| ~ 5 (|alpha u| in the hundreds with the trained parameters); tiny: |x| ~ 1e-4; constant: rows constant in
    t, a different value per row (a padding error shows at both ends of every row)."""
    if family == "constant":
        return np.repeat(rng.normal(size=(B, C, 1)) * 2.0, T, axis=2).astype(F32)
    scale = {"synthetic": 1.0, "trained": 5.0, "tiny": 1e-4}[family]
    return (rng.normal(size=(B, C, T)) * scale).astype(F32)


def snake_case(family, T, seed=0, B=SNAKE_B, C=SNAKE_C, operands=1):
    """(x, x2, x3, alpha_eff, inv_beta, up, down) of a case; x2 = x3 = None with one operand.  Up and down taps differ (the down filter is the
    design scaled off symmetry by a per-tap factor) so that a swap of the two tables, or of two taps, changes the result."""
    rng = np.random.default_rng([seed, T, SNAKE_FAMILIES.index(family), operands])
    alpha, inv_beta = snake_params(family, C, rng)
    taps = kaiser_sinc_taps()
    up = (taps * (1.0 + 0.05 * rng.normal(size=12))).astype(F32)
    down = (taps * (1.0 + 0.05 * rng.normal(size=12))).astype(F32)
    xs = [snake_input(family, B, C, T, rng) for _ in range(operands)]
    return (xs[0], xs[1] if operands == 3 else None, xs[2] if operands == 3 else None, alpha, inv_beta, up, down)


def host_mean3(x, x2, x3):
    """((x + x2) + x3) * float32(1/3) in float32: the kernel's three-operand mean, operation for operation."""
    return (((x + x2).astype(F32) + x3).astype(F32) * F32(1.0 / 3.0)).astype(F32)


# (B, C, T): C at 1 and -1 around every CMAX step (256, 512, 1024) and around the 64-row chunks, the three widths of the recorded NaN (320, 384,
# 640), T at 1, at -1 / 0 / +1 of a 32-column tile and several tiles, B * n_tiles both no multiple of 8 and above 8
DWLN_SHAPES = [(3, 1, 33), (3, 7, 33), (1, 64, 1), (3, 65, 94), (2, 100, 31), (1, 256, 65), (3, 257, 6), (2, 320, 33), (1, 384, 94),
               (3, 512, 32), (1, 513, 33), (2, 640, 65), (1, 1000, 31), (3, 1024, 94), (1, 1025, 33), (2, 1100, 7)]
DWLN_ODD_K_SHAPES = [(3, 65, 94), (1, 513, 33), (2, 1100, 7)]    # k = 3 and 9 run here
DWLN_FAMILIES = ("unequal", "offset", "lowvar")
DWLN_EPS = (1e-6, 1e-5)


def dwln_case(family, B, C, T, k, seed=0):
    """(x, dw_w, dw_b, ln_w, ln_b); k = 0: LayerNorm alone (dw_w = dw_b = None).
    unequal: channels of unequal scale (0.3 to 3 times); offset: the same plus a common +30; lowvar: |x| ~ 1e-3 on even and 3e-4 on odd
    batch items, so that var ~ eps."""
    rng = np.random.default_rng([seed, B, C, T, k, DWLN_FAMILIES.index(family)])
    x = rng.normal(size=(B, C, T))
    if family == "lowvar":
        x = x * np.where(np.arange(B) % 2 == 0, 1e-3, 3e-4)[:, None, None]
    else:
        x = x * np.exp(rng.uniform(np.log(0.3), np.log(3.0), size=C))[None, :, None]
        if family == "offset":
            x = x + 30.0
    ln_w = (1.0 + 0.3 * rng.normal(size=C)).astype(F32)
    ln_b = (0.5 * rng.normal(size=C)).astype(F32)
    if k == 0:
        return x.astype(F32), None, None, ln_w, ln_b
    dw_w = (rng.normal(size=(C, k)) / np.sqrt(k)).astype(F32)
    # lowvar: a bias of the input's size keeps var ~ eps after the conv
    dw_b = (rng.normal(size=C) * (1e-3 if family == "lowvar" else 0.5)).astype(F32)
    return x.astype(F32), dw_w, dw_b, ln_w, ln_b
