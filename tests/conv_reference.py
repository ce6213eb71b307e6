"""float64 references and the per-output error bounds for the direct-sum conv kernel (conv_mfma_impl.h) and the fused ResBlock (c1, c2) pair
kernels (conv_pair.hip): shared by the GPU instance tests (test_gpu_conv_instances.py, test_gpu_pair_instances.py) and the CPU tests that show
the bounds catch subtly wrong kernels (test_conv_checker.py, test_pair_checker.py).  CPU only: numpy and torch.nn.functional in float64."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24   # unit round-off of fp32

# Per-output bound  |y - ref| <= C_BOUND * U * (sqrt(K) + A_BOUND) * A,   A = sum |w| |act(x)| + |b| + |res|  (the float64 absolute-value conv of
# the same layer), K = the terms of the sum (C_in x GEMM taps).  sqrt(K): the fp32 accumulation chain of the MFMAs, whose rounding errors add up
# like a random walk; A_BOUND: a fixed number of roundings per output that does not grow with K — the pre-activation of every operand (SiLU through
# exp / rcp: a few ulp each, relative), the bias and the residual additions.  Calibrated once on an MI355X over every instance of
# test_gpu_conv_instances.py (heavy-tailed layers, all its activations and residuals): the largest ratio |y - ref| / (U (sqrt(K) + 8) A) measured
# was 0.55 on the tiled kernel, 0.44 on the split-K kernels (staged and direct alike), 0.16 on the generic one — C_BOUND = 1 leaves 1.8 x of
# margin, while a tap, a channel chunk or a phase gone wrong is orders of magnitude past it (test_conv_checker.py).
C_BOUND = 1.0
A_BOUND = 8.0
# post-activations act on the finished sum: the bound of the sum times the slope of the function (<= 1.13 for GELU, <= 1 for tanh), plus the
# activation's own error — tanhf a few ulp of its value, the kernels' GELU (gelu_fast, conv_mfma_impl.h) 4.3e-7 absolute
POST_SLOPE = 1.13
POST_ABS = {"none": 0.0, "tanh": 0.0, "gelu": 4.3e-7}
POST_REL = {"none": 0.0, "tanh": 4 * U, "gelu": 4 * U}


def heavy_tailed_weight(rng, c_out, c_in, k, transposed=False):
    """A folded weight-norm layer w = g * v / ||v|| (hifigan.py:31) with the per-output-channel gain g log-uniform over 100 x and 0.4 % of
    the taps 30 x larger than their neighbours.  Conv1d layout (c_out, c_in, k), or ConvTranspose1d's (c_in, c_out, k) with the gain and the
    norm still per OUTPUT channel.  The draws for a square Conv1d are those test_gpu_conv.py has always made."""
    shape = (c_in, c_out, k) if transposed else (c_out, c_in, k)
    v = rng.normal(size=shape)
    hit = rng.random(size=v.shape) < 0.004
    v = np.where(hit, 30.0 * v, v)
    if transposed:
        g = np.exp(rng.uniform(np.log(0.03), np.log(3.0), size=(1, c_out, 1)))
        return (g * v / np.sqrt((v * v).sum(axis=(0, 2), keepdims=True))).astype(np.float32)
    g = np.exp(rng.uniform(np.log(0.03), np.log(3.0), size=(c_out, 1, 1)))
    return (g * v / np.sqrt((v * v).sum(axis=(1, 2), keepdims=True))).astype(np.float32)


def unequal_channels(rng, B, c, T):
    """Input whose channels differ in scale (0.3 ... 3 x), as the outputs of a trained layer do."""
    return (rng.normal(size=(B, c, T)) * np.exp(rng.uniform(np.log(0.3), np.log(3.0), size=(1, c, 1)))).astype(np.float32)


def act64(x, act, slope=0.0):
    x = np.asarray(x, dtype=np.float64)
    if act == "none":
        return x
    if act == "silu":
        return x / (1.0 + np.exp(-x))
    if act == "leaky":
        return np.where(x >= 0, x, x * slope)
    if act == "tanh":
        return np.tanh(x)
    if act == "gelu":
        return F.gelu(torch.from_numpy(x)).numpy()
    raise ValueError(act)


def conv64(x, w, *, transposed=False, stride=1, padding=0, dilation=1):
    """torch.nn.functional.conv1d / conv_transpose1d in float64 on the CPU (no bias)."""
    xt, wt = torch.from_numpy(np.asarray(x, dtype=np.float64)), torch.from_numpy(np.asarray(w, dtype=np.float64))
    if transposed:
        return F.conv_transpose1d(xt, wt, stride=stride, padding=padding).numpy()
    return F.conv1d(xt, wt, padding=padding, dilation=dilation).numpy()


def layer_ref(x, w, b, geo, pre="none", post="none", slope=0.0, res=None):
    """(ref, lin, A): the float64 output, the float64 value in front of the post-activation, and the absolute-value conv A of the layer
    pre-act -> conv -> + bias [+ res] -> post-act.  geo: dict(transposed, stride, padding, dilation)."""
    xa = act64(x, pre, slope)
    lin = conv64(xa, w, **geo)
    A = conv64(np.abs(xa), np.abs(np.asarray(w, dtype=np.float64)), **geo)
    if b is not None:
        lin = lin + np.asarray(b, dtype=np.float64)[None, :, None]
        A = A + np.abs(np.asarray(b, dtype=np.float64))[None, :, None]
    if res is not None:
        lin = lin + res
        A = A + np.abs(np.asarray(res, dtype=np.float64))
    return act64(lin, post), lin, A


def terms(c_in, k, transposed=False, stride=1):
    """K of the bound: the products of one output's sum in the GEMM view (polyphase: ceil(k / stride) taps per phase)."""
    return c_in * ((k + stride - 1) // stride if transposed else k)


def bound(A, K, ref=None, post="none"):
    """The per-output bound (see C_BOUND)."""
    e = C_BOUND * U * (np.sqrt(K) + A_BOUND) * A
    if post != "none":
        e = POST_SLOPE * e + POST_ABS[post] + POST_REL[post] * np.abs(ref)
    return e


def error_ratio(y, ref, A, K, post="none"):
    """max over the outputs of |y - ref| / bound: <= 1 passes."""
    return float((np.abs(np.asarray(y, dtype=np.float64) - ref) / bound(A, K, ref, post)).max())


def check_per_output(y, ref, A, K, post="none", what=""):
    """The per-output bound, and the suite's older global bar (2e-5 of the output's scale, tests/test_gpu_conv.py _check)."""
    y64 = np.asarray(y, dtype=np.float64)
    assert y64.shape == ref.shape, (what, y64.shape, ref.shape)
    assert np.isfinite(y64).all(), what
    err = np.abs(y64 - ref)
    bnd = bound(A, K, ref, post)
    bad = err > bnd
    if bad.any():
        i = np.unravel_index(int(np.argmax(err / bnd)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} outputs past the per-output bound; worst at {tuple(int(v) for v in i)}: "
                             f"|d| = {err[i]:.3e}, bound {bnd[i]:.3e}, ref {ref[i]:.6e}, A {A[i]:.3e}")
    scale = float(np.abs(ref).max())
    assert float(err.max()) <= 2e-5 * max(scale, 1.0), (what, float(err.max()), scale)


def impulse_input(B, c_in, T, positions, channels, gap, seed=0):
    """A zero input with +-1 / +-2^j impulses: every wanted (t) position of `positions` lands in some batch item, impulses of one item are more
    than `gap` samples apart (so every output receives at most one product), channels cycle through `channels`, and each item gets another
    set.  Returns (x, list of (b, c, t, value)); B grows as far as the positions need (at least the B asked for)."""
    rng = np.random.default_rng(seed)
    vals = [1.0, -1.0, 2.0 ** 3, -(2.0 ** -5), 2.0 ** 7, -(2.0 ** 2), 2.0 ** -9, -(2.0 ** 11)]
    items = [[] for _ in range(B)]
    for t in sorted(set(int(t) for t in positions if 0 <= t < T)):
        for it in items:
            if all(abs(t - u) > gap for u in it):
                it.append(t)
                break
        else:
            items.append([t])
    x = np.zeros((len(items), c_in, T), dtype=np.float32)
    placed, n = [], 0
    for bi, it in enumerate(items):
        off = int(rng.integers(0, len(channels)))
        for t in it:
            c = channels[(n + off) % len(channels)]
            v = vals[(n + bi) % len(vals)]
            x[bi, c, t] = v
            placed.append((bi, c, t, v))
            n += 1
    return x, placed


def conv1d_loops(x, w, b, dilation, padding):
    """Conv1d by its definition, in plain loops (the arbiter of conv64 on small shapes)."""
    B, C, T = x.shape
    O, _, k = w.shape
    To = T + 2 * padding - dilation * (k - 1)
    y = np.zeros((B, O, To))
    for bi in range(B):
        for o in range(O):
            for t in range(To):
                s = 0.0 if b is None else float(b[o])
                for c in range(C):
                    for j in range(k):
                        ti = t - padding + j * dilation
                        if 0 <= ti < T:
                            s += float(w[o, c, j]) * float(x[bi, c, ti])
                y[bi, o, t] = s
    return y


def conv_transpose1d_loops(x, w, b, stride, padding):
    """ConvTranspose1d by its definition (scatter of every input sample), in plain loops."""
    B, C, T = x.shape
    _, O, k = w.shape
    To = (T - 1) * stride - 2 * padding + k
    y = np.zeros((B, O, To))
    if b is not None:
        y += np.asarray(b, dtype=np.float64)[None, :, None]
    for bi in range(B):
        for c in range(C):
            for q in range(T):
                for o in range(O):
                    for j in range(k):
                        t = q * stride - padding + j
                        if 0 <= t < To:
                            y[bi, o, t] += float(w[c, o, j]) * float(x[bi, c, q])
    return y


# ---- the fused ResBlock pair  y = x + c2(silu(c1(silu(x))))  (conv_pair.hip) ------------------------------------------------------------------
# The pair's bound is the single layer's, composed:  e1 = b(A1, K) for the intermediate h, e = b(A2, K) + SILU_SLOPE * conv(e1, |w2|) for the
# output (|silu'| <= 1.0998; silu's own rounding is inside A_BOUND).  b() per kernel family of conv_pair_run:
#   direct  (resblock_pair)            b = bound(A, K): the constants above, unchanged
#   f16x3   (pair_f16x3, both kernels) b = bound(A, K) + C_F16 * 2^-22 * A + 2^-25 * sum|w| + 2^-38 * max|w| * sum|a|.  Both operands are split
#           into two fp16 planes and the lo * lo product is dropped: every product carries a systematic relative error of order 2^-22; the
#           activation's low plane bottoms out at fp16's subnormal spacing (2^-25 absolute per activation, times the row's sum|w|), the weight's
#           — scaled so that max|w| s lies in [2^13, 2^14), conv_pack.hip — at 2^-25 / s <= 2^-38 max|w| per weight, times the window's sum|a|
#   wino23 / wino44 (pair_wino, pair_wino44)  b = M_WINO * U * (sqrt(K) + A_BOUND) * A_W: the transforms mix neighbouring samples of a channel
#           and the taps of one (o, i), so A_W[o, t] = sum_i (sum_j |w[o, i, j]|) max_{|t' - t| <= r} |a[i, t']| + |b| + |res| takes A's place,
#           r = the kernel's tile span (2 d for F(2,3), 4 d for F(4,4)) + (k - 1) d / 2.  A_W >= A, and it is still per output channel.
# The three multipliers cannot be derived: each is twice the largest value measured on an MI355X against the float64 reference over every
# instance of its family (test_gpu_pair_instances.py, all its lengths, batch sizes and alignments; heavy-tailed weights, unequal channels) —
# the margin C_BOUND has over its 0.55.  The measured unit is |y - ref| over the bound's multiplied part with the multiplier at 1 (f16x3: over
# the composed 2^-22 A term alone, so the fp32 term b(A, K) and the floors stay on top of the doubled measurement).  Measured (PAIR_MEASURED;
# profiles/r20_pair_instances.txt): direct 0.235 of its bound (C_BOUND = 1, A_BOUND = 8 unchanged: 4 x of margin); f16x3 0.837 on the wide
# kernels, 0.610 on the C = 16 layout -> C_F16 = 1.7; F(2,3) 0.316 -> M_WINO23 = 0.64; F(4,4) 0.325 -> M_WINO44 = 0.65 (below 1: A_W counts
# every tap at the neighbourhood's largest activation).  Never calibrated against another kernel of the project.
SILU_SLOPE = 1.1
PAIR_MEASURED = {"direct": 0.235, "f16x3": 0.837, "wino23": 0.316, "wino44": 0.325}   # largest ratio measured on an MI355X, multiplier at 1
C_F16 = 1.7
M_WINO23 = 0.64
M_WINO44 = 0.65
PAIR_FAMILIES = ("direct", "f16x3", "wino23", "wino44")


def _pair_layers(x, w1, b1, w2, b2, k, d):
    g1 = dict(transposed=False, padding=(k - 1) * d // 2, dilation=d)
    g2 = dict(transposed=False, padding=(k - 1) // 2, dilation=1)
    h, _, A1 = layer_ref(x, w1, b1, g1, pre="silu")
    ref, _, A2 = layer_ref(h, w2, b2, g2, pre="silu", res=np.asarray(x, dtype=np.float64))
    return ref, h, A1, A2, int(np.asarray(w1).shape[1]) * k


def pair_ref(x, w1, b1, w2, b2, k, d):
    """(ref, A1, A2, K) of y = x + c2(silu(c1(silu x) + b1)) + b2 in float64, from layer_ref: A1 / A2 the absolute-value convs of the two layers
    (A2 with the residual |x|), K = C k the terms of either sum."""
    ref, _, A1, A2, K = _pair_layers(x, w1, b1, w2, b2, k, d)
    return ref, A1, A2, K


def _window_max(a, r):
    """max over |t' - t| <= r of a[..., t'] (a >= 0; positions outside the row count as 0)."""
    if r == 0:
        return a
    return F.max_pool1d(F.pad(torch.from_numpy(np.ascontiguousarray(a)), (r, r)), kernel_size=2 * r + 1, stride=1).numpy()


def wino_A(a, w, b, r, res=None):
    """A_W of one layer on the activated input a (see above)."""
    w1 = np.abs(np.asarray(w, dtype=np.float64)).sum(axis=2)            # (O, I)
    A = np.einsum("oi,bit->bot", w1, _window_max(np.abs(np.asarray(a, dtype=np.float64)), r))
    if b is not None:
        A = A + np.abs(np.asarray(b, dtype=np.float64))[None, :, None]
    if res is not None:
        A = A + np.abs(np.asarray(res, dtype=np.float64))
    return A


def pair_bound_parts(family, x, w1, b1, w2, b2, k, d):
    """(ref, fixed, unit): the float64 output, and the family's per-output bound as fixed + multiplier * unit (direct: no multiplier, unit =
    fixed = the bound)."""
    x64 = np.asarray(x, dtype=np.float64)
    ref, h, A1, A2, K = _pair_layers(x, w1, b1, w2, b2, k, d)
    aw1, aw2 = np.abs(np.asarray(w1, dtype=np.float64)), np.abs(np.asarray(w2, dtype=np.float64))
    pad1, pad2 = (k - 1) * d // 2, (k - 1) // 2
    scale = C_BOUND * U * (np.sqrt(K) + A_BOUND)      # bound(A, K) = scale * A

    def through_c2(e1):
        return SILU_SLOPE * conv64(e1, aw2, padding=pad2)

    if family in ("direct", "f16x3"):
        A12 = A2 + through_c2(A1)                     # the composition is linear in (A1, A2)
        if family == "direct":
            return ref, scale * A12, scale * A12
        ones = np.ones((1,) + aw1.shape[1:])
        f1 = 2.0 ** -25 * aw1.sum(axis=(1, 2))[None, :, None] + 2.0 ** -38 * aw1.max() * conv64(np.abs(act64(x64, "silu")), ones, padding=pad1, dilation=d)
        f2 = 2.0 ** -25 * aw2.sum(axis=(1, 2))[None, :, None] + 2.0 ** -38 * aw2.max() * conv64(np.abs(act64(h, "silu")), ones, padding=pad2)
        return ref, scale * A12 + f2 + through_c2(f1), 2.0 ** -22 * A12
    span = {"wino23": 2, "wino44": 4}[family]
    AW1 = wino_A(act64(x64, "silu"), w1, b1, span * d + pad1)
    AW2 = wino_A(act64(h, "silu"), w2, b2, span + pad2, res=x64)
    return ref, np.zeros_like(ref), U * (np.sqrt(K) + A_BOUND) * (AW2 + through_c2(AW1))


def pair_multiplier(family):
    return {"direct": 0.0, "f16x3": C_F16, "wino23": M_WINO23, "wino44": M_WINO44}[family]


def pair_bound(family, x, w1, b1, w2, b2, k, d):
    """The per-output bound of the family's pair kernel."""
    _, fixed, unit = pair_bound_parts(family, x, w1, b1, w2, b2, k, d)
    return fixed + pair_multiplier(family) * unit


def pair_ratio(y, ref, unit):
    """max |y - ref| / unit: what the family multipliers were measured in (direct: <= 1 passes)."""
    return float((np.abs(np.asarray(y, dtype=np.float64) - ref) / unit).max())


def check_pair_per_output(y, ref, bnd, what=""):
    """Every output finite and within its bound."""
    y64 = np.asarray(y, dtype=np.float64)
    assert y64.shape == ref.shape, (what, y64.shape, ref.shape)
    assert np.isfinite(y64).all(), f"{what}: non-finite outputs"
    err = np.abs(y64 - ref)
    bad = err > bnd
    if bad.any():
        i = np.unravel_index(int(np.argmax(err / bnd)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} outputs past the per-output bound; worst at {tuple(int(v) for v in i)}: "
                             f"|d| = {err[i]:.3e}, bound {bnd[i]:.3e} ({err[i] / bnd[i]:.2f} x), ref {ref[i]:.6e}")
