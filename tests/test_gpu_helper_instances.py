"""GPU: the two helper kernels with the most code between the convs, on their own and instance by instance (fv_aa_snake_forward,
fv_dwconv_ln_forward), against the float64 references and per-output bounds of helper_reference.py (whose teeth test_helper_checker.py shows).

aa_snake_pk_kernel: the 16-byte "vec4" form and the pair form, the three-operand input mean, clamped edge tiles and clamp-free interior tiles,
at every length where the code changes its path (helper_reference.SNAKE_T).  launch_dwconv_ln: the ten dwconv_ln_tile_kernel<K, CMAX, NG>
instances, dwconv_ln_reg_kernel and dwconv_ln_kernel under the default choice, FV_DWLN_NG8, FV_DWLN_RR and FV_OLD_DWLN
(helper_reference.DWLN_SHAPES).  INSTANCES lists every (form, class of shapes); every launch asserts _lib.last_kernel(); every output of every
case is checked.  Arbiters: the float64 bound per output; the bit-for-bit relations between the forms (vec4 == pair, misaligned == aligned,
three operands == the host's float32 mean, a row alone == the row in its batch, FV_DWLN_RR == default, a column far from the end == the same
column of a shorter run, C = 1 -> ln_b); NaN around every input (a NaN in y is a read outside the rows) and sentinels around every output.
test_every_instance_ran (last in the module) prints the table — instance, cases, largest |y - ref| / bound — and fails on any row that no case
reached: run the module as a whole."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import helper_reference as hr
from conftest import load_golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
GUARD = 64          # floats of NaN / sentinel on either side of a tensor (a multiple of 4: the tensor keeps its 16-byte alignment)
SENTINEL = 12345.678


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
def _snake_class(T):
    return ("short" if T in hr.SNAKE_T_SHORT else "seam" if T in hr.SNAKE_T_SEAM else "interior" if T in hr.SNAKE_T_INTERIOR else "many")


def _has_vec4(T):
    return T % 4 == 0 and T >= 8


def _instances():
    rows = []
    for cls, Ts in (("short", hr.SNAKE_T_SHORT), ("seam", hr.SNAKE_T_SEAM), ("interior", hr.SNAKE_T_INTERIOR), ("many", hr.SNAKE_T_MANY)):
        assert any(_has_vec4(T) for T in Ts) and any(not _has_vec4(T) for T in Ts)
        rows += [("aa_snake<vec4>", cls), ("aa_snake<pair>", cls), ("aa_snake<pair> sum3", cls)]
    for k in (1, 7):
        for cmax, ng in ((256, 8), (512, 16), (512, 8), (1024, 16), (1024, 8)):
            rows.append((f"dwconv_ln_tile<k={k} cmax={cmax} ng={ng}>", ""))
    rows += [(f"dwconv_ln_reg<k={k}>", "") for k in (1, 3, 7, 9)] + [(f"dwconv_ln<k={k}>", "") for k in (1, 3, 7, 9)]
    return rows


INSTANCES = _instances()
_SEEN = {}     # row -> cases that ran it
_RATIO = {}    # row -> largest |y - ref| / bound


def _record(name, cls="", ratio=None):
    key = (name, cls)
    _SEEN[key] = _SEEN.get(key, 0) + 1
    if ratio is not None:
        _RATIO[key] = max(_RATIO.get(key, 0.0), ratio)


def _dev():
    assert torch.cuda.is_available(), "GPU test on a box without a GPU"
    return torch.device("cuda:0")


@contextlib.contextmanager
def _knobs(**env):
    """Set FV_* variables (None = unset: the three FV_DWLN_* / FV_OLD_DWLN knobs are presence knobs) and re-read the library's knobs; restore both."""
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


_ALL_OFF = dict(FV_AA_VEC4=None, FV_DWLN_NG8=None, FV_DWLN_RR=None, FV_OLD_DWLN=None)


# ---- guarded tensors -------------------------------------------------------------------------------------------------------------------------
def _guarded_in(a, shift=0):
    """The array as a contiguous view inside a NaN-filled allocation, GUARD (+ shift) floats from its start: a read outside the tensor brings NaN."""
    buf = torch.full((a.size + 2 * GUARD + shift,), float("nan"), dtype=torch.float32, device=_dev())
    view = buf[GUARD + shift:GUARD + shift + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * (GUARD + shift)
    return view


def _guarded_out(shape, shift=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=torch.float32, device=_dev())
    return buf, buf[GUARD + shift:GUARD + shift + n].view(*shape)


def _fetch(buf, out, what):
    """The output as numpy, after checking that the sentinels before and after it survived."""
    torch.cuda.synchronize()
    flat = buf.cpu().numpy()
    n = out.numel()
    lo = (out.data_ptr() - buf.data_ptr()) // 4
    assert np.all(flat[:lo] == F32(SENTINEL)), f"{what}: a store in front of the output"
    assert np.all(flat[lo + n:] == F32(SENTINEL)), f"{what}: a store behind the output"
    return flat[lo:lo + n].reshape(tuple(out.shape)).copy()


def _vec(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


# ---- snake -----------------------------------------------------------------------------------------------------------------------------------
def _snake_run(x, al, ib, up, dn, x2=None, x3=None, shift=0):
    """One launch on guarded tensors -> (y, kernel name).  shift = 1: every tensor one float off its 16-byte alignment."""
    from vocoder_amd import _lib
    from vocoder_amd.engine import aa_snake
    xs = [None if a is None else _guarded_in(a, shift) for a in (x, x2, x3)]
    buf, out = _guarded_out(x.shape, shift)
    if shift:
        assert xs[0].data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    else:
        assert xs[0].data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    y = aa_snake(xs[0], _vec(al), _vec(ib), _vec(up), _vec(dn), x2=xs[1], x3=xs[2], out=out)
    assert y.data_ptr() == out.data_ptr()
    name = _lib.last_kernel()
    return _fetch(buf, out, name), name


def _same(a, b, what):
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} outputs differ, first at {tuple(int(v) for v in bad[0])}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}")


@pytest.mark.parametrize("T", hr.SNAKE_T)
def test_snake_forms_against_float64_and_each_other(T):
    cls = _snake_class(T)
    lines = []
    for family in hr.SNAKE_FAMILIES:
        x, _, _, al, ib, up, dn = hr.snake_case(family, T)
        ref, bound = hr.snake_ref(x, al, ib, up, dn)
        what = f"snake {family} T={T}"
        with _knobs(**_ALL_OFF):
            y_def, n_def = _snake_run(x, al, ib, up, dn)
        assert n_def == ("aa_snake<vec4>" if _has_vec4(T) else "aa_snake<pair>"), (T, n_def)   # vec4 exactly where T % 4 == 0 and T >= 8
        r_def = hr.check_per_output(y_def, ref, bound, f"{what} {n_def}")
        _record(n_def, cls, r_def)
        with _knobs(**dict(_ALL_OFF, FV_AA_VEC4="0")):
            y_pair, n_pair = _snake_run(x, al, ib, up, dn)
        assert n_pair == "aa_snake<pair>", n_pair
        r_pair = hr.check_per_output(y_pair, ref, bound, f"{what} FV_AA_VEC4=0 {n_pair}")
        _record(n_pair, cls, r_pair)
        _same(y_def, y_pair, f"{what}: {n_def} vs the pair form")
        with _knobs(**_ALL_OFF):
            if T % 4 == 0:   # every row still starts at a multiple of 16 bytes from the base: only the base is off
                y_off, n_off = _snake_run(x, al, ib, up, dn, shift=1)
                assert n_off == "aa_snake<pair>", n_off
                _record(n_off, cls, hr.check_per_output(y_off, ref, bound, f"{what} misaligned {n_off}"))
                _same(y_off, y_def, f"{what}: misaligned vs aligned")
            # a row alone == the row in its batch (its own channel's parameters)
            for b, c in ((0, 0), (hr.SNAKE_B - 1, hr.SNAKE_C - 1)):
                y_row, n_row = _snake_run(x[b:b + 1, c:c + 1], al[c:c + 1], ib[c:c + 1], up, dn)
                assert n_row == n_def, (n_row, n_def)
                _record(n_row, cls)
                _same(y_row[0, 0], y_def[b, c], f"{what}: row ({b}, {c}) alone vs in the batch")
            # three operands: the float64 bound of their own, and the one-operand run on the host's float32 mean bit for bit
            x1, x2, x3, al3, ib3, up3, dn3 = hr.snake_case(family, T, operands=3)
            ref3, bound3 = hr.snake_ref(x1, al3, ib3, up3, dn3, x2, x3)
            y3, n3 = _snake_run(x1, al3, ib3, up3, dn3, x2, x3)
            assert n3 == "aa_snake<pair> sum3", n3
            r3 = hr.check_per_output(y3, ref3, bound3, f"{what} {n3}")
            _record(n3, cls, r3)
            y_mean, n_mean = _snake_run(hr.host_mean3(x1, x2, x3), al3, ib3, up3, dn3)
            _record(n_mean, cls)
            _same(y3, y_mean, f"{what}: three operands vs the host mean ({n_mean})")
        lines.append(f"{family} {n_def.split('<')[1][:-1]} {r_def:.3f} / pair {r_pair:.3f} / sum3 {r3:.3f}")
    print(f"T = {T} ({cls}): largest |y - ref| / bound: " + "; ".join(lines))


def test_snake_golden_activation_through_the_op():
    g = load_golden("activation1d.npz")
    al = np.exp(g["alpha"].astype(np.float64)).astype(F32)
    ib = (1.0 / (np.exp(g["beta"].astype(np.float64)) + 1e-9)).astype(F32)
    ref, bound = hr.snake_ref(g["x"], al, ib, g["taps"], g["taps"])
    with _knobs(**_ALL_OFF):
        y, name = _snake_run(g["x"], al, ib, g["taps"], g["taps"])
    assert name == "aa_snake<pair>", name     # T = 37
    r = hr.check_per_output(y, ref, bound, f"golden activation {name}")
    _record(name, "short", r)     # both row ends inside one tile
    print(f"golden activation1d through {name}: largest |y - ref| / bound {r:.3f}, max |y - golden y| {np.abs(y - g['y']).max():.2e}")
    assert np.abs(y - g["y"]).max() <= 2e-6


# ---- depthwise conv + LayerNorm ----------------------------------------------------------------------------------------------------------------
def _dwln_expected(C, T, k, ng8, old):
    """The kernel launch_dwconv_ln must take (small_kernels.hip: dwln_form), from the shape and the knobs; k = 0: LayerNorm alone."""
    kk = k if k else 1
    if kk in (1, 7) and not old and C <= 1024:
        cmax = 256 if C <= 256 else 512 if C <= 512 else 1024
        return f"dwconv_ln_tile<k={kk} cmax={cmax} ng={8 if (cmax == 256 or ng8) else 16}>"
    return f"dwconv_ln_reg<k={kk}>" if C <= 1024 else f"dwconv_ln<k={kk}>"


def _dwln_run(xd, wd, eps, shape):
    """One launch on a guarded input (already on the device) -> (y, kernel name); wd = the four parameter tensors."""
    from vocoder_amd import _lib
    from vocoder_amd.engine import dwconv_layernorm
    buf, out = _guarded_out(shape)
    y = dwconv_layernorm(xd, wd[0], wd[1], wd[2], wd[3], eps=eps, out=out)
    assert y.data_ptr() == out.data_ptr()
    name = _lib.last_kernel()
    return _fetch(buf, out, name), name


DWLN_SETTINGS = [("default", {}), ("ng8", dict(FV_DWLN_NG8="1")), ("rr", dict(FV_DWLN_RR="1")), ("old", dict(FV_OLD_DWLN="1"))]


@pytest.mark.parametrize("B,C,T", hr.DWLN_SHAPES, ids=[f"B{b}-C{c}-T{t}" for b, c, t in hr.DWLN_SHAPES])
def test_dwconv_ln_instances_against_float64_and_each_other(B, C, T):
    ks = [0, 7] + ([3, 9] if (B, C, T) in hr.DWLN_ODD_K_SHAPES else [])
    worst = {}
    for k in ks:
        for family in hr.DWLN_FAMILIES:
            x, dw_w, dw_b, ln_w, ln_b = hr.dwln_case(family, B, C, T, k)
            xd = _guarded_in(x)
            wd = [_vec(dw_w), _vec(dw_b), _vec(ln_w), _vec(ln_b)]
            for eps in hr.DWLN_EPS:
                ref, bound = hr.dwln_ref(x, dw_w, dw_b, ln_w, ln_b, eps)
                what = f"dwln {family} {(B, C, T)} k={k} eps={eps}"
                ys = {}
                for tag, env in DWLN_SETTINGS:
                    with _knobs(**dict(_ALL_OFF, **env)):
                        y, name = _dwln_run(xd, wd, eps, x.shape)
                    assert name == _dwln_expected(C, T, k, tag == "ng8", tag == "old"), (tag, name)
                    r = hr.check_per_output(y, ref, bound, f"{what} {tag} {name}")
                    _record(name, "", r)
                    worst[name] = max(worst.get(name, 0.0), r)
                    ys[tag] = (y, name)
                    if C == 1:   # d = h - h = 0: the output is ln_b, whatever h and eps are
                        _same(y, np.broadcast_to(ln_b[None, :, None], y.shape), f"{what} {tag}: C = 1 must give ln_b")
                _same(ys["rr"][0], ys["default"][0], f"{what}: FV_DWLN_RR vs the default")
                if ys["ng8"][1] == ys["default"][1]:
                    _same(ys["ng8"][0], ys["default"][0], f"{what}: the same instance under FV_DWLN_NG8")
                if eps != hr.DWLN_EPS[0]:
                    continue
                for tag, env in (DWLN_SETTINGS[0], DWLN_SETTINGS[3]):
                    with _knobs(**dict(_ALL_OFF, **env)):
                        # a row alone == the row in its batch
                        for b in sorted({0, B - 1}):
                            yb, nb = _dwln_run(_guarded_in(x[b:b + 1]), wd, eps, (1, C, T))
                            assert nb == ys[tag][1], (nb, ys[tag][1])
                            _record(nb)
                            _same(yb[0], ys[tag][0][b], f"{what} {tag}: item {b} alone vs in the batch")
                        # a column at least 4 frames (the widest halo here: k = 9) from the end == the same column of a shorter run
                        if T >= 8:
                            Tc = T - 3
                            yc, nc = _dwln_run(_guarded_in(x[:, :, :Tc]), wd, eps, (B, C, Tc))
                            assert nc == ys[tag][1], (nc, ys[tag][1])
                            _record(nc)
                            _same(yc[:, :, :Tc - 4], ys[tag][0][:, :, :Tc - 4], f"{what} {tag}: columns of the run cut to {Tc} frames")
    print(f"{(B, C, T)}: largest |y - ref| / bound: " + ", ".join(f"{n} {r:.3f}" for n, r in sorted(worst.items())))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def _refused(call, args, named, out, what):
    from vocoder_amd import _lib
    L = _lib.lib()
    before = out.clone()
    st = call(*args)
    torch.cuda.synchronize()
    msg = L.fv_last_error().decode()
    assert st == _lib.FV_ERR_INVALID, (what, st, msg)
    assert named in msg, (what, named, msg)
    assert torch.equal(out, before), f"{what}: the output was written"


def test_snake_refusals_name_the_argument_and_write_nothing():
    from vocoder_amd import _lib
    L = _lib.lib()
    B, C, T = 2, 3, 16
    dev = _dev()
    x, x2, x3 = (torch.randn(B, C, T, device=dev) for _ in range(3))
    big = torch.full((2 * B * C * T,), SENTINEL, device=dev)
    y = big[:B * C * T].view(B, C, T)
    al, ib, up, dn = torch.ones(C, device=dev), torch.ones(C, device=dev), torch.ones(12, device=dev), torch.ones(12, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()

    def args(x_=x, x2_=None, x3_=None, y_=y, al_=al, ib_=ib, up_=up, dn_=dn, B_=B, C_=C, T_=T):
        return (p(x_), p(x2_), p(x3_), p(y_) if isinstance(y_, torch.Tensor) else y_, p(al_), p(ib_), p(up_), p(dn_), B_, C_, T_, stream)

    f = L.fv_aa_snake_forward
    assert f(*args()) == 0
    torch.cuda.synchronize()
    big.fill_(SENTINEL)
    for kw, named in ((dict(x_=None), "d_x"), (dict(y_=None), "d_y"), (dict(al_=None), "d_alpha"), (dict(ib_=None), "d_inv_beta"),
                      (dict(up_=None), "d_up_taps"), (dict(dn_=None), "d_down_taps"), (dict(x2_=x2), "d_x3"), (dict(x3_=x3), "d_x2"),
                      (dict(C_=0), "channels"), (dict(C_=-3), "channels"), (dict(T_=-1), "T = "), (dict(T_=2 ** 31), "T = "), (dict(T_=2 ** 40), "T = "),
                      (dict(B_=-1), "batch"), (dict(B_=2 ** 20, C_=2 ** 20, T_=4096), "workgroups")):
        _refused(f, args(**kw), named, big, f"aa_snake {sorted(kw)}")
    # d_y overlapping an input: the input itself, an input that starts inside y, y starting inside the last input
    xin = big[4:4 + B * C * T].view(B, C, T)
    tail = big[B * C * T - 4:2 * B * C * T - 4].view(B, C, T)
    for kw, named in ((dict(x_=y), "d_x"), (dict(x_=xin), "d_x"), (dict(x_=tail), "d_x"), (dict(x2_=x2, x3_=tail), "d_x3"),
                      (dict(x2_=xin, x3_=x3), "d_x2"), (dict(al_=big[1:1 + C]), "d_alpha"), (dict(dn_=big[8:20]), "d_down_taps")):
        _refused(f, args(**kw), named, big, f"aa_snake overlap {sorted(kw)}")
        assert "overlaps" in L.fv_last_error().decode()
    # no-ops: nothing is read or written, even through NULL
    assert f(*args(B_=0)) == 0 and f(*args(T_=0)) == 0 and f(*args(x_=None, y_=None, T_=0)) == 0
    torch.cuda.synchronize()
    assert bool((big == SENTINEL).all())


def test_dwconv_ln_refusals_name_the_argument_and_write_nothing():
    from vocoder_amd import _lib
    L = _lib.lib()
    B, C, T, k = 2, 5, 16, 7
    dev = _dev()
    x = torch.randn(B, C, T, device=dev)
    big = torch.full((2 * B * C * T,), SENTINEL, device=dev)
    y = big[:B * C * T].view(B, C, T)
    w, b, g, beta = torch.randn(C, k, device=dev), torch.randn(C, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()

    def args(x_=x, w_=w, b_=b, g_=g, beta_=beta, y_=y, B_=B, C_=C, T_=T, k_=k, eps_=1e-6):
        return (p(x_), p(w_), p(b_), p(g_), p(beta_), p(y_), B_, C_, T_, k_, eps_, stream)

    f = L.fv_dwconv_ln_forward
    assert f(*args()) == 0 and f(*args(b_=None)) == 0 and f(*args(w_=None, b_=None, k_=1)) == 0
    torch.cuda.synchronize()
    big.fill_(SENTINEL)
    for kw, named in ((dict(x_=None), "d_x"), (dict(g_=None), "d_ln_weight"), (dict(beta_=None), "d_ln_bias"), (dict(y_=None), "d_y"),
                      (dict(C_=0), "channels"), (dict(T_=-1), "T = "), (dict(T_=2 ** 31), "T = "), (dict(B_=-1), "batch"),
                      (dict(k_=4), "kernel_size"), (dict(k_=0), "kernel_size"), (dict(k_=-7), "kernel_size"),
                      (dict(w_=None, b_=None, k_=7), "kernel_size"), (dict(w_=None, k_=1), "d_dw_bias"), (dict(eps_=-1.0), "eps"),
                      (dict(eps_=float("nan")), "eps")):
        _refused(f, args(**kw), named, big, f"dwconv_ln {sorted(kw)}")
    xin = big[4:4 + B * C * T].view(B, C, T)
    tail = big[B * C * T - 4:2 * B * C * T - 4].view(B, C, T)
    for kw, named in ((dict(x_=y), "d_x"), (dict(x_=xin), "d_x"), (dict(x_=tail), "d_x"), (dict(w_=big[0:C * k]), "d_dw_weight"),
                      (dict(b_=big[3:3 + C]), "d_dw_bias"), (dict(g_=big[9:9 + C]), "d_ln_weight"), (dict(beta_=big[B * C * T - 1:B * C * T - 1 + C]), "d_ln_bias")):
        _refused(f, args(**kw), named, big, f"dwconv_ln overlap {sorted(kw)}")
        assert "overlaps" in L.fv_last_error().decode()
    assert f(*args(B_=0)) == 0 and f(*args(T_=0)) == 0 and f(*args(x_=None, y_=None, T_=0)) == 0
    torch.cuda.synchronize()
    assert bool((big == SENTINEL).all())


def test_wrappers_pass_a_contiguous_view_at_its_own_address():
    """engine.aa_snake / dwconv_layernorm hand the kernel data_ptr() of the tensor they are given: a contiguous view one float into an allocation
    reaches the kernel misaligned (the pair form), and a non-contiguous operand is copied, not mis-strided."""
    from vocoder_amd import _lib
    from vocoder_amd.engine import aa_snake, dwconv_layernorm
    x, _, _, al, ib, up, dn = hr.snake_case("synthetic", 1024)
    ref, bound = hr.snake_ref(x, al, ib, up, dn)
    base = torch.zeros(x.size + 1, device=_dev())
    xo = base[1:].view(*x.shape)
    xo.copy_(torch.from_numpy(x))
    with _knobs(**_ALL_OFF):
        y = aa_snake(xo, _vec(al), _vec(ib), _vec(up), _vec(dn))
        assert _lib.last_kernel() == "aa_snake<pair>"          # x is 4 bytes off: no 16-byte accesses
        _record("aa_snake<pair>", "seam", hr.check_per_output(y.cpu().numpy(), ref, bound, "misaligned x, fresh out"))
        xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(_dev()).transpose(1, 2)    # (B, C, T), strides of (B, T, C)
        assert not xt.is_contiguous()
        y2 = aa_snake(xt, _vec(al), _vec(ib), _vec(up), _vec(dn))
        assert _lib.last_kernel() == "aa_snake<vec4>"
        _record("aa_snake<vec4>", "seam", hr.check_per_output(y2.cpu().numpy(), ref, bound, "transposed x"))
        _same(y.cpu().numpy(), y2.cpu().numpy(), "misaligned vs copied operand")
        xc, w, b, g, beta = hr.dwln_case("unequal", 2, 100, 31, 7)
        refd, boundd = hr.dwln_ref(xc, w, b, g, beta, 1e-6)
        yd = dwconv_layernorm(_vec(xc), _vec(w.reshape(100, 1, 7)), _vec(b), _vec(g), _vec(beta))     # the Conv1d weight layout (C, 1, k)
        name = _lib.last_kernel()
        assert name == "dwconv_ln_tile<k=7 cmax=256 ng=8>", name
        _record(name, "", hr.check_per_output(yd.cpu().numpy(), refd, boundd, "dwconv_layernorm (C, 1, k) weight"))


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------------
def test_every_instance_ran():
    """Every row of INSTANCES ran at least once in this module (the other tests record what they launched); the table goes to profiles/LOG.md."""
    missing = [row for row in INSTANCES if _SEEN.get(row, 0) == 0]
    print(f"\n{'instance':40s} {'lengths':9s} {'cases':>6s} {'largest ratio':>14s}")
    for row in INSTANCES:
        n = _SEEN.get(row, 0)
        print(f"{row[0]:40s} {row[1]:9s} {n:6d} {_RATIO.get(row, float('nan')):14.3f}{'' if n else '   NOT RUN'}")
    extra = sorted(k for k in _SEEN if k not in INSTANCES)
    assert not extra, f"launched instances missing from the table: {extra}"
    assert not missing, f"{len(missing)} instances never ran: {missing}"
    over = {row: r for row, r in _RATIO.items() if not r <= 1.0}
    assert not over, over
