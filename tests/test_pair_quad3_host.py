"""CPU: the arithmetic pair_wino4_impl.h implements for the wide k = 3 ResBlock pairs — ONE Winograd F(4,3) tap group on the dilated quad lattice,
points 0, +-1, +-2, inf, six planes and six products per output quad and (c_out, c_in) — restated in numpy (float64) against a float64 direct conv,
and the weight packer pack_pair_wino4 (conv_pack.hip, through fv_pair_wino4_pack) against a float64 transform, fragment order included.  Exact in
real arithmetic: an indexing or sign error in the scheme cannot hide behind a tolerance."""
import ctypes

import numpy as np
import pytest


def transformed_weights43(w):
    """(C_out, C_in, 6): U = G w of the taps (g0, g1, g2), in the kernel's plane order."""
    g0, g1, g2 = (w[..., i] for i in range(3))
    return np.stack([g0 / 4, -(g0 + g1 + g2) / 6, -(g0 - g1 + g2) / 6, g0 / 24 + g1 / 12 + g2 / 6, g0 / 24 - g1 / 12 + g2 / 6, g2], axis=-1)


def quad3_conv1d(x, w, d):
    """The kernel's scheme: quad column n = q d + r <-> u0 = 4 d q + r, X_j[n] = x'[u0 + j d], x4 / x5 = X0 / X1 at n + d."""
    B, C, T = x.shape
    assert w.shape[-1] == 3
    pad = d
    nq = -(-T // (4 * d))                      # blocks of 4 d samples
    NP = nq * d                                # quad columns
    xp = np.zeros((B, C, 4 * d * (nq + 1) + 4 * d + pad))
    xp[..., pad:pad + T] = x                   # x'[tau] = x[tau - pad]
    n = np.arange(NP + d)
    t0 = 4 * d * (n // d) + n % d
    x0, x1, x2, x3 = (xp[..., t0 + j * d] for j in range(4))
    x4, x5 = np.roll(x0, -d, axis=-1), np.roll(x1, -d, axis=-1)
    e4, o4, e1, o1 = x4 - 4 * x2, x3 - 4 * x1, x4 - x2, x3 - x1
    V = [4 * x0 - 5 * x2 + x4, e4 + o4, e4 - o4, e1 + 2 * o1, e1 - 2 * o1, 4 * x1 - 5 * x3 + x5]
    U = transformed_weights43(w)
    m = [np.einsum("oc,bcn->bon", U[..., p], V[p][..., :NP]) for p in range(6)]
    s1, d1, s2, d2 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    y = np.zeros((B, w.shape[0], 4 * d * nq))
    tt = 4 * d * (np.arange(NP) // d) + np.arange(NP) % d
    y[..., tt] = (m[0] + s1) + s2
    y[..., tt + d] = d1 + 2 * d2
    y[..., tt + 2 * d] = s1 + 4 * s2
    y[..., tt + 3 * d] = (d1 + 8 * d2) + m[5]
    return y[..., :T]


@pytest.mark.parametrize("d,T", [(1, 1), (1, 17), (1, 128), (3, 2), (3, 50), (3, 121), (5, 9), (5, 40), (5, 333)])
def test_one_group_quad_lattice_equals_the_direct_conv(d, T):
    rng = np.random.default_rng(100 * d + T)
    x = rng.normal(size=(2, 6, T)).astype(np.float32).astype(np.float64)
    w = rng.normal(size=(5, 6, 3)).astype(np.float32).astype(np.float64)
    y = quad3_conv1d(x, w, d)
    xp = np.pad(x, ((0, 0), (0, 0), (d, d)))
    direct = sum(np.einsum("oc,bct->bot", w[..., j], xp[..., j * d:j * d + T]) for j in range(3))
    assert y.shape == direct.shape
    assert np.abs(y - direct).max() <= 1e-10   # exact in real arithmetic; the transform constants reach 8


def test_the_bias_plane():
    """m1's coefficient is 1 in all four outputs (and no other plane's is): the bias rides in plane 1."""
    At = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)
    assert [p for p in range(6) if (At[:, p] == 1).all()] == [1]


def test_products_per_output_quad():
    assert transformed_weights43(np.zeros((1, 1, 3))).shape[-1] == 6   # against 8 for two F(2,3) pairs and 12 for the direct sum


@pytest.mark.parametrize("C", [64, 128])
def test_packed_weights_against_a_float64_transform(C):
    """fv_pair_wino4_pack: float4 [(m_tile * C / 8 + chunk) * 6 + plane] * 64 + lane, component pp = U[32 m_tile + (lane & 31)][8 chunk + 2 pp +
    (lane >> 5)][plane] — the A fragment of v_mfma_f32_32x32x2_f32 — then 8 zero fragments (the kernel's weight ring runs past the end).  Every value is
    the float64 transform rounded once to float32."""
    from vocoder_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(C)
    w = (rng.normal(size=(C, C, 3)) * np.exp(rng.uniform(-3, 3, size=(C, C, 1)))).astype(np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    n = int(L.fv_pair_wino4_pack(w.ctypes.data_as(fp), C, None, 0))
    frags = (C // 32) * (C // 8) * 6
    assert n == (frags + 8) * 64 * 4
    out = np.full(n, np.nan, dtype=np.float32)
    assert int(L.fv_pair_wino4_pack(w.ctypes.data_as(fp), C, out.ctypes.data_as(fp), n)) == n
    assert (out[frags * 256:] == 0).all()
    packed = out[:frags * 256].reshape(C // 32, C // 8, 6, 64, 4)
    U = transformed_weights43(w.astype(np.float64))
    mt, ch, pl, lane, pp = np.meshgrid(np.arange(C // 32), np.arange(C // 8), np.arange(6), np.arange(64), np.arange(4), indexing="ij")
    want = U[32 * mt + (lane & 31), 8 * ch + 2 * pp + (lane >> 5), pl]
    assert (np.abs(packed.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-45).all()   # one rounding to float32
    # plane 0 and plane 5 are exact in float32: g0 / 4 and g2
    assert np.array_equal(packed[:, :, 0], (want[:, :, 0]).astype(np.float32)) and np.array_equal(packed[:, :, 5], want[:, :, 5].astype(np.float32))
    assert L.fv_pair_wino4_pack(w.ctypes.data_as(fp), 32, None, 0) == 0       # no instance at that width


def test_tile_widths():
    """PQ3Geom::TT: 32 (C = 128) or 64 (C = 64) quad columns in whole blocks of 4 d samples, less c2's two halo samples."""
    from vocoder_amd import _lib
    L = _lib.lib()
    got = {(C, d): int(L.fv_pair_wino4_tile(C, d)) for C in (64, 128) for d in (1, 3, 5)}
    assert got == {(64, 1): 254, (64, 3): 250, (64, 5): 238, (128, 1): 126, (128, 3): 118, (128, 5): 118}
    assert L.fv_pair_wino4_tile(32, 1) == 0 and L.fv_pair_wino4_tile(64, 2) == 0
