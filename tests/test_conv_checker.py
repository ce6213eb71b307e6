"""CPU: the arbiter of the conv-kernel instance tests (conv_reference.py) has teeth.  Float32 "mutants" of the float64 reference — the errors
a direct-sum conv kernel makes when an index is off — must fail the per-output check that test_gpu_conv_instances.py applies, while the correctly
rounded output passes; and the float64 references themselves equal Conv1d / ConvTranspose1d written out as loops."""
import numpy as np
import pytest

import conv_reference as cr

pytest.importorskip("torch")


def _layer(seed, cin, cout, k, tr=False, u=1, d=1, B=2, T=40):
    rng = np.random.default_rng(seed)
    w = cr.heavy_tailed_weight(rng, cout, cin, k, transposed=tr)
    b = rng.normal(size=cout).astype(np.float32)
    x = cr.unequal_channels(rng, B, cin, T)
    geo = dict(transposed=True, stride=u, padding=(k - u) // 2) if tr else dict(transposed=False, padding=(k - 1) * d // 2, dilation=d)
    ref, _, A = cr.layer_ref(x, w, b, geo, pre="silu")
    return x, w, b, geo, ref, A, cr.terms(cin, k, tr, u)


def _caught(y, ref, A, K):
    with pytest.raises(AssertionError):
        cr.check_per_output(y, ref, A, K, what="mutant")


def test_the_rounded_reference_passes():
    for args in ((1, 40, 24, 7, False, 1, 3), (2, 72, 16, 16, True, 8, 1), (3, 100, 33, 1, False, 1, 1)):
        x, w, b, geo, ref, A, K = _layer(*args)
        cr.check_per_output(ref.astype(np.float32), ref, A, K, what="rounded")


def test_a_tap_dropped_on_an_edge_column_is_caught():
    x, w, b, geo, ref, A, K = _layer(4, 40, 24, 7, d=3)
    w2 = w.copy()
    w2[:, :, 0] = 0.0                    # tap 0 missing ...
    bad, _, _ = cr.layer_ref(x, w2, b, geo, pre="silu")
    y = ref.copy()
    y[:, :, -1] = bad[:, :, -1]          # ... on the last output column only (a halo / crop error)
    _caught(y.astype(np.float32), ref, A, K)


def test_the_last_partial_channel_chunk_dropped_is_caught():
    x, w, b, geo, ref, A, K = _layer(5, 40, 24, 3)     # 40 channels: one whole 32-channel chunk and 8 more
    x2 = x.copy()
    x2[:, 32:, :] = 0.0
    bad, _, _ = cr.layer_ref(x2, w, b, geo, pre="silu")
    _caught(bad.astype(np.float32), ref, A, K)


def test_one_polyphase_phase_shifted_is_caught():
    x, w, b, geo, ref, A, K = _layer(6, 32, 8, 16, tr=True, u=8)
    y = ref.astype(np.float32).copy()
    y[:, :, 3::8] = np.roll(y[:, :, 3::8], 1, axis=2)   # phase 3 of every output channel one sample late
    _caught(y, ref, A, K)


def test_one_low_gain_row_off_by_1e_3_is_caught_where_the_global_bar_is_not():
    x, w, b, geo, ref, A, K = _layer(7, 64, 32, 7, T=200)
    b = np.zeros_like(b)                 # a row whose size is its weights' gain alone
    ref, _, A = cr.layer_ref(x, w, b, geo, pre="silu")
    row = int(np.argmin(np.abs(ref).max(axis=(0, 2))))
    assert np.abs(ref[:, row]).max() < 0.05 * np.abs(ref).max()   # the weights' gains spread over 100 x
    y = ref.copy()
    y[:, row] *= 1.0 + 1e-3
    y = y.astype(np.float32)
    assert np.abs(y - ref).max() <= 2e-5 * max(np.abs(ref).max(), 1.0)   # the old global bar lets it through ...
    _caught(y, ref, A, K)                                              # ... the per-output bound does not


def test_float64_references_equal_the_loop_definitions():
    rng = np.random.default_rng(8)
    for cin, cout, k, d, T in ((3, 4, 3, 1, 9), (5, 2, 5, 2, 17), (1, 3, 1, 1, 6), (4, 4, 4, 1, 11)):
        x = rng.normal(size=(2, cin, T))
        w = rng.normal(size=(cout, cin, k))
        b = rng.normal(size=cout)
        pad = (k - 1) * d // 2
        got = cr.conv64(x, w, padding=pad, dilation=d) + b[None, :, None]
        assert np.allclose(got, cr.conv1d_loops(x, w, b, d, pad), rtol=1e-12, atol=1e-12)
    for cin, cout, k, u, T in ((3, 2, 16, 8, 5), (2, 3, 4, 2, 7), (4, 2, 2, 2, 6), (2, 2, 7, 3, 5), (3, 1, 8, 2, 4)):
        x = rng.normal(size=(2, cin, T))
        w = rng.normal(size=(cin, cout, k))
        b = rng.normal(size=cout)
        pad = (k - u) // 2
        got = cr.conv64(x, w, transposed=True, stride=u, padding=pad) + b[None, :, None]
        assert np.allclose(got, cr.conv_transpose1d_loops(x, w, b, u, pad), rtol=1e-12, atol=1e-12)
    # the absolute-value conv bounds the magnitude of every output
    x = rng.normal(size=(1, 6, 30))
    w = rng.normal(size=(5, 6, 3))
    ref, _, A = cr.layer_ref(x, w, None, dict(transposed=False, padding=1, dilation=1))
    assert (np.abs(ref) <= A * (1 + 1e-12)).all()


def test_impulse_inputs_keep_one_product_per_output():
    T, gap = 300, 31
    x, placed = cr.impulse_input(2, 40, T, [0, T - 1, 127, 128, 255, 256], [0, 7, 8, 31, 32, 39], gap)
    assert sorted(t for _, _, t, _ in placed) == [0, 127, 128, 255, 256, T - 1]
    for bi in range(x.shape[0]):
        ts = sorted(t for b_, _, t, _ in placed if b_ == bi)
        assert all(t2 - t1 > gap for t1, t2 in zip(ts, ts[1:]))
    assert {v for *_, v in placed} <= {1.0, -1.0, 8.0, -(2.0 ** -5), 128.0, -4.0, 2.0 ** -9, -(2.0 ** 11)}
