"""GPU: the refusals the layer streams and pools share (fv_wnstream_*, fv_cnxstream_*, fv_wnpool_*, fv_cnxpool_*), called through ctypes
with one bad argument at a time.  The Python owners catch most of them before the library sees the call, so only a direct call pins the
library's own words: every expected string is written out here as the sources format it, and the status is compared too.  Every refusal
is made before anything is enqueued, and the counters are afterwards what they were.  The encoders are the smallest that hold a stream;
``max_chunk`` is 4 everywhere.
"""
import ctypes

import pytest
import torch

from vocoder_amd import _lib
from vocoder_amd.modules.encoders import convnext, posterior_encoder
from vocoder_amd.modules.encoders.convnext import ConvNeXtEncoder
from vocoder_amd.modules.encoders.posterior_encoder import PosteriorEncoder

pytestmark = pytest.mark.gpu

INVALID, STATE = _lib.FV_ERR_INVALID, _lib.FV_ERR_STATE
MAX_CHUNK = 4


def encoder(kind):
    torch.manual_seed(0)
    if kind == "cnx":
        m = ConvNeXtEncoder(input_channels=4, depths=(1,), dims=(8,)).eval().cuda()
        m.batch_invariant = True
        return m
    return PosteriorEncoder(in_channels=4, out_channels=4, hidden_channels=8, n_layers=2).eval().cuda()


# kind -> (the entries' prefix, the output pointer's name, the output pointers that follow the first one, schedule)
KINDS = {
    "cnx": ("fv_cnx", "d_y", (), convnext.schedule),
    "wn": ("fv_wn", "d_z", (None, None), posterior_encoder.schedule),
}


def refused(L, status, want_status, want_text):
    assert status == want_status
    assert L.fv_last_error().decode() == want_text


@pytest.mark.parametrize("kind", list(KINDS))
def test_stream_refusals(kind):
    prefix, out_name, rest, schedule = KINDS[kind]
    L, m = _lib.lib(), encoder(kind)
    owner = m.layer_stream(1, MAX_CHUNK) if kind == "cnx" else m.stream(1, MAX_CHUNK)
    h, R = owner._h, owner.lookahead_frames
    entry = lambda name: getattr(L, f"{prefix}stream_{name}")      # noqa: E731
    push_fn, flush_fn, reset_fn = f"{prefix}stream_push", f"{prefix}stream_flush", f"{prefix}stream_reset"
    x = torch.randn(1, 4, MAX_CHUNK + 1, device="cuda")
    y = torch.empty(1, owner.out_channels, 2 * MAX_CHUNK, device="cuda")
    got = ctypes.c_int64(-7)
    run = int(torch.cuda.current_stream().cuda_stream)

    def push(d_x, xb, xr, c, d_y, yr):
        return entry("push")(h, d_x, xb, xr, c, d_y, *rest, yr, ctypes.byref(got), run)

    def flush(d_y, yr):
        return entry("flush")(h, d_y, *rest, yr, ctypes.byref(got), run)

    xp, yp, xb, xr = x.data_ptr(), y.data_ptr(), x.stride(0), x.stride(1)
    # a flushed stream (an empty utterance: the flush emits nothing)
    assert flush(None, 1) == 0 and got.value == 0
    refused(L, push(xp, xb, xr, 1, yp, 8), STATE, f"{push_fn}: the stream was flushed at 0 frames: {reset_fn} starts the next utterance")
    refused(L, flush(yp, 8), STATE, f"{flush_fn}: the stream was flushed at 0 frames: {reset_fn} starts the next utterance")
    assert entry("pending")(h) == 0
    assert entry("reset")(h) == 0
    # the chunk
    refused(L, push(xp, xb, xr, 5, yp, 8), INVALID, f"{push_fn}: c = 5 must lie in [0, max_chunk = 4]")
    refused(L, push(xp, xb, xr, -1, yp, 8), INVALID, f"{push_fn}: c = -1 must lie in [0, max_chunk = 4]")
    refused(L, push(None, xb, xr, 1, yp, 8), INVALID, f"{push_fn}: null d_x with c = 1")
    refused(L, push(xp, 8, 1, 2, yp, 8), INVALID,
            f"{push_fn}: x_row_stride = 1 (the stride between channels) is shorter than a chunk of c = 2 frames, or x_batch_stride = 8 is negative")
    refused(L, push(xp, -1, xr, 2, yp, 8), INVALID,
            f"{push_fn}: x_row_stride = {xr} (the stride between channels) is shorter than a chunk of c = 2 frames, or x_batch_stride = -1 is "
            "negative")
    if kind == "wn":      # the posterior stream's own refusal sits after the chunk's range and before the chunk's pointer
        pf = entry("push")
        refused(L, pf(h, None, xb, xr, 1, yp, yp, None, 8, ctypes.byref(got), run), INVALID,
                f"{push_fn}: d_mean must be NULL in vqvae mode (posterior_encoder.py:159-160 returns one tensor)")
        refused(L, pf(h, None, xb, xr, 5, yp, None, yp, 8, ctypes.byref(got), run), INVALID, f"{push_fn}: c = 5 must lie in [0, max_chunk = 4]")
    assert entry("pending")(h) == 0 and got.value == 0
    # a valid push of 4 frames, then the refusals of a call that emits
    plan = schedule([MAX_CHUNK], R)
    assert plan == [(0, 0), (0, 4)]        # R >= 4: the push emits nothing, the flush all 4
    assert push(xp, xb, xr, MAX_CHUNK, None, 1) == 0 and got.value == plan[0][1] - plan[0][0]
    assert entry("pending")(h) == 4
    refused(L, flush(None, 8), INVALID, f"{flush_fn}: null {out_name} for the 4 frames this call emits")
    refused(L, flush(yp, 3), INVALID, f"{flush_fn}: y_row_stride = 3 is shorter than the 4 frames this call emits")
    if R < 2 * MAX_CHUNK:      # a push that emits: N = 8, E' = 8 - R
        k = 2 * MAX_CHUNK - R
        refused(L, push(xp, xb, xr, MAX_CHUNK, None, 8), INVALID, f"{push_fn}: null {out_name} for the {k} frames this call emits")
        refused(L, push(xp, xb, xr, MAX_CHUNK, yp, k - 1), INVALID,
                f"{push_fn}: y_row_stride = {k - 1} is shorter than the {k} frames this call emits")
    assert entry("pending")(h) == 4 and got.value == 0
    assert flush(yp, 8) == 0 and got.value == plan[1][1] - plan[1][0]
    assert entry("pending")(h) == 0
    refused(L, push(xp, xb, xr, 0, None, 1), STATE, f"{push_fn}: the stream was flushed at 4 frames: {reset_fn} starts the next utterance")
    torch.cuda.synchronize()
    # the 4 frames are the whole-utterance forward's
    assert torch.equal(y[:, :, :4], m(x[:, :, :4].contiguous()))
    owner.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_pool_refusals(kind):
    prefix, out_name, rest, schedule = KINDS[kind]
    L, m = _lib.lib(), encoder(kind)
    owner = m.layer_pool(2, MAX_CHUNK) if kind == "cnx" else m.pool(2, MAX_CHUNK)
    h, R = owner._h, owner.lookahead_frames
    entry = lambda name: getattr(L, f"{prefix}pool_{name}")      # noqa: E731
    fn, reset_fn = f"{prefix}pool_step", f"{prefix}pool_reset"
    x = torch.randn(2, 4, MAX_CHUNK + 1, device="cuda")
    y = torch.empty(2, owner.out_channels, MAX_CHUNK, device="cuda")
    got = (ctypes.c_int64 * 2)(-7, -7)
    run = int(torch.cuda.current_stream().cuda_stream)
    xp, yp, xi, xr = x.data_ptr(), y.data_ptr(), x.stride(0), x.stride(1)

    def step(items, d_x, item_stride, row_stride, d_y, cols):
        arr = (_lib.WavPoolItem * len(items))(*[_lib.WavPoolItem(*it) for it in items])
        return entry("step")(h, arr, len(items), d_x, item_stride, row_stride, d_y, *rest, cols, got, run)

    def counters():
        return [(entry("received")(h, s), entry("emitted")(h, s), entry("pending")(h, s)) for s in range(2)]

    # slot 1 is flushed after an empty utterance
    assert step([(1, 0, 1)], None, 0, 0, None, 0) == 0 and got[0] == 0
    got[0] = -7
    before = counters()
    assert before == [(0, 0, 0), (0, 0, 0)]
    refused(L, step([(1, 1, 0)], xp, xi, xr, yp, 4), STATE, f"{fn}: session 1 was flushed (item 0); {reset_fn} it before the next utterance")
    refused(L, step([(0, 5, 0)], xp, xi, xr, yp, 4), INVALID, f"{fn}: item 0 (session 0) has 5 frames, outside [0, max_chunk = 4]")
    refused(L, step([(0, -1, 0)], xp, xi, xr, yp, 4), INVALID, f"{fn}: item 0 (session 0) has -1 frames, outside [0, max_chunk = 4]")
    refused(L, step([(0, 1, 0)], None, xi, xr, yp, 4), INVALID, f"{fn}: null chunk buffer although item 0 (session 0) has 1 frames")
    refused(L, step([(0, 2, 0)], xp, xi, 1, yp, 4), INVALID,
            f"{fn}: row stride 1 is shorter than the longest chunk, the 2 frames of item 0 (session 0)")
    # what a step refuses after its items are admitted
    refused(L, step([(0, 4, 1)], xp, -1, xr, yp, 4), INVALID, f"{fn}: x_item_stride = -1 is negative")
    refused(L, step([(0, 4, 1)], xp, xi, xr, yp, (1 << 30) + 1), INVALID, f"{fn}: out_cols = 1073741825 is more than 2^30")
    refused(L, step([(0, 4, 1)], xp, xi, xr, yp, 3), INVALID, f"{fn}: out_cols = 3, but item 0 (session 0) emits 4 frames in this step")
    refused(L, step([(0, 4, 1)], xp, xi, xr, None, 4), INVALID, f"{fn}: null output although item 0 (session 0) emits 4 frames")
    refused(L, step([(0, 4, 0)], xp, xi, xr, None, 4), INVALID,
            f"{fn}: null {out_name} although every row's first out_cols = 4 columns are written")
    assert counters() == before and got[0] == -7
    # a valid push of 4 frames and the flush
    plan = schedule([MAX_CHUNK], R)
    assert plan == [(0, 0), (0, 4)]
    assert step([(0, 4, 0)], xp, xi, xr, None, 0) == 0 and got[0] == plan[0][1] - plan[0][0]
    assert counters()[0] == (4, 0, 4)
    refused(L, step([(0, 0, 1)], None, 0, 0, yp, 3), INVALID, f"{fn}: out_cols = 3, but item 0 (session 0) emits 4 frames in this step")
    assert counters()[0] == (4, 0, 4)
    assert step([(0, 0, 1)], None, 0, 0, yp, 4) == 0 and got[0] == plan[1][1] - plan[1][0]
    assert counters() == [(4, 4, 0), (0, 0, 0)]
    assert entry("received")(h, 2) == -1 and entry("emitted")(h, -1) == -1 and entry("pending")(h, 2) == -1
    torch.cuda.synchronize()
    assert torch.equal(y[:1], m(x[:1, :, :4].contiguous()))
    owner.close()
