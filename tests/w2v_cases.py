"""What the wav2vec2 tests share (test_gpu_w2v.py, test_gpu_w2v_shapes.py, test_w2v_host.py): the parity bar, bit comparison, the C ABI
handle, and the table of configs of the shape sweep with their synthetic weights, waves and float64 restatements (w2v_reference.py).  The
sweep's configs have no golden from the reference: their expected values rest on the restatement alone, which the host suite pins to the
reference's goldens at the two fixture configs."""
import ctypes
import functools
import zlib

import numpy as np
import torch

import w2v_reference as wref
from vocoder_amd import _lib
from vocoder_amd import synthetic as syn

BAR = 1e-4      # the project's parity bar: max |d| over the expected tensor's own peak


def bits(a) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b) -> bool:
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def mask_of(lengths, T):
    return (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).to(torch.int64).cuda()


def parity(tag, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
    print(f"{tag}: max |d| / peak = {err:.2e} (peak {np.abs(want).max():.3g})")
    assert got.shape == want.shape and np.isfinite(got).all() and err <= BAR, (tag, err)
    return err


class Handle:
    """A finalized fv_w2v with the calls the tests make on the C ABI."""

    def __init__(self, cfg, sd, post):
        self.cfg, self.post, self.L, self.h = cfg, post, _lib.lib(), ctypes.c_void_p()
        n = len(cfg["conv_dim"])
        arr = lambda v: (ctypes.c_int32 * 8)(*v, *([0] * (8 - n)))      # noqa: E731
        c = _lib.W2VConfig(cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["intermediate_size"], n,
                           arr(cfg["conv_dim"]), arr(cfg["conv_kernel"]), arr(cfg["conv_stride"]), cfg["num_conv_pos_embeddings"],
                           cfg["num_conv_pos_embedding_groups"], post)
        _lib.check(self.L.fv_w2v_create(ctypes.byref(c), ctypes.byref(self.h)))
        for k, v in sd.items():
            if not post and k.startswith("post."):
                continue
            a = np.ascontiguousarray(v, np.float32)
            _lib.check(self.L.fv_w2v_load_weight(self.h, k.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                 (ctypes.c_int64 * max(a.ndim, 1))(*a.shape), a.ndim))
        _lib.check(self.L.fv_w2v_finalize(self.h))

    def frames(self, n, stage):
        return int(self.L.fv_w2v_frames(self.h, n, stage))

    def run(self, x, lengths, hidden=False, guard=0):
        """x: (B, T) device tensor -> (out, hidden states or None, the workspace tensor with `guard` extra bytes after it)."""
        B, T = x.shape
        F, F2 = self.frames(T, 0), self.frames(T, 1)
        H, nl = self.cfg["hidden_size"], self.cfg["num_hidden_layers"]
        out = torch.full((B, self.post, F2) if self.post else (B, F, H), float("nan"), device="cuda")
        hs = torch.full((nl + 1, B, F, H), float("nan"), device="cuda") if hidden else None
        need = int(self.L.fv_w2v_workspace_bytes(self.h, B, T))
        assert need > 0 and need % 4 == 0
        ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        lp = None if lengths is None else (ctypes.c_int32 * B)(*lengths)
        _lib.check(self.L.fv_w2v_forward(self.h, x.data_ptr(), T, lp, B, out.data_ptr(), hs.data_ptr() if hidden else None, ws.data_ptr(), need,
                                         int(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return out, hs, ws

    def close(self):
        torch.cuda.synchronize()
        self.L.fv_w2v_destroy(self.h)


# -- the shape sweep ------------------------------------------------------------------------------------------------------------------------
_FAMILY = dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, feat_proj_layer_norm=True)


def _cfg(hidden=128, heads=2, intermediate=256, conv_dim=(32, 64), conv_kernel=(10, 3), conv_stride=(5, 2), pos_k=16, pos_groups=4, post=96,
         layers=2):
    """hubert_tiny unless told otherwise."""
    return dict(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=intermediate, conv_dim=list(conv_dim),
                conv_kernel=list(conv_kernel), conv_stride=list(conv_stride), num_conv_pos_embeddings=pos_k,
                num_conv_pos_embedding_groups=pos_groups, output_size=post, **_FAMILY)


_REAL_CONVS = dict(conv_dim=(512, 512), conv_kernel=(10, 3), conv_stride=(5, 2), pos_k=128, pos_groups=16)
# name -> (config, backbone frames of its rows).  37 frames leave a ragged last 32-frame sub-tile of the GEMM and a ragged second key tile
# of the attention; 131 adds a second 128-query block, a third 64-frame tile and a fifth key tile of three keys.
SWEEP = {
    # the real widths: LayerNorm slots 0-3 all full (C = 1024) / three slots (768) / two (512); K = 4096, 3072, 1536, 1024, 768, 512
    "large": (_cfg(1024, 16, 4096, post=512, **_REAL_CONVS), (37,)),
    "base": (_cfg(768, 12, 3072, post=256, **_REAL_CONVS), (37,)),
    # N = 36, 260, 100, 68 (no multiple of 32); K = 108, 260, 100, 204, 68 on the 16-byte path (no multiple of 32); the positional conv
    # 64 groups of 3 on the single-float path, k = 5 (odd: SamePad drops nothing); LayerNorm C = 36 and C = 260 (slot 1, one lane)
    "odd": (_cfg(192, 3, 100, conv_dim=(36, 260), conv_kernel=(7, 3), conv_stride=(3, 2), pos_k=5, pos_groups=64, post=68), (37, 131)),
    # LayerNorm + GELU and the projection's LayerNorm at a partly filled slot 2, a partly filled slot 3 and the limit
    "ln516": (_cfg(conv_dim=(32, 516)), (37, 131)),
    "ln1020": (_cfg(conv_dim=(32, 1020)), (37, 131)),
    "ln1024": (_cfg(conv_dim=(32, 1024)), (37, 131)),
    # K below one stage on the 16-byte path: the second conv K = 3 x 4 = 12 and the projection K = 12; then both K = 4
    "k12": (_cfg(conv_dim=(4, 12)), (37, 131)),
    "k4": (_cfg(conv_dim=(4, 4), conv_kernel=(10, 1)), (37, 131)),
    # the positional conv's grouping: depthwise (Cg = 1), Cg = 2, one group of 192 (several column tiles per group), k = 1 and k = 2
    "depthwise": (_cfg(pos_groups=128), (37, 131)),
    "cg2": (_cfg(pos_groups=64), (37, 131)),
    "onegroup": (_cfg(192, 3, 384, pos_groups=1), (37, 131)),
    "posk1": (_cfg(pos_k=1), (37, 131)),
    "posk2": (_cfg(pos_k=2), (37, 131)),
    # the first conv layer: K = 32 (exactly one single-float stage, the limit) and 17; later layers: stride above the kernel, and the limits
    "first32": (_cfg(conv_kernel=(32, 3)), (37, 131)),
    "first17": (_cfg(conv_kernel=(17, 3)), (37, 131)),
    "k1s3": (_cfg(conv_dim=(32, 32, 64), conv_kernel=(10, 1, 3), conv_stride=(5, 3, 2)), (37, 131)),
    "k64s64": (_cfg(conv_kernel=(10, 64), conv_stride=(5, 64)), (37, 131)),
}
SWEEP_CASES = [(name, F) for name, (_, Fs) in SWEEP.items() for F in Fs]
BACKBONE_ONLY = [("odd", 37), ("base", 37)]       # post_channels = 0 at one odd and one real width


def sweep_seed(name) -> int:
    return zlib.crc32(name.encode()) % 100000


def with_layers(cfg, layers):
    return dict(cfg, num_hidden_layers=layers)


def samples_for(cfg, F) -> int:
    """The fewest samples that cfg's conv layers turn into exactly F frames."""
    n = F
    for k, s in zip(reversed(cfg["conv_kernel"]), reversed(cfg["conv_stride"])):
        n = (n - 1) * s + k
    return n


@functools.lru_cache(maxsize=2)
def sweep_state_dict(name, layers=None):
    """The weights of a sweep config (``layers`` transformer layers in place of its own); the two most recent are kept, large's are 100 MB."""
    cfg = SWEEP[name][0]
    return syn.hubert_state_dict(cfg if layers is None else with_layers(cfg, layers), sweep_seed(name))


def sweep_wave(name, F) -> np.ndarray:
    cfg = SWEEP[name][0]
    return np.random.default_rng(sweep_seed(name) * 1000 + F).standard_normal(samples_for(cfg, F)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sweep_restated(name, F):
    """The float64 restatement of the sweep's row (name, F): computed once, shared, never written to."""
    out = wref.forward(sweep_state_dict(name), SWEEP[name][0], sweep_wave(name, F))
    for a in out.values():
        a.setflags(write=False)
    return out
