"""Float64 numpy restatement of the reference's HubertEncoder (modules/encoders/hubert.py over HF's HubertModel, stable-layer-norm family) for
ONE unpadded row, with every hidden state.  The host tests pin it to the goldens; the GPU tests hold the kernels to it where no golden exists.
``forward(..., dtype=np.float32)`` evaluates the same statements in float32 (erf and the fold of the positional conv's weight norm included,
each rounded to float32): the host tests use it to show how far float32 arithmetic alone moves a result."""
from __future__ import annotations

from math import erf

import numpy as np

_erf = np.vectorize(erf, otypes=[np.float64])
_POS = "model.encoder.pos_conv_embed.conv."


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / x.dtype.type(np.sqrt(2.0))).astype(x.dtype, copy=False))


def silu(x):
    return x / (1.0 + np.exp(-x))


def layer_norm(x, w, b, eps=1e-5):
    """x: (F, C), over C."""
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def conv1d(x, w, b, stride=1, pad=0, groups=1):
    """x: (Cin, T); w: (Cout, Cin / groups, k) -> (Cout, floor((T + 2 pad - k) / stride) + 1)."""
    cout, cg, k = w.shape
    x = np.pad(x, ((0, 0), (pad, pad)))
    n = (x.shape[1] - k) // stride + 1
    if n <= 0:
        return np.zeros((cout, 0), x.dtype)
    idx = np.arange(n)[:, None] * stride + np.arange(k)[None, :]
    og = cout // groups
    out = np.empty((cout, n), x.dtype)
    for g in range(groups):
        win = x[g * cg:(g + 1) * cg][:, idx]                    # (cg, n, k)
        out[g * og:(g + 1) * og] = np.einsum("cnk,ock->on", win, w[g * og:(g + 1) * og])
    return out + b[:, None]


def frames(cfg: dict, samples: int, backbone: bool = False) -> int:
    f = int(samples)
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        f = (f - k) // s + 1 if f >= k else 0
    return f if backbone else ((f - 1) // 2 + 1 if f > 0 else 0)


def pos_conv_weight(sd: dict, dtype=np.float64) -> np.ndarray:
    g = np.asarray(sd[_POS + "parametrizations.weight.original0"], dtype)
    v = np.asarray(sd[_POS + "parametrizations.weight.original1"], dtype)
    return g * v / np.sqrt((v ** 2).sum((0, 1), keepdims=True))


def forward(sd: dict, cfg: dict, wave: np.ndarray, dtype=np.float64) -> dict:
    """wave: (T,) -> dict(hidden_states (L + 1, F, H), last_hidden_state (F, H), out (O, F_post)), every statement evaluated in ``dtype``."""
    p = {k: np.asarray(v, dtype) for k, v in sd.items()}
    heads = cfg["num_attention_heads"]
    x = np.asarray(wave, dtype)[None, :]
    for i in range(len(cfg["conv_dim"])):
        pfx = f"model.feature_extractor.conv_layers.{i}."
        x = conv1d(x, p[pfx + "conv.weight"], p[pfx + "conv.bias"], stride=cfg["conv_stride"][i])
        x = gelu(layer_norm(x.T, p[pfx + "layer_norm.weight"], p[pfx + "layer_norm.bias"])).T
    h = layer_norm(x.T, p["model.feature_projection.layer_norm.weight"], p["model.feature_projection.layer_norm.bias"])
    h = h @ p["model.feature_projection.projection.weight"].T + p["model.feature_projection.projection.bias"]
    F, H = h.shape
    k = cfg["num_conv_pos_embeddings"]
    pos = conv1d(h.T, pos_conv_weight(sd, dtype), p[_POS + "bias"], pad=k // 2, groups=cfg["num_conv_pos_embedding_groups"])[:, :F]   # SamePad
    h = h + gelu(pos).T
    hidden = [h]
    d = H // heads
    for i in range(cfg["num_hidden_layers"]):
        pfx = f"model.encoder.layers.{i}."
        lin = lambda v, name: v @ p[pfx + name + ".weight"].T + p[pfx + name + ".bias"]      # noqa: E731
        y = layer_norm(h, p[pfx + "layer_norm.weight"], p[pfx + "layer_norm.bias"])
        q, kk, v = (lin(y, f"attention.{n}_proj").reshape(F, heads, d).transpose(1, 0, 2) for n in "qkv")
        s = q @ kk.transpose(0, 2, 1) * d ** -0.5
        s = np.exp(s - s.max(-1, keepdims=True))
        a = (s / s.sum(-1, keepdims=True)) @ v
        h = h + lin(a.transpose(1, 0, 2).reshape(F, H), "attention.out_proj")
        y = layer_norm(h, p[pfx + "final_layer_norm.weight"], p[pfx + "final_layer_norm.bias"])
        h = h + lin(gelu(lin(y, "feed_forward.intermediate_dense")), "feed_forward.output_dense")
        hidden.append(h)
    last = layer_norm(h, p["model.encoder.layer_norm.weight"], p["model.encoder.layer_norm.bias"])
    y = silu(conv1d(last.T, p["post.0.weight"], p["post.0.bias"], pad=1))
    y = silu(conv1d(y, p["post.2.weight"], p["post.2.bias"], stride=2, pad=1))
    y = conv1d(y, p["post.4.weight"], p["post.4.bias"])
    return dict(hidden_states=np.stack(hidden), last_hidden_state=last, out=y)
