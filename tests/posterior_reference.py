"""float64 numpy restatement of the posterior encoder's eval arithmetic (include/fishvoc.h, "posterior encoder"), written from the
formulas and not from the reference's text; test_posterior_host.py pins it to the reference's goldens.  It takes the fp32 state dict
(``vocoder_amd.synthetic.posterior_state_dict``'s keys) and fp32 inputs and computes everything in float64.

    h = pre(x) m;  out = 0
    layer i:  a = in_i(h), dilation d_i = rate ** (i % cycle), zero padding (k - 1) d_i / 2;  g = tanh(a[:C]) sigmoid(a[C:]);  r = rs_i(g)
              i < n - 1:  h = (h + r[:C]) m, out += r[C:];   last:  out += r
    y = proj(out m) m;  vae: mean, logvar = y[:O], clamp(y[O:], -30, 20);  bnvae: mean = BN_eval(mean);  z = mean m
"""
import numpy as np

BN_EPS = 1e-5


def fold(sd, prefix):
    """g v / |v| per output channel (the old nn.utils.weight_norm, dim 0)."""
    g, v = sd[f"{prefix}.weight_g"].astype(np.float64), sd[f"{prefix}.weight_v"].astype(np.float64)
    norm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(1)).reshape(-1, 1, 1)
    return g * v / norm


def conv1d(x, w, b, dilation=1):
    """x (B, Cin, T), w (M, Cin, k), 'same' zero padding (k odd)."""
    B, _, T = x.shape
    M, _, k = w.shape
    pad = (k - 1) * dilation // 2
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad)))
    y = np.zeros((B, M, T))
    for j in range(k):
        y += np.einsum("mc,bct->bmt", w[:, :, j], xp[:, :, j * dilation: j * dilation + T])
    return y + b.astype(np.float64)[None, :, None]


def reach_frames(cfg):
    k = cfg.get("kernel_size", 5)
    return sum((k - 1) * cfg.get("dilation_rate", 1) ** (i % cfg.get("dilation_cycle", 1)) // 2 for i in range(cfg.get("n_layers", 16)))


def forward(cfg, sd, x, lengths=None):
    """-> dict(y=...) for "vqvae", dict(z, mean, logvar, mask) for the vae modes; float64."""
    x = np.asarray(x, np.float64)
    B, _, T = x.shape
    C, O, n = cfg["hidden_channels"], cfg["out_channels"], cfg.get("n_layers", 16)
    rate, cycle, mode = cfg.get("dilation_rate", 1), cfg.get("dilation_cycle", 1), cfg.get("mode", "vqvae")
    lengths = np.full(B, T) if lengths is None else np.asarray(lengths)
    m = (np.arange(T)[None, :] < lengths[:, None]).astype(np.float64)[:, None, :]
    h = conv1d(x, sd["pre.weight"].astype(np.float64), sd["pre.bias"]) * m
    out = np.zeros((B, C, T))
    for i in range(n):
        a = conv1d(h, fold(sd, f"enc.in_layers.{i}"), sd[f"enc.in_layers.{i}.bias"], rate ** (i % cycle))
        g = np.tanh(a[:, :C]) / (1.0 + np.exp(-a[:, C:]))
        r = conv1d(g, fold(sd, f"enc.res_skip_layers.{i}"), sd[f"enc.res_skip_layers.{i}.bias"])
        if i < n - 1:
            h = (h + r[:, :C]) * m
            out = out + r[:, C:]
        else:
            out = out + r
    y = conv1d(out * m, sd["proj.weight"].astype(np.float64), sd["proj.bias"]) * m
    if mode == "vqvae":
        return dict(y=y)
    mean, logvar = y[:, :O], np.clip(y[:, O:], -30.0, 20.0)
    if mode == "bnvae":
        f = lambda k: sd[f"mu_bn.{k}"].astype(np.float64)[None, :, None]      # noqa: E731
        mean = (mean - f("running_mean")) / np.sqrt(f("running_var") + BN_EPS) * f("weight") + f("bias")
    return dict(z=mean * m, mean=mean, logvar=logvar, mask=m)
