"""Host (no GPU): the posterior encoder's surface (include/fishvoc.h fv_posterior_*, vocoder_amd/modules/encoders/posterior_encoder.py) — the
declared entry points and the config mirror, the state dict's keys against the reference's recorded ones, the refusals that name their
field, the float64 restatement (posterior_reference.py) against the reference's goldens, and the reach."""
import ctypes
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import posterior_reference as pref
from vocoder_amd import _lib
from vocoder_amd import synthetic as syn
from vocoder_amd.modules.encoders import PosteriorEncoder

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
MODES = ("vqvae", "vae", "bnvae")
ENTRIES = ("fv_posterior_create", "fv_posterior_load_weight", "fv_posterior_finalize", "fv_posterior_reach_frames", "fv_posterior_output_channels",
           "fv_posterior_workspace_bytes", "fv_posterior_forward", "fv_posterior_destroy")
BAR = 1e-4      # the project's parity bar: max |d| over the expected tensor's own peak (test_gpu_models.py::test_refinegan_golden)


@functools.lru_cache(maxsize=None)
def golden(mode):
    g = np.load(os.path.join(GOLDEN, f"posterior_{mode}.npz"))
    cfg = json.loads(bytes(g["config"]).decode())
    return cfg, int(g["seed"]), {k: g[k] for k in g.files}


def tensors(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def create(**over):
    cfg = dict(in_channels=20, out_channels=8, hidden_channels=32, kernel_size=5, dilation_rate=1, dilation_cycle=1, n_layers=2, mode=0)
    cfg.update(over)
    L, h = _lib.lib(), ctypes.c_void_p()
    st = L.fv_posterior_create(ctypes.byref(_lib.PosteriorConfig(*[cfg[k] for k, _ in _lib.PosteriorConfig._fields_])), ctypes.byref(h))
    return st, h, L.fv_last_error().decode()


def load(h, name, arr):
    arr = np.ascontiguousarray(arr, np.float32)
    shape = (ctypes.c_int64 * max(arr.ndim, 1))(*arr.shape)
    return _lib.lib().fv_posterior_load_weight(h, name.encode(), arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), shape, arr.ndim)


def test_entry_points_are_declared_exported_and_present():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_posterior_\w+)\s*\(", hdr))
    assert declared == set(ENTRIES)
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    assert L.fv_abi_version() == 5 and _lib.FV_ABI_VERSION == 5
    assert re.search(r"#define FV_ABI_VERSION 5\b", hdr)


def test_config_mirror_matches_the_header_field_for_field():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    body = re.search(r"typedef struct fv_posterior_config \{(.*?)\} fv_posterior_config;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M)
    assert [t for t, _ in fields] == ["int32_t"] * 8
    assert [n for _, n in fields] == [n for n, _ in _lib.PosteriorConfig._fields_]
    assert all(t is ctypes.c_int32 for _, t in _lib.PosteriorConfig._fields_) and ctypes.sizeof(_lib.PosteriorConfig) == 32
    assert _lib.POSTERIOR_MODES == {"vqvae": 0, "vae": 1, "bnvae": 2}


@pytest.mark.parametrize("mode", MODES)
def test_state_dict_keys_are_the_references_and_load_strictly(mode):
    cfg, seed, g = golden(mode)
    keys = json.loads(bytes(g["keys"]).decode())
    m = PosteriorEncoder(**cfg)
    assert list(m.state_dict()) == keys
    sd = syn.posterior_state_dict(cfg, seed)
    assert list(sd) == keys
    res = m.load_state_dict(tensors(sd), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in sd.items():
        assert np.array_equal(m.state_dict()[k].numpy(), v), k
    missing = dict(tensors(sd))
    del missing["enc.res_skip_layers.0.weight_g"]
    with pytest.raises(RuntimeError, match="enc.res_skip_layers.0.weight_g"):
        PosteriorEncoder(**cfg).load_state_dict(missing, strict=True)
    if mode == "bnvae":
        assert m.mu_bn.weight.requires_grad is False and torch.all(PosteriorEncoder(**cfg).mu_bn.weight == 0.5)
    else:
        assert not hasattr(m, "mu_bn")


def test_synthetic_weights_are_what_the_issue_asks_for():
    cfg, seed, _ = golden("bnvae")
    sd = syn.posterior_state_dict(cfg, seed)
    v, g = sd["enc.in_layers.0.weight_v"], sd["enc.in_layers.0.weight_g"].reshape(-1)
    ratio = g / np.sqrt((v.reshape(v.shape[0], -1).astype(np.float64) ** 2).sum(1))
    assert 0.75 < ratio.min() and ratio.max() < 1.3 and np.abs(ratio - 1).min() > 0          # near |v|, never equal to it
    assert all(np.abs(sd[k]).min() > 0 for k in sd if k.endswith(".bias"))
    assert np.abs(sd["mu_bn.running_mean"]).max() > 0.1 and np.abs(sd["mu_bn.running_var"] - 1).max() > 0.1
    for k, a in syn.posterior_state_dict(cfg, seed).items():
        assert np.array_equal(a, sd[k])


def test_constructor_signature_defaults_and_alias():
    import inspect

    from vocoder_amd import config
    sig = inspect.signature(PosteriorEncoder.__init__)
    assert list(sig.parameters)[1:] == ["in_channels", "out_channels", "hidden_channels", "kernel_size", "dilation_rate", "dilation_cycle",
                                        "n_layers", "mode"]
    assert [sig.parameters[k].default for k in ("kernel_size", "dilation_rate", "dilation_cycle", "n_layers", "mode")] == [5, 1, 1, 16, "vqvae"]
    assert config.locate("fish_vocoder.modules.encoders.posterior_encoder.PosteriorEncoder") is PosteriorEncoder
    m = config.instantiate({"_target_": "fish_vocoder.modules.encoders.posterior_encoder.PosteriorEncoder", "in_channels": 20, "out_channels": 8,
                            "hidden_channels": 32, "n_layers": 2})
    assert isinstance(m, PosteriorEncoder) and m.mode == "vqvae" and m.remove_weight_norm() is None


def test_python_refusals():
    m = PosteriorEncoder(20, 8, 32, n_layers=2).eval()
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m(torch.zeros(1, 20, 3))
    with pytest.raises(ValueError, match="fp32 only"):
        m.precision = "f16x3"
    m.precision = "f32"
    assert m.precision == "f32"
    with pytest.raises(ValueError, match="mode"):
        PosteriorEncoder(20, 8, 32, mode="ae")
    with pytest.raises(ValueError, match="hidden_channels = 1025"):
        PosteriorEncoder(20, 8, 1025)
    with pytest.raises(ValueError, match="kernel_size = 4"):
        PosteriorEncoder(20, 8, 32, kernel_size=4)


@pytest.mark.parametrize("over,field,status", [
    (dict(hidden_channels=0), "hidden_channels", -1), (dict(hidden_channels=1025), "hidden_channels", -1),
    (dict(in_channels=0), "in_channels", -1), (dict(in_channels=4097), "in_channels", -1),
    (dict(out_channels=0), "out_channels", -1), (dict(out_channels=4097), "out_channels", -1),
    (dict(kernel_size=4), "kernel_size", -1), (dict(kernel_size=13), "kernel_size", -1), (dict(kernel_size=0), "kernel_size", -1),
    (dict(n_layers=0), "n_layers", -1), (dict(n_layers=65), "n_layers", -1),
    (dict(dilation_rate=0), "dilation_rate", -1), (dict(dilation_cycle=0), "dilation_cycle", -1),
    (dict(mode=3), "mode", -1),
    (dict(kernel_size=11, dilation_rate=3, dilation_cycle=5, n_layers=5), "dilation_rate", -2),      # 10 * 81 = 810 fits, 10 * 243 would not: see below
])
def test_create_refuses_each_limit_by_name(over, field, status):
    if status == -2:
        st, h, _ = create(**over)                  # d up to 81: a window of 810 + 128 columns is inside the budget
        assert st == 0
        _lib.lib().fv_posterior_destroy(h)
        over = dict(over, dilation_cycle=6, n_layers=6)
    st, h, msg = create(**over)
    assert st == status and not h.value
    assert msg.startswith("fv_posterior_create:") and f"{field} =" in msg, msg
    if status == -2:
        assert "LDS budget" in msg and st == _lib.FV_ERR_UNSUPPORTED


def test_a_huge_dilation_is_refused_not_overflowed():
    st, h, msg = create(kernel_size=3, dilation_rate=1 << 20, dilation_cycle=64, n_layers=64)
    assert st == _lib.FV_ERR_UNSUPPORTED and not h.value and "LDS budget" in msg


def test_load_weight_and_finalize_name_what_is_wrong():
    L = _lib.lib()
    cfg = dict(in_channels=20, out_channels=8, hidden_channels=32, kernel_size=3, dilation_rate=3, dilation_cycle=2, n_layers=1, mode="bnvae")
    sd = syn.posterior_state_dict(cfg, 0)
    st, h, _ = create(**dict(cfg, mode=2))
    assert st == 0
    try:
        assert L.fv_posterior_output_channels(h) == 8
        assert load(h, "enc.cond_layer.weight", np.zeros(3)) == _lib.FV_ERR_INVALID and "enc.cond_layer.weight" in L.fv_last_error().decode()
        assert load(h, "enc.in_layers.0.weight_v", np.zeros((64, 32, 5))) == -4
        msg = L.fv_last_error().decode()
        assert "enc.in_layers.0.weight_v" in msg and "(64, 32, 5)" in msg and "(64, 32, 3)" in msg
        # the one layer is the last: its res_skip conv has C rows, not 2C
        assert load(h, "enc.res_skip_layers.0.bias", np.zeros(64)) == -4 and "(32)" in L.fv_last_error().decode()
        for k, v in sd.items():
            if k != "proj.bias":
                assert load(h, k, v) == 0, (k, L.fv_last_error())
        assert L.fv_posterior_finalize(h) == -3 and "proj.bias" in L.fv_last_error().decode()       # before any device work
        # a forward on an encoder that is not finalized, and shapes a host can see
        assert L.fv_posterior_forward(h, None, 4, None, None, None, None, 1, 4, None, 0, None) == _lib.FV_ERR_STATE
        assert L.fv_posterior_workspace_bytes(h, 2, 5) == 3 * 2 * 32 * 5 * 4
        assert L.fv_posterior_workspace_bytes(h, 0, 5) == 0
        assert L.fv_posterior_workspace_bytes(h, -1, 5) == 0 and "batch" in L.fv_last_error().decode()
        assert L.fv_posterior_workspace_bytes(h, 65536, 5) == 0 and "batch" in L.fv_last_error().decode()
        assert L.fv_posterior_workspace_bytes(h, 3, 1 << 29) == 0 and "T =" in L.fv_last_error().decode()
    finally:
        L.fv_posterior_destroy(h)


@pytest.mark.parametrize("mode", MODES)
def test_restatement_against_the_references_goldens(mode):
    """Pins posterior_reference to the real reference: every returned tensor, the bnvae mean in padded frames included."""
    cfg, seed, g = golden(mode)
    out = pref.forward(cfg, syn.posterior_state_dict(cfg, seed), g["x"], g["lengths"])
    names = ("y",) if mode == "vqvae" else ("z", "mean", "logvar", "mask")
    assert set(out) == set(names)
    for k in names:
        err = np.abs(out[k] - g[k]).max() / np.abs(g[k]).max()
        print(f"posterior_{mode} {k}: fp64 restatement vs the reference's fp32, max |d| / peak = {err:.2e}")
        assert out[k].shape == g[k].shape and err <= BAR
    T = g["x"].shape[2]
    pad = np.arange(T)[None, :] >= g["lengths"][:, None]
    for k in names:
        if k not in ("mean", "mask"):
            assert not g[k].transpose(0, 2, 1)[pad].any()               # exact zeros past each length
    if mode == "bnvae":
        const = g["mean"].transpose(0, 2, 1)[pad]                       # BN(0): one constant per channel
        assert np.abs(const).min() > 0 and np.array_equal(const, np.broadcast_to(const[0], const.shape))
        assert np.abs(out["mean"].transpose(0, 2, 1)[pad] - const).max() <= BAR * np.abs(g["mean"]).max()


def test_reach_frames_is_the_formula():
    for mode, want in (("vqvae", 32), ("vae", 2 * (1 + 2 + 4 + 1)), ("bnvae", 1)):
        cfg, _, _ = golden(mode)
        assert pref.reach_frames(cfg) == want
        assert PosteriorEncoder(**cfg).reach_frames == want
        st, h, _ = create(**dict(cfg, mode=_lib.POSTERIOR_MODES[cfg["mode"]]))
        assert st == 0 and _lib.lib().fv_posterior_reach_frames(h) == want
        _lib.lib().fv_posterior_destroy(h)
