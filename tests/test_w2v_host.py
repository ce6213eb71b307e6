"""Host (no GPU): the wav2vec2 / HuBERT encoder's surface (include/fishvoc.h fv_w2v_*, vocoder_amd/modules/encoders/hubert.py) — the declared
entry points and the config mirror, the state dict's keys against the reference's recorded ones, the refusals that name their field, that
nothing reaches for the network, the frame formula, and the float64 restatement (w2v_reference.py) against the reference's goldens.
For the configs of the shape sweep (w2v_cases.py, run on the GPU by test_gpu_w2v_shapes.py), which have no golden: float32 arithmetic alone
stays a factor of 10 under the parity bar, and the faults the sweep is there to catch move the restatement a factor of 10 above it.

The 30-sample row of ``hubert_tiny`` gives TWO frames ((30 - 10) // 5 + 1 = 5, then (5 - 3) // 2 + 1 = 2), not the one frame its place in
the fixture list was meant for; the fixture keeps it and carries a 24-sample row, which gives exactly one."""
import ctypes
import functools
import inspect
import json
import os
import re
import socket

import numpy as np
import pytest
import torch

import w2v_cases as wc
import w2v_reference as wref
from vocoder_amd import _lib
from vocoder_amd import synthetic as syn
from vocoder_amd.modules.encoders import HubertEncoder

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FIXTURES = ("tiny", "shape")
ENTRIES = ("fv_w2v_create", "fv_w2v_load_weight", "fv_w2v_finalize", "fv_w2v_frames", "fv_w2v_workspace_bytes", "fv_w2v_forward", "fv_w2v_destroy")
BAR = wc.BAR     # the project's parity bar: max |d| over the expected tensor's own peak
POS = "model.encoder.pos_conv_embed.conv."


@functools.lru_cache(maxsize=None)
def golden(name):
    g = np.load(os.path.join(GOLDEN, f"hubert_{name}.npz"))
    cfg = json.loads(bytes(g["config"]).decode())
    return cfg, int(g["seed"]), {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def restated(name, row):
    cfg, seed, g = golden(name)
    return wref.forward(syn.hubert_state_dict(cfg, seed), cfg, g["waves"][row, : int(g["lengths"][row])])


def tensors(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def module(cfg):
    return HubertEncoder(config={k: v for k, v in cfg.items() if k != "output_size"}, output_size=cfg["output_size"])


def w2v_config(cfg, **over):
    n = len(cfg["conv_dim"])
    arr = lambda v: (ctypes.c_int32 * 8)(*v, *([0] * (8 - n)))      # noqa: E731
    c = _lib.W2VConfig(cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["intermediate_size"], n, arr(cfg["conv_dim"]),
                       arr(cfg["conv_kernel"]), arr(cfg["conv_stride"]), cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"],
                       cfg["output_size"])
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


def create(cfg, **over):
    L, h = _lib.lib(), ctypes.c_void_p()
    st = L.fv_w2v_create(ctypes.byref(w2v_config(cfg, **over)), ctypes.byref(h))
    return st, h, L.fv_last_error().decode()


def load(h, name, arr):
    arr = np.ascontiguousarray(arr, np.float32)
    shape = (ctypes.c_int64 * max(arr.ndim, 1))(*arr.shape)
    return _lib.lib().fv_w2v_load_weight(h, name.encode(), arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), shape, arr.ndim)


def test_entry_points_are_declared_exported_and_present():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_w2v_\w+)\s*\(", hdr))
    assert declared == set(ENTRIES)
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    assert L.fv_abi_version() == 5 and _lib.FV_ABI_VERSION == 5


def test_config_mirror_matches_the_header_field_for_field():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    body = re.search(r"typedef struct fv_w2v_config \{(.*?)\} fv_w2v_config;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    assert [t for t, _, _ in fields] == ["int32_t"] * 11
    assert [n for _, n, _ in fields] == [n for n, _ in _lib.W2VConfig._fields_]
    for (_, name, dim), (_, ctype) in zip(fields, _lib.W2VConfig._fields_):
        assert ctypes.sizeof(ctype) == 4 * int(dim or 1), name
    assert ctypes.sizeof(_lib.W2VConfig) == 4 * (8 + 3 * 8) and _lib.W2V_MAX_CONV == 8


def test_constructor_signature_defaults_and_alias():
    from vocoder_amd import config
    sig = inspect.signature(HubertEncoder.__init__)
    assert list(sig.parameters)[1:] == ["model_name", "freeze_backbone", "output_size", "config"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == ["facebook/hubert-large-ll60k", True, 1024, None]
    assert config.locate("fish_vocoder.modules.encoders.hubert.HubertEncoder") is HubertEncoder
    cfg, _, _ = golden("tiny")
    m = config.instantiate({"_target_": "fish_vocoder.modules.encoders.hubert.HubertEncoder", "output_size": 96,
                            "config": {k: v for k, v in cfg.items() if k != "output_size"}})
    assert isinstance(m, HubertEncoder) and m.output_size == 96 and not any(p.requires_grad for p in m.model.parameters())


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_are_the_references_and_load_strictly(name):
    cfg, seed, g = golden(name)
    keys = json.loads(bytes(g["keys"]).decode())
    m = module(cfg)
    assert list(m.state_dict()) == keys
    sd = syn.hubert_state_dict(cfg, seed)
    assert list(sd) == keys
    res = m.load_state_dict(tensors(sd), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in sd.items():
        assert np.array_equal(m.state_dict()[k].numpy(), v), k
    missing = dict(tensors(sd))
    del missing["model.encoder.layers.1.attention.q_proj.bias"]
    with pytest.raises(RuntimeError, match="model.encoder.layers.1.attention.q_proj.bias"):
        module(cfg).load_state_dict(missing, strict=True)
    with pytest.raises(RuntimeError, match="model.encoder.adapter"):
        module(cfg).load_state_dict(dict(tensors(sd), **{"model.encoder.adapter.weight": torch.zeros(1)}), strict=True)


def test_legacy_weight_norm_names_load_and_masked_spec_embed_is_optional():
    cfg, seed, _ = golden("tiny")
    sd = tensors(syn.hubert_state_dict(cfg, seed))
    legacy = {}
    for k, v in sd.items():
        if k == "model.masked_spec_embed":
            continue
        legacy[k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")] = v
    assert POS + "weight_g" in legacy and POS + "weight_v" in legacy
    m = module(cfg)
    res = m.load_state_dict(legacy, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k in (POS + "parametrizations.weight.original0", POS + "parametrizations.weight.original1", "post.4.bias"):
        assert torch.equal(m.state_dict()[k], sd[k])


def test_synthetic_weights_are_what_the_issue_asks_for():
    cfg, seed, _ = golden("shape")
    sd = syn.hubert_state_dict(cfg, seed)
    v, g = sd[POS + "parametrizations.weight.original1"].astype(np.float64), sd[POS + "parametrizations.weight.original0"].reshape(-1)
    assert g.shape == (128,) and sd[POS + "parametrizations.weight.original0"].shape == (1, 1, 128)
    ratio = g / np.sqrt((v ** 2).sum((0, 1)))
    assert 0.65 < ratio.min() and ratio.max() < 1.45 and np.abs(ratio - 1).min() > 0
    assert all(np.abs(sd[k]).min() > 0 for k in sd if k.endswith(".bias"))
    assert all(np.abs(sd[k] - 1).max() > 0.2 for k in sd if k.endswith("layer_norm.weight"))
    for k, a in syn.hubert_state_dict(cfg, seed).items():
        assert np.array_equal(a, sd[k])
    out = restated("shape", 0)
    assert all(0.1 < np.abs(h).std() < 20 for h in out["hidden_states"])         # O(1) activations through the stack


def test_load_weight_and_finalize_name_what_is_wrong():
    L = _lib.lib()
    cfg, seed, _ = golden("tiny")
    sd = syn.hubert_state_dict(cfg, seed)
    st, h, _ = create(cfg)
    assert st == 0
    try:
        assert load(h, "model.encoder.adapter.weight", np.zeros(3)) == _lib.FV_ERR_INVALID and "model.encoder.adapter.weight" in L.fv_last_error().decode()
        assert load(h, "post.0.weight", np.zeros((96, 128, 5))) == -4
        msg = L.fv_last_error().decode()
        assert "post.0.weight" in msg and "(96, 128, 5)" in msg and "(96, 128, 3)" in msg
        assert load(h, POS + "weight_g", np.zeros((1, 1, 15))) == -4 and "(1, 1, 16)" in L.fv_last_error().decode()
        for k, v in sd.items():
            if k not in ("model.encoder.layers.0.final_layer_norm.bias", POS + "parametrizations.weight.original0"):
                assert load(h, k, v) == 0, (k, L.fv_last_error())
        assert load(h, POS + "weight_g", sd[POS + "parametrizations.weight.original0"]) == 0         # the legacy name fills original0
        assert L.fv_w2v_finalize(h) == -3 and "model.encoder.layers.0.final_layer_norm.bias" in L.fv_last_error().decode()    # before any device work
        assert L.fv_w2v_forward(h, None, 4000, None, 1, None, None, None, 0, None) == _lib.FV_ERR_STATE
        assert L.fv_w2v_workspace_bytes(h, 0, 4000) == 0 and L.fv_w2v_workspace_bytes(h, 2, 14) == 0      # no frame comes out
        assert L.fv_w2v_workspace_bytes(h, 2, 4000) > 0
        assert L.fv_w2v_workspace_bytes(h, -1, 5) == 0 and "batch" in L.fv_last_error().decode()
        assert L.fv_w2v_workspace_bytes(h, 3, 1 << 29) == 0 and "T =" in L.fv_last_error().decode()
    finally:
        L.fv_w2v_destroy(h)


@pytest.mark.parametrize("over,field,status", [
    (dict(hidden=0), "hidden", -1), (dict(hidden=1088, heads=17), "hidden", -1), (dict(hidden=126), "hidden", -1),
    (dict(layers=0), "layers", -1), (dict(layers=65), "layers", -1),
    (dict(heads=0), "heads", -1), (dict(heads=3), "heads", -1), (dict(heads=4), "heads", _lib.FV_ERR_UNSUPPORTED), (dict(heads=1), "heads", _lib.FV_ERR_UNSUPPORTED),
    (dict(intermediate=0), "intermediate", -1), (dict(intermediate=8196), "intermediate", -1), (dict(intermediate=254), "intermediate", -1),
    (dict(n_conv=0), "n_conv", -1), (dict(n_conv=9), "n_conv", -1),
    (dict(conv_dim=(1, 0)), "conv_dim[1]", -1), (dict(conv_dim=(0, 1028)), "conv_dim[0]", -1), (dict(conv_dim=(1, 62)), "conv_dim[1]", -1),
    (dict(conv_kernel=(0, 33)), "conv_kernel[0]", -1), (dict(conv_kernel=(1, 0)), "conv_kernel[1]", -1), (dict(conv_kernel=(1, 65)), "conv_kernel[1]", -1),
    (dict(conv_stride=(0, 0)), "conv_stride[0]", -1), (dict(conv_stride=(1, 65)), "conv_stride[1]", -1),
    (dict(pos_conv_kernel=0), "pos_conv_kernel", -1), (dict(pos_conv_kernel=257), "pos_conv_kernel", -1),
    (dict(pos_conv_groups=0), "pos_conv_groups", -1), (dict(pos_conv_groups=3), "pos_conv_groups", -1),
    (dict(post_channels=-4), "post_channels", -1), (dict(post_channels=8196), "post_channels", -1), (dict(post_channels=98), "post_channels", -1),
])
def test_create_refuses_each_limit_by_name(over, field, status):
    cfg, _, _ = golden("tiny")
    st, h, msg = create(cfg, **over)
    assert st == status and not h.value
    assert msg.startswith("fv_w2v_create:") and f"{field} =" in msg, msg


def test_create_takes_the_large_config_and_backbone_only():
    large = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, conv_dim=[512] * 7,
                 conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
                 output_size=1024)
    for post in (1024, 0):
        st, h, msg = create(large, post_channels=post)
        assert st == 0, msg
        assert _lib.lib().fv_w2v_frames(h, 16000, 0) == 49 and _lib.lib().fv_w2v_frames(h, 16000, 1) == 25
        _lib.lib().fv_w2v_destroy(h)


@pytest.mark.parametrize("field,value", [
    ("feat_extract_norm", "group"), ("do_stable_layer_norm", False), ("conv_bias", False), ("feat_proj_layer_norm", False),
    ("feat_extract_activation", "relu"), ("hidden_act", "relu"), ("layer_norm_eps", 1e-12), ("conv_pos_batch_norm", True)])
def test_other_families_are_refused_by_field(field, value):
    cfg, _, _ = golden("tiny")
    hf = {k: v for k, v in cfg.items() if k != "output_size"}
    with pytest.raises(ValueError, match=rf"{field} = "):
        HubertEncoder(config=dict(hf, **{field: value}), output_size=96)
    # HF's defaults are the group-norm / post-LN "base" family: a config that leaves the family fields out is that family
    base = {k: v for k, v in hf.items() if k not in ("feat_extract_norm", "do_stable_layer_norm", "conv_bias")}
    with pytest.raises(ValueError, match="feat_extract_norm = 'group'"):
        HubertEncoder(config=base, output_size=96)


def test_python_refusals(tmp_path):
    cfg, _, _ = golden("tiny")
    hf = {k: v for k, v in cfg.items() if k != "output_size"}
    m = module(cfg).eval()
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m(torch.zeros(1, 400))
    with pytest.raises(ValueError, match="fp32 only"):
        m.precision = "f16x3"
    m.precision = "f32"
    assert m.precision == "f32"
    with pytest.raises(ValueError, match="freeze_backbone"):
        HubertEncoder(config=hf, freeze_backbone=False)
    with pytest.raises(ValueError, match="head size"):
        HubertEncoder(config=dict(hf, num_attention_heads=4), output_size=96)
    with pytest.raises(ValueError, match="post_channels = 98"):
        HubertEncoder(config=hf, output_size=98)
    # an object with HF's field names, and a local directory with a config.json
    obj = type("Cfg", (), hf)()
    assert list(HubertEncoder(config=obj, output_size=96).state_dict()) == list(m.state_dict())
    (tmp_path / "config.json").write_text(json.dumps(hf))
    assert list(HubertEncoder(model_name=str(tmp_path), output_size=96).state_dict()) == list(m.state_dict())


def test_no_config_and_no_local_directory_raises_without_touching_the_network(monkeypatch, tmp_path):
    def refuse(*args, **kwargs):
        pytest.fail("HubertEncoder tried to open a connection")

    monkeypatch.setattr(socket.socket, "connect", refuse)
    monkeypatch.setattr(socket.socket, "connect_ex", refuse)
    with pytest.raises(ValueError, match="local directory"):
        HubertEncoder()
    with pytest.raises(ValueError, match="config.json"):
        HubertEncoder(model_name=str(tmp_path))          # a directory without a config.json
    src = open(os.path.join(REPO, "vocoder_amd", "modules", "encoders", "hubert.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(transformers|huggingface_hub)", src, re.M) and "from_pretrained(" not in src


def test_frames_equal_the_floor_formula():
    L = _lib.lib()
    for name in FIXTURES:
        cfg, _, g = golden(name)
        st, h, _ = create(cfg)
        assert st == 0
        m = module(cfg)
        field = sum((k - 1) * int(np.prod(cfg["conv_stride"][:i])) for i, k in enumerate(cfg["conv_kernel"])) + 1      # samples of one frame
        try:
            for n in list(range(0, 60)) + [field - 1, field, field + 1, 399, 400, 401, 719, 720, 1500, 8000, 16000, 480000]:
                f = n
                for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
                    f = max((f - k) // s + 1, 0) if f >= k else 0
                f2 = (f + 2 - 3) // 2 + 1 if f else 0
                assert L.fv_w2v_frames(h, n, 0) == f == m.frames(n, backbone=True) == wref.frames(cfg, n, backbone=True), n
                assert L.fv_w2v_frames(h, n, 1) == f2 == m.frames(n) == wref.frames(cfg, n), n
            assert L.fv_w2v_frames(h, field - 1, 0) == 0 and L.fv_w2v_frames(h, field, 0) == 1 and L.fv_w2v_frames(h, field, 1) == 1
            assert L.fv_w2v_frames(h, -1, 0) == -1 and L.fv_w2v_frames(h, 5, 2) == -1
            assert [L.fv_w2v_frames(h, int(n), 0) for n in g["lengths"]] == list(g["frames"])
        finally:
            L.fv_w2v_destroy(h)
    assert list(golden("tiny")[2]["frames"]) == [149, 60, 2, 1] and list(golden("shape")[2]["frames"]) == [24, 13, 1]


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_the_references_goldens(name):
    """Pins w2v_reference to the real reference: every stored tensor."""
    cfg, seed, g = golden(name)
    for b in range(len(g["lengths"])):
        out = restated(name, b)
        pairs = [("out", out["out"], g[f"out_{b}"]), ("last_hidden_state", out["last_hidden_state"], g[f"last_hidden_state_{b}"])]
        if b == int(g["hidden_row"]):
            # HF's tuple ends with the normed state, so the goldens hold layer 0's input and the outputs of all layers but the last
            pairs.append(("hidden_states", out["hidden_states"][:-1], g["hidden_states"]))
            assert g["hidden_states"].shape[0] == cfg["num_hidden_layers"] and g["hidden_states"].shape[1] > 1
        for key, got, want in pairs:
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"hubert_{name} row {b} {key}: fp64 restatement vs the reference's fp32, max |d| / peak = {err:.2e}")
            assert got.shape == want.shape and err <= BAR


def moved(want, got) -> float:
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("name,F", wc.SWEEP_CASES)
def test_float32_arithmetic_alone_stays_a_tenth_of_the_bar_at_every_sweep_config(name, F):
    """A condition on the sweep's inputs: the restatement evaluated in float32 lies within BAR / 10 of the float64 one's peak in every hidden
    state, the normed state and the output, so a kernel in exact fp32 has a factor of 10 of room under the bar.  A config that breaks it gets
    another seed or scale, not another condition."""
    cfg = wc.SWEEP[name][0]
    want = wc.sweep_restated(name, F)
    got = wref.forward(wc.sweep_state_dict(name), cfg, wc.sweep_wave(name, F), dtype=np.float32)
    assert want["hidden_states"].dtype == np.float64 and want["hidden_states"].shape == (cfg["num_hidden_layers"] + 1, F, cfg["hidden_size"])
    assert want["out"].shape == (cfg["output_size"], (F - 1) // 2 + 1)
    pairs = [(f"hidden state {i}", got["hidden_states"][i], want["hidden_states"][i]) for i in range(cfg["num_hidden_layers"] + 1)]
    pairs += [(k, got[k], want[k]) for k in ("last_hidden_state", "out")]
    for key, g, w in pairs:
        err = moved(w, g)
        print(f"{name} {F} frames {key}: float32 restatement vs float64, max |d| / peak = {err:.2e}")
        assert g.dtype == np.float32 and g.shape == w.shape and err <= BAR / 10, (key, err)


def altered(name, key, index):
    """The restatement of the sweep's first row of `name` with sd[key][index] zeroed."""
    cfg, Fs = wc.SWEEP[name]
    sd = wc.sweep_state_dict(name)
    w = sd[key].copy()
    assert np.abs(w[index]).min() > 0
    w[index] = 0
    return wc.sweep_restated(name, Fs[0]), wref.forward(dict(sd, **{key: w}), cfg, wc.sweep_wave(name, Fs[0]))


@pytest.mark.parametrize("name", ("large", "base", "odd"))
def test_a_dropped_k_tail_tap_or_quad_moves_the_next_state_ten_bars(name):
    """What a kernel that drops the last four k of a product, one tap of a conv or the last quad of a LayerNorm row would compute, stated as
    altered weights of the float64 restatement: the first state downstream moves by more than 10 BAR of its peak, so a sweep case that passes
    at the bar has excluded it."""
    cfg = wc.SWEEP[name][0]
    last, nc = cfg["num_hidden_layers"] - 1, len(cfg["conv_dim"])
    tail = (slice(None), slice(-4, None))
    cases = [("the projection's last four k", "model.feature_projection.projection.weight", tail, lambda o: o["hidden_states"][0]),
             ("the second FFN product's last four k", f"model.encoder.layers.{last}.feed_forward.output_dense.weight", tail,
              lambda o: o["hidden_states"][last + 1]),
             ("the final LayerNorm's last four gammas", "model.encoder.layer_norm.weight", slice(-4, None), lambda o: o["last_hidden_state"])]
    for l in range(nc):
        cases.append((f"the last tap of channel 5 of conv layer {l}", f"model.feature_extractor.conv_layers.{l}.conv.weight",
                      (5, slice(None), cfg["conv_kernel"][l] - 1), lambda o: o["hidden_states"][0]))
    for what, key, index, state in cases:
        want, got = altered(name, key, index)
        err = moved(state(want), state(got))
        print(f"{name}: {what} zeroed moves the next state by {err:.2e} of its peak")
        assert err > 10 * BAR, (what, err)


@pytest.mark.parametrize("name", ("large", "base"))
def test_one_zeroed_element_of_q_proj_moves_the_output_a_bar(name):
    cfg = wc.SWEEP[name][0]
    for layer in (0, cfg["num_hidden_layers"] - 1):
        want, got = altered(name, f"model.encoder.layers.{layer}.attention.q_proj.weight", (0, 0))
        err = moved(want["out"], got["out"])
        print(f"{name}: q_proj.weight[0, 0] of layer {layer} zeroed moves the output by {err:.2e} of its peak")
        assert err > BAR, (layer, err)


def test_the_restatement_in_float64_is_the_default_and_float32_is_float32_throughout():
    cfg, seed, g = golden("tiny")
    sd, wave = syn.hubert_state_dict(cfg, seed), g["waves"][1, : int(g["lengths"][1])]
    a, b = restated("tiny", 1), wref.forward(sd, cfg, wave, dtype=np.float64)
    assert all(v.dtype == np.float64 and np.array_equal(v, b[k]) for k, v in a.items())
    c = wref.forward(sd, cfg, wave, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in c.values()) and 0 < moved(a["out"], c["out"]) <= BAR / 10
