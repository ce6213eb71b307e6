"""Host (no GPU): MMSEncoder's surface (include/fishvoc.h fv_mms_*, vocoder_amd/modules/encoders/mms.py) — the declared entry points, the
constructor and the alias, the state dict's keys against the reference's recorded ones, the refusals, the frame counts, and the float64
restatements (mms_reference.py) against the reference's goldens and against ``torch.nn.functional.interpolate`` on the CPU."""
import ctypes
import functools
import inspect
import json
import math
import os
import re
import socket

import numpy as np
import pytest
import torch

import mms_reference as mref
from resample_reference import Filter
from vocoder_amd import _lib
from vocoder_amd import synthetic as syn
from vocoder_amd.modules.encoders import MMSEncoder

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FIXTURES = ("tiny", "rate")
ENTRIES = ("fv_mms_normalize_workspace_bytes", "fv_mms_normalize", "fv_mms_interpolate", "fv_mms_nearest_index")
POS = "model.encoder.pos_conv_embed.conv."
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def golden(name):
    g = np.load(os.path.join(GOLDEN, f"mms_{name}.npz"))
    return json.loads(bytes(g["config"]).decode()), int(g["seed"]), {k: g[k] for k in g.files}


def tensors(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def module(name, hop=None):
    cfg, _, g = golden(name)
    return MMSEncoder(sampling_rate=int(g["sampling_rate"]), hop_length=int(g["hops"][0]) if hop is None else hop, config=cfg)


def fixture_pairs():
    """Every (F, N) of the fixtures."""
    pairs = []
    for name in FIXTURES:
        _, _, g = golden(name)
        for hop in g["hops"]:
            pairs += [(int(f), int(n) // int(hop)) for f, n in zip(g["frames"], g["lengths"])]
    return pairs


def test_entry_points_are_declared_exported_and_present():
    hdr = open(os.path.join(REPO, "include", "fishvoc.h")).read()
    declared = set(re.findall(r"FV_API\s+[\w\s\*]+?\b(fv_mms_\w+)\s*\(", hdr))
    assert declared == set(ENTRIES)
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    assert L.fv_abi_version() == 5 and _lib.FV_ABI_VERSION == 5
    # each declaration's comment cites the reference lines it replaces
    for name in ENTRIES:
        comment = hdr[: hdr.index(f" {name}(")].rsplit("/*", 1)[1]
        assert re.search(r"mms\.py:\d+", comment), name


def test_constructor_signature_defaults_and_alias():
    from vocoder_amd import config
    sig = inspect.signature(MMSEncoder.__init__)
    assert list(sig.parameters)[1:] == ["sampling_rate", "hop_length", "model_name", "config"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [44100, 512, "facebook/mms-300m", None]
    assert config.locate("fish_vocoder.modules.encoders.mms.MMSEncoder") is MMSEncoder
    cfg, _, _ = golden("tiny")
    m = config.instantiate({"_target_": "fish_vocoder.modules.encoders.mms.MMSEncoder", "sampling_rate": 16000, "hop_length": 4, "config": cfg})
    assert isinstance(m, MMSEncoder) and m.hop_length == 4 and m.sample_rate == 16000 and not any(p.requires_grad for p in m.model.parameters())
    assert MMSEncoder.takes_audio is True
    assert m.resample is None and module("rate").resample.table == "global"


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_are_the_references_and_load_strictly(name):
    cfg, seed, g = golden(name)
    keys = json.loads(bytes(g["keys"]).decode())
    m = module(name)
    assert list(m.state_dict()) == keys and not any(k.startswith("processor") for k in keys)
    sd = syn.mms_state_dict(cfg, seed)
    assert list(sd) == keys
    res = m.load_state_dict(tensors(sd), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in sd.items():
        assert np.array_equal(m.state_dict()[k].numpy(), v), k
    # the backbone's weights are the HuBERT generator's, minus post
    hub = syn.hubert_state_dict(dict(cfg, output_size=8), seed)
    assert all(np.array_equal(sd[k], hub[k]) for k in sd) and set(hub) - set(sd) == {f"post.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")}
    missing = dict(tensors(sd))
    del missing["model.encoder.layers.1.attention.q_proj.bias"]
    with pytest.raises(RuntimeError, match="model.encoder.layers.1.attention.q_proj.bias"):
        module(name).load_state_dict(missing, strict=True)
    with pytest.raises(RuntimeError, match="post.0.weight"):
        module(name).load_state_dict(dict(tensors(sd), **{"post.0.weight": torch.zeros(1)}), strict=True)


def test_legacy_weight_norm_names_load_and_masked_spec_embed_is_optional():
    cfg, seed, _ = golden("tiny")
    sd = tensors(syn.mms_state_dict(cfg, seed))
    legacy = {}
    for k, v in sd.items():
        if k == "model.masked_spec_embed":
            continue
        legacy[k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")] = v
    assert POS + "weight_g" in legacy and POS + "weight_v" in legacy
    m = module("tiny")
    res = m.load_state_dict(legacy, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k in (POS + "parametrizations.weight.original0", POS + "parametrizations.weight.original1", "model.encoder.layer_norm.bias"):
        assert torch.equal(m.state_dict()[k], sd[k])


def test_python_refusals(tmp_path):
    cfg, _, _ = golden("tiny")
    m = module("tiny")
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        m(torch.zeros(1, 400))
    m.eval()
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m(torch.zeros(1, 400))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m(torch.zeros(1, 1, 400))
    with pytest.raises(ValueError, match="fp32 only"):
        m.precision = "f16x3"
    m.precision = "f32"
    assert m.precision == "f32"
    # a row with output frames but no backbone frame: the error names the row and the minimum length (hubert_tiny's field is 20 samples)
    with pytest.raises(ValueError, match=r"row 1 holds 19 samples.*at least 20 samples"):
        m(torch.zeros(2, 400), lengths=[400, 19])
    with pytest.raises(ValueError, match=r"row 0 holds 19 samples"):
        m(torch.zeros(1, 19))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m(torch.zeros(2, 400), lengths=[400, 3])           # 3 samples give no output frame at hop 4: nothing to refuse but the device
    with pytest.raises(ValueError, match="lengths for 2 rows"):
        m(torch.zeros(2, 400), lengths=[400])
    with pytest.raises(ValueError, match=r"row 1, 401, lies outside"):
        m(torch.zeros(2, 400), lengths=[400, 401])
    with pytest.raises(ValueError, match=r"\(B, 1, L\)"):
        m(torch.zeros(2, 2, 400))
    r = module("rate")
    assert r.min_samples() == 1100 and r.backbone_frames(1100) == 1 and r.backbone_frames(1099) == 0
    with pytest.raises(ValueError, match=r"row 0 holds 1099 samples.*at least 1100 samples"):
        r.eval()(torch.zeros(1, 1099))
    with pytest.raises(ValueError, match="head size"):
        MMSEncoder(config=dict(cfg, num_attention_heads=4))
    with pytest.raises(ValueError, match="add_adapter"):
        MMSEncoder(config=dict(cfg, add_adapter=True))
    with pytest.raises(ValueError, match="hop_length"):
        MMSEncoder(hop_length=0, config=cfg)
    # an object with HF's field names, and a local directory with a config.json
    obj = type("Cfg", (), cfg)()
    assert list(MMSEncoder(config=obj).state_dict()) == list(m.state_dict())
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    assert list(MMSEncoder(model_name=str(tmp_path)).state_dict()) == list(m.state_dict())


@pytest.mark.parametrize("field,value", [
    ("feat_extract_norm", "group"), ("do_stable_layer_norm", False), ("conv_bias", False), ("feat_extract_activation", "relu"),
    ("hidden_act", "relu"), ("layer_norm_eps", 1e-12)])
def test_other_families_are_refused_by_field(field, value):
    cfg, _, _ = golden("tiny")
    with pytest.raises(ValueError, match=rf"MMSEncoder: {field} = "):
        MMSEncoder(config=dict(cfg, **{field: value}))
    base = {k: v for k, v in cfg.items() if k not in ("feat_extract_norm", "do_stable_layer_norm", "conv_bias")}
    with pytest.raises(ValueError, match="feat_extract_norm = 'group'"):
        MMSEncoder(config=base)


def test_no_config_and_no_local_directory_raises_without_touching_the_network(monkeypatch, tmp_path):
    def refuse(*args, **kwargs):
        pytest.fail("MMSEncoder tried to open a connection")

    monkeypatch.setattr(socket.socket, "connect", refuse)
    monkeypatch.setattr(socket.socket, "connect_ex", refuse)
    with pytest.raises(ValueError, match="MMSEncoder: .*local directory"):
        MMSEncoder()
    with pytest.raises(ValueError, match="config.json"):
        MMSEncoder(model_name=str(tmp_path))
    src = open(os.path.join(REPO, "vocoder_amd", "modules", "encoders", "mms.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(transformers|huggingface_hub|torchaudio)", src, re.M) and "from_pretrained(" not in src


def test_c_abi_refusals_name_their_argument_before_any_launch():
    """Every call here passes NULL device pointers: a refusal that came after a launch would have had nothing to launch on."""
    L = _lib.lib()
    err = lambda: L.fv_last_error().decode()      # noqa: E731
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
    assert L.fv_mms_normalize_workspace_bytes(3, 8000) == 3 * 2 * 16 and L.fv_mms_normalize_workspace_bytes(3, 8192) == 3 * 2 * 16
    assert L.fv_mms_normalize_workspace_bytes(3, 8193) == 3 * 3 * 16
    assert L.fv_mms_normalize_workspace_bytes(0, 8000) == 0 and L.fv_mms_normalize_workspace_bytes(2, 0) == 0
    assert L.fv_mms_normalize_workspace_bytes(-1, 5) == 0 and "batch = -1" in err()
    assert L.fv_mms_normalize_workspace_bytes(3, 1 << 29) == 0 and "T =" in err()
    assert L.fv_mms_normalize(None, 100, i32(100, 101), 2, None, None, 0, None) == _lib.FV_ERR_INVALID and "host_lengths[1] = 101" in err()
    assert L.fv_mms_normalize(None, 100, i32(-1, 5), 2, None, None, 0, None) == _lib.FV_ERR_INVALID and "host_lengths[0] = -1" in err()
    assert L.fv_mms_normalize(None, 100, None, 2, None, None, 0, None) == _lib.FV_ERR_INVALID and "workspace" in err()
    assert L.fv_mms_normalize(None, 100, None, 70000, None, None, 0, None) == _lib.FV_ERR_INVALID and "batch = 70000" in err()
    assert L.fv_mms_normalize(None, 0, None, 2, None, None, 0, None) == 0 and L.fv_mms_normalize(None, 100, None, 0, None, None, 0, None) == 0
    itp = lambda F, H, fr, nr, B, N: L.fv_mms_interpolate(None, F, H, fr, nr, B, None, N, None)      # noqa: E731
    assert itp(10, 128, i32(10, 0), i32(25, 1), 2, 25) == _lib.FV_ERR_INVALID and "row 1 has no source frame" in err()
    assert itp(0, 128, None, None, 1, 4) == _lib.FV_ERR_INVALID and "row 0 has no source frame" in err()
    assert itp(10, 126, None, None, 1, 25) == _lib.FV_ERR_INVALID and "H = 126" in err()
    assert itp(10, 0, None, None, 1, 25) == _lib.FV_ERR_INVALID and "H = 0" in err()
    assert itp(10, 128, i32(11), None, 1, 25) == _lib.FV_ERR_INVALID and "host_frames[0] = 11" in err()
    assert itp(10, 128, None, i32(26), 1, 25) == _lib.FV_ERR_INVALID and "host_out_frames[0] = 26" in err()
    assert itp(-1, 128, None, None, 1, 25) == _lib.FV_ERR_INVALID and "F = -1" in err()
    assert itp(10, 128, None, None, 1, -2) == _lib.FV_ERR_INVALID and "N = -2" in err()
    assert itp(10, 128, None, None, 1, 25) == _lib.FV_ERR_INVALID and "null d_y" in err()
    assert itp(10, 128, None, None, 0, 25) == 0 and itp(10, 128, None, None, 2, 0) == 0 and itp(0, 128, i32(0, 0), i32(0, 0), 2, 0) == 0


def test_frame_counts_match_the_fixtures():
    cfg, _, g = golden("tiny")
    assert list(g["lengths"]) == [1500, 613, 40] and list(g["frames"]) == [149, 60, 3] and list(g["hops"]) == [4, 32]
    for hop, want in ((4, [375, 153, 10]), (32, [46, 19, 1])):
        m = module("tiny", hop)
        assert [m.frames(int(n)) for n in g["lengths"]] == want == [g[f"out_h{hop}_{b}"].shape[1] for b in range(3)]
        assert [m.backbone_frames(int(n)) for n in g["lengths"]] == list(g["frames"])
        assert [m.resampled(int(n)) for n in g["lengths"]] == list(g["lengths"])
    _, _, g = golden("rate")
    m = module("rate")
    assert list(g["lengths"]) == [22050, 11911, 1200] and list(g["hops"]) == [512]
    assert [m.resampled(int(n)) for n in g["lengths"]] == [8000, 4322, 436] == [g[f"input_values_{b}"].shape[0] for b in range(3)]
    assert [m.backbone_frames(int(n)) for n in g["lengths"]] == [24, 13, 1] == list(g["frames"])
    assert [m.frames(int(n)) for n in g["lengths"]] == [43, 23, 2] == [g["out_h512_%d" % b].shape[1] for b in range(3)]
    assert m.frames(511) == 0 and m.frames(512) == 1 and m.backbone_frames(0) == 0
    for n in (0, 1, 399, 400, 401, 16000, 44100, 441000):
        assert m.resampled(n) == -((-160 * n) // 441)


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_normalisation_against_the_processors_output(name):
    """The stored ``input_values`` are HF's fp32 arithmetic: a pairwise fp32 mean (error at most (log2 n + 2) u mean|x|), a variance about
    it and a square root (relative error at most (log2 n + 5) u), one subtraction and one division (u each).  Against the exact
    z = (x - m) / s that is |d| <= (log2 n + 8) u |z| + (log2 n + 2) u mean|x| / s."""
    _, _, g = golden(name)
    rate = int(g["sampling_rate"])
    for b, n in enumerate(g["lengths"]):
        x = g["waves"][b, : int(n)]
        if rate != 16000:
            x = Filter(rate, 16000)(x).astype(np.float32)         # what the generator's stand-in resampler hands the processor
        z = mref.normalize(x)
        want = g[f"input_values_{b}"]
        assert want.shape == z.shape and want.dtype == np.float32
        lg = math.log2(len(x))
        s = math.sqrt(np.asarray(x, np.float64).var() + mref.EPS)
        bound = (lg + 8) * U * np.abs(z) + (lg + 2) * U * np.abs(x).mean() / s
        d = np.abs(want - z)
        print(f"mms_{name} row {b}: processor fp32 vs fp64 restatement, max |d| = {d.max():.2e}, max d / bound = {(d / bound).max():.3f}")
        assert (d <= bound).all()
        assert abs(z.mean()) < 1e-12 and abs(z.var() - 1) < 1e-5
    assert not mref.normalize(np.full(100, 3.25)).any() and mref.normalize(np.zeros(0)).shape == (0,)


def torch_nearest(F, N):
    idx = torch.nn.functional.interpolate(torch.arange(F, dtype=torch.float32).reshape(1, 1, F), size=N, mode="nearest")
    return idx.reshape(N).to(torch.int64).numpy()


def test_index_rule_equals_torch_on_the_whole_grid():
    bad = []
    for F in range(1, 65):
        for N in range(1, 201):
            if not np.array_equal(mref.nearest_index(F, N), torch_nearest(F, N)):
                bad.append((F, N))
    assert not bad, bad[:20]
    for F, N in fixture_pairs():
        assert np.array_equal(mref.nearest_index(F, N), torch_nearest(F, N)), (F, N)
    assert list(mref.nearest_index(3, 1)) == [0] and list(mref.nearest_index(1, 2)) == [0, 0]          # the one-frame rows of the fixtures
    assert list(mref.nearest_index(2, 5)) == [0, 0, 0, 1, 1]                                          # 2.5 outputs per frame, unevenly


def test_the_librarys_index_helper_equals_the_restated_rule():
    L = _lib.lib()
    pairs = fixture_pairs() + [(F, N) for F in (1, 2, 3, 5, 7, 24, 49, 63, 64) for N in (1, 2, 3, 7, 43, 64, 100, 127, 200)]
    for F, N in pairs:
        assert [L.fv_mms_nearest_index(F, N, j) for j in range(N)] == list(mref.nearest_index(F, N)), (F, N)
    assert L.fv_mms_nearest_index(0, 5, 0) == -1 and L.fv_mms_nearest_index(5, 0, 0) == -1
    assert L.fv_mms_nearest_index(5, 5, 5) == -1 and L.fv_mms_nearest_index(5, 5, -1) == -1


@pytest.mark.parametrize("name", FIXTURES)
def test_the_references_output_is_the_gather_of_its_own_frames(name):
    """Every column of a stored output is some backbone frame, repeated or skipped as the restated rule says: columns that the rule maps to
    one source frame are bit-equal, and the number of distinct columns is the number of distinct source frames."""
    _, _, g = golden(name)
    for hop in g["hops"]:
        for b, (n, F) in enumerate(zip(g["lengths"], g["frames"])):
            out = g[f"out_h{hop}_{b}"]
            src = mref.nearest_index(int(F), out.shape[1])
            for j in range(1, out.shape[1]):
                assert np.array_equal(out[:, j], out[:, j - 1]) == (src[j] == src[j - 1]), (hop, b, j)
