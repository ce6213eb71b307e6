#!/usr/bin/env python
"""Generate ``hubert_{tiny,shape}.npz`` by RUNNING THE REFERENCE's HubertEncoder on the CPU, over HF's ``HubertModel`` with synthetic weights.

Like gen_golden_posterior.py this runs only where the reference checkout is (``FV_REFERENCE``) and where ``transformers`` is installed; the
fixtures are plain data — config, seed, waves, lengths, the state dict's key names in order and the outputs — and travel with the repository.
Weights are not stored: the tests regenerate them with ``vocoder_amd.synthetic.hubert_state_dict`` (numpy PCG64).

Nothing is downloaded: ``HF_HUB_OFFLINE`` / ``TRANSFORMERS_OFFLINE`` are set before ``transformers`` is imported, and ``HubertModel.
from_pretrained`` is replaced, before the reference class is constructed, by a function that builds ``HubertModel(HubertConfig(**cfg))`` with
eager attention, so the hub name is never resolved.  Every row runs ALONE and unpadded (fp32, one thread): that is what the kernels promise for
a row of a ragged batch.  The archives are written with a fixed time stamp, so two runs give the same bytes.
Usage:  python tests/golden/gen_golden_hubert.py

The fixtures are the smallest shapes at which the kernels can go wrong:
  hubert_tiny   head size 64 in a tiny model; 1500 samples give 149 frames (five key tiles of 32, the last one ragged), 613 a ragged middle,
                30 give two frames, 24 exactly one (one key; the positional conv all padding)
  hubert_shape  the real seven conv layers' kernels and strides and the real positional conv, k = 128 (even: SamePad drops a sample), 16
                groups of 12 channels, wider than any of the sequences (24, 13 and 1 frames)
"""
from __future__ import annotations

import os

os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import importlib.util  # noqa: E402
import json  # noqa: E402
import sys  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from gen_golden_posterior import REFERENCE, write_npz  # noqa: E402
from vocoder_amd import synthetic as syn  # noqa: E402

FAMILY = dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, feat_proj_layer_norm=True)
FIXTURES = {
    "tiny": dict(cfg=dict(syn.HUBERT_TINY, **FAMILY), seed=21, lengths=[1500, 613, 30, 24]),
    "shape": dict(cfg=dict(hidden_size=192, num_hidden_layers=3, num_attention_heads=3, intermediate_size=384, conv_dim=[64] * 7,
                           conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], num_conv_pos_embeddings=128,
                           num_conv_pos_embedding_groups=16, output_size=64, **FAMILY), seed=22, lengths=[8000, 4321, 400]),
}


def hubert_waves(lengths, seed: int) -> np.ndarray:
    """(B, max length) fp32, zero past each row's length; O(1) values from PCG64 (the tests draw theirs the same way)."""
    rng = np.random.default_rng(seed + 1000)
    x = np.zeros((len(lengths), max(lengths)), np.float32)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.standard_normal(n).astype(np.float32)
    return x


def load_reference(hf_cfg: dict):
    import transformers
    from transformers import HubertConfig, HubertModel

    def build(*args, **kwargs):
        return HubertModel(HubertConfig(**hf_cfg, attn_implementation="eager"))

    transformers.HubertModel.from_pretrained = staticmethod(build)
    spec = importlib.util.spec_from_file_location("fv_reference_hubert", os.path.join(REFERENCE, "fish_vocoder/modules/encoders/hubert.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HubertEncoder


def main() -> None:
    torch.set_num_threads(1)             # one summation order, whatever the machine
    for name, fx in FIXTURES.items():
        cfg, seed, lengths = fx["cfg"], fx["seed"], fx["lengths"]
        hf_cfg = {k: v for k, v in cfg.items() if k != "output_size"}
        model = load_reference(hf_cfg)(model_name="never-resolved", output_size=cfg["output_size"])
        sd = syn.hubert_state_dict(cfg, seed)
        res = model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert list(model.state_dict()) == list(sd), "synthetic.hubert_state_dict must keep the reference's key order"
        model.eval()
        waves = hubert_waves(lengths, seed)
        arrays = dict(config=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8), seed=np.int64(seed), waves=waves,
                      lengths=np.asarray(lengths, np.int64), keys=np.frombuffer(json.dumps(list(model.state_dict())).encode(), dtype=np.uint8))
        frames = []
        with torch.no_grad():
            for b, n in enumerate(lengths):
                x = torch.from_numpy(waves[b:b + 1, :n])
                arrays[f"out_{b}"] = model(x, torch.ones(1, n, dtype=torch.long))[0].numpy()
                back = model.model(x, output_hidden_states=True)
                arrays[f"last_hidden_state_{b}"] = back.last_hidden_state[0].numpy()
                frames.append(int(back.last_hidden_state.shape[1]))
                # HF's tuple: the input of layer 0, every layer's output — and the LAST entry after the final norm; that one is
                # last_hidden_state again and is left out, so the stored states are the ones before the final norm
                arrays[f"_hs_{b}"] = torch.stack(back.hidden_states[:-1])[:, 0].numpy()
        pick = min((i for i, f in enumerate(frames) if f > 1), key=lambda i: frames[i])
        arrays["hidden_row"] = np.int64(pick)
        arrays["hidden_states"] = arrays[f"_hs_{pick}"]          # (layers, F, H): layer 0's input and the outputs of all layers but the last
        for b in range(len(lengths)):
            del arrays[f"_hs_{b}"]
        arrays["frames"] = np.asarray(frames, np.int64)
        path = os.path.join(HERE, f"hubert_{name}.npz")
        write_npz(path, arrays)
        size = os.path.getsize(path)
        assert size <= 300 * 1024, size
        print(f"wrote hubert_{name}.npz: " + ", ".join(f"{k}{tuple(np.asarray(v).shape)}" for k, v in arrays.items()), f"[{size / 1024:.1f} KiB]")


if __name__ == "__main__":
    main()
