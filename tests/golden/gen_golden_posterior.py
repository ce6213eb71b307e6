#!/usr/bin/env python
"""Generate ``posterior_{vqvae,vae,bnvae}.npz`` by IMPORTING THE REFERENCE's PosteriorEncoder on the CPU.

Like gen_golden.py this runs only where the reference checkout is (``FV_REFERENCE``, default the path gen_golden.py uses); the fixtures are plain
data — config, seed, input, lengths, every tensor the eval forward returns, and the state dict's key names in order — and travel with the
repository.  Weights are not stored: the tests regenerate them with ``vocoder_amd.synthetic.posterior_state_dict`` (numpy PCG64).

``fish_vocoder/utils/__init__.py`` imports hydra, which is not installed: bare ``fish_vocoder`` / ``fish_vocoder.utils`` package stubs go into
``sys.modules`` and ``utils/mask.py`` and ``modules/encoders/posterior_encoder.py`` are loaded by path.  The archives are written with a fixed
time stamp, so two runs give the same bytes.  Usage:  python tests/golden/gen_golden_posterior.py
"""
from __future__ import annotations

import importlib.util
import io
import json
import os
import sys
import types
import warnings
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REFERENCE = os.environ.get("FV_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)

from vocoder_amd import synthetic as syn  # noqa: E402

FIXTURES = {
    "vqvae": dict(cfg=dict(syn.POSTERIOR_DEFAULT), seed=11, T=40, lengths=[40, 23]),
    "vae": dict(cfg=dict(in_channels=20, out_channels=8, hidden_channels=48, kernel_size=5, dilation_rate=2, dilation_cycle=3, n_layers=4,
                         mode="vae"), seed=12, T=131, lengths=[131, 66, 1]),
    "bnvae": dict(cfg=dict(in_channels=20, out_channels=8, hidden_channels=32, kernel_size=3, dilation_rate=3, dilation_cycle=2, n_layers=1,
                           mode="bnvae"), seed=13, T=9, lengths=[9, 5, 1]),
}


def posterior_input(cfg: dict, batch: int, T: int, seed: int) -> np.ndarray:
    """(B, in_channels, T) fp32, O(1) values from PCG64 (the tests draw theirs the same way)."""
    return np.random.default_rng(seed + 1000).standard_normal((batch, cfg["in_channels"], T)).astype(np.float32)


def load_reference():
    def by_path(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REFERENCE, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    for pkg in ("fish_vocoder", "fish_vocoder.utils"):
        stub = types.ModuleType(pkg)
        stub.__path__ = []
        sys.modules[pkg] = stub
    by_path("fish_vocoder.utils.mask", "fish_vocoder/utils/mask.py")
    return by_path("fv_reference_posterior_encoder", "fish_vocoder/modules/encoders/posterior_encoder.py").PosteriorEncoder


def write_npz(path: str, arrays: dict) -> None:
    """np.savez_compressed's format with a fixed time stamp per member: byte-stable."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main() -> None:
    torch.set_num_threads(1)             # one summation order, whatever the machine
    Ref = load_reference()
    for name, fx in FIXTURES.items():
        cfg, seed, T, lengths = fx["cfg"], fx["seed"], fx["T"], fx["lengths"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = Ref(**cfg)
        sd = syn.posterior_state_dict(cfg, seed)
        res = model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert list(model.state_dict()) == list(sd), "synthetic.posterior_state_dict must keep the reference's key order"
        model.eval()
        x = posterior_input(cfg, len(lengths), T, seed)
        with torch.no_grad():
            out = model(torch.from_numpy(x), torch.tensor(lengths))
        arrays = dict(config=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8), seed=np.int64(seed), x=x,
                      lengths=np.asarray(lengths, np.int64), keys=np.frombuffer(json.dumps(list(model.state_dict())).encode(), dtype=np.uint8))
        if cfg["mode"] == "vqvae":
            arrays["y"] = out.numpy()
        else:
            for key, t in zip(("z", "mean", "logvar", "mask"), out):
                arrays[key] = t.numpy()
        path = os.path.join(HERE, f"posterior_{name}.npz")
        write_npz(path, arrays)
        print(f"wrote posterior_{name}.npz: " + ", ".join(f"{k}{tuple(np.asarray(v).shape)}" for k, v in arrays.items()),
              f"[{os.path.getsize(path) / 1024:.1f} KiB]")


if __name__ == "__main__":
    main()
