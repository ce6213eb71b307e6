#!/usr/bin/env python
"""Generate ``mms_{tiny,rate}.npz`` by RUNNING THE REFERENCE's MMSEncoder.forward on the CPU, over HF's ``Wav2Vec2Model`` with synthetic weights.

Like gen_golden_hubert.py this runs only where the reference checkout is (``FV_REFERENCE``) and where ``transformers`` is installed; the
fixtures are plain data — config, seed, rate, hops, waves, lengths, the state dict's key names in order, the processor's ``input_values`` and
the module's outputs — and travel with the repository.  Weights are not stored: the tests regenerate them with
``vocoder_amd.synthetic.mms_state_dict`` (numpy PCG64).

Nothing is downloaded: ``HF_HUB_OFFLINE`` / ``TRANSFORMERS_OFFLINE`` are set before ``transformers`` is imported, and before the reference class
is constructed ``Wav2Vec2Model.from_pretrained`` is replaced by a function that builds ``Wav2Vec2Model(Wav2Vec2Config(**cfg))`` with eager
attention and ``Wav2Vec2FeatureExtractor.from_pretrained`` by one that builds ``Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000,
padding_value=0.0, do_normalize=True, return_attention_mask=True)`` — the settings of facebook/mms-300m's preprocessor — so the hub name is
never resolved.  Every row runs ALONE and unpadded (fp32, one thread): that is what the kernels promise for a row of a ragged batch.  The
archives are written with a fixed time stamp, so two runs give the same bytes.

The same bytes on another CPU take more than that.  Left to itself PyTorch picks its kernels by the instruction sets of the machine it runs
on — ATen's vectorised loops, oneDNN's convolutions and matrix products, MKL's sgemm — and each choice adds the backbone's fp32 sums in
another order: on one AVX-512 machine ``ATEN_CPU_CAPABILITY=avx2`` alone moves every output by a few 1e-7 of its peak, and two machines of
different make disagree in the same way.  So the generator pins all three to their portable forms before torch is imported
(``ATEN_CPU_CAPABILITY=default``, ``MKL_CBWR=COMPATIBLE``, which is MKL's documented mode for identical results across processors) and
switches oneDNN off.  The reference's graph and its fp32 arithmetic are untouched; only the order inside a sum is fixed.

``torchaudio`` is not installed where this is built, so a stand-in module is put into ``sys.modules`` before the reference is imported.  Its
``functional.resample`` returns its input when the rates are equal, which is what torchaudio does, and otherwise applies
tests/resample_reference.py's float64 ``Filter`` (the same polyphase windowed-sinc design, restated) and casts to fp32.  ``mms_tiny`` runs at
16 kHz and is therefore the pure reference path; the parity of ``mms_rate`` (44.1 kHz) is UNPINNED against torchaudio itself, like encodec
for the quantiser.
Usage:  python tests/golden/gen_golden_mms.py

The fixtures are the smallest shapes at which the kernels can go wrong:
  mms_tiny   synthetic.HUBERT_TINY (stride 10, field 20) at 16 kHz; hop 4 gives N > F (frames repeat in an uneven 2.5 pattern), hop 32
             N < F (frames are skipped); rows of 1500 (149 frames), 613 (a ragged middle) and 40 samples (3 frames; N = 1 at hop 32)
  mms_rate   hubert_shape's seven conv layers, hidden 192, 44100 -> 16000, hop 512; rows of 22050, 11911 and 1200 samples give 8000 /
             4322 / 436 samples at 16 kHz, 24 / 13 / 1 backbone frames and N = 43 / 23 / 2: the last row maps every output to frame 0
Waves are multiples of 2^-8 (they deflate to half their size; the archives stay under 300 KiB).
"""
from __future__ import annotations

import os

os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"
# One arithmetic whatever the CPU (see the docstring): set before torch is imported, and whatever the caller's environment says
os.environ["ATEN_CPU_CAPABILITY"] = "default"
os.environ["MKL_CBWR"] = "COMPATIBLE"

import importlib.util  # noqa: E402
import json  # noqa: E402
import sys  # noqa: E402
import types  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

from gen_golden_posterior import REFERENCE, write_npz  # noqa: E402
from resample_reference import Filter  # noqa: E402
from vocoder_amd import synthetic as syn  # noqa: E402

FAMILY = dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, feat_proj_layer_norm=True)
TINY = {k: v for k, v in syn.HUBERT_TINY.items() if k != "output_size"}
FIXTURES = {
    "tiny": dict(cfg=dict(TINY, **FAMILY), seed=31, sampling_rate=16000, hops=[4, 32], lengths=[1500, 613, 40]),
    "rate": dict(cfg=dict(hidden_size=192, num_hidden_layers=3, num_attention_heads=3, intermediate_size=384, conv_dim=[64] * 7,
                          conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], num_conv_pos_embeddings=128,
                          num_conv_pos_embedding_groups=16, **FAMILY), seed=32, sampling_rate=44100, hops=[512], lengths=[22050, 11911, 1200]),
}


def mms_waves(lengths, seed: int) -> np.ndarray:
    """(B, max length) fp32, zero past each row's length; O(1) multiples of 2^-8 from PCG64."""
    rng = np.random.default_rng(seed + 1000)
    x = np.zeros((len(lengths), max(lengths)), np.float32)
    for b, n in enumerate(lengths):
        x[b, :n] = (np.round(rng.standard_normal(n) * 256.0) / 256.0).astype(np.float32)
    return x


def torchaudio_stand_in() -> types.ModuleType:
    def resample(waveform, orig_freq, new_freq, **kwargs):
        assert not kwargs, kwargs
        if int(orig_freq) == int(new_freq):
            return waveform
        return torch.from_numpy(Filter(int(orig_freq), int(new_freq))(waveform.numpy()).astype(np.float32))

    mod, functional = types.ModuleType("torchaudio"), types.ModuleType("torchaudio.functional")
    functional.resample = resample
    mod.functional = functional
    return mod


def load_reference(hf_cfg: dict):
    import transformers
    from transformers import Wav2Vec2Config, Wav2Vec2FeatureExtractor, Wav2Vec2Model

    def build_model(*args, **kwargs):
        return Wav2Vec2Model(Wav2Vec2Config(**hf_cfg, attn_implementation="eager"))

    def build_processor(*args, **kwargs):
        return Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=True)

    transformers.Wav2Vec2Model.from_pretrained = staticmethod(build_model)
    transformers.Wav2Vec2FeatureExtractor.from_pretrained = staticmethod(build_processor)
    sys.modules["torchaudio"] = torchaudio_stand_in()
    sys.modules["torchaudio.functional"] = sys.modules["torchaudio"].functional
    spec = importlib.util.spec_from_file_location("fv_reference_mms", os.path.join(REFERENCE, "fish_vocoder/modules/encoders/mms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MMSEncoder


def main() -> None:
    torch.set_num_threads(1)             # one summation order, whatever the number of cores
    torch.backends.mkldnn.enabled = False        # convs and linears through im2col and MKL's sgemm, not oneDNN's per-ISA kernels
    for name, fx in FIXTURES.items():
        cfg, seed, rate, hops, lengths = fx["cfg"], fx["seed"], fx["sampling_rate"], fx["hops"], fx["lengths"]
        Ref = load_reference(cfg)
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in syn.mms_state_dict(cfg, seed).items()}
        waves = mms_waves(lengths, seed)
        arrays = dict(config=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8), seed=np.int64(seed), sampling_rate=np.int64(rate),
                      hops=np.asarray(hops, np.int64), waves=waves, lengths=np.asarray(lengths, np.int64))
        frames = []
        for hop in hops:
            model = Ref(sampling_rate=rate, hop_length=hop)
            res = model.load_state_dict(sd, strict=True)
            assert not res.missing_keys and not res.unexpected_keys
            assert list(model.state_dict()) == list(sd), "synthetic.mms_state_dict must keep the reference's key order"
            model.eval()
            arrays["keys"] = np.frombuffer(json.dumps(list(model.state_dict())).encode(), dtype=np.uint8)
            with torch.no_grad():
                for b, n in enumerate(lengths):
                    x = torch.from_numpy(waves[b:b + 1, :n])
                    out = model(x)
                    assert out.shape == (1, cfg["hidden_size"], n // hop), out.shape
                    arrays[f"out_h{hop}_{b}"] = out[0].numpy()
                    if hop == hops[0]:
                        # the processor's output for this row, by the call the reference makes (mms.py:20-26)
                        at16k = sys.modules["torchaudio"].functional.resample(x, orig_freq=rate, new_freq=16000)
                        values = model.processor([i.cpu().numpy() for i in at16k], return_tensors="pt", padding=True, sampling_rate=16000).input_values
                        arrays[f"input_values_{b}"] = values[0].numpy()
                        frames.append(int(model.model(values).last_hidden_state.shape[1]))
        arrays["frames"] = np.asarray(frames, np.int64)
        path = os.path.join(HERE, f"mms_{name}.npz")
        write_npz(path, arrays)
        size = os.path.getsize(path)
        assert size <= 300 * 1024, size
        print(f"wrote mms_{name}.npz: " + ", ".join(f"{k}{tuple(np.asarray(v).shape)}" for k, v in arrays.items()), f"[{size / 1024:.1f} KiB]")


if __name__ == "__main__":
    main()
