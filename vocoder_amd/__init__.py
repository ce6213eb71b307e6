"""vocoder_amd — MI355X-native (gfx950) inference engine behind the fish_vocoder generator API.

Public surface (mirrors /root/reference/fish_vocoder for the generator hot path only):

* ``vocoder_amd.modules.generators.{HiFiGANGenerator, BigVGANGenerator, ISTFTHead, UnifyGenerator}``,
  ``vocoder_amd.modules.encoders.ConvNeXtEncoder`` — drop-in ``nn.Module`` classes (same ctor kwargs, state-dict keys,
  ``forward(mel) -> waveform``);
* ``vocoder_amd.config`` — loads the reference's ``configs/model/generator/*.yaml`` keys and instantiates ``_target_``;
* ``vocoder_amd.engine`` — thin handle on the C ABI (``include/fishvoc.h``, ``csrc/libfishvoc_hip.so``);
* ``vocoder_amd.resample`` — ``Resample``, the GPU drop-in for ``torchaudio.transforms.Resample`` (whole rows, ragged rows, streaming);
* ``vocoder_amd.scoring`` — ``MelDistance`` / ``MultiResolutionSTFTDistance``, the reference's ``eval.py`` mel distance and the STFT loss's two
  formulas as GPU metrics; ``python -m vocoder_amd.eval SOURCE GENERATED`` scores a directory;
* ``vocoder_amd.f0`` — ``YinF0``, ``PitchTemplate`` and ``template_from_audio``: the F0 track and the pitch template that
  ``RefineGANGenerator`` and the ``use_template=True`` generators take next to the mel, made on the GPU from the audio, whole rows, ragged rows and
  chunk by chunk (``YinF0Stream``, ``PitchTemplateStream``, ``TemplateStream``) and per session (``YinF0Pool``, ``PitchTemplatePool``,
  ``TemplatePool``); exported here;
* ``vocoder_amd.sharding`` — utterance-batch sharding helpers for one process per GPU.

The compute path is hand-written HIP only; importing works on a CPU-only box (for config/host logic), running does not.
"""
__version__ = "0.1.0"

__all__ = ["PitchTemplate", "PitchTemplatePool", "PitchTemplateStream", "TemplatePool", "TemplateStream", "YinF0", "YinF0Pool", "YinF0Stream",
           "frames_ready", "template_from_audio"]


def __getattr__(name: str):
    # resolved on first use: importing the package (for config / host logic) does not import torch
    if name in __all__:
        from . import f0
        return getattr(f0, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
