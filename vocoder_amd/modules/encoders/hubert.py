"""Drop-in for the reference's ``HubertEncoder`` (fish_vocoder/modules/encoders/hubert.py): HF's ``HubertModel`` in its "stable layer norm"
form, then the ``post`` conv stack, in eval mode on the ``fv_w2v_*`` kernels (include/fishvoc.h, vocoder_amd/csrc/w2v.hip).

The module holds ordinary torch parameters under exactly the keys the reference module has — ``model.`` + HF's keys, the positional conv under
``parametrizations.weight.original0`` / ``original1``, then ``post.{0,2,4}.{weight,bias}`` — so a checkpoint loads strictly; the holders are
never called.  The legacy ``...conv.weight_g`` / ``weight_v`` names are taken too, and ``model.masked_spec_embed`` may be absent (it has no
eval arithmetic).

It never downloads anything: the architecture comes from ``config`` (a dict or an object with HF's field names) or from the ``config.json`` of a
local directory, the weights from ``load_state_dict``.  ``transformers`` is not imported.

A row has the same bits alone, in any batch and padded to any T; samples and frames past a row's length are never read, and the output and
every hidden state hold exact zeros there.  On a padded batch this differs from the reference on purpose ("Encoders"): it
equals the reference on the row run alone.  Not built: the group-norm / post-LN family, gradients (``freeze_backbone=False``), dropout,
SpecAugment, f16x3.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import json
import os

import torch
from torch import nn

from ... import _lib
from ..._lib import check

# HF's HubertConfig defaults for the fields read here (a config.json stores only what differs)
_HF_DEFAULTS = dict(
    hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu", layer_norm_eps=1e-5,
    feat_extract_norm="group", feat_extract_activation="gelu", conv_dim=(512,) * 7, conv_stride=(5, 2, 2, 2, 2, 2, 2),
    conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_bias=False, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
    conv_pos_batch_norm=False, do_stable_layer_norm=False, feat_proj_layer_norm=True)
# the one family with kernels: field -> required value
_FAMILY = dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, feat_proj_layer_norm=True, feat_extract_activation="gelu",
               hidden_act="gelu", layer_norm_eps=1e-5, conv_pos_batch_norm=False)

_POS = "model.encoder.pos_conv_embed.conv."
_LEGACY = {_POS + "weight_g": _POS + "parametrizations.weight.original0", _POS + "weight_v": _POS + "parametrizations.weight.original1"}


def resolve_config(config, model_name: str, who: str = "HubertEncoder") -> dict:
    """HF's fields as a dict, defaults filled in; from ``config`` or from ``model_name``/config.json.  Never touches the network.  ``who``
    names the module in the refusals."""
    if config is None:
        path = os.path.join(str(model_name), "config.json")
        if not os.path.isdir(str(model_name)) or not os.path.isfile(path):
            raise ValueError(
                f"{who}: model_name = {model_name!r} is not a local directory holding a config.json, and this module never downloads "
                "from the hub; pass config= (a dict or an object with HF's field names) or a local directory, then load_state_dict the weights")
        with open(path, "r", encoding="utf-8") as fh:
            config = json.load(fh)
    get = config.get if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
    cfg = {k: get(k, d) for k, d in _HF_DEFAULTS.items()}
    for field, want in _FAMILY.items():
        if cfg[field] != want:
            raise ValueError(f"{who}: {field} = {cfg[field]!r} is not supported: only the stable-layer-norm family "
                             f"({field} = {want!r}) has kernels")
    for field in ("conv_dim", "conv_kernel", "conv_stride"):
        cfg[field] = [int(v) for v in cfg[field]]
    n = len(cfg["conv_dim"])
    if len(cfg["conv_kernel"]) != n or len(cfg["conv_stride"]) != n:
        raise ValueError(f"{who}: conv_kernel and conv_stride must have len(conv_dim) = {n} entries")
    if not 1 <= n <= _lib.W2V_MAX_CONV:
        raise ValueError(f"{who}: conv_dim has {n} layers; the library takes 1 to {_lib.W2V_MAX_CONV}")
    return cfg


class _W2VEngine:
    """One finalized ``fv_w2v`` handle on one device."""

    def __init__(self, cfg: "_lib.W2VConfig", state_dict, device: torch.device):
        self.device, self._h = device, ctypes.c_void_p()
        L = _lib.lib()
        check(L.fv_w2v_create(ctypes.byref(cfg), ctypes.byref(self._h)))
        try:
            with torch.cuda.device(device):
                for name, t in state_dict.items():
                    host = t.detach().to("cpu", torch.float32).contiguous()
                    shape = (ctypes.c_int64 * max(host.dim(), 1))(*host.shape)
                    check(L.fv_w2v_load_weight(self._h, name.encode(), ctypes.cast(host.data_ptr(), ctypes.POINTER(ctypes.c_float)), shape, host.dim()))
                check(L.fv_w2v_finalize(self._h))
        except Exception:
            self.close()
            raise

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def close(self) -> None:
        if self._h is not None and self._h.value:
            if torch.cuda.is_available():
                torch.cuda.synchronize(self.device)     # kernels that read the weights may still be running
            _lib.lib().fv_w2v_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _holder(**children) -> nn.Module:
    m = nn.Module()
    for name, child in children.items():
        setattr(m, name, child)
    return m


def _backbone(cfg: dict) -> nn.Module:
    """Holder of HF's ``HubertModel`` parameters, in its registration order; never called."""
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    dims = cfg["conv_dim"]
    model = nn.Module()
    model.masked_spec_embed = nn.Parameter(torch.zeros(H))
    model.feature_extractor = _holder(conv_layers=nn.ModuleList(
        _holder(conv=nn.Conv1d(dims[i - 1] if i else 1, dims[i], cfg["conv_kernel"][i], stride=cfg["conv_stride"][i]), layer_norm=nn.LayerNorm(dims[i]))
        for i in range(len(dims))))
    model.feature_projection = _holder(layer_norm=nn.LayerNorm(dims[-1]), projection=nn.Linear(dims[-1], H))
    k = cfg["num_conv_pos_embeddings"]
    conv = nn.utils.parametrizations.weight_norm(nn.Conv1d(H, H, k, padding=k // 2, groups=cfg["num_conv_pos_embedding_groups"]), name="weight", dim=2)
    layers = nn.ModuleList(
        _holder(attention=_holder(k_proj=nn.Linear(H, H), v_proj=nn.Linear(H, H), q_proj=nn.Linear(H, H), out_proj=nn.Linear(H, H)),
                layer_norm=nn.LayerNorm(H), feed_forward=_holder(intermediate_dense=nn.Linear(H, I), output_dense=nn.Linear(I, H)),
                final_layer_norm=nn.LayerNorm(H))
        for _ in range(cfg["num_hidden_layers"]))
    model.encoder = _holder(pos_conv_embed=_holder(conv=conv), layer_norm=nn.LayerNorm(H), layers=layers)
    return model


class _BackboneModule(nn.Module):
    """What the encoders over the wav2vec2 backbone share: the parameter holder under ``model.``, the key hooks of its state dict, the
    fp32-only precision switch, the conv stack's frame count and the cache of one finalized ``fv_w2v`` engine."""
    post_channels = 0       # fv_w2v_config.post_channels of the engine: 0 = the backbone alone

    def _init_backbone(self, config, model_name: str) -> None:
        self.hf_config = resolve_config(config, model_name, type(self).__name__)
        self._config()                  # the library's limits, by name, before any parameter is allocated
        self.model = _backbone(self.hf_config)
        for p in self.model.parameters():
            p.requires_grad = False
        object.__setattr__(self, "_engine", None)
        self._register_load_state_dict_pre_hook(self._legacy_keys)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_engine())

    def _legacy_keys(self, state_dict, prefix, *_):
        for old, new in _LEGACY.items():
            if prefix + old in state_dict and prefix + new not in state_dict:
                state_dict[prefix + new] = state_dict.pop(prefix + old)
        spec = prefix + "model.masked_spec_embed"       # SpecAugment's vector: no eval arithmetic, so a checkpoint without it loads
        if spec not in state_dict:
            state_dict[spec] = self.model.masked_spec_embed.detach()

    def _config(self) -> "_lib.W2VConfig":
        """The validated config; a refusal is the library's own message (``fv_w2v_create`` does no device work)."""
        c = self.hf_config
        n = len(c["conv_dim"])
        pad = [0] * (_lib.W2V_MAX_CONV - n)
        arr = ctypes.c_int32 * _lib.W2V_MAX_CONV
        cfg = _lib.W2VConfig(int(c["hidden_size"]), int(c["num_hidden_layers"]), int(c["num_attention_heads"]), int(c["intermediate_size"]), n,
                             arr(*c["conv_dim"], *pad), arr(*c["conv_kernel"], *pad), arr(*c["conv_stride"], *pad),
                             int(c["num_conv_pos_embeddings"]), int(c["num_conv_pos_embedding_groups"]), int(self.post_channels))
        h = ctypes.c_void_p()
        L = _lib.lib()
        if L.fv_w2v_create(ctypes.byref(cfg), ctypes.byref(h)) != 0:
            raise ValueError(L.fv_last_error().decode("utf-8", "replace"))
        L.fv_w2v_destroy(h)
        return cfg

    # -- arithmetic: exact fp32 only ------------------------------------------------------------
    @property
    def precision(self) -> str:
        return "f32"

    @precision.setter
    def precision(self, value: str) -> None:
        if value == "f16x3":
            raise ValueError(f"{type(self).__name__} is fp32 only: there is no f16x3 form of the wav2vec2 kernels")
        if value != "f32":
            raise ValueError(f"precision must be 'f32', got {value!r}")

    def conv_frames(self, samples: int) -> int:
        """Frames the backbone gives for ``samples`` samples at its own rate: HF's ``_get_feat_extract_output_lengths``."""
        f = int(samples)
        for k, s in zip(self.hf_config["conv_kernel"], self.hf_config["conv_stride"]):
            f = (f - k) // s + 1 if f >= k else 0
        return f

    # -- engine cache (as PosteriorEncoder keeps its own) -------------------------------------------
    def invalidate_engine(self) -> None:
        eng = self.__dict__.get("_engine")
        if eng is not None:
            eng.close()
        object.__setattr__(self, "_engine", None)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_engine()
        return super()._apply(fn, *args, **kwargs)

    def engine(self, device: torch.device) -> _W2VEngine:
        eng = self.__dict__.get("_engine")
        if eng is None or eng.device != device:
            self.invalidate_engine()
            eng = _W2VEngine(self._config(), self.state_dict(), device)
            object.__setattr__(self, "_engine", eng)
        return eng


class HubertEncoder(_BackboneModule):
    def __init__(self, model_name: str = "facebook/hubert-large-ll60k", freeze_backbone: bool = True, output_size: int = 1024, config=None):
        super().__init__()
        if not freeze_backbone:
            raise ValueError("HubertEncoder: freeze_backbone = False needs gradients through the backbone; the kernels are inference-only")
        self.model_name, self.freeze_backbone, self.output_size = model_name, True, int(output_size)
        if self.output_size < 1:
            raise ValueError(f"HubertEncoder: output_size = {output_size} must be >= 1")
        self._init_backbone(config, model_name)
        H, O = self.hf_config["hidden_size"], self.output_size
        self.post = nn.Sequential(nn.Conv1d(H, O, kernel_size=3, padding=1), nn.SiLU(), nn.Conv1d(O, O, stride=2, kernel_size=3, padding=1), nn.SiLU(),
                                  nn.Conv1d(O, O, kernel_size=1))

    @property
    def post_channels(self) -> int:
        return self.output_size

    def frames(self, samples: int, backbone: bool = False) -> int:
        """Frames that ``samples`` samples give after ``post`` (or after the backbone): HF's ``_get_feat_extract_output_lengths``, then
        ``floor((F - 1) / 2) + 1``."""
        f = self.conv_frames(samples)
        return f if backbone else ((f - 1) // 2 + 1 if f > 0 else 0)

    # -- calls ---------------------------------------------------------------------------------
    def _run(self, x: torch.Tensor, lengths, want_hidden: bool, what: str):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError(
                f"{what} needs a CUDA/HIP tensor (got {getattr(x, 'device', type(x))}); vocoder_amd has no CPU path — move the model and "
                "input to the GPU")
        if self.training:
            raise RuntimeError(f"{type(self).__name__} is inference-only: call .eval() first")
        x = x.detach().to(torch.float32).contiguous()
        B, T = (int(v) for v in x.shape)
        if lengths is not None:
            if len(lengths) != B:
                raise ValueError(f"{what}: {len(lengths)} lengths for {B} rows")
            for b, v in enumerate(lengths):
                if not 0 <= v <= T:
                    raise ValueError(f"{what}: the length of row {b}, {v}, lies outside [0, T = {T}]")
        H, nl = self.hf_config["hidden_size"], self.hf_config["num_hidden_layers"]
        F, F2 = self.frames(T, backbone=True), self.frames(T)
        out = torch.empty((B, self.output_size, F2), dtype=torch.float32, device=x.device)
        hidden = torch.empty((nl + 1, B, F, H), dtype=torch.float32, device=x.device) if want_hidden else None
        if B and F:
            eng, L = self.engine(x.device), _lib.lib()
            with torch.cuda.device(x.device):
                need = int(L.fv_w2v_workspace_bytes(eng.handle, B, T))
                ws = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
                lptr = None if lengths is None else (ctypes.c_int32 * B)(*lengths)
                check(L.fv_w2v_forward(eng.handle, x.data_ptr(), T, lptr, B, out.data_ptr(), hidden.data_ptr() if want_hidden else None,
                                       ws.data_ptr(), need, int(torch.cuda.current_stream().cuda_stream)))
        return (out, hidden) if want_hidden else out

    def forward(self, x: torch.Tensor, mask: torch.Tensor = None, output_hidden_states: bool = False):
        """hubert.py:32-51 in eval mode.  ``x``: (B, T) or (B, 1, T); ``mask``: a 0/1 prefix mask of the same shape, a row's length is its sum
        (as HF computes it).  Returns (B, output_size, F_post); with ``output_hidden_states`` also (layers + 1, B, F, hidden): the input of
        layer 0 and every layer's output, HF's ``hidden_states`` without the final norm."""
        what = f"{type(self).__name__}.forward"
        if isinstance(x, torch.Tensor) and x.dim() == 3:
            if x.shape[1] != 1 or (mask is not None and (mask.dim() != 3 or mask.shape[1] != 1)):
                raise ValueError(f"{what}: a 3-d input must be (B, 1, T) with a mask of the same shape, got {tuple(x.shape)}")
            x = x[:, 0]
            mask = None if mask is None else mask[:, 0]
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise ValueError(f"{what}: expected (B, T) or (B, 1, T), got {tuple(getattr(x, 'shape', ()))}")
        lengths = None
        if mask is not None:
            if tuple(mask.shape) != tuple(x.shape):
                raise ValueError(f"{what}: mask {tuple(mask.shape)} does not match x {tuple(x.shape)}")
            lengths = [int(v) for v in mask.sum(-1).tolist()]
        return self._run(x, lengths, output_hidden_states, what)

    def forward_list(self, waves) -> list:
        """A list of 1-d waves -> a list of (output_size, F_post_i) through one padded call."""
        waves = list(waves)
        if not waves:
            return []
        what = f"{type(self).__name__}.forward_list"
        for x in waves:
            if not isinstance(x, torch.Tensor) or x.dim() != 1:
                raise ValueError(f"{what}: expected 1-d tensors, got {tuple(getattr(x, 'shape', ()))}")
        lengths = [int(x.shape[0]) for x in waves]
        padded = torch.zeros((len(waves), max(lengths)), dtype=torch.float32, device=waves[0].device)
        for b, x in enumerate(waves):
            padded[b, : lengths[b]] = x
        out = self._run(padded, lengths, False, what)
        return [out[b, :, : self.frames(n)] for b, n in enumerate(lengths)]

    def extra_repr(self) -> str:
        c = self.hf_config
        return (f"hidden_size={c['hidden_size']}, layers={c['num_hidden_layers']}, heads={c['num_attention_heads']}, "
                f"output_size={self.output_size}, backend=libfishvoc_hip (gfx950)")
