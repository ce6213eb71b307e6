"""What the two critics share (``mpd.py``, ``mrd.py``): the weight-normed parameter holders, one finalized ``fv_disc`` handle per device, the
padded call with per-row lengths, and the reference's nesting of scores and feature maps over the channel-last output buffer
(include/fishvoc.h ``fv_disc_*``, vocoder_amd/csrc/disc.hip).  Eval only, fp32 only; there is no CPU path."""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from ... import _lib
from ..._lib import check

S_FM, S_ADV_FAKE, S_FAKE, S_ADV_REAL, S_COUNT = range(5)        # columns of fv_disc_distance's sums


def normed_conv(cin: int, cout: int, kernel, stride=1, padding=0) -> nn.Module:
    """``weight_norm(nn.Conv2d(...))`` as the reference builds it: a holder of ``bias`` and ``parametrizations.weight.original0 / original1``."""
    return nn.utils.parametrizations.weight_norm(nn.Conv2d(cin, cout, kernel, stride, padding=padding))


def refuse_spectral_norm(who: str, use_spectral_norm: bool) -> None:
    if use_spectral_norm:
        raise ValueError(f"{who}: use_spectral_norm = True is not supported: only the weight-norm form has kernels")


_LEGACY = {".weight_g": ".parametrizations.weight.original0", ".weight_v": ".parametrizations.weight.original1"}


class _DiscEngine:
    """One finalized ``fv_disc`` handle on one device."""

    def __init__(self, cfg: "_lib.DiscConfig", state_dict, device: torch.device):
        self.device, self._h = device, ctypes.c_void_p()
        L = _lib.lib()
        check(L.fv_disc_create(ctypes.byref(cfg), ctypes.byref(self._h)))
        try:
            with torch.cuda.device(device):
                for name, t in state_dict.items():
                    host = t.detach().to("cpu", torch.float32).contiguous()
                    shape = (ctypes.c_int64 * max(host.dim(), 1))(*host.shape)
                    check(L.fv_disc_load_weight(self._h, name.encode(), ctypes.cast(host.data_ptr(), ctypes.POINTER(ctypes.c_float)), shape, host.dim()))
                check(L.fv_disc_finalize(self._h))
        except Exception:
            self.close()
            raise
        self.n_maps = ctypes.c_int32()
        L.fv_disc_layout(self._h, 0, 0, None, 0, ctypes.byref(self.n_maps))

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def layout(self, batch: int, T: int):
        """(floats of the output buffer, the maps in (sub, layer) order)."""
        maps = (_lib.DiscMap * self.n_maps.value)()
        total = int(_lib.lib().fv_disc_layout(self._h, batch, T, maps, self.n_maps.value, None))
        if total < 0:
            raise ValueError(_lib.lib().fv_last_error().decode("utf-8", "replace"))
        return total, list(maps)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            if torch.cuda.is_available():
                torch.cuda.synchronize(self.device)     # kernels that read the weights may still be running
            _lib.lib().fv_disc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Critic(nn.Module):
    """Base of the four drop-ins.  A subclass sets ``_multi`` (a ``discriminators`` list, or one discriminator that is its own list),
    builds its holders, and answers ``_disc_config()`` and ``_sub_extents(i, L)``."""
    _multi = True

    def _init_critic(self) -> None:
        self._disc_config(validate=True)        # the library's limits, by name
        for p in self.parameters():
            p.requires_grad = False
        object.__setattr__(self, "_engine", None)
        self._register_load_state_dict_pre_hook(self._legacy_keys)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_engine())
        self.eval()

    def _legacy_keys(self, state_dict, prefix, *_):
        for key in [k for k in state_dict if k.startswith(prefix)]:
            for old, new in _LEGACY.items():
                if key.endswith(old) and key[: -len(old)] + new not in state_dict:
                    state_dict[key[: -len(old)] + new] = state_dict.pop(key)

    def _subs(self) -> list:
        return list(self.discriminators) if self._multi else [self]

    def _validated(self, cfg: "_lib.DiscConfig", validate: bool) -> "_lib.DiscConfig":
        if validate:
            h, L = ctypes.c_void_p(), _lib.lib()
            if L.fv_disc_create(ctypes.byref(cfg), ctypes.byref(h)) != 0:
                raise ValueError(L.fv_last_error().decode("utf-8", "replace"))
            L.fv_disc_destroy(h)
        return cfg

    # -- shapes ------------------------------------------------------------------------------------
    def extents(self, L: int):
        """(H, W) of every layer's feature map for a row of ``L`` samples, conv_post's score map last: per sub-discriminator for the
        multi modules, one list for a single discriminator."""
        ext = [self._sub_extents(i, int(L)) for i in range(len(self._subs()))]
        return ext if self._multi else ext[0]

    @property
    def precision(self) -> str:
        return "f32"

    @precision.setter
    def precision(self, value: str) -> None:
        if value != "f32":
            raise ValueError(f"{type(self).__name__} is fp32 only: there is no {value!r} form of the critics' kernels")

    # -- engine cache ------------------------------------------------------------------------------
    def invalidate_engine(self) -> None:
        eng = self.__dict__.get("_engine")
        if eng is not None:
            eng.close()
        object.__setattr__(self, "_engine", None)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_engine()
        return super()._apply(fn, *args, **kwargs)

    def engine(self, device: torch.device) -> _DiscEngine:
        eng = self.__dict__.get("_engine")
        if eng is None or eng.device != device:
            self.invalidate_engine()
            sd = self.state_dict()
            if not self._multi:
                sd = {"discriminators.0." + k: v for k, v in sd.items()}
            eng = _DiscEngine(self._disc_config(), sd, device)
            object.__setattr__(self, "_engine", eng)
        return eng

    # -- calls -------------------------------------------------------------------------------------
    def _waves(self, x, lengths, what: str):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError(f"{what} needs a CUDA/HIP tensor (got {getattr(x, 'device', type(x))}); vocoder_amd has no CPU path — move the "
                               "module and input to the GPU")
        if self.training:
            raise RuntimeError(f"{type(self).__name__} is inference-only: call .eval() first")
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"{what}: expected (B, 1, T), got {tuple(x.shape)}")
        x = x.detach().to(torch.float32)[:, 0].contiguous()
        B, T = (int(v) for v in x.shape)
        if lengths is not None:
            lengths = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
            if len(lengths) != B:
                raise ValueError(f"{what}: {len(lengths)} lengths for {B} rows")
        return x, lengths, B, T

    def run(self, x: torch.Tensor, lengths=None, what: str = "forward"):
        """The raw call: ``x`` (B, 1, T) -> (the channel-last output buffer, its ``fv_disc_map`` entries in (sub, layer) order)."""
        what = f"{type(self).__name__}.{what}"
        x, lengths, B, T = self._waves(x, lengths, what)
        eng, L = self.engine(x.device), _lib.lib()
        total, maps = eng.layout(B, T)
        out = torch.empty(max(total, 4), dtype=torch.float32, device=x.device)
        if B:
            with torch.cuda.device(x.device):
                need = int(L.fv_disc_workspace_bytes(eng.handle, B, T))
                ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
                lptr = None if lengths is None else (ctypes.c_int32 * B)(*lengths)
                check(L.fv_disc_forward(eng.handle, x.data_ptr(), T, lptr, B, out.data_ptr(), total, ws.data_ptr(), need,
                                        int(torch.cuda.current_stream().cuda_stream)))
        return out, maps

    def _nest(self, out: torch.Tensor, maps, B: int):
        """The buffer as the reference's (scores per sub-discriminator, feature maps per sub-discriminator and layer): (B, C, H, W) views."""
        n_sub = len(self._subs())
        nl = len(maps) // n_sub
        scores, fmaps = [], []
        for i in range(n_sub):
            fm = []
            for m in maps[i * nl: (i + 1) * nl]:
                fm.append(out[m.offset: m.offset + B * m.H * m.W * m.C].view(B, m.H, m.W, m.C).permute(0, 3, 1, 2))
            fmaps.append(fm)
            scores.append(fm[-1].reshape(B, -1))
        return scores, fmaps

    def _shape_result(self, scores, fmaps):
        if not self._multi:
            return scores[0], fmaps[0]
        return scores, fmaps

    def forward(self, x: torch.Tensor, lengths=None):
        """``x``: (B, 1, T) -> (scores, feature_map) in the reference's nesting; feature maps are (B, C, H, W) views of the channel-last
        buffer.  With ``lengths`` every row runs at its own extent and holds exact zeros past it."""
        out, maps = self.run(x, lengths)
        return self._shape_result(*self._nest(out, maps, int(x.shape[0])))

    def forward_list(self, waves) -> list:
        """A list of 1-d waves -> per wave what ``forward(wave[None, None])`` gives, through one padded call."""
        waves = list(waves)
        if not waves:
            return []
        for w in waves:
            if not isinstance(w, torch.Tensor) or w.dim() != 1:
                raise ValueError(f"{type(self).__name__}.forward_list: expected 1-d tensors, got {tuple(getattr(w, 'shape', ()))}")
        lengths = [int(w.shape[0]) for w in waves]
        x = torch.zeros((len(waves), 1, max(max(lengths), 1)), dtype=torch.float32, device=waves[0].device)
        for b, w in enumerate(waves):
            x[b, 0, : lengths[b]] = w
        out, maps = self.run(x, lengths, "forward_list")
        _, fmaps = self._nest(out, maps, len(waves))
        results = []
        for b, n in enumerate(lengths):
            ext = [self._sub_extents(i, n) for i in range(len(fmaps))]
            fm = [[f[b: b + 1, :, :h, :w] for f, (h, w) in zip(fmaps[i], ext[i])] for i in range(len(fmaps))]
            results.append(self._shape_result([f[-1].reshape(1, -1) for f in fm], fm))
        return results

    def distance_sums(self, real: torch.Tensor, fake: torch.Tensor, lengths=None) -> torch.Tensor:
        """gan.py:149 / 155 / 204 as sums: ``real`` / ``fake`` (B, 1, T) -> (B, subs, layers, 5) float64 on the device, per row,
        sub-discriminator and layer ``sum |real - fake|``, ``sum (1 - fake)^2``, ``sum fake^2``, ``sum (real - 1)^2`` over the row's own
        extent and its element count (columns ``S_FM, S_ADV_FAKE, S_FAKE, S_ADV_REAL, S_COUNT``)."""
        what = f"{type(self).__name__}.distance_sums"
        if tuple(real.shape) != tuple(fake.shape):
            raise ValueError(f"{what}: real {tuple(real.shape)} and fake {tuple(fake.shape)} differ in shape")
        out_r, maps = self.run(real, lengths, "distance_sums")
        out_f, _ = self.run(fake, lengths, "distance_sums")
        _, lengths, B, T = self._waves(real, lengths, what)
        n_sub = len(self._subs())
        sums = torch.zeros((B, n_sub, len(maps) // n_sub, 5), dtype=torch.float64, device=real.device)
        if B:
            eng, L = self.engine(real.device), _lib.lib()
            with torch.cuda.device(real.device):
                need = int(L.fv_disc_workspace_bytes(eng.handle, B, T))
                ws = torch.empty(max(need, 16), dtype=torch.uint8, device=real.device)
                lptr = None if lengths is None else (ctypes.c_int32 * B)(*lengths)
                check(L.fv_disc_distance(eng.handle, out_r.data_ptr(), out_f.data_ptr(), T, lptr, B, sums.data_ptr(), ws.data_ptr(), need,
                                         int(torch.cuda.current_stream().cuda_stream)))
        return sums
