"""Drop-ins for the quantisers of the reference's ``VQVAEModel`` (vae.py:66-78): encodec's ``VectorQuantization`` and
``ResidualVectorQuantization`` (``encodec.quantization.core_vq``), inference only, on the ``fv_vq_*`` kernels (include/fishvoc.h).

Buffers carry encodec's names, so a ``VQVAEModel`` checkpoint's ``vq.*`` keys load strictly: ``_codebook.inited``, ``_codebook.cluster_size``,
``_codebook.embed``, ``_codebook.embed_avg`` and ``layers.{i}._codebook.*`` for the residual form.  Only ``embed`` is read.  The arithmetic is
restated from encodec's specification (the package is not a dependency, so parity with it is unpinned)::

    search(x, embed) = argmax_j (x . e_j - |e_j|^2 / 2)      lowest index on equal scores; a NaN score never wins, all NaN -> code 0
    r_0 = x;  c_q = search(r_q, embed_q);  r_{q+1} = r_q - e_{c_q};  z = ((e_{c_0} + e_{c_1}) + ...)

A frame's scores are formed in an order that depends on ``dim`` alone: its codes and ``z`` have the same bits alone, in any batch and under
any chunking along T, so a decode streams: ``module.code_stream(vq, ...)`` / ``code_pool`` keep the codes in the ring and return the bits of
``module.stream().push(vq.from_codes(codes[..., a:b])[0])`` (``VQVAECodec.decode_stream`` / ``decode_pool``).  Not built: EMA updates, k-means init,
dead-code expiry, the straight-through estimator, the commitment loss (returned as zeros) and ``project_in`` / ``project_out``
(``codebook_dim != dim`` is refused).  No CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch
from torch import nn

from .. import _lib
from .._handle import _require_cuda
from .._lib import check

MAX_DIM, MAX_CODEBOOK_SIZE, MAX_QUANTIZERS = 4096, 65536, 32     # include/fishvoc.h, fv_vq_create


class VQResult(NamedTuple):
    """Unpacks as encodec's ``(quantize, codes, loss)`` (vae.py:82) and serves unify.py:22-23,41 through ``.z`` / ``.codes``."""
    z: torch.Tensor
    codes: torch.Tensor
    loss: torch.Tensor


class _VQEngine:
    """One ``fv_vq`` handle on one device with its codebooks loaded."""

    def __init__(self, dim: int, codebook_size: int, embeds, device: torch.device):
        self.device, self._h = device, ctypes.c_void_p()
        L = _lib.lib()
        check(L.fv_vq_create(ctypes.byref(_lib.VQConfig(dim, codebook_size, len(embeds))), ctypes.byref(self._h)))
        try:
            with torch.cuda.device(device):
                for q, e in enumerate(embeds):
                    host = e.detach().to("cpu", torch.float32).contiguous()
                    check(L.fv_vq_load_codebook(self._h, q, ctypes.cast(host.data_ptr(), ctypes.POINTER(ctypes.c_float))))
        except Exception:
            self.close()
            raise

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def close(self) -> None:
        if self._h is not None and self._h.value:
            torch.cuda.synchronize(self.device)     # kernels that read the codebooks may still be running
            _lib.lib().fv_vq_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EuclideanCodebook(nn.Module):
    """Holder of encodec's codebook buffers (``core_vq.EuclideanCodebook``); never called."""

    def __init__(self, dim: int, codebook_size: int, kmeans_init: bool = False):
        super().__init__()
        embed = torch.randn(codebook_size, dim) if not kmeans_init else torch.zeros(codebook_size, dim)   # encodec: kaiming uniform; any init is overwritten by a checkpoint
        self.register_buffer("inited", torch.Tensor([not kmeans_init]))
        self.register_buffer("cluster_size", torch.zeros(codebook_size))
        self.register_buffer("embed", embed)
        self.register_buffer("embed_avg", embed.clone())


class _Quantizer(nn.Module):
    """What the two forms share: the lazily built engine (as ``EngineModule`` keeps its own) and the calls into it."""

    def __init__(self, dim: int, codebook_size: int, num_quantizers: int):
        super().__init__()
        self.dim, self.codebook_size, self.num_quantizers = int(dim), int(codebook_size), int(num_quantizers)
        if not 1 <= self.dim <= MAX_DIM:
            raise ValueError(f"dim ({self.dim}) must lie in [1, {MAX_DIM}]")
        if not 1 <= self.codebook_size <= MAX_CODEBOOK_SIZE:
            raise ValueError(f"codebook_size ({self.codebook_size}) must lie in [1, {MAX_CODEBOOK_SIZE}]")
        if not 1 <= self.num_quantizers <= MAX_QUANTIZERS:
            raise ValueError(f"num_quantizers ({self.num_quantizers}) must lie in [1, {MAX_QUANTIZERS}]")
        object.__setattr__(self, "_engine", None)
        object.__setattr__(self, "_slices", 0)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_engine())

    def _embeds(self):  # pragma: no cover - abstract
        raise NotImplementedError

    def invalidate_engine(self) -> None:
        eng = self.__dict__.get("_engine")
        if eng is not None:
            eng.close()
        object.__setattr__(self, "_engine", None)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_engine()
        return super()._apply(fn, *args, **kwargs)

    def engine(self, device: torch.device) -> _VQEngine:
        eng = self.__dict__.get("_engine")
        if eng is None or eng.device != device:
            self.invalidate_engine()
            eng = _VQEngine(self.dim, self.codebook_size, self._embeds(), device)
            if self._slices:
                check(_lib.lib().fv_vq_set_slices(eng.handle, self._slices))
            object.__setattr__(self, "_engine", eng)
        return eng

    @property
    def slices(self) -> int:
        """Codebook slices of the search's grid, 0 = by launch size.  Results do not depend on it (the tests hold it to that)."""
        return self.__dict__.get("_slices", 0)

    @slices.setter
    def slices(self, value: int) -> None:
        if int(value) < 0:
            raise ValueError(f"slices ({value}) must be >= 0")
        object.__setattr__(self, "_slices", int(value))
        eng = self.__dict__.get("_engine")
        if eng is not None:
            check(_lib.lib().fv_vq_set_slices(eng.handle, int(value)))

    # -- calls -----------------------------------------------------------------------------
    def _check(self, what: str) -> None:
        if self.training:
            raise RuntimeError(f"{type(self).__name__} is inference-only: call .eval() first")

    @staticmethod
    def _host_frames(lengths, B: int, T: int, what: str):
        if lengths is None:
            return None
        host = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(host) != B:
            raise ValueError(f"{what}: {len(host)} lengths for {B} rows")
        for b, v in enumerate(host):
            if not 0 <= v <= T:
                raise ValueError(f"{what}: lengths[{b}] = {v} lies outside [0, T = {T}]")
        return (ctypes.c_int32 * max(B, 1))(*host)

    def _encode(self, x: torch.Tensor, lengths, want_z: bool, what: str):
        self._check(what)
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{what}: expected a tensor, got {type(x).__name__}")
        _require_cuda(x, what)
        if x.dim() != 3 or x.shape[1] != self.dim:
            raise ValueError(f"{what}: expected (B, {self.dim}, T), got {tuple(x.shape)}")
        B, D, T = (int(v) for v in x.shape)
        x = x.detach()
        # a slice along T of a contiguous tensor passes as it is (fv_vq_encode's x_row_stride)
        if T and B and not (x.stride(2) == 1 and x.stride(1) >= T and (B == 1 or x.stride(0) == D * x.stride(1))):
            x = x.contiguous()
        fptr = self._host_frames(lengths, B, T, what)
        codes = torch.empty((self.num_quantizers, B, T), dtype=torch.int32, device=x.device)
        z = torch.empty((B, D, T), dtype=torch.float32, device=x.device) if want_z else None
        if B and T:
            eng, lib = self.engine(x.device), _lib.lib()
            with torch.cuda.device(x.device):
                need = int(lib.fv_vq_workspace_bytes(eng.handle, B, T))
                ws = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
                check(lib.fv_vq_encode(eng.handle, x.data_ptr(), x.stride(1), fptr, codes.data_ptr(), None if z is None else z.data_ptr(), B, T,
                                       ws.data_ptr(), need, int(torch.cuda.current_stream().cuda_stream)))
        return z, codes.to(torch.int64)

    def _decode(self, codes: torch.Tensor, lengths, what: str) -> torch.Tensor:
        self._check(what)
        if not isinstance(codes, torch.Tensor) or not codes.is_cuda:
            raise RuntimeError(f"{what}: expected codes on a HIP device; vocoder_amd has no CPU path")
        if codes.dtype not in (torch.int64, torch.int32):
            raise TypeError(f"{what}: expected int64 or int32 codes, got {codes.dtype}")
        if codes.dim() == 2:
            codes = codes[None]
        if codes.dim() != 3 or not 1 <= codes.shape[0] <= self.num_quantizers:
            raise ValueError(f"{what}: expected codes of shape (B, T) or (n_q <= {self.num_quantizers}, B, T), got {tuple(codes.shape)}")
        nq, B, T = (int(v) for v in codes.shape)
        z = torch.empty((B, self.dim, T), dtype=torch.float32, device=codes.device)
        if not (B and T):
            return z
        if int(codes.max()) >= self.codebook_size:      # the one host check, as nn.Embedding raises
            raise IndexError(f"{what}: code {int(codes.max())} is out of range for a codebook of {self.codebook_size}")
        c32 = torch.full((self.num_quantizers, B, T), -1, dtype=torch.int32, device=codes.device)
        c32[:nq] = codes
        fptr = self._host_frames(lengths, B, T, what)
        eng = self.engine(codes.device)
        with torch.cuda.device(codes.device):
            check(_lib.lib().fv_vq_decode(eng.handle, c32.data_ptr(), fptr, z.data_ptr(), B, T, int(torch.cuda.current_stream().cuda_stream)))
        return z

    def _shape_codes(self, codes: torch.Tensor) -> torch.Tensor:
        return codes[0] if self.num_quantizers == 1 and type(self) is VectorQuantization else codes

    def _loss(self, device) -> torch.Tensor:
        raise NotImplementedError

    def forward(self, x: torch.Tensor, lengths=None) -> VQResult:
        """``x (B, D, T)`` -> ``VQResult(z (B, D, T), codes int64, loss zeros)``; with ``lengths``, frames at or past ``lengths[b]`` are
        never read, get code -1 and exact zeros in ``z``."""
        z, codes = self._encode(x, lengths, True, f"{type(self).__name__}.forward")
        return VQResult(z, self._shape_codes(codes), self._loss(x.device))

    def encode(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        return self._shape_codes(self._encode(x, lengths, False, f"{type(self).__name__}.encode")[1])

    def decode(self, codes: torch.Tensor, lengths=None) -> torch.Tensor:
        return self._decode(codes, lengths, f"{type(self).__name__}.decode")

    def from_codes(self, codes: torch.Tensor):
        """``(z, codes)``: what unify.py:47 indexes with ``[0]``."""
        return self._decode(codes, None, f"{type(self).__name__}.from_codes"), codes

    def extra_repr(self) -> str:
        return f"dim={self.dim}, codebook_size={self.codebook_size}, num_quantizers={self.num_quantizers}, backend=libfishvoc_hip (gfx950)"


class VectorQuantization(_Quantizer):
    """encodec's ``VectorQuantization(dim, codebook_size, codebook_dim=None, decay, epsilon, kmeans_init, kmeans_iters,
    threshold_ema_dead_code, commitment_weight)``; the training knobs are recorded and unused.  ``codes`` is ``(B, T)``."""

    def __init__(self, dim: int, codebook_size: int, codebook_dim: int | None = None, decay: float = 0.99, epsilon: float = 1e-5,
                 kmeans_init: bool = True, kmeans_iters: int = 50, threshold_ema_dead_code: int = 2, commitment_weight: float = 1.0):
        if codebook_dim is not None and int(codebook_dim) != int(dim):
            raise ValueError(f"codebook_dim ({codebook_dim}) != dim ({dim}): the project_in / project_out Linear layers are out of scope")
        super().__init__(dim, codebook_size, 1)
        self.training_kwargs = dict(decay=decay, epsilon=epsilon, kmeans_init=kmeans_init, kmeans_iters=kmeans_iters,
                                    threshold_ema_dead_code=threshold_ema_dead_code, commitment_weight=commitment_weight)
        self._codebook = EuclideanCodebook(self.dim, self.codebook_size, kmeans_init=kmeans_init)

    def _embeds(self):
        return [self._codebook.embed]

    def _loss(self, device) -> torch.Tensor:
        return torch.zeros(1, device=device)


class ResidualVectorQuantization(_Quantizer):
    """encodec's ``ResidualVectorQuantization(*, num_quantizers, **kwargs)``: ``layers.{i}`` are ``VectorQuantization`` holders and the
    whole cascade runs on one engine.  ``codes`` is ``(n_q, B, T)``, ``loss`` zeros ``(n_q, 1)``.  ``decode`` takes the first
    ``n <= n_q`` layers of codes."""

    def __init__(self, *, num_quantizers: int, **kwargs):
        layers = [VectorQuantization(**kwargs) for _ in range(int(num_quantizers))] if 1 <= int(num_quantizers) <= MAX_QUANTIZERS else []
        dim, codebook_size = kwargs.get("dim"), kwargs.get("codebook_size")
        super().__init__(dim, codebook_size, num_quantizers)
        self.layers = nn.ModuleList(layers)

    def _embeds(self):
        return [layer._codebook.embed for layer in self.layers]

    def _loss(self, device) -> torch.Tensor:
        return torch.zeros(self.num_quantizers, 1, device=device)
