"""What every Python owner of a library handle shares: the tensor check in front of a call, the life cycle of one handle (``_Handle``), one
handle per device (``_DeviceHandles``), and the skeleton of a stream's push / flush (``_emit``)."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import FishVocError, check


def _require_cuda(x: torch.Tensor, what: str, device_error: type = RuntimeError, dtype_error: type = TypeError) -> None:
    """The engine's callers raise RuntimeError / TypeError; the resampler's and the pitch shift's pass ValueError for both."""
    if not x.is_cuda:
        raise device_error(
            f"{what}: expected a CUDA/HIP tensor on an MI355X, got device '{x.device}'. "
            "vocoder_amd runs only through its HIP kernels (no CPU fallback).")
    if x.dtype != torch.float32:
        raise dtype_error(f"{what}: expected float32, got {x.dtype}")


class _Handle:
    """Owner of one library handle ``_h``, with the name of its destroy function and the message of a call on a closed one; optionally a
    workspace tensor ``_ws`` and an event ``_done``, recorded after the last call that used either on the device."""
    _destroy = ""
    _closed = ""
    _h: "ctypes.c_void_p | None" = None            # class defaults: close() also serves an object whose __init__ raised half way
    _ws: "torch.Tensor | None" = None
    _done: "torch.cuda.Event | None" = None

    def _check_open(self) -> None:
        if not self._h.value:
            raise FishVocError(_lib.FV_ERR_STATE, self._closed)

    def _record_done(self, stream) -> None:
        if self._done is None:
            self._done = torch.cuda.Event()
        self._done.record(stream)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            if self._done is not None:
                self._done.synchronize()    # what the handle owns on the device and the workspace may still be in use there
            getattr(self._lib, self._destroy)(self._h)
            self._h = ctypes.c_void_p()
            self._ws = None

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceHandles:
    """One library handle per device index (an object's tables live on one device), made on first use and freed by ``close``."""

    def __init__(self, destroy: str):
        self._destroy, self._by_index = destroy, {}

    def get(self, device: torch.device, create) -> ctypes.c_void_p:
        """The handle of ``device``; ``create(ctypes.byref(handle)) -> fv_status`` makes it, under that device's guard."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        h = self._by_index.get(idx)
        if h is None:
            h = ctypes.c_void_p()
            with torch.cuda.device(idx):
                check(create(ctypes.byref(h)))
            self._by_index[idx] = h
        return h

    def close(self) -> None:
        for h in self._by_index.values():
            getattr(_lib.lib(), self._destroy)(h)
        self._by_index = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _emit(shape: tuple, k: int, device, enqueue, mismatch: str) -> torch.Tensor:
    """One push or flush of a stream whose Python rule says it emits ``k``: allocates ``out`` of ``shape``, runs
    ``enqueue(out's pointer or None when k == 0, a reference to the library's count)`` and compares the two counts (``mismatch`` is the
    message, with ``{got}`` and ``{k}``).  ``enqueue`` raises when the library refuses the call; the caller moves its counters after ``_emit``
    has returned, so a refused call leaves them as they were."""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    got = ctypes.c_int64(0)
    enqueue(out.data_ptr() if k else None, ctypes.byref(got))
    if got.value != k:
        raise RuntimeError(mismatch.format(got=got.value, k=k))
    return out
