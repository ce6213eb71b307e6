"""What every Python owner of a library handle shares: the tensor check in front of a call, the life cycle of one handle (``_Handle``), one
handle per device (``_DeviceHandles``), the skeleton of a sample pool's step (``_SamplePoolHandle`` and the plain functions it shares with
``engine.WavPool``), and the skeleton of a stream's push / flush (``_emit``)."""
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


def _gather(items, device, require, what: str, noun: str = "chunk of samples"):
    """A pool step's ``(session, 1-D tensor or None, end)`` tuples -> the integer items and the padded ``(count, longest)`` buffer (None: no
    samples).  ``require(x, what)`` is the caller's tensor check."""
    meta, rows = [], []
    for it in map(tuple, items):
        s, x, end = it[0], it[1], it[2] if len(it) > 2 else False
        if x is not None:
            require(x, what)
            if x.dim() != 1:
                raise ValueError(f"expected a 1-D {noun}, got {tuple(x.shape)}")
        rows.append(x)
        meta.append((int(s), 0 if x is None else int(x.shape[0]), bool(end)))
    longest = max((c for _, c, _ in meta), default=0)
    chunks = None
    if longest:
        chunks = torch.zeros((len(meta), longest), dtype=torch.float32, device=device)
        for i, x in enumerate(rows):
            if x is not None and x.shape[0]:
                chunks[i, :x.shape[0]] = x
    return meta, chunks


def _pool_items(items) -> tuple:
    """The ``(session, samples, end)`` integers of a ``step_padded`` -> (the items, the library's item array, room for its counts)."""
    items = [(int(s), int(c), bool(f)) for s, c, f in items]
    arr = (_lib.WavPoolItem * max(len(items), 1))(*[_lib.WavPoolItem(s, c, int(f)) for s, c, f in items])
    return items, arr, (ctypes.c_int64 * max(len(items), 1))()


def _pool_moved(counters, items, plan, got, mismatch: str) -> list:
    """After the library's step: its counts per item; the Python counters move as the library's did, and the two must agree (``mismatch`` is
    the message, with ``{emit}`` and ``{plan}``)."""
    emit = [int(got[i]) for i in range(len(items))]
    counters.commit(items, plan)
    if plan != emit:
        raise RuntimeError(mismatch.format(emit=emit, plan=plan))
    return emit


def _require_value(x: torch.Tensor, what: str) -> None:
    _require_cuda(x, what, ValueError, ValueError)


class _SamplePoolHandle(_Handle):
    """What the Python owners of a per-session sample pool share (csrc/sample_pool.h; ``fv_respool``, ``fv_pvpool``, ``fv_yinpool``,
    ``fv_oscpool``): the handle on one device, the library's counters, the padded chunk buffer of ``step``, the checks of ``step_padded``
    and its call on torch's current stream.  A pool names its entries (``_prefix``) and keeps its Python ``counters``, the slicing of
    ``step`` and the one library call of ``step_padded``."""
    _prefix = ""                      # "fv_respool": the library's entries are _prefix + "_create", "_received", ...
    _bound = "max_outputs"            # the most one item emits in one step: the attribute, and the library's getter _prefix + "_" + _bound
    _noun = "chunk of samples"
    _mismatch = ""                    # _pool_moved's message

    def __init__(self, parent, sessions: int, max_chunk: int, device=None):
        self._parent, self._lib = parent, _lib.lib()
        self.sessions, self.max_chunk = int(sessions), int(max_chunk)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._h = ctypes.c_void_p()
        self._entry = {name: getattr(self._lib, f"{self._prefix}_{name}") for name in ("received", "emitted", "pending", "reset")}
        with torch.cuda.device(self.device):
            check(getattr(self._lib, self._prefix + "_create")(parent._handle(self.device), self.sessions, self.max_chunk, ctypes.byref(self._h)))
        setattr(self, self._bound, int(getattr(self._lib, f"{self._prefix}_{self._bound}")(self._h)))
        self._what = type(self).__name__

    # -- counters (the library's own; host-side: reading them never synchronises) --
    def received(self, session: int) -> int:
        self._check_open()
        return int(self._entry["received"](self._h, int(session)))

    def emitted(self, session: int) -> int:
        self._check_open()
        return int(self._entry["emitted"](self._h, int(session)))

    def pending(self, session: int) -> int:
        """What an ``end`` of the session would emit now, as the library counts it."""
        self._check_open()
        return int(self._entry["pending"](self._h, int(session)))

    def _gather(self, items):
        self._check_open()
        return _gather(items, self.device, _require_value, self._what + ".step", self._noun)

    def _padded(self, items, chunks):
        """The checks of ``step_padded``'s inputs -> (items, the C item array, room for the counts, the chunk pointer, the chunk row stride)."""
        self._check_open()
        items, arr, got = _pool_items(items)
        count, stride = len(items), 0
        if chunks is not None:
            _require_value(chunks, self._what + ".step_padded")
            if chunks.dim() != 2 or chunks.shape[0] < count or (chunks.shape[1] > 1 and chunks.stride(1) != 1):
                raise ValueError(f"expected chunks of shape ({count}, chunk_stride) with contiguous rows, got {tuple(chunks.shape)}")
            stride = int(chunks.stride(0)) if chunks.shape[0] > 1 else int(chunks.shape[1])
            if stride < chunks.shape[1]:
                raise ValueError("the rows of chunks overlap")
        return items, arr, got, chunks.data_ptr() if chunks is not None and chunks.numel() else None, stride

    def _out(self, out, lead: tuple, cols: int, shape: str) -> torch.Tensor:
        """``out`` of shape ``lead + (out_cols,)``, made with ``cols`` columns when not given; ``shape`` names it in the refusal."""
        if out is None:
            return torch.empty(lead + (cols,), dtype=torch.float32, device=self.device)
        _require_value(out, self._what + ".step_padded")
        if out.dim() != len(lead) + 1 or tuple(out.shape[:-1]) != lead or not out.is_contiguous():
            raise ValueError(f"expected a contiguous out of shape {shape}, got {tuple(out.shape)}")
        return out

    def _run(self, call) -> None:
        """``call(stream) -> fv_status``, the library's step, on torch's current stream of the pool's device."""
        with torch.cuda.device(self.device):
            run = torch.cuda.current_stream()
            check(call(int(run.cuda_stream)))
            self._record_done(run)          # what the pool carries on the device (and its workspace) is in use until then

    def _moved(self, items, plan, got) -> list:
        return _pool_moved(self.counters, items, plan, got, self._mismatch)

    def reset(self, session: int) -> None:
        """Start the next utterance in one slot: its counters go to 0; what it carries is kept."""
        self._check_open()
        check(self._entry["reset"](self._h, int(session)))
        self.counters.reset(int(session))


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
