"""Drop-in for the reference's ``PosteriorEncoder`` (fish_vocoder/modules/encoders/posterior_encoder.py:91-163), the WaveNet encoder of
VITS / RVC, in eval mode on the ``fv_posterior_*`` kernels (include/fishvoc.h, vocoder_amd/csrc/wavenet.hip).

Parameters are ordinary torch parameters under the reference's keys and order — ``pre.{weight,bias}``, ``enc.in_layers.{i}.{bias,weight_g,
weight_v}``, ``enc.res_skip_layers.{i}.{bias,weight_g,weight_v}`` (the old ``nn.utils.weight_norm(name="weight")`` naming), ``proj.{weight,
bias}`` and, for ``mode="bnvae"``, ``mu_bn.*`` — so a checkpoint loads strictly; the holders are never called.  ``forward(x, x_lengths)``
returns what the reference's eval forward returns: ``y`` for ``"vqvae"``, ``(z, mean, logvar, x_mask)`` for ``"vae"`` / ``"bnvae"``.  A row has
the same bits alone, in any batch and padded to any T; frames at or past a row's length, and the padding of ``x``, are never read.
``stream(batch, max_chunk_frames)`` is the encoder chunk by chunk (``PosteriorStream``, ``fv_wnstream_*``): the whole utterance's bits under
any chunking, ``reach_frames`` frames behind the input; ``pool(sessions, max_chunk_frames)`` is the same for sessions that advance
independently (``PosteriorPool``, ``fv_wnpool_*``).  Not built: the training-mode draw, dropout, f16x3.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import weakref

import torch
from torch import nn

from ... import _lib
from ..._handle import _Handle, _pool_items, _pool_moved
from ..._lib import check
from ...sample_pool import SamplePoolCounters

_MSG_INFERENCE = "{} is inference-only: call .eval() first"
_MSG_DEVICE = ("{} needs a CUDA/HIP tensor (got {}); vocoder_amd has no CPU path — move the model and "
               "input to the GPU")


def schedule(chunks, R: int) -> list:
    """The frames a stream of reach ``R`` emits: ``(E, E')`` for every push of ``chunks`` (frame counts, zeros allowed) — the push emits the
    frames ``[E, E')``, ``E' = max(E, N - R)`` — and last ``(E, N)`` for the flush."""
    out, N, E = [], 0, 0
    for c in chunks:
        N += int(c)
        E2 = max(E, N - int(R))
        out.append((E, E2))
        E = E2
    out.append((E, N))
    return out


class PosteriorPoolCounters(SamplePoolCounters):
    """The host counters of a posterior pool and the plan of ``fv_wnpool_plan`` in plain Python: ``schedule``'s rule per session.  An item
    ``(session, frames, flush)`` takes its slot to ``N' = N + frames`` and ``E' = N' if flush else max(E, N' - R)`` and emits ``[E, E')``;
    ``plan(items)`` gives ``E' - E`` per item and refuses what the library refuses (``SamplePoolCounters``), counting frames."""
    _unit, _chunk_limit, _chunk_limit_name, _length_limit, _length_limit_name = "frames", 1 << 20, "2^20", 1 << 30, "2^30"

    def __init__(self, reach: int, sessions: int, max_chunk: int):
        super().__init__(sessions, max_chunk)
        self.R = int(reach)
        self.max_frames = self.max_chunk + self.R        # a flush with max_chunk frames after R pending ones

    def _emission(self, i: int, s: int, c: int, flush: bool, N2: int, E: int) -> int:
        return N2 if flush else max(E, N2 - self.R)

    def pending(self, session: int) -> int:
        return self.received[session] - self.emitted[session]


class _PosteriorEngine:
    """One finalized ``fv_posterior`` handle on one device."""

    def __init__(self, cfg: "_lib.PosteriorConfig", state_dict, device: torch.device):
        self.device, self._h = device, ctypes.c_void_p()
        self._streams: weakref.WeakSet = weakref.WeakSet()      # live PosteriorStreams: closed before the handle is destroyed
        L = _lib.lib()
        check(L.fv_posterior_create(ctypes.byref(cfg), ctypes.byref(self._h)))
        try:
            with torch.cuda.device(device):
                for name, t in state_dict.items():
                    host = t.detach().to("cpu", torch.float32).contiguous()
                    shape = (ctypes.c_int64 * max(host.dim(), 1))(*host.shape)
                    check(L.fv_posterior_load_weight(self._h, name.encode(), ctypes.cast(host.data_ptr(), ctypes.POINTER(ctypes.c_float)),
                                                     shape, host.dim()))
                check(L.fv_posterior_finalize(self._h))
        except Exception:
            self.close()
            raise

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def close(self) -> None:
        for st in list(getattr(self, "_streams", ())):
            st.close()
        if self._h is not None and self._h.value:
            if torch.cuda.is_available():
                torch.cuda.synchronize(self.device)     # kernels that read the weights may still be running
            _lib.lib().fv_posterior_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PosteriorStream(_Handle):
    """``PosteriorEncoder`` chunk by chunk (``fv_wnstream_*``, include/fishvoc.h): ``push`` a ``(B, in_channels, c)`` chunk, ``c <=
    max_chunk_frames``, and get what ``forward`` returns for the frames that need no later input — ``[E, max(E, N - R))``, ``R =
    lookahead_frames``, possibly none; ``flush`` ends the utterance at ``N`` and returns the rest, then pushes raise until ``reset()``.  The
    concatenation has the bits of ``forward`` over the whole utterance under any chunking (``schedule`` gives the counts).  The ``batch`` rows
    advance in lockstep.  A stream dies with the module's engine: ``load_state_dict`` or ``.to()`` closes it, create a new one then."""
    _destroy = "fv_wnstream_destroy"
    _closed = ("this posterior stream is closed (its engine was closed or rebuilt — e.g. load_state_dict or .to() on "
               "the module): create a new stream")

    def __init__(self, module: "PosteriorEncoder", engine: _PosteriorEngine, batch: int, max_chunk_frames: int):
        self._lib, self._h = _lib.lib(), ctypes.c_void_p()
        self._module, self._engine = module, engine
        with torch.cuda.device(engine.device):
            check(self._lib.fv_wnstream_create(engine.handle, int(batch), int(max_chunk_frames), ctypes.byref(self._h)))
        engine._streams.add(self)
        self.batch, self.max_chunk_frames = int(batch), int(max_chunk_frames)
        self.in_channels, self.out_channels = module.in_channels, module.out_channels
        self._R = int(self._lib.fv_wnstream_lookahead(self._h))
        self._N = self._E = 0
        self._flushed = False
        self._last_stream = None

    # -- counters (host-side: reading them never synchronises) --
    @property
    def received_frames(self) -> int:
        return self._N

    @property
    def emitted_frames(self) -> int:
        return self._E

    @property
    def pending_frames(self) -> int:
        """Frames received and not yet emitted, as the library counts them (``fv_wnstream_pending``)."""
        self._check_open()
        return int(self._lib.fv_wnstream_pending(self._h))

    @property
    def lookahead_frames(self) -> int:
        return self._R

    def push(self, x: torch.Tensor):
        self._check_open()
        what = f"{type(self).__name__}.push"
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError(_MSG_DEVICE.format(what, getattr(x, "device", type(x))))
        if x.dim() != 3 or x.shape[0] != self.batch or x.shape[1] != self.in_channels:
            raise ValueError(f"{what}: expected ({self.batch}, {self.in_channels}, c), got {tuple(x.shape)}")
        x = x.detach().to(torch.float32)
        c = int(x.shape[2])
        # a slice along T passes as it is (fv_wnstream_push's strides)
        if c and not ((c == 1 or x.stride(2) == 1) and x.stride(1) >= c and x.stride(0) >= 0):
            x = x.contiguous()
        return self._call(x, c, flush=False)

    def flush(self):
        """The frames ``[E, N)`` against the utterance's end; pushes raise afterwards until ``reset()``."""
        self._check_open()
        return self._call(None, 0, flush=True)

    def _call(self, x, c: int, flush: bool):
        m, dev = self._module, self._engine.device
        if m.training:
            raise RuntimeError(_MSG_INFERENCE.format(type(m).__name__))
        if x is not None and x.device != dev:
            raise RuntimeError(f"{type(self).__name__}.push: the chunk is on {x.device}, the stream on {dev}")
        refused = self._flushed or c > self.max_chunk_frames      # a refused call emits nothing; the library says why
        k = 0 if refused else (self._N - self._E if flush else max(self._E, self._N + c - self._R) - self._E)
        vae = m.mode != "vqvae"
        new = lambda: torch.empty((self.batch, self.out_channels, k), dtype=torch.float32, device=dev)      # noqa: E731
        z, mean, logvar = new(), (new() if vae else None), (new() if vae else None)
        ptr = lambda t: t.data_ptr() if t is not None and k else None      # noqa: E731
        got = ctypes.c_int64(0)
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            if self._done is not None and self._last_stream != cur.cuda_stream:
                cur.wait_event(self._done)       # the rings are the stream's own: order after the previous call when it ran on another stream
            tail = (ptr(z), ptr(mean), ptr(logvar), max(k, 1), ctypes.byref(got), int(cur.cuda_stream))
            if flush:
                check(self._lib.fv_wnstream_flush(self._h, *tail))
            else:
                check(self._lib.fv_wnstream_push(self._h, x.data_ptr() if c else None, x.stride(0) if c else 0, x.stride(1) if c else 0, c, *tail))
            self._record_done(cur)
            self._last_stream = cur.cuda_stream
        if got.value != k:
            raise RuntimeError(f"posterior stream emitted {got.value} frames where the rule says {k}")
        self._N += c
        self._E += k
        self._flushed = flush
        if not vae:
            return z
        return z, mean, logvar, torch.ones(self.batch, 1, k, dtype=torch.float32, device=dev)

    def reset(self) -> None:
        """Start the next utterance: N = E = 0; the rings are kept (nothing they hold is read again)."""
        self._check_open()
        check(self._lib.fv_wnstream_reset(self._h))
        self._N = self._E = 0
        self._flushed = False


class PosteriorPool(_Handle):
    """``PosteriorEncoder`` for sessions that advance independently (``fv_wnpool_*``, include/fishvoc.h): what ``PosteriorStream`` is to rows
    in lockstep, for ``sessions`` slots with their own counters.  ``step(items)`` takes ``(session, x, flush)`` tuples — ``x``: ``(in_channels,
    n)`` with ``n <= max_chunk_frames``, or ``None`` for no frames; ``flush``: the utterance ends with these frames — and returns per item what
    ``forward`` returns for the frames that session emits in this step: ``z (out_channels, k)``, or ``(z, mean, logvar, mask)``; ``k`` may be
    0.  A session appears at most once per step and refuses items after its flush until ``reset(session)``.  The whole step is checked before
    anything moves: a refused step leaves every session as it was.  A session's concatenated tensors have the bits of ``forward`` over its
    whole utterance, whatever the other sessions do.  One step is at most ``2 n_layers + 2`` launches per 128 items.  Work is enqueued on
    torch's current stream and calls must be ordered; the pool dies with the module's engine, as a ``PosteriorStream`` does."""
    _destroy = "fv_wnpool_destroy"
    _closed = ("this posterior pool is closed (its engine was closed or rebuilt — e.g. load_state_dict or .to() on "
               "the module): create a new pool")

    def __init__(self, module: "PosteriorEncoder", engine: _PosteriorEngine, sessions: int, max_chunk_frames: int):
        self._lib, self._h = _lib.lib(), ctypes.c_void_p()
        self._module, self._engine = module, engine
        with torch.cuda.device(engine.device):
            check(self._lib.fv_wnpool_create(engine.handle, int(sessions), int(max_chunk_frames), ctypes.byref(self._h)))
        engine._streams.add(self)
        self.sessions, self.max_chunk_frames = int(sessions), int(max_chunk_frames)
        self.in_channels, self.out_channels = module.in_channels, module.out_channels
        self.lookahead_frames = int(self._lib.fv_wnpool_lookahead(self._h))
        self.max_frames = int(self._lib.fv_wnpool_max_frames(self._h))
        self.counters = PosteriorPoolCounters(self.lookahead_frames, self.sessions, self.max_chunk_frames)
        self._last_stream = None

    # -- counters (host-side: reading them never synchronises) --
    def received_frames(self, session: int) -> int:
        return self.counters.received[session]

    def emitted_frames(self, session: int) -> int:
        return self.counters.emitted[session]

    def pending_frames(self, session: int) -> int:
        """Frames one session has received and not yet emitted, as the library counts them (``fv_wnpool_pending``)."""
        self._check_open()
        return int(self._lib.fv_wnpool_pending(self._h, int(session)))

    @property
    def last_step_launches(self) -> int:
        """The kernel launches the last accepted step enqueued (``fv_wnpool_launches``)."""
        self._check_open()
        return int(self._lib.fv_wnpool_launches(self._h))

    def step(self, items) -> list:
        """One step for ``items`` (see the class); returns each item's tensors, views of the step's output buffers."""
        self._check_open()
        what = f"{type(self).__name__}.step"
        meta, rows = [], []
        for it in map(tuple, items):
            s, x, flush = it[0], it[1], it[2] if len(it) > 2 else False
            if x is not None:
                if not isinstance(x, torch.Tensor) or not x.is_cuda:
                    raise RuntimeError(_MSG_DEVICE.format(what, getattr(x, "device", type(x))))
                if x.dim() != 2 or x.shape[0] != self.in_channels:
                    raise ValueError(f"{what}: expected ({self.in_channels}, n) or None, got {tuple(x.shape)}")
            rows.append(x)
            meta.append((int(s), 0 if x is None else int(x.shape[1]), bool(flush)))
        longest = max((c for _, c, _ in meta), default=0)
        chunks = None
        if longest:
            chunks = torch.zeros((len(meta), self.in_channels, longest), dtype=torch.float32, device=self._engine.device)
            for i, x in enumerate(rows):
                if x is not None and x.shape[1]:
                    chunks[i, :, :x.shape[1]] = x
        out, emit = self.step_padded(meta, chunks)
        if self._module.mode == "vqvae":
            return [out[i, :, :k] for i, k in enumerate(emit)]
        return [tuple(t[i, :, :k] for t in out) + (torch.ones(1, k, dtype=torch.float32, device=self._engine.device),) for i, k in enumerate(emit)]

    def step_padded(self, items, chunks: "torch.Tensor | None", out=None) -> tuple:
        """The step on the caller's padded buffers, as ``fv_wnpool_step`` takes them: ``items``: ``(session, frames, flush)`` integers;
        ``chunks``: ``(count, in_channels, stride)`` with item i's frames first in row i (the rest, NaN included, is never read) — the output
        of ``WavPool.step_padded`` passes as it is — or ``None`` when no item has frames; ``out``: ``z``, or ``(z, mean, logvar)`` in the vae
        modes, each contiguous ``(count, out_channels, out_cols)``, sized from the Python plan when not given.  Returns ``(out, frames emitted
        per item)``: row i holds item i's frames first and zeros after them."""
        self._check_open()
        m, dev, what = self._module, self._engine.device, f"{type(self).__name__}.step_padded"
        if m.training:
            raise RuntimeError(_MSG_INFERENCE.format(type(m).__name__))
        items, arr, got = _pool_items(items)
        count, xptr, istride, rstride = len(items), None, 0, 0
        if chunks is not None:
            if not isinstance(chunks, torch.Tensor) or not chunks.is_cuda:
                raise RuntimeError(_MSG_DEVICE.format(what, getattr(chunks, "device", type(chunks))))
            if chunks.device != dev:
                raise RuntimeError(f"{what}: the chunks are on {chunks.device}, the pool on {dev}")
            if chunks.dim() != 3 or chunks.shape[0] != count or chunks.shape[1] != self.in_channels or chunks.dtype != torch.float32:
                raise ValueError(f"{what}: expected float32 chunks of shape ({count}, {self.in_channels}, stride), got {tuple(chunks.shape)}")
            if chunks.numel() and not ((chunks.shape[2] == 1 or chunks.stride(2) == 1) and chunks.stride(1) >= chunks.shape[2] and chunks.stride(0) >= 0):
                chunks = chunks.contiguous()
            if chunks.numel():
                xptr, istride, rstride = chunks.data_ptr(), int(chunks.stride(0)), int(chunks.stride(1))
        plan = self.counters.plan(items)                          # sizes the output before anything is launched; refuses what the library would
        vae = m.mode != "vqvae"
        if out is None:
            new = lambda: torch.empty((count, self.out_channels, max(plan, default=0)), dtype=torch.float32, device=dev)      # noqa: E731
            outs = (new(), new(), new()) if vae else (new(),)
        else:
            outs = tuple(out) if vae else (out,)
            ok = len(outs) == (3 if vae else 1) and all(
                isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.dim() == 3 and t.shape[:2] == (count, self.out_channels)
                and t.shape == outs[0].shape and t.is_contiguous() for t in outs)
            if not ok:
                raise ValueError(f"{what}: expected out as {'(z, mean, logvar), each ' if vae else ''}a contiguous float32 tensor of shape "
                                 f"({count}, {self.out_channels}, out_cols) on {dev}")
        cols = int(outs[0].shape[2])
        ptr = lambda t: t.data_ptr() if t.numel() else None      # noqa: E731
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            if self._done is not None and self._last_stream != cur.cuda_stream:
                cur.wait_event(self._done)       # the rings are the pool's own: order after the previous step when it ran on another stream
            check(self._lib.fv_wnpool_step(self._h, arr, count, xptr, istride, rstride, ptr(outs[0]), ptr(outs[1]) if vae else None,
                                           ptr(outs[2]) if vae else None, cols, got, int(cur.cuda_stream)))
            self._record_done(cur)
            self._last_stream = cur.cuda_stream
        emit = _pool_moved(self.counters, items, plan, got, "the posterior pool emitted {emit} frames where the rule says {plan}")
        return (outs if vae else outs[0]), emit

    def reset(self, session: int) -> None:
        """Start the next utterance in one slot: its counters go to 0; its ring rows are kept (nothing they hold is read again)."""
        self._check_open()
        check(self._lib.fv_wnpool_reset(self._h, int(session)))
        self.counters.reset(int(session))


class WaveNet(nn.Module):
    """Holder of the reference's ``enc.*`` parameters (posterior_encoder.py:11-55); never called."""

    def __init__(self, hidden_channels, kernel_size, dilation_rate, dilation_cycle, n_layers, p_dropout=0):
        super().__init__()
        self.in_layers = nn.ModuleList()
        self.res_skip_layers = nn.ModuleList()
        for i in range(n_layers):
            dilation = dilation_rate ** (i % dilation_cycle)
            padding = (kernel_size * dilation - dilation) // 2
            self.in_layers.append(nn.utils.weight_norm(
                nn.Conv1d(hidden_channels, 2 * hidden_channels, kernel_size, dilation=dilation, padding=padding), name="weight"))
            rows = 2 * hidden_channels if i < n_layers - 1 else hidden_channels
            self.res_skip_layers.append(nn.utils.weight_norm(nn.Conv1d(hidden_channels, rows, 1), name="weight"))


class PosteriorEncoder(nn.Module):
    takes_lengths = True       # codec.VQVAECodec.encode hands its lengths to such an encoder

    def __init__(self, in_channels, out_channels, hidden_channels, kernel_size=5, dilation_rate=1, dilation_cycle=1, n_layers=16, mode="vqvae"):
        super().__init__()
        if mode not in _lib.POSTERIOR_MODES:
            raise ValueError(f"mode must be one of {sorted(_lib.POSTERIOR_MODES)}, got {mode!r}")
        self.mode = mode
        self.in_channels, self.out_channels, self.hidden_channels = int(in_channels), int(out_channels), int(hidden_channels)
        self.kernel_size, self.dilation_rate, self.dilation_cycle, self.n_layers = int(kernel_size), int(dilation_rate), int(dilation_cycle), int(n_layers)
        self._config()                   # the library's limits, by name, before any parameter is allocated
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # torch deprecates nn.utils.weight_norm; it is what gives the checkpoint's weight_g / weight_v keys
            self.pre = nn.Conv1d(self.in_channels, self.hidden_channels, 1)
            self.enc = WaveNet(self.hidden_channels, self.kernel_size, self.dilation_rate, self.dilation_cycle, self.n_layers)
            self.proj = nn.Conv1d(self.hidden_channels, self.out_channels * 2 if mode != "vqvae" else self.out_channels, 1)
        if mode == "bnvae":
            self.mu_bn = nn.BatchNorm1d(self.out_channels, affine=True)
            self.mu_bn.weight.requires_grad = False
            with torch.no_grad():
                self.mu_bn.weight.fill_(0.5)
        object.__setattr__(self, "_engine", None)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_engine())

    def _config(self) -> "_lib.PosteriorConfig":
        """The validated config; a refusal is the library's own message (``fv_posterior_create`` does no device work)."""
        cfg = _lib.PosteriorConfig(self.in_channels, self.out_channels, self.hidden_channels, self.kernel_size, self.dilation_rate,
                                   self.dilation_cycle, self.n_layers, _lib.POSTERIOR_MODES[self.mode])
        h = ctypes.c_void_p()
        L = _lib.lib()
        st = L.fv_posterior_create(ctypes.byref(cfg), ctypes.byref(h))
        if st != 0:
            raise ValueError(L.fv_last_error().decode("utf-8", "replace"))
        reach = int(L.fv_posterior_reach_frames(h))
        L.fv_posterior_destroy(h)
        object.__setattr__(self, "_reach", reach)
        return cfg

    # -- arithmetic: exact fp32 only ------------------------------------------------------------
    @property
    def precision(self) -> str:
        return "f32"

    @precision.setter
    def precision(self, value: str) -> None:
        if value == "f16x3":
            raise ValueError("PosteriorEncoder is fp32 only: there is no f16x3 form of the WaveNet kernels")
        if value != "f32":
            raise ValueError(f"precision must be 'f32', got {value!r}")

    @property
    def reach_frames(self) -> int:
        """R: output frame t depends on the input frames [t - R, t + R] only (``fv_posterior_reach_frames``)."""
        return self.__dict__["_reach"]

    # -- engine cache (as _base.EngineModule keeps its own) ------------------------------------------
    def invalidate_engine(self) -> None:
        eng = self.__dict__.get("_engine")
        if eng is not None:
            eng.close()
        object.__setattr__(self, "_engine", None)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_engine()
        return super()._apply(fn, *args, **kwargs)

    def engine(self, device: torch.device) -> _PosteriorEngine:
        eng = self.__dict__.get("_engine")
        if eng is None or eng.device != device:
            self.invalidate_engine()
            eng = _PosteriorEngine(self._config(), self.state_dict(), device)
            object.__setattr__(self, "_engine", eng)
        return eng

    # -- calls ---------------------------------------------------------------------------------
    def _run(self, x: torch.Tensor, x_lengths, what: str):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError(
                f"{what} needs a CUDA/HIP tensor (got {getattr(x, 'device', type(x))}); vocoder_amd has no CPU path — move the model and "
                "input to the GPU")
        if self.training:
            raise RuntimeError(_MSG_INFERENCE.format(type(self).__name__))
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError(f"{what}: expected (B, {self.in_channels}, T), got {tuple(x.shape)}")
        x = x.detach().to(torch.float32)
        B, Cin, T = (int(v) for v in x.shape)
        # a slice along T of a contiguous tensor passes as it is (fv_posterior_forward's x_row_stride)
        if T and B and not (x.stride(2) == 1 and x.stride(1) >= T and (B == 1 or x.stride(0) == Cin * x.stride(1))):
            x = x.contiguous()
        host = None
        if x_lengths is not None:
            host = [int(v) for v in (x_lengths.tolist() if torch.is_tensor(x_lengths) else x_lengths)]
            if len(host) != B:
                raise ValueError(f"{what}: {len(host)} lengths for {B} rows")
            for b, v in enumerate(host):
                if not 0 <= v <= T:
                    raise ValueError(f"{what}: x_lengths[{b}] = {v} lies outside [0, T = {T}]")
        vae = self.mode != "vqvae"
        new = lambda: torch.empty((B, self.out_channels, T), dtype=torch.float32, device=x.device)      # noqa: E731
        z, mean, logvar = new(), (new() if vae else None), (new() if vae else None)
        if B and T:
            eng, L = self.engine(x.device), _lib.lib()
            with torch.cuda.device(x.device):
                need = int(L.fv_posterior_workspace_bytes(eng.handle, B, T))
                ws = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
                lptr = None if host is None else (ctypes.c_int32 * B)(*host)
                check(L.fv_posterior_forward(eng.handle, x.data_ptr(), x.stride(1), lptr, z.data_ptr(), mean.data_ptr() if vae else None,
                                             logvar.data_ptr() if vae else None, B, T, ws.data_ptr(), need,
                                             int(torch.cuda.current_stream().cuda_stream)))
        if not vae:
            return z
        if host is None:
            mask = torch.ones(B, 1, T, dtype=torch.float32, device=x.device)
        else:       # mask.py:4-10
            mask = (torch.arange(T, device=x.device)[None, :] < torch.tensor(host, device=x.device)[:, None])[:, None, :].to(torch.float32)
        return z, mean, logvar, mask

    def forward(self, x: torch.Tensor, x_lengths=None):
        """posterior_encoder.py:133-160 in eval mode: ``y (B, out_channels, T)`` in ``"vqvae"`` mode, ``(z, mean, logvar, x_mask)`` in the vae
        modes, ``x_mask`` the float mask ``(B, 1, T)``."""
        return self._run(x, x_lengths, f"{type(self).__name__}.forward")

    def forward_list(self, xs) -> list:
        """A list of ``(in_channels, T_i)`` inputs -> a list of ``(out_channels, T_i)`` latents (``z`` in the vae modes) through one padded call."""
        xs = list(xs)
        if not xs:
            return []
        what = f"{type(self).__name__}.forward_list"
        for x in xs:
            if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != self.in_channels:
                raise ValueError(f"{what}: expected tensors of shape ({self.in_channels}, T_i), got {tuple(getattr(x, 'shape', ()))}")
        lengths = [int(x.shape[1]) for x in xs]
        padded = torch.zeros((len(xs), self.in_channels, max(lengths)), dtype=torch.float32, device=xs[0].device)
        for b, x in enumerate(xs):
            padded[b, :, : lengths[b]] = x
        res = self._run(padded, lengths, what)
        z = res if self.mode == "vqvae" else res[0]
        return [z[b, :, :n] for b, n in enumerate(lengths)]

    stream_is_bit_exact = True      # codec.VQVAECodec.encode_stream: a stream's latents are forward's own bits, so its codes are encode's

    def stream(self, batch: int = 1, max_chunk_frames: int = 64) -> PosteriorStream:
        """The encoder chunk by chunk (``PosteriorStream``): ``push`` at most ``max_chunk_frames`` frames per row, ``flush`` at the utterance's
        end; a latent frame comes out ``reach_frames`` frames after its own input.  Reloading the weights or moving the module rebuilds the
        engine and closes its streams: create a new one then."""
        return PosteriorStream(self, self._live_engine("stream"), batch, max_chunk_frames)

    def pool(self, sessions: int, max_chunk_frames: int = 64) -> PosteriorPool:
        """The encoder for ``sessions`` sessions that advance independently (``PosteriorPool``): every ``step`` serves any subset of them, each
        with its own chunk of at most ``max_chunk_frames`` frames, in the launches one stream's push takes.  It dies with the engine, as a
        stream does."""
        return PosteriorPool(self, self._live_engine("pool"), sessions, max_chunk_frames)

    def _live_engine(self, method: str) -> _PosteriorEngine:
        """The engine a stream or pool attaches to; refuses a module that is not on a device or not in eval mode, in that order."""
        dev = self.pre.weight.device
        if dev.type != "cuda":
            raise RuntimeError(_MSG_DEVICE.format(f"{type(self).__name__}.{method}", dev).replace("a CUDA/HIP tensor", "the module on a CUDA/HIP device"))
        if self.training:
            raise RuntimeError(_MSG_INFERENCE.format(type(self).__name__))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return self.engine(dev)

    def remove_weight_norm(self):
        """Kept for API compatibility (posterior_encoder.py:162-163, which raises AttributeError on ``gin_channels``): weight norm is folded
        inside the engine at load time, so this is a harmless no-op."""
        return None

    def extra_repr(self) -> str:
        return (f"in_channels={self.in_channels}, out_channels={self.out_channels}, hidden_channels={self.hidden_channels}, "
                f"kernel_size={self.kernel_size}, n_layers={self.n_layers}, mode={self.mode!r}, backend=libfishvoc_hip (gfx950)")
