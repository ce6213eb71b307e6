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
from ..._frames import _MSG_DEVICE, _MSG_INFERENCE, FramePoolCounters, _FramePool, _FrameStream, schedule      # noqa: F401  (schedule: re-exported)
from ..._lib import check

PosteriorPoolCounters = FramePoolCounters


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


class _PosteriorOutputs:
    """What a posterior stream or pool takes and returns per call: ``z`` in ``"vqvae"`` mode; ``z, mean, logvar`` in the vae modes, returned
    with the float mask as ``forward`` returns them."""
    _slots = 3
    _out_names = "(z, mean, logvar)"

    def _attach(self, module, engine) -> tuple:
        return engine.handle, module.in_channels, module.out_channels

    def _count(self) -> int:
        return 1 if self._module.mode == "vqvae" else 3

    def _wrap(self, outs, mask_shape: tuple):
        if len(outs) == 1:
            return outs[0]
        return (*outs, torch.ones(mask_shape, dtype=torch.float32, device=self._engine.device))


class PosteriorStream(_PosteriorOutputs, _FrameStream):
    """``PosteriorEncoder`` chunk by chunk (``fv_wnstream_*``, include/fishvoc.h): ``push`` a ``(B, in_channels, c)`` chunk, ``c <=
    max_chunk_frames``, and get what ``forward`` returns for the frames that need no later input — ``[E, max(E, N - R))``, ``R =
    lookahead_frames``, possibly none; ``flush`` ends the utterance at ``N`` and returns the rest, then pushes raise until ``reset()``.  The
    concatenation has the bits of ``forward`` over the whole utterance under any chunking (``schedule`` gives the counts).  The ``batch`` rows
    advance in lockstep.  A stream dies with the module's engine: ``load_state_dict`` or ``.to()`` closes it, create a new one then."""
    _prefix, _noun = "fv_wnstream", "posterior stream"


class PosteriorPool(_PosteriorOutputs, _FramePool):
    """``PosteriorEncoder`` for sessions that advance independently (``fv_wnpool_*``, include/fishvoc.h): what ``PosteriorStream`` is to rows
    in lockstep, for ``sessions`` slots with their own counters.  ``step(items)`` takes ``(session, x, flush)`` tuples — ``x``: ``(in_channels,
    n)`` with ``n <= max_chunk_frames``, or ``None`` for no frames; ``flush``: the utterance ends with these frames — and returns per item what
    ``forward`` returns for the frames that session emits in this step: ``z (out_channels, k)``, or ``(z, mean, logvar, mask)``; ``k`` may be
    0.  ``step_padded`` takes and returns ``z``, or ``(z, mean, logvar)`` in the vae modes.  A session appears at most once per step and
    refuses items after its flush until ``reset(session)``.  The whole step is checked before anything moves: a refused step leaves every
    session as it was.  A session's concatenated tensors have the bits of ``forward`` over its whole utterance, whatever the other sessions
    do.  One step is at most ``2 n_layers + 2`` launches per 128 items.  Work is enqueued on torch's current stream and calls must be
    ordered; the pool dies with the module's engine, as a ``PosteriorStream`` does."""
    _prefix, _noun = "fv_wnpool", "posterior pool"


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
