"""The inference face of the reference's ``VQVAEModel`` (fish_vocoder/models/vae.py:51-109): audio -> codes, codes -> audio.

``VQVAECodec(encoder, decoder, vq, frontend=None)`` runs ``generator.encoder`` -> ``vq`` -> ``generator.decoder`` (vae.py:81-87) on the
drop-in modules, every stage on the HIP engine; the quantiser is ``modules.quantizers`` (``fv_vq_*``).  A Lightning checkpoint's
``generator.encoder.*``, ``generator.decoder.*`` and ``vq.*`` keys are the module's own ``encoder.*``, ``decoder.*`` and ``vq.*``
(``load_checkpoint``).  Command line::

    python -m vocoder_amd.codec encode -i a.wav -o out/ [--checkpoint ckpt]      # writes out/a.codes.npy, int64 (n_q, T) or (T,)
    python -m vocoder_amd.codec decode -i out/a.codes.npy -o out/                 # writes out/a.wav
    python -m vocoder_amd.codec decode -i out/a.codes.npy -o out/ --chunk-frames 64     # through decode_stream, 64 frames a push
    python -m vocoder_amd.codec encode -i a.wav -o out/ --chunk-samples 4096 --batch-invariant    # through encode_stream (ConvNeXt layer stream)

``decode_stream`` / ``decode_pool`` serve the decode direction chunk by chunk (``CodecDecodeStream``, ``CodecDecodePool``): the ring in front of
the decoder keeps the codes, not the latent.  ``encode_pool(layers=True)`` and ``decode_pool(backbone="layers")`` run a ConvNeXt encoder /
backbone as its layer pool (``ConvNeXtEncoder.layer_pool``): per-slot rings, only the new frames, the batch-invariant ``forward``'s bits.

The architecture defaults to configs/model/vqvae.yaml's (vocos-small-vae at 24000_2048_3072, 512 latent channels, 4096 codes, one
quantiser); ``vocoder_amd.inference``'s command line is untouched.
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np
import torch
from torch import nn

from ._handle import _gather, _require_cuda


class VQVAECodec(nn.Module):
    def __init__(self, encoder: nn.Module, decoder: nn.Module, vq: nn.Module, frontend: nn.Module | None = None, hop_length: int | None = None):
        super().__init__()
        self.encoder, self.decoder, self.vq, self.frontend = encoder, decoder, vq, frontend
        hop = hop_length if hop_length is not None else getattr(frontend, "hop_length", None)
        self.hop_length = None if hop is None else int(hop)

    def _latent(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """Audio ``(B, 1, L)`` / ``(B, L)`` goes through the front-end first (vae.py:14 ``mel_transforms.input``); a spectrogram
        ``(B, C, T)`` with more than one channel goes straight into the encoder.  An encoder that declares ``takes_audio`` receives the audio
        itself, without the front-end; ``lengths`` (latent frames) do not reach such an encoder, which counts in samples, so it runs every
        row over its whole width, padding included — for ragged audio call the encoder with its own ``lengths=`` (samples) and quantise its
        output with ``vq.encode(z, frames)``."""
        if getattr(self.encoder, "takes_audio", False):        # vae.py:81 generator.encoder(audio, mask): an encoder of raw audio (MMSEncoder)
            if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[1] != 1):
                raise ValueError(f"VQVAECodec: an encoder that takes audio expects (B, 1, L) or (B, L); got {tuple(x.shape)}")
            return self.encoder(x)
        if self.frontend is not None and (x.dim() == 2 or x.shape[1] == 1):
            x = self.frontend(x if x.dim() == 3 else x[:, None, :])
        elif x.dim() != 3:
            raise ValueError(f"VQVAECodec: expected audio (B, 1, L) with a front-end, or a spectrogram (B, C, T); got {tuple(x.shape)}")
        if lengths is not None and getattr(self.encoder, "takes_lengths", False):
            return self.encoder(x, lengths)
        return self.encoder(x)

    def encode(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """``codes``: int64 ``(B, T)`` for one quantiser, ``(n_q, B, T)`` for the residual form; ``lengths`` are latent frames per row, handed
        to an encoder that takes them (``PosteriorEncoder``: a row's latent then has the bits of the row alone).  Ragged encoding
        is not supported through an encoder of raw audio (``takes_audio``, ``MMSEncoder``): see ``_latent``."""
        return self.vq.encode(self._latent(x, lengths), lengths)

    def encode_stream(self, batch: int = 1, max_chunk_samples: int = 4096) -> "CodecEncodeStream":
        """``encode`` chunk by chunk (``CodecEncodeStream``): audio in, codes out after the front-end's and the encoder's lookahead.  For an
        encoder of spectrograms whose own stream has ``forward``'s bits: a ``PosteriorEncoder``, or a ``ConvNeXtEncoder`` with
        ``batch_invariant = True`` (its ``layer_stream``); with the front-end in its batch-invariant mode the concatenated codes are
        ``encode``'s."""
        return CodecEncodeStream(self, batch, max_chunk_samples)

    def encode_pool(self, sessions: int, max_chunk_samples: int = 4096, layers: bool = False) -> "CodecEncodePool":
        """``encode`` for ``sessions`` live sources that advance at their own pace (``CodecEncodePool``): one step serves any subset of them in
        the launches one ``encode_stream`` push takes.  A ``PosteriorEncoder`` by default; ``layers=True`` takes a ``ConvNeXtEncoder`` with
        ``batch_invariant = True`` through its ``layer_pool``.  With the front-end in its batch-invariant mode a session's concatenated codes
        are ``encode``'s of its whole utterance."""
        return CodecEncodePool(self, sessions, max_chunk_samples, layers)

    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        y = self.decoder(self.vq.from_codes(codes)[0])
        return y[:, None, :] if y.ndim == 2 else y

    def decode_stream(self, batch: int = 1, max_chunk_frames: int = 64, backbone: str = "window") -> "CodecDecodeStream":
        """``decode`` chunk by chunk (``CodecDecodeStream``): codes in, audio out after the decoder's lookahead.  ``backbone="window"``: the
        rings keep codes and every push recomputes the backbone's window; ``"layers"``: the ConvNeXt backbone of a two-stage decoder runs
        as its ``layer_stream`` — only the new frames, with the bits of its batch-invariant ``forward``."""
        return CodecDecodeStream(self.decoder, self.vq, batch, max_chunk_frames, backbone)

    def decode_pool(self, sessions: int, max_chunk_frames: int = 64, backbone: str = "window") -> "CodecDecodePool":
        """``decode`` for ``sessions`` clients that advance at their own pace (``CodecDecodePool``): one step serves any subset of them.
        ``backbone`` as in ``decode_stream``: ``"window"`` recomputes the backbone's window per session and step, ``"layers"`` runs the ConvNeXt
        backbone of a two-stage decoder as its ``layer_pool`` — only the new frames, with the bits of its batch-invariant ``forward``."""
        return CodecDecodePool(self.decoder, self.vq, sessions, max_chunk_frames, backbone)

    def forward(self, audio: torch.Tensor, mask=None):
        """vae.py:80-109: ``(fake_audio, 0)``, trimmed / zero-padded to the input's length, which it may miss by a hop at most."""
        if audio.dim() == 2:
            audio = audio[:, None, :]
        quantize, _, _ = self.vq(self._latent(audio))
        fake = self.decoder(quantize)
        fake = fake[:, None, :] if fake.ndim == 2 else fake
        if self.hop_length is not None:
            assert abs(fake.size(2) - audio.size(2)) <= self.hop_length, (fake.size(2), audio.size(2), self.hop_length)   # vae.py:89
        if fake.size(2) > audio.size(2):
            fake = fake[:, :, : audio.size(2)]
        else:
            fake = torch.nn.functional.pad(fake, (0, audio.size(2) - fake.size(2)))
        return fake, 0

    def load_checkpoint(self, ckpt, trust_checkpoint: bool = False):
        """A path or dict; Lightning's ``state_dict`` wrapper and its ``generator.`` prefix are taken off, other prefixes
        (discriminators, mel_transforms) dropped; loads strictly."""
        if isinstance(ckpt, (str, Path)):
            try:
                ckpt = torch.load(ckpt, map_location="cpu", weights_only=True)
            except Exception:
                if not trust_checkpoint:
                    raise
                ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
        sd = ckpt.get("state_dict", ckpt)
        own = {}
        for k, v in sd.items():
            if k.startswith("generator.encoder.") or k.startswith("generator.decoder."):
                own[k[len("generator."):]] = v
            elif k.startswith(("vq.", "encoder.", "decoder.", "frontend.")):
                own[k] = v
        for k, v in self.state_dict().items():          # the front-end's window is a constant, not a checkpoint key
            if k.startswith("frontend."):
                own.setdefault(k, v)
        return self.load_state_dict(own, strict=True)


def _streaming_encoder(codec: VQVAECodec, what: str, layers: bool = False) -> nn.Module:
    """The encoder of a codec that can encode chunk by chunk with ``encode``'s codes; ``what`` (``encode_stream`` / ``encode_pool``) refuses
    the others by name.  ``layers`` (``encode_pool(layers=True)``): the pool of a layered encoder is its ``layer_pool``."""
    enc, name = codec.encoder, type(codec.encoder).__name__
    if getattr(enc, "takes_audio", False):
        raise ValueError(f"{what}: {name} takes raw audio (takes_audio), not a streamed spectrogram: it has no streaming encode")
    layered = hasattr(enc, "layer_stream")        # ConvNeXtEncoder: bit-exact through layer_stream, in its batch-invariant mode only
    hint = layered and (what == "encode_stream" or layers)
    if not getattr(enc, "stream_is_bit_exact", False):
        raise ValueError(f"{what}: {name}.stream() is not bit-exact — a windowed engine stream promises 2e-5, not forward's bits, so "
                         "codes could differ from encode(); use a PosteriorEncoder (build_vqvae(encoder='posterior'))"
                         + (" or set encoder.batch_invariant = True" if hint else "")
                         + (" and encoder.conv_algorithm = 'direct' (its C -> C stem has a Winograd form, whose bits depend on the launch)"
                            if hint and getattr(enc, "stem_has_winograd_form", False) else ""))
    if layers and not hasattr(enc, "layer_pool"):
        raise ValueError(f"{what}: layers=True needs an encoder with a layer pool (a ConvNeXtEncoder); {name} has no layer_pool — call "
                         f"{what}() without it")
    if layered and what != "encode_stream" and not layers:
        raise ValueError(f"{what}: {name} has a layer stream (encode_stream) but its pool form is not built: there is no session pool of "
                         "layer streams; use encode_stream per source, or a PosteriorEncoder")
    if codec.frontend is None:
        raise ValueError(f"{what}: the codec has no front-end to turn the audio chunks into spectrogram frames")
    return enc


class _Stages:
    """What the codec's streams and pools repeat over their stages (``_stages()``: the handles a call runs through, in order): ``reset`` and
    ``close`` every one, and close on leaving a ``with`` block."""

    def _stages(self) -> tuple:
        raise NotImplementedError

    def reset(self, *session) -> None:
        """Start the next utterance (a pool: of one ``session``) in every stage."""
        for st in self._stages():
            st.reset(*session)

    def close(self) -> None:
        for st in self._stages():
            st.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()


class CodecEncodePool(_Stages):
    """``VQVAECodec.encode`` for live sources that advance independently: ``frontend.wav_pool()`` -> ``encoder.pool()`` (with ``layers``:
    ``encoder.layer_pool()``, a ``ConvNeXtEncoder`` in its batch-invariant mode) -> ``vq.encode``.  The
    front-end's padded frames go straight into the encoder pool's ``step_padded`` and its padded latents into the quantiser with the frame
    counts per item: nothing goes through the host.  ``step(items)`` takes ``(session, wave, flush)`` tuples — ``wave``: 1-D, at most
    ``max_chunk_samples`` samples, or ``None``; ``flush``: the utterance ends with them — and returns per item the int64 codes of the latent
    frames that are final, ``(k,)`` or ``(n_q, k)`` for the residual form, ``k`` possibly 0.  Both stages are planned before either is
    launched, so a refused step moves neither pool.  ``reset(session)`` starts a slot's next utterance."""

    def __init__(self, codec: VQVAECodec, sessions: int, max_chunk_samples: int = 4096, layers: bool = False):
        enc = _streaming_encoder(codec, "encode_pool", bool(layers))
        self._vq = codec.vq
        self.sessions, self.max_chunk_samples = int(sessions), int(max_chunk_samples)
        self.wav_pool = codec.frontend.wav_pool(self.sessions, self.max_chunk_samples)
        self.enc_pool = (enc.layer_pool if layers else enc.pool)(self.sessions, self.wav_pool.max_frames)

    def received_samples(self, session: int) -> int:
        return self.wav_pool.received_samples(session)

    def emitted_frames(self, session: int) -> int:
        return self.enc_pool.emitted_frames(session)

    def step(self, items) -> list:
        wp, ep = self.wav_pool, self.enc_pool
        wp._check_open(), ep._check_open()
        meta, chunks = _gather(items, wp._engine.device, _require_cuda, "CodecEncodePool.step")
        codes, emit = self.step_padded(meta, chunks)
        return [codes[..., i, :k] for i, k in enumerate(emit)]

    def step_padded(self, items, chunks: "torch.Tensor | None") -> tuple:
        """The step on padded buffers: ``items``: ``(session, samples, flush)`` integers; ``chunks``: ``(count, longest)`` samples, item i's
        first in row i, or ``None`` when no item has samples.  Returns ``(codes (..., count, k_max), latent frames emitted per item)``."""
        wp, ep = self.wav_pool, self.enc_pool
        wp._check_open(), ep._check_open()
        frames = wp.counters.plan(items)                        # both plans before either launch: a refusal moves neither pool
        enc_items = [(s, f, flush) for (s, _, flush), f in zip(items, frames)]
        ep.plan_frames(enc_items)
        spec, _ = wp.step_padded(items, chunks)
        z, emit = ep.step_padded(enc_items, spec if spec.numel() else None)
        z = z[0] if isinstance(z, tuple) else z
        return self._vq.encode(z, emit), emit

    def _stages(self) -> tuple:
        return self.wav_pool, self.enc_pool


class CodecEncodeStream(_Stages):
    """``VQVAECodec.encode`` on a live source: ``frontend.stream()`` -> ``encoder.stream()`` -> ``vq.encode``, every stage on the device.
    ``push(wave (B, c) or (B, 1, c))``, ``c <= max_chunk_samples``, returns the codes of the latent frames that are final — ``(B, k)``, or
    ``(n_q, B, k)`` for the residual form, ``k`` possibly 0; ``flush()`` ends the utterance and returns the rest; ``reset()`` starts the next
    one.  The quantiser is frame-independent, so the concatenated codes are ``encode``'s whenever both streams have their whole-row bits."""

    def __init__(self, codec: VQVAECodec, batch: int = 1, max_chunk_samples: int = 4096):
        enc = _streaming_encoder(codec, "encode_stream")
        self._vq = codec.vq
        self._fe = codec.frontend.stream(batch, max_chunk_samples)
        self.batch, self.max_chunk_samples = int(batch), int(max_chunk_samples)
        self._max_frames = self.max_chunk_samples // int(codec.frontend.hop_length) + 2      # per encoder push; longer runs go in pieces
        # a ConvNeXtEncoder's stream() is the windowed one; its whole-row bits come from layer_stream
        self._enc = (enc.layer_stream if hasattr(enc, "layer_stream") else enc.stream)(batch, self._max_frames)

    @property
    def received_samples(self) -> int:
        return self._fe.received_samples

    @property
    def emitted_frames(self) -> int:
        return self._enc.emitted_frames

    def _latents(self, spec: torch.Tensor) -> list:
        return [self._enc.push(spec[:, :, a:a + self._max_frames]) for a in range(0, int(spec.shape[2]), self._max_frames)]

    def _codes(self, zs: list) -> torch.Tensor:
        return self._vq.encode(zs[0] if len(zs) == 1 else torch.cat(zs, dim=2))

    def push(self, wave: torch.Tensor) -> torch.Tensor:
        spec = self._fe.push(wave)
        return self._codes(self._latents(spec) or [self._enc.push(spec)])

    def flush(self) -> torch.Tensor:
        return self._codes(self._latents(self._fe.flush()) + [self._enc.flush()])

    def _stages(self) -> tuple:
        return self._fe, self._enc


def _decoder_stages(decoder: nn.Module, vq, what: str) -> list:
    """The engine modules codes pass through on their way to audio: ``[decoder]`` for a single engine (a ``HiFiGANGenerator``, a head alone),
    ``[backbone, head]`` for a ``UnifyGenerator`` with a backbone; ``what`` (``decode_stream`` / ``decode_pool``) refuses the others by name."""
    from .modules.generators.unify import UnifyGenerator
    if vq is None:
        raise ValueError(f"{what}: there is no quantiser to decode the codes with")
    if isinstance(decoder, UnifyGenerator):
        if decoder.vq is not None:
            raise ValueError(f"{what}: the decoder is a UnifyGenerator with a quantiser of its own; call its own {what}()")
        stages = [decoder.backbone, decoder.head]
    else:
        stages = [decoder]
    for m in stages:
        if not (hasattr(m, "code_stream") and hasattr(m, "session_pool")):
            raise ValueError(f"{what}: {type(m).__name__} has no engine to stream on (it is not one of the package's engine modules)")
    return stages


class CodecDecodeStream(_Stages):
    """``VQVAECodec.decode`` for a live client: ``push(codes (B, c) or (n_q, B, c))``, ``c <= max_chunk_frames``, returns the audio
    ``(B, C_out, k * hop)`` of the frames that are final, ``k`` possibly 0; ``flush()`` ends the utterance and returns the rest; ``reset()``
    starts the next one.  The first stage is a ``CodeStream``: its ring keeps the codes, and its window is decoded from them in the launch
    that forms it — no ``from_codes`` launch, no latent tensor.  A two-stage decoder (``UnifyGenerator`` with a backbone) feeds the
    backbone's frames to ``head.stream()`` on the device; ``lookahead_frames`` is the sum of the stages'.  Every call's output has the bits of
    the same chain on float streams fed ``vq.from_codes``.  ``template`` (a use_template generator) goes to a single-engine decoder."""

    def __init__(self, decoder: nn.Module, vq, batch: int = 1, max_chunk_frames: int = 64, backbone: str = "window"):
        stages = _decoder_stages(decoder, vq, "decode_stream")
        self.batch, self.max_chunk_frames = int(batch), int(max_chunk_frames)
        if backbone not in ("window", "layers"):
            raise ValueError(f"decode_stream: backbone must be 'window' or 'layers', got {backbone!r}")
        self.backbone = backbone
        if backbone == "layers":
            if len(stages) != 2 or not hasattr(stages[0], "layer_stream"):
                raise ValueError("decode_stream: backbone='layers' needs a two-stage decoder whose backbone has a layer stream "
                                 f"(a ConvNeXtEncoder); got {[type(m).__name__ for m in stages]}")
            self.codes = _LayerBackbone(vq, stages[0].layer_stream(self.batch, self.max_chunk_frames))
        else:
            self.codes = stages[0].code_stream(vq, self.batch, self.max_chunk_frames)
        self.head = None
        if len(stages) == 2:
            # one backbone call emits at most max_chunk_frames frames (a push) or its lookahead (the flush)
            self._head_chunk = max(self.max_chunk_frames, self.codes.lookahead_frames, 1)
            self.head = stages[1].stream(self.batch, self._head_chunk)
        last = self.head or self.codes
        self.hop, self.out_channels = last.hop * (self.codes.hop if self.head else 1), last.out_channels
        self.lookahead_frames = self.codes.lookahead_frames + (self.head.lookahead_frames if self.head else 0)

    @property
    def received_frames(self) -> int:
        return self.codes.received_frames

    @property
    def emitted_frames(self) -> int:
        return (self.head or self.codes).emitted_frames

    @property
    def ring_bytes(self) -> int:
        return self.codes.ring_bytes + (self.head.ring_bytes if self.head else 0)

    def push(self, codes: torch.Tensor, template: torch.Tensor | None = None, validate: bool = True) -> torch.Tensor:
        if self.head is None:
            return self.codes.push(codes, template, validate)
        if template is not None:
            raise ValueError("CodecDecodeStream.push: a template belongs to a single-engine decoder")
        self.head._check_open()
        return self.head.push(self.codes.push(codes, validate=validate))

    def flush(self) -> torch.Tensor:
        if self.head is None:
            return self.codes.flush()
        self.head._check_open()
        rest = self.codes.flush()
        return torch.cat([self.head.push(rest), self.head.flush()], dim=2)

    def _stages(self) -> tuple:
        return (self.codes,) if self.head is None else (self.codes, self.head)


class _LayerBackbone:
    """The first stage of ``CodecDecodeStream(backbone="layers")`` with the face of a ``CodeStream``: ``push(codes)`` runs
    ``vq.from_codes(chunk)`` -> ``backbone.layer_stream`` on the device.  Nothing is kept of the codes: the backbone's rings hold its
    blocks' last columns.  ``check`` makes the refusals a host can see before anything is launched; the count a call emits is the
    stream's host arithmetic (``ConvNeXtStream.plan``).  ``validate`` has no effect here: ``from_codes`` checks the codes itself."""
    hop = 1

    def __init__(self, vq, stream):
        self._vq, self.stream = vq, stream
        self.batch, self.max_chunk_frames, self.out_channels = stream.batch, stream.max_chunk_frames, stream.out_channels
        self.lookahead_frames = stream.lookahead_frames

    received_frames = property(lambda self: self.stream.received_frames)
    emitted_frames = property(lambda self: self.stream.emitted_frames)
    ring_bytes = property(lambda self: self.stream.state_bytes)

    def _check_open(self) -> None:
        self.stream._check_open()

    def check(self, codes: torch.Tensor) -> int:
        """The refusals a host can see, before any stage launches; returns the chunk's frames."""
        self.stream._check_open()
        if not isinstance(codes, torch.Tensor) or not codes.is_cuda:
            raise RuntimeError(f"CodecDecodeStream.push needs a CUDA/HIP tensor of codes (got {getattr(codes, 'device', type(codes))})")
        if codes.dim() not in (2, 3) or codes.shape[-2] != self.batch:
            raise ValueError(f"CodecDecodeStream.push: expected codes ({self.batch}, c) or (n_q, {self.batch}, c), got {tuple(codes.shape)}")
        c = int(codes.shape[-1])
        if c > self.max_chunk_frames:
            raise ValueError(f"CodecDecodeStream.push: c = {c} is more than max_chunk_frames = {self.max_chunk_frames}")
        if self.stream._flushed:
            raise RuntimeError("CodecDecodeStream.push: the stream was flushed: reset() starts the next utterance")
        return c

    def push(self, codes: torch.Tensor, template=None, validate: bool = True) -> torch.Tensor:
        c = self.check(codes)
        if c == 0:
            return self.stream.push(torch.empty((self.batch, self.stream.in_channels, 0), dtype=torch.float32, device=codes.device))
        return self.stream.push(self._vq.from_codes(codes)[0])

    def flush(self) -> torch.Tensor:
        return self.stream.flush()

    def reset(self) -> None:
        self.stream.reset()

    def close(self) -> None:
        self.stream.close()


class CodecDecodePool(_Stages):
    """``VQVAECodec.decode`` for clients that advance independently: ``step(items)`` takes ``(session, codes, flush)`` tuples — ``codes``:
    ``(n,)`` or ``(n_q, n)`` with ``n <= max_chunk_frames``, or ``None``; ``flush``: the utterance ends with them — and returns one audio
    tensor ``(C_out, k * hop)`` per item, ``k`` possibly 0.  The first stage is a ``CodeSessionPool``: a slot's ring keeps ``n_q`` int32 per
    frame, not the latent's channels.  A two-stage decoder hands the backbone pool's padded frames to ``head.session_pool()``'s
    ``step_padded`` on the device; both stages are planned before either is launched, so a refused step moves neither pool.
    ``reset(session)`` starts a slot's next utterance.  ``backbone="layers"``: the first stage of a two-stage decoder is ``vq.from_codes`` on
    the step's padded codes and the ConvNeXt backbone's ``layer_pool`` (``_LayerBackbonePool``) — only the frames that are new, with the bits
    of the backbone's batch-invariant ``forward``; no ring keeps codes, the backbone's rings hold its blocks' last columns."""

    def __init__(self, decoder: nn.Module, vq, sessions: int, max_chunk_frames: int = 64, backbone: str = "window"):
        stages = _decoder_stages(decoder, vq, "decode_pool")
        self.sessions, self.max_chunk_frames = int(sessions), int(max_chunk_frames)
        if backbone not in ("window", "layers"):
            raise ValueError(f"decode_pool: backbone must be 'window' or 'layers', got {backbone!r}")
        self.backbone = backbone
        if backbone == "layers":
            if len(stages) != 2 or not hasattr(stages[0], "layer_pool"):
                raise ValueError("decode_pool: backbone='layers' needs a two-stage decoder whose backbone has a layer pool "
                                 f"(a ConvNeXtEncoder); got {[type(m).__name__ for m in stages]}")
            self.codes = _LayerBackbonePool(vq, stages[0].layer_pool(self.sessions, self.max_chunk_frames))
        else:
            self.codes = stages[0].code_pool(vq, self.sessions, self.max_chunk_frames)
        self.head = None
        if len(stages) == 2:
            # an item that ends its utterance emits its own frames and the backbone's lookahead in one step
            self.head = stages[1].session_pool(self.sessions, self.max_chunk_frames + self.codes.lookahead_frames)
        last = self.head or self.codes
        self.hop, self.out_channels = last.hop * (self.codes.hop if self.head else 1), last.out_channels
        self.lookahead_frames = self.codes.lookahead_frames + (self.head.lookahead_frames if self.head else 0)

    def received_frames(self, session: int) -> int:
        return self.codes.received_frames(session)

    def emitted_frames(self, session: int) -> int:
        return (self.head or self.codes).emitted_frames(session)

    @property
    def ring_bytes(self) -> int:
        return self.codes.ring_bytes + (self.head.ring_bytes if self.head else 0)

    def step(self, items, validate: bool = True) -> list:
        cp, hp = self.codes, self.head
        cp._check_open()
        if hp is None:
            return cp.step(items, validate)
        hp._check_open()
        meta, chunks, tmpl = cp.gather(items, validate)
        if tmpl is not None:
            raise ValueError("CodecDecodePool.step: a template belongs to a single-engine decoder")
        out, emit = self.step_padded(meta, chunks)
        return [out[i, :, :k * hp.hop] for i, k in enumerate(emit)]

    def step_padded(self, items, chunks: "torch.Tensor | None") -> tuple:
        """The step of a two-stage decoder on padded codes: ``items``: ``(session, frames, flush)`` integers; ``chunks``: contiguous int32
        ``(num_quantizers, count, longest)``, item i's codes first in row i of every layer, or ``None`` when no item has frames.  Returns
        ``(audio (count, C_out, k_max * hop), frames emitted per item)``.  The codes are not validated here."""
        cp, hp = self.codes, self.head
        if hp is None:
            raise ValueError("CodecDecodePool.step_padded: a single-engine decoder's pool is self.codes: call its step_padded")
        cp._check_open(), hp._check_open()
        items = [(int(s), int(n), bool(f)) for s, n, f in items]
        frames = cp.plan_frames(items)                            # every plan before the first launch: a refusal moves no pool
        head_items = [(s, k, flush) for (s, _, flush), k in zip(items, frames)]
        hp.plan_frames(head_items)
        z, _ = cp.step_padded(items, chunks)
        return hp.step_padded(head_items, z if z.numel() else None)

    def _stages(self) -> tuple:
        return (self.codes,) if self.head is None else (self.codes, self.head)


class _LayerBackbonePool:
    """The first stage of ``CodecDecodePool(backbone="layers")`` with the face of a ``CodeSessionPool``: ``gather`` validates and pads the
    items' codes — with code 0, a valid code whose frames the pool never reads — and ``step_padded`` runs ``vq.from_codes`` on the padded
    ``(n_q, count, n_max)`` codes and hands the latents to ``backbone.layer_pool().step_padded``.  Nothing is kept of the codes."""
    hop = 1

    def __init__(self, vq, pool):
        if not (hasattr(vq, "from_codes") and hasattr(vq, "num_quantizers") and hasattr(vq, "codebook_size")):
            raise ValueError("decode_pool: expected one of the package's quantisers (modules.quantizers), got " + type(vq).__name__)
        self._vq, self.pool = vq, pool
        self.num_quantizers, self.codebook_size = int(vq.num_quantizers), int(vq.codebook_size)
        self.sessions, self.max_chunk_frames, self.out_channels = pool.sessions, pool.max_chunk_frames, pool.out_channels
        self.lookahead_frames = pool.lookahead_frames

    ring_bytes = property(lambda self: self.pool.state_bytes)

    def received_frames(self, session: int) -> int:
        return self.pool.received_frames(session)

    def emitted_frames(self, session: int) -> int:
        return self.pool.emitted_frames(session)

    def _check_open(self) -> None:
        self.pool._check_open()

    def plan_frames(self, items) -> list:
        return self.pool.plan_frames(items)

    def gather(self, items, validate: bool = True):
        """``step``'s items -> ``(the (session, n, flush) integers, the padded int32 codes (num_quantizers, count, longest) or None, None)``.
        Nothing moves."""
        from .engine import _validate_codes, code_chunk
        what, dev = "CodecDecodePool.step", self.pool._engine.device
        meta, rows = [], []
        for it in map(tuple, items):
            s, codes, flush = it[0], it[1], it[2] if len(it) > 2 else False
            if len(it) > 3 and it[3] is not None:
                raise ValueError(f"{what}: a template belongs to a single-engine decoder")
            n = 0
            if codes is not None:
                codes, n = code_chunk(codes, self.num_quantizers, None, self.max_chunk_frames, what)
                if validate:
                    _validate_codes(codes, self.codebook_size, what)
            rows.append(codes)
            meta.append((int(s), n, bool(flush)))
        longest = max((n for _, n, _ in meta), default=0)
        chunks = None
        if longest:
            chunks = torch.zeros((self.num_quantizers, len(meta), longest), dtype=torch.int32, device=dev)
            for i, codes in enumerate(rows):
                if codes is not None and codes.shape[2]:
                    chunks[:codes.shape[0], i, :codes.shape[2]] = codes[:, 0]
                    chunks[codes.shape[0]:, i, :codes.shape[2]] = -1        # layers the item does not give: no code
        return meta, chunks, None

    def step_padded(self, items, chunks: "torch.Tensor | None", templates=None, out=None) -> tuple:
        z = None if chunks is None else self._vq.from_codes(chunks)[0]
        return self.pool.step_padded(items, z, out)

    def step(self, items, validate: bool = True) -> list:
        meta, chunks, _ = self.gather(items, validate)
        out, emit = self.step_padded(meta, chunks)
        return [out[i, :, :k] for i, k in enumerate(emit)]

    def reset(self, session: int) -> None:
        self.pool.reset(session)

    def close(self) -> None:
        self.pool.close()


def build_vqvae(n_fft: int = 3072, hop_length: int = 2048, win_length: int = 3072, latent_size: int = 512, codebook_size: int = 4096,
                num_quantizers: int = 1, encoder_depths=(6,), encoder_dims=(512,), decoder_depths=(6, 3), decoder_dims=(512, 1024),
                kernel_size: int = 7, encoder: str = "convnext", hidden_channels: int = 192, posterior_layers: int = 16,
                posterior_kernel_size: int = 5) -> VQVAECodec:
    """configs/model/vqvae.yaml + generator/vocos-small-vae.yaml with the drop-in modules.  ``encoder="posterior"`` puts the reference's
    ``PosteriorEncoder(mode="vqvae", out_channels=latent_size)`` into the encoder slot instead of the ConvNeXt one."""
    from .data.transforms.spectrogram import LinearSpectrogram
    from .modules.encoders.convnext import ConvNeXtEncoder
    from .modules.generators.unify import UnifyGenerator
    from .modules.generators.vocos import ISTFTHead
    from .modules.quantizers import ResidualVectorQuantization, VectorQuantization
    if encoder == "posterior":
        from .modules.encoders.posterior_encoder import PosteriorEncoder
        enc = PosteriorEncoder(in_channels=n_fft // 2 + 1, out_channels=latent_size, hidden_channels=hidden_channels,
                               kernel_size=posterior_kernel_size, n_layers=posterior_layers, mode="vqvae")
    elif encoder == "convnext":
        if encoder_dims[-1] != latent_size:
            raise ValueError(f"latent_size ({latent_size}) must equal the encoder's last width ({encoder_dims[-1]})")
        enc = ConvNeXtEncoder(input_channels=n_fft // 2 + 1, depths=list(encoder_depths), dims=list(encoder_dims), kernel_size=kernel_size)
    else:
        raise ValueError(f"encoder must be 'convnext' or 'posterior', got {encoder!r}")
    decoder = UnifyGenerator(
        backbone=ConvNeXtEncoder(input_channels=latent_size, depths=list(decoder_depths), dims=list(decoder_dims), kernel_size=kernel_size),
        head=ISTFTHead(dim=decoder_dims[-1], n_fft=n_fft, hop_length=hop_length, win_length=win_length, padding="same"))
    if num_quantizers > 1:      # vae.py:66-78
        vq = ResidualVectorQuantization(dim=latent_size, codebook_size=codebook_size, num_quantizers=num_quantizers, kmeans_init=False)
    else:
        vq = VectorQuantization(dim=latent_size, codebook_size=codebook_size, kmeans_init=False)
    return VQVAECodec(enc, decoder, vq, frontend=LinearSpectrogram(n_fft, win_length, hop_length), hop_length=hop_length)


def main(argv=None):
    from .inference import read_wav, write_wav
    ap = argparse.ArgumentParser(prog="python -m vocoder_amd.codec", description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=("encode", "decode"))
    ap.add_argument("-i", "--input", required=True, help="encode: a PCM .wav; decode: a .codes.npy")
    ap.add_argument("-o", "--output-dir", default="generated")
    ap.add_argument("--checkpoint", default=None, help="Lightning checkpoint or state dict (default: the untrained initialisation)")
    ap.add_argument("--trust-checkpoint", action="store_true")
    ap.add_argument("--sample-rate", type=int, default=24000)
    ap.add_argument("--n-fft", type=int, default=3072)
    ap.add_argument("--hop-length", type=int, default=2048)
    ap.add_argument("--win-length", type=int, default=3072)
    ap.add_argument("--latent-size", type=int, default=512)
    ap.add_argument("--codebook-size", type=int, default=4096)
    ap.add_argument("--num-quantizers", type=int, default=1)
    ap.add_argument("--encoder", choices=("convnext", "posterior"), default="convnext", help="the encoder slot: ConvNeXtEncoder or PosteriorEncoder")
    ap.add_argument("--hidden-channels", type=int, default=192, help="--encoder posterior: the WaveNet's width")
    ap.add_argument("--chunk-samples", type=int, default=None,
                    help="encode: run the file through encode_stream in chunks of this many samples (same codes; needs --encoder posterior, "
                         "or --batch-invariant with the ConvNeXt encoder)")
    ap.add_argument("--batch-invariant", action="store_true",
                    help="encode: the encoder and the front-end in their batch-invariant mode, whole-file or chunked: the mode in which the "
                         "ConvNeXt encoder's layer stream gives the whole-file codes")
    ap.add_argument("--chunk-frames", type=int, default=None,
                    help="decode: run the codes through decode_stream in chunks of this many frames (the rings keep codes)")
    a = ap.parse_args(argv)
    if a.chunk_frames is not None:
        if a.mode != "decode":
            ap.error("--chunk-frames belongs to decode: encode streams samples (--chunk-samples)")
        if a.chunk_frames < 1:
            ap.error(f"--chunk-frames = {a.chunk_frames} must be at least 1")
    if a.chunk_samples is not None:
        if a.mode != "encode":
            ap.error("--chunk-samples belongs to encode: decode streams frames of codes (--chunk-frames)")
        if a.encoder != "posterior" and not a.batch_invariant:
            ap.error("--chunk-samples needs --encoder posterior: the ConvNeXt encoder's stream is not bit-exact, so its codes could differ "
                     "from a whole-file encode; or add --batch-invariant, the mode in which its layer stream has the whole file's bits")
        if a.chunk_samples < 1:
            ap.error(f"--chunk-samples = {a.chunk_samples} must be at least 1")
    if a.batch_invariant and a.mode != "encode":
        ap.error("--batch-invariant belongs to encode: it sets the encoder's and the front-end's mode")
    if not torch.cuda.is_available():
        raise SystemExit("vocoder_amd.codec needs a HIP device: there is no CPU path")
    model = build_vqvae(a.n_fft, a.hop_length, a.win_length, a.latent_size, a.codebook_size, a.num_quantizers,
                        encoder_dims=(a.latent_size,), decoder_dims=(a.latent_size, 2 * a.latent_size), encoder=a.encoder,
                        hidden_channels=a.hidden_channels)
    if a.checkpoint:
        model.load_checkpoint(a.checkpoint, a.trust_checkpoint)
    model = model.eval().cuda()
    out = Path(a.output_dir)
    out.mkdir(parents=True, exist_ok=True)
    src = Path(a.input)
    if a.mode == "encode":
        wav, sr = read_wav(src)
        if sr != a.sample_rate:
            raise SystemExit(f"{src}: {sr} Hz, the model runs at {a.sample_rate} Hz (resample with vocoder_amd.inference --resample first)")
        audio = torch.from_numpy(wav.mean(0, keepdims=True))[None].cuda()
        if a.batch_invariant:
            model.encoder.batch_invariant = model.frontend.batch_invariant = True
            if getattr(model.encoder, "stem_has_winograd_form", False):      # n_fft / 2 + 1 == latent_size: a C -> C stem, direct sums as well
                model.encoder.conv_algorithm = "direct"
        if a.chunk_samples is None:
            codes = model.encode(audio)
        else:
            model.frontend.batch_invariant = True       # the mode in which the front-end's stream has its whole-row bits
            with model.encode_stream(1, a.chunk_samples) as st:
                parts = [st.push(audio[:, :, n:n + a.chunk_samples]) for n in range(0, audio.shape[2], a.chunk_samples)]
                codes = torch.cat(parts + [st.flush()], dim=-1)
        codes = codes[:, 0] if codes.dim() == 3 else codes[0]
        dst = out / f"{src.stem}.codes.npy"
        np.save(dst, codes.cpu().numpy())
    else:
        codes = torch.from_numpy(np.load(src)).to(torch.int64).cuda()
        codes = codes[:, None, :] if codes.dim() == 2 else codes[None, :]
        if a.chunk_frames is None:
            audio = model.decode(codes)
        else:
            with model.decode_stream(1, a.chunk_frames) as st:
                parts = [st.push(codes[..., n:n + a.chunk_frames]) for n in range(0, codes.shape[-1], a.chunk_frames)]
                audio = torch.cat(parts + [st.flush()], dim=2)
        stem = src.name[: -len(".codes.npy")] if src.name.endswith(".codes.npy") else src.stem
        dst = out / f"{stem}.wav"
        write_wav(dst, audio[0, 0].cpu().numpy(), a.sample_rate)
    print(dst)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
