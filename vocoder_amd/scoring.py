"""Scoring generated audio on the GPU (include/fishvoc.h ``fv_spec_distance*``): how far a generated waveform is from its source.

The reference answers that in two places.  ``eval.py:29-33`` prints ``spec_diff``, the mean absolute difference of two
``LogMelSpectrogram(sr, 1024, 1024, 256, 128, center=False)`` outputs (``MelDistance``); ``modules/losses/stft.py:55,74`` are the spectral
convergence and the log-magnitude L1 that ``models/gan.py:97-101`` sums over several STFT resolutions (``MultiResolutionSTFTDistance``, as a
metric: no gradients).  Both are ratios of four per-row sums over two spectrogram tensors, which one kernel forms for rows of different
lengths in a fixed order (``spec_distance``)::

    S_l1 = sum |est - ref|    S_sq = sum (est - ref)^2    S_ref = sum ref^2    S_log = sum |log ref - log est|        c < C, t < frames[b]

The front-ends run batch-invariant, and the reduction's order depends on nothing but the row itself, so a pair's score is the same bits
whether it is scored alone or in any batch.  eval.py's PESQ is not computed (a standardised CPU algorithm).

``CriticDistance`` adds what the reference logs per critic during training (``models/gan.py:149``, ``:155``, ``:204``): the adversarial terms
and the feature-matching L1 of a (real, generated) pair under the multi-period and multi-resolution discriminators, from the per-row sums of
``fv_disc_distance``.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _lib
from ._handle import _require_cuda
from ._lib import check

S_L1, S_SQ, S_REF, S_LOG = range(4)     # columns of spec_distance's result


def _layout(x: torch.Tensor):
    """(ld, row_stride) in floats if ``fv_spec_distance`` can address ``x`` (B, C, T) in place, else None."""
    B, C, T = (int(d) for d in x.shape)
    if T > 1 and x.stride(2) != 1:
        return None
    ld = int(x.stride(1)) if C > 1 else T
    if ld < T:
        return None
    row = int(x.stride(0)) if B > 1 else C * ld
    return (ld, row) if row >= C * ld else None


def spec_distance(est: torch.Tensor, ref: torch.Tensor, frames=None, log_term: bool = False) -> torch.Tensor:
    """``est`` / ``ref``: fp32 ``(B, C, T)`` on the GPU; ``frames[b] <= T`` valid columns per row (host integers; default: all ``T``) ->
    ``(B, 4)`` float64 on the device, the sums ``S_l1, S_sq, S_ref, S_log`` of row ``b`` over ``c < C, t < frames[b]``.  ``S_log`` is formed
    only with ``log_term`` (positive magnitudes), otherwise it is exactly 0.  Terms are fp32, one rounding per operation, accumulated in fp64 in
    a fixed order: a row's result is bit-identical alone, in any batch, at any ``T`` and on every run.  Columns at or past ``frames[b]`` are
    never read; an empty row gives zeros.  Tensors that share a column stride ``ld >= T`` and a row stride ``>= C * ld`` (a view such as
    ``mel[:, :, 1:]`` of both) are read in place; anything else is made contiguous first.  Enqueued on torch's current stream."""
    _require_cuda(est, "spec_distance est", ValueError, ValueError)
    _require_cuda(ref, "spec_distance ref", ValueError, ValueError)
    if est.dim() != 3 or est.shape != ref.shape or est.device != ref.device:
        raise ValueError(f"spec_distance: expected two (B, C, T) tensors of one shape on one device, got {tuple(est.shape)} and {tuple(ref.shape)}")
    B, C, T = (int(d) for d in est.shape)
    if C < 1:
        raise ValueError("spec_distance: no channels")
    if frames is None:
        frames = [T] * B
    frames = [int(v) for v in (frames.tolist() if torch.is_tensor(frames) else frames)]
    if len(frames) != B:
        raise ValueError(f"spec_distance: {len(frames)} frame counts for {B} rows")
    out = torch.zeros((B, 4), dtype=torch.float64, device=est.device)
    if B == 0 or (T == 0 and not any(frames)):
        return out
    lay = _layout(est)
    if lay is None or lay != _layout(ref):
        est, ref, lay = est.contiguous(), ref.contiguous(), (T, C * T)
    lib = _lib.lib()
    need = int(lib.fv_spec_distance_workspace_bytes(B, T))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=est.device)
    with torch.cuda.device(est.device):
        check(lib.fv_spec_distance(est.data_ptr(), ref.data_ptr(), lay[1], lay[0], C, T, (ctypes.c_int32 * B)(*frames), B,
                                   _lib.FV_SPEC_DISTANCE_LOG if log_term else 0, out.data_ptr(), ws.data_ptr(), need,
                                   int(torch.cuda.current_stream().cuda_stream)))
    return out


def _waves(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dim() == 3 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 2:
        raise ValueError(f"{what}: expected waveforms of shape (B, L) or (B, 1, L), got {tuple(x.shape)}")
    return x


class _PairDistance(nn.Module):
    """What the two metrics share: the three ways to hand over pairs of waveforms.  A subclass names its front-ends (``_fronts``), whether
    the kernel forms ``S_log`` for them, and how the sums of every front-end become the result (``_result``)."""
    _log_term = False

    def _fronts(self) -> list:  # pragma: no cover - abstract
        raise NotImplementedError

    def _result(self, sums: list, counts: list):  # pragma: no cover - abstract
        raise NotImplementedError

    def too_short(self, L: int) -> bool:
        """A pair of ``L`` samples that a front-end of this metric refuses (no frame, or not longer than the reflect padding)."""
        return any(f._framing().too_short(int(L)) for f in self._fronts())

    def _check_lengths(self, lengths, what: str) -> None:
        for b, n in enumerate(lengths):
            for f in self._fronts():
                if n != 0 and f._framing().too_short(n):
                    raise ValueError(f"{what}: row {b} holds {n} samples, too few for the front-end n_fft = {f.n_fft}, hop = {f.hop_length} "
                                     "(no frame, or not longer than the reflect padding)")

    def _score(self, specs):
        sums, counts = [], []
        for f in self._fronts():
            ref, est, frames = specs(f)
            s = spec_distance(est, ref, frames, log_term=self._log_term)
            sums.append(s)
            counts.append(torch.tensor(frames, dtype=torch.float64, device=s.device) * int(ref.shape[1]))
        return self._result(sums, counts)

    def forward(self, target: torch.Tensor, preds: torch.Tensor):
        """``target`` / ``preds``: ``(B, L)`` or ``(B, 1, L)``, rows of one length -> one value per row (``B == 1``: the reference's call)."""
        target, preds = _waves(target, "forward target"), _waves(preds, "forward preds")
        if target.shape != preds.shape:
            raise ValueError(f"forward: target {tuple(target.shape)} and preds {tuple(preds.shape)} differ in shape")
        B, L = int(target.shape[0]), int(target.shape[1])
        if L == 0 or B == 0:
            return self.forward_ragged(target, preds, [0] * B)
        self._check_lengths([L] * B, "forward")

        def specs(f):
            ref = f(target)
            return ref, f(preds), [int(ref.shape[-1])] * B
        return self._score(specs)

    def forward_ragged(self, target: torch.Tensor, preds: torch.Tensor, lengths):
        """Padded batches ``(B, L_max)`` with ``lengths[b]`` valid samples per row: both go through the front-end's ``forward_ragged`` and the
        kernel scores the frames each row has.  A length of 0 scores NaN (0 / 0); a row the front-end would refuse is refused with its index."""
        target, preds = _waves(target, "forward_ragged target"), _waves(preds, "forward_ragged preds")
        if target.shape != preds.shape:
            raise ValueError(f"forward_ragged: target {tuple(target.shape)} and preds {tuple(preds.shape)} differ in shape")
        lengths = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(lengths) != target.shape[0]:
            raise ValueError(f"forward_ragged: {len(lengths)} lengths for {target.shape[0]} rows")
        self._check_lengths(lengths, "forward_ragged")
        if not any(lengths):        # nothing for a front-end to frame: every sum is empty and every score 0 / 0
            zero = torch.zeros((len(lengths), 4), dtype=torch.float64, device=target.device)
            return self._result([zero] * len(self._fronts()), [zero[:, 0]] * len(self._fronts()))

        def specs(f):
            ref, fl = f.forward_ragged(target, lengths)
            est, _ = f.forward_ragged(preds, lengths)
            return ref, est, fl
        return self._score(specs)

    def forward_list(self, targets, preds):
        """Lists of ``(L_i,)`` or ``(1, L_i)`` waveforms, pair by pair: both are cropped to the shorter of the two (eval.py:70-74) and the
        pairs are scored in one ``forward_ragged`` call."""
        targets, preds = [t.reshape(-1) for t in targets], [p.reshape(-1) for p in preds]
        if len(targets) != len(preds):
            raise ValueError(f"forward_list: {len(targets)} targets for {len(preds)} preds")
        if not targets:
            return self.forward_ragged(torch.zeros((0, 1), device=self._device()), torch.zeros((0, 1), device=self._device()), [])
        lengths = [min(int(t.shape[0]), int(p.shape[0])) for t, p in zip(targets, preds)]
        shape = (len(targets), max(max(lengths), 1))
        x = torch.zeros(shape, dtype=torch.float32, device=targets[0].device)
        y = torch.zeros(shape, dtype=torch.float32, device=targets[0].device)
        for b, n in enumerate(lengths):
            x[b, :n], y[b, :n] = targets[b][:n], preds[b][:n]
        return self.forward_ragged(x, y, lengths)

    def _device(self):
        return next(self.buffers()).device


class MelDistance(_PairDistance):
    """``spec_diff`` of the reference's eval.py (eval.py:29-33, :55): per row, ``mean |logmel(target) - logmel(preds)|`` =
    ``S_l1 / (n_mels * frames)`` as float64.  Owns one ``LogMelSpectrogram`` in batch-invariant mode; the defaults are eval.py:55's.
    Inference only: move it to the GPU (``.cuda()``) and hand it GPU waveforms."""

    def __init__(self, sample_rate: int, n_fft: int = 1024, win_length: int = 1024, hop_length: int = 256, n_mels: int = 128,
                 f_min: float = 0.0, f_max: float | None = None):
        super().__init__()
        from .data.transforms import LogMelSpectrogram
        self.mel = LogMelSpectrogram(sample_rate=sample_rate, n_fft=n_fft, win_length=win_length, hop_length=hop_length, n_mels=n_mels,
                                     center=False, f_min=f_min, f_max=f_max)
        self.mel.batch_invariant = True
        self.eval()

    def _fronts(self) -> list:
        return [self.mel]

    def _result(self, sums: list, counts: list) -> torch.Tensor:
        return sums[0][:, S_L1] / counts[0]


class MultiResolutionSTFTDistance(_PairDistance):
    """The two formulas of the reference's multi-resolution STFT loss (modules/losses/stft.py) as metrics: per row ``(sc, mag)`` float64,

        sc  = mean over resolutions of sqrt(S_sq) / sqrt(S_ref)        stft.py:55, ||y_mag - x_mag||_F / ||y_mag||_F
        mag = mean over resolutions of S_log / count                   stft.py:74, mean |log y_mag - log x_mag|

    with ``y`` the target and ``x`` the prediction.  Each resolution is an ``(n_fft, hop)`` pair; the defaults are those of
    configs/model/gan.yaml:49-53.  Deviation: the magnitudes are this project's ``LinearSpectrogram(n_fft, n_fft, hop)`` —
    ``win_length = n_fft``, ``center=False`` with its own reflect padding, ``sqrt(re^2 + im^2 + 1e-6)`` — not stft.py:24-36's
    ``torch.stft(center=True, win_length < n_fft)`` with a clamp at 1e-6: the front-end's config (frozen at ABI 5) has neither, so the numbers
    are close to the training loss's terms but not equal to them.  No gradients: a metric, not a loss."""
    _log_term = True

    def __init__(self, resolutions=((1024, 120), (2048, 240), (4096, 480), (512, 50))):
        super().__init__()
        from .data.transforms.spectrogram import LinearSpectrogram
        self.resolutions = tuple((int(n), int(h)) for n, h in resolutions)
        if not self.resolutions:
            raise ValueError("MultiResolutionSTFTDistance: no resolutions")
        self.spectrograms = nn.ModuleList(LinearSpectrogram(n, n, h) for n, h in self.resolutions)
        for s in self.spectrograms:
            s.batch_invariant = True
        self.eval()

    def _fronts(self) -> list:
        return list(self.spectrograms)

    def _result(self, sums: list, counts: list):
        sc = sum(torch.sqrt(s[:, S_SQ]) / torch.sqrt(s[:, S_REF]) for s in sums) / len(sums)
        mag = sum(s[:, S_LOG] / n for s, n in zip(sums, counts)) / len(sums)
        return sc, mag


# -- the critics' numbers (models/gan.py:142-155, :197-206) ---------------------------------------------------------------------------------
from .modules.discriminators._critic import S_ADV_FAKE, S_ADV_REAL, S_COUNT, S_FAKE, S_FM  # noqa: E402

CRITIC_KEYS = ("mpd", "mrd")


def reference_losses(sums, key: str) -> dict:
    """gan.py's three batch numbers of one critic from per-row sums ``(B, subs, layers, 5)`` (``fv_disc_distance``'s columns; a tensor or an
    array): ``adv`` (gan.py:149), ``fm`` (gan.py:155) and ``disc`` (gan.py:204), as float64.  They are the reference's for rows of one
    length.  ``key`` is "mpd" or "mrd": gan.py:148 and :203 iterate the scores, which for MPD is a list over sub-discriminators — a mean
    over (B, n) per sub-discriminator, summed — but for MRD the concatenated (B, sum n) tensor, which iterates by batch ROW: a mean over
    all resolutions' scores per row, summed over the rows."""
    if key not in CRITIC_KEYS:
        raise ValueError(f"reference_losses: key = {key!r} must be one of {CRITIC_KEYS}")
    s = sums.detach().to("cpu", torch.float64) if torch.is_tensor(sums) else torch.as_tensor(sums, dtype=torch.float64)
    fm = float((s[..., S_FM].sum(0) / s[..., S_COUNT].sum(0)).sum())
    score = s[:, :, -1]                                         # (B, subs, 5): conv_post's map is the score
    if key == "mpd":
        n = score[..., S_COUNT].sum(0)
        adv = float((score[..., S_ADV_FAKE].sum(0) / n).sum())
        disc = float((score[..., S_ADV_REAL].sum(0) / n + score[..., S_FAKE].sum(0) / n).sum())
    else:
        n = score[..., S_COUNT].sum(1)
        adv = float((score[..., S_ADV_FAKE].sum(1) / n).sum())
        disc = float((score[..., S_ADV_REAL].sum(1) / n + score[..., S_FAKE].sum(1) / n).sum())
    return dict(adv=adv, fm=fm, disc=disc)


class CriticScores(dict):
    """``CriticDistance``'s result: per critic key a dict of per-row float64 tensors ``adv_fake`` (sum over sub-discriminators of
    mean (1 - s_fake)^2), ``adv_real`` (of mean (s_real - 1)^2), ``fm`` (sum over sub-discriminators and layers of mean |f_real - f_fake|)
    and ``sums``, the (B, subs, layers, 5) sums and counts behind them."""

    def reference_losses(self, key: str) -> dict:
        return reference_losses(self[key]["sums"], key)


class CriticDistance(nn.Module):
    """The critics' view of ragged (real, generated) pairs in one call per critic.  ``mpd`` / ``mrd``: a ``MultiPeriodDiscriminator`` /
    ``MultiResolutionDiscriminator`` of this package (either may be None).  Inference only; a row's numbers are the same bits alone and in
    any batch."""

    def __init__(self, mpd=None, mrd=None):
        super().__init__()
        if mpd is None and mrd is None:
            raise ValueError("CriticDistance: no critic (mpd= and mrd= are both None)")
        self.mpd, self.mrd = mpd, mrd
        self.eval()

    @classmethod
    def from_checkpoint(cls, path: str, periods=None, resolutions=None, map_location="cpu"):
        """The ``discriminators.mpd.`` / ``discriminators.mrd.`` prefixes of a Lightning checkpoint (``GANModel.discriminators``), loaded
        strictly.  ``periods`` / ``resolutions`` default to configs/model/gan.yaml's; a critic whose prefix the checkpoint lacks is left out."""
        from .modules.discriminators import MultiPeriodDiscriminator, MultiResolutionDiscriminator
        ckpt = torch.load(path, map_location=map_location, weights_only=True)
        state = ckpt.get("state_dict", ckpt)
        periods = [3, 5, 7, 11, 17, 23, 37] if periods is None else periods
        resolutions = [(2048, 512, 2048), (1024, 120, 600), (2048, 240, 1200)] if resolutions is None else resolutions
        critics = {}
        for key, make in (("mpd", lambda: MultiPeriodDiscriminator(periods)), ("mrd", lambda: MultiResolutionDiscriminator(resolutions))):
            pfx = f"discriminators.{key}."
            sub = {k[len(pfx):]: v for k, v in state.items() if k.startswith(pfx)}
            if sub:
                critics[key] = make()
                critics[key].load_state_dict(sub, strict=True)
        if not critics:
            raise ValueError(f"CriticDistance.from_checkpoint: {path} holds no 'discriminators.mpd.' or 'discriminators.mrd.' weights")
        return cls(**critics)

    def critics(self) -> dict:
        return {k: m for k, m in (("mpd", self.mpd), ("mrd", self.mrd)) if m is not None}

    def min_length(self) -> int:
        return max([1] + [m.min_length() for m in self.critics().values() if hasattr(m, "min_length")])

    def forward_ragged(self, real: torch.Tensor, fake: torch.Tensor, lengths) -> CriticScores:
        """Padded batches ``(B, L_max)`` or ``(B, 1, L_max)`` with ``lengths[b]`` valid samples per row."""
        real, fake = _waves(real, "forward_ragged real"), _waves(fake, "forward_ragged fake")
        if real.shape != fake.shape:
            raise ValueError(f"forward_ragged: real {tuple(real.shape)} and fake {tuple(fake.shape)} differ in shape")
        out = CriticScores()
        for key, critic in self.critics().items():
            s = critic.distance_sums(real[:, None], fake[:, None], lengths)
            mean = s[..., :4] / s[..., S_COUNT:]
            out[key] = dict(adv_fake=mean[:, :, -1, S_ADV_FAKE].sum(1), adv_real=mean[:, :, -1, S_ADV_REAL].sum(1),
                            fm=mean[..., S_FM].sum((1, 2)), sums=s)
        return out

    def forward(self, real: torch.Tensor, fake: torch.Tensor) -> CriticScores:
        """Rows of one length: ``(B, L)`` or ``(B, 1, L)``."""
        return self.forward_ragged(real, fake, None)

    def forward_list(self, reals, fakes) -> CriticScores:
        """Lists of 1-d waveforms, pair by pair: both are cropped to the shorter of the two (eval.py:70-74)."""
        reals, fakes = [t.reshape(-1) for t in reals], [p.reshape(-1) for p in fakes]
        if len(reals) != len(fakes) or not reals:
            raise ValueError(f"forward_list: {len(reals)} real waveforms for {len(fakes)} generated ones (at least one pair)")
        lengths = [min(int(t.shape[0]), int(p.shape[0])) for t, p in zip(reals, fakes)]
        shape = (len(reals), max(max(lengths), 1))
        x = torch.zeros(shape, dtype=torch.float32, device=reals[0].device)
        y = torch.zeros(shape, dtype=torch.float32, device=reals[0].device)
        for b, n in enumerate(lengths):
            x[b, :n], y[b, :n] = reals[b][:n], fakes[b][:n]
        return self.forward_ragged(x, y, lengths)
