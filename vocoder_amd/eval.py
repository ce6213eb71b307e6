"""``python -m vocoder_amd.eval SOURCE GENERATED``: the reference's eval.py on the GPU — how far a directory of generated wavs is from the
directory of source wavs they were made from.

For every file under SOURCE that matches ``--glob-pattern`` the file of the same relative path under GENERATED is its partner
(eval.py:51-65); a pair is loaded at ``--sr``, cropped to the shorter of the two (eval.py:70-74) and scored:

    spec_diff   mean |log-mel(source) - log-mel(generated)|, LogMelSpectrogram(sr, 1024, 1024, 256, 128) (eval.py:29-33, :55)
    stft_sc     spectral convergence, mean over four STFT resolutions (modules/losses/stft.py:55)          [--no-stft leaves both out]
    stft_mag    log-magnitude L1, mean over the same resolutions (modules/losses/stft.py:74)

    critic_{mpd,mrd}_{adv_fake,adv_real,fm}   with ``--critics CKPT``: what the checkpoint's discriminators make of the pair, the terms
                of models/gan.py:149, :204 and :155 per file (``vocoder_amd.scoring.CriticDistance``)

and the means over the files are printed in eval.py:95-97's format, followed by the counts of scored and skipped pairs.  ``--json PATH`` writes
the per-file values.  Pairs are scored ``--batch-size`` at a time; a pair's values do not depend on the batch it was scored in.

Differences from the reference, all printed where they bite: PESQ is not computed (a standardised CPU algorithm whose packages are not
dependencies).  PCM wav only: a generated ``.flac`` (eval.py:60-61's fallback) is reported as unsupported, there is no decoder.  A file not at
``--sr`` is resampled on the GPU with torchaudio's windowed-sinc kernel (``vocoder_amd.resample``), not librosa's soxr, as ``--resample`` of
``vocoder_amd.inference`` does; channels are averaged to mono as ``librosa.load(mono=True)`` does.  A pair whose lengths differ by 1000
samples or more is skipped (eval.py:71 asserts there), as is one too short for a front-end.  The STFT metrics use this project's
LinearSpectrogram magnitudes (``win_length = n_fft``, ``center=False``), see ``vocoder_amd.scoring.MultiResolutionSTFTDistance``.
"""
from __future__ import annotations

import argparse
import json
import sys
import wave
from dataclasses import dataclass
from pathlib import Path

MAX_LENGTH_DIFFERENCE = 1000      # eval.py:71
METRICS = ("spec_diff", "stft_sc", "stft_mag")
CRITIC_METRICS = tuple(f"critic_{key}_{name}" for key in ("mpd", "mrd") for name in ("adv_fake", "adv_real", "fm"))


@dataclass(frozen=True)
class Pair:
    name: str               # the source file's path relative to SOURCE
    source: Path
    generated: Path
    source_length: int      # samples at --sr
    generated_length: int
    length: int             # what is scored: the shorter of the two


def length_at(frames: int, rate: int, sr: int) -> int:
    """Samples of a file of ``frames`` samples at ``rate`` once it is at ``sr``: ``ceil(sr * frames / rate)``, the resampler's output length."""
    return int(frames) if rate == sr else -((-int(sr) * int(frames)) // int(rate))


def _wav_length(path: Path, sr: int) -> int:
    with wave.open(str(path), "rb") as w:
        return length_at(w.getnframes(), w.getframerate(), sr)


def plan_pairs(source, generated, sr: int, glob_pattern: str = "*.wav"):
    """The pairing of eval.py:51-74 from the directory listing and the wav headers alone (no GPU): ``(pairs, skipped)`` where ``skipped`` is a
    list of ``(name, reason)``.  Skipped: a source whose partner is missing; one whose partner exists only as ``.flac``; a pair whose lengths
    at ``sr`` differ by ``MAX_LENGTH_DIFFERENCE`` samples or more.  A smaller difference is cropped to the shorter file."""
    source, generated = Path(source), Path(generated)
    pairs, skipped = [], []
    for src in sorted(source.rglob(glob_pattern)):
        rel = src.relative_to(source)
        gen = generated / rel
        if not gen.exists():
            flac = gen.with_suffix(".flac")
            if flac.exists():
                skipped.append((str(rel), f"{flac}: .flac is not supported (PCM wav only: there is no decoder here)"))
            else:
                skipped.append((str(rel), f"{gen} does not exist"))
            continue
        try:
            ls, lg = _wav_length(src, sr), _wav_length(gen, sr)
        except (wave.Error, EOFError) as exc:
            skipped.append((str(rel), f"not a PCM wav ({exc})"))
            continue
        n = min(ls, lg)
        if max(ls - n, lg - n) >= MAX_LENGTH_DIFFERENCE:
            skipped.append((str(rel), f"lengths differ by {abs(ls - lg)} samples at {sr} Hz ({ls} and {lg}); the limit is {MAX_LENGTH_DIFFERENCE}"))
            continue
        pairs.append(Pair(str(rel), src, gen, ls, lg, n))
    return pairs, skipped


def load_mono(path, sr: int, device, resamplers: dict):
    """A PCM wav as one ``(L,)`` float32 tensor on ``device`` at ``sr``: ``inference.read_wav``, channels averaged, and the project's
    ``Resample`` (one per source rate, kept in ``resamplers``) when the file is at another rate."""
    import torch
    from .inference import read_wav
    from .resample import Resample
    audio, rate = read_wav(path)
    x = torch.from_numpy(audio.mean(axis=0, dtype="float32")).to(device)
    if rate != sr:
        if rate not in resamplers:
            resamplers[rate] = Resample(rate, sr)
        x = resamplers[rate](x[None])[0]
    return x


def score_pairs(pairs, sr: int, batch_size: int = 16, stft: bool = True, device="cuda", critics=None):
    """``(values, skipped)``: ``values[name] = {metric: float}`` for every pair scored, ``batch_size`` pairs per ``forward_list`` call.
    ``critics``: a ``CriticDistance`` whose three numbers per critic join the values."""
    if not pairs:
        return {}, []
    import torch
    from .scoring import MelDistance, MultiResolutionSTFTDistance
    device = torch.device(device)
    mel = MelDistance(sr).to(device)
    mr = MultiResolutionSTFTDistance().to(device) if stft else None
    if critics is not None:
        critics = critics.to(device)
    resamplers: dict = {}
    values, skipped, todo = {}, [], []
    for p in pairs:
        if mel.too_short(p.length) or (mr is not None and mr.too_short(p.length)) or (critics is not None and p.length < critics.min_length()):
            skipped.append((p.name, f"{p.length} samples are too few for the front-ends"))
        else:
            todo.append(p)
    for i in range(0, len(todo), max(int(batch_size), 1)):
        batch = todo[i:i + max(int(batch_size), 1)]
        src = [load_mono(p.source, sr, device, resamplers) for p in batch]
        gen = [load_mono(p.generated, sr, device, resamplers) for p in batch]
        cols = {"spec_diff": mel.forward_list(src, gen)}
        if mr is not None:
            cols["stft_sc"], cols["stft_mag"] = mr.forward_list(src, gen)
        if critics is not None:
            for key, row in critics.forward_list(src, gen).items():
                for name in ("adv_fake", "adv_real", "fm"):
                    cols[f"critic_{key}_{name}"] = row[name]
        cols = {k: v.tolist() for k, v in cols.items()}
        for b, p in enumerate(batch):
            values[p.name] = {k: cols[k][b] for k in cols}
    return values, skipped


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m vocoder_amd.eval", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="directory of source wavs")
    ap.add_argument("generated", help="directory of generated wavs, same relative paths")
    ap.add_argument("--sr", type=int, default=24000, help="rate the pairs are scored at (eval.py's default)")
    ap.add_argument("--glob-pattern", default="*.wav")
    ap.add_argument("--batch-size", type=int, default=16, help="pairs per call")
    ap.add_argument("--no-stft", action="store_true", help="spec_diff only")
    ap.add_argument("--critics", default=None, metavar="CKPT", help="a Lightning checkpoint whose discriminators.mpd. / discriminators.mrd. "
                    "weights score every pair: adds critic_{mpd,mrd}_{adv_fake,adv_real,fm}")
    ap.add_argument("--periods", type=int, nargs="+", default=None, help="the checkpoint's MPD periods (default: configs/model/gan.yaml's)")
    ap.add_argument("--resolutions", nargs="+", default=None, metavar="N_FFT,HOP,WIN", help="the checkpoint's MRD resolutions (default: gan.yaml's)")
    ap.add_argument("--json", default=None, metavar="PATH", help="write the per-file values, the means and the skipped pairs here")
    a = ap.parse_args(argv)
    for d in (a.source, a.generated):
        if not Path(d).is_dir():
            ap.error(f"{d} is not a directory")
    pairs, skipped = plan_pairs(a.source, a.generated, a.sr, a.glob_pattern)
    critics = None
    if a.critics:
        from .scoring import CriticDistance
        resolutions = None if a.resolutions is None else [tuple(int(v) for v in r.split(",")) for r in a.resolutions]
        critics = CriticDistance.from_checkpoint(a.critics, periods=a.periods, resolutions=resolutions)
    values, more = score_pairs(pairs, a.sr, a.batch_size, stft=not a.no_stft, critics=critics)
    skipped = skipped + more
    for name, reason in skipped:
        print(f"skipped {name}: {reason}")
    means = {k: sum(v[k] for v in values.values()) / len(values) for k in METRICS + CRITIC_METRICS if values and k in next(iter(values.values()))}
    print("Average scores:")
    for k, v in means.items():
        print(f"    {k}: {v:.2f}")
    print(f"scored {len(values)} pairs, skipped {len(skipped)}")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"sr": a.sr, "files": values, "mean": means, "skipped": [{"name": n, "reason": r} for n, r in skipped]}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
