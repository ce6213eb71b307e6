"""What the critics' tests share (test_disc_host.py, test_gpu_disc.py): the parity bar, the goldens, the modules built from a fixture's config,
and the table of configs of the shape sweep with their synthetic weights, waves and float64 restatements (disc_reference.py).  The sweep's
configs have no golden from the reference: their expected values rest on the restatement alone, which the host suite pins to the
reference's goldens at the two fixture configs."""
import functools
import json
import os
import zlib

import numpy as np
import torch

import disc_reference as dref
from vocoder_amd import synthetic as syn

BAR = 1e-4      # the project's parity bar: max |d| over the expected tensor's own peak
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("mpd", "mrd")
NARROW = [1, 12, 36, 68, 100, 132]
REAL = list(dref.DEFAULT_CHANNELS)


@functools.lru_cache(maxsize=None)
def golden(kind):
    g = np.load(os.path.join(GOLDEN, f"disc_{kind}_tiny.npz"))
    return json.loads(bytes(g["config"]).decode()), int(g["seed"]), {k: g[k] for k in g.files}


def tensors(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def subs(kind, cfg) -> list:
    return cfg["periods"] if kind == "mpd" else [tuple(r) for r in cfg["resolutions"]]


def state_dict(kind, cfg, seed):
    if kind == "mpd":
        return syn.mpd_state_dict(cfg["periods"], cfg["channels"], seed=seed)
    return syn.mrd_state_dict(cfg["resolutions"], seed=seed)


def module(kind, cfg, sd=None):
    """The multi module of a fixture or sweep config (MPD with the config's channel list per DiscriminatorP), on the CPU."""
    from vocoder_amd.modules.discriminators import DiscriminatorP, MultiPeriodDiscriminator, MultiResolutionDiscriminator
    if kind == "mpd":
        m = MultiPeriodDiscriminator(cfg["periods"])
        m.discriminators = torch.nn.ModuleList(DiscriminatorP(period=p, channels=cfg["channels"]) for p in cfg["periods"])
    else:
        m = MultiResolutionDiscriminator(cfg["resolutions"])
    if sd is not None:
        res = m.load_state_dict(tensors(sd), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    return m.eval()


def extents(kind, sub, L) -> list:
    return dref.period_extents(L, sub) if kind == "mpd" else dref.resolution_extents(L, sub[0], sub[1])


def restate(kind, sub, layers, wave, dtype=np.float64, extent=None) -> list:
    """The fmap list (C, H, W) of one row under one sub-discriminator; fewer than six ``layers`` are the first convs of the stack."""
    cut = len(layers) < 6
    if kind == "mpd":
        return dref.period_forward(wave, sub, layers, dtype=dtype, extent=extent, truncated=cut)
    return dref.resolution_forward(wave, sub[0], sub[1], sub[2], layers, dtype=dtype, extent=extent, truncated=cut)


def parity(tag, got, want, bar=BAR):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
    print(f"{tag}: max |d| / peak = {err:.2e} (peak {np.abs(want).max():.3g})")
    assert np.isfinite(got).all() and err <= bar, (tag, err)
    return err


def moved(want, got) -> float:
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def bits(a) -> np.ndarray:
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b) -> bool:
    return tuple(a.shape) == tuple(b.shape) and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def golden_restated(kind, i, row):
    cfg, seed, g = golden(kind)
    layers = dref.folded_layers(state_dict(kind, cfg, seed), i, 5)
    return restate(kind, subs(kind, cfg)[i], layers, g["waves"][row, : int(g["lengths"][row])])


# -- the shape sweep ------------------------------------------------------------------------------------------------------------------------
# name -> (kind, config of ONE sub-discriminator, the lengths of its rows).  One real-width sub-discriminator per case keeps the upload small.
SWEEP = {
    # the real widths, K up to 2560: H 163 -> 55 -> 19 -> 7 -> 3, a handful of positions in the widest layers
    "real_p3": ("mpd", dict(periods=[3], channels=REAL), (489,)),
    # several M tiles in the first layers: H0 = 222 rows of 37
    "real_p37": ("mpd", dict(periods=[37], channels=REAL), (8192,)),
    # no width a multiple of 32; a single position, one folded row short of, at and past the period, and several tiles
    "narrow_p2": ("mpd", dict(periods=[2], channels=NARROW), (1, 2, 3, 8192)),
    "narrow_p11": ("mpd", dict(periods=[11], channels=NARROW), (1, 10, 11, 12, 8192)),
    "narrow_p37": ("mpd", dict(periods=[37], channels=NARROW), (1, 36, 37, 38, 8192)),
    # 513 bins; W 8 -> 4 -> 2 -> 1 -> 1 and 17 -> 9 -> 5 -> 3
    "res1024": ("mrd", dict(resolutions=[[1024, 120, 600]]), (1031, 2100)),
    # win == n_fft, 1025 bins, 8 frames
    "res2048": ("mrd", dict(resolutions=[[2048, 512, 2048]]), (4096,)),
}
SWEEP_CASES = [(name, L) for name, (_, _, Ls) in SWEEP.items() for L in Ls]
LONGEST = [(name, max(Ls)) for name, (_, _, Ls) in SWEEP.items()]      # the rows at which the last tap and the padding reach data


def sweep_seed(name) -> int:
    return zlib.crc32(name.encode()) % 100000


@functools.lru_cache(maxsize=2)
def sweep_state_dict(name):
    kind, cfg, _ = SWEEP[name]
    return state_dict(kind, cfg, sweep_seed(name))


@functools.lru_cache(maxsize=2)
def sweep_layers(name):
    return dref.folded_layers(sweep_state_dict(name), 0, 5)


def sweep_wave(name, L) -> np.ndarray:
    return np.random.default_rng(sweep_seed(name) * 1000 + L).standard_normal(L).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sweep_restated(name, L):
    """The float64 restatement of the sweep's row (name, L): computed once, shared, never written to."""
    kind, cfg, _ = SWEEP[name]
    out = restate(kind, subs(kind, cfg)[0], sweep_layers(name), sweep_wave(name, L))
    for a in out:
        a.setflags(write=False)
    return out
