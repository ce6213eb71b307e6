"""The fp64 restatement of the quantiser's arithmetic (vocoder_amd/modules/quantizers.py) the VQ tests compare against, and the
per-frame decidability bound that says which frames a correct fp32 search MUST agree on.

    h_j = fl32(|e_j|^2 / 2), the square sum formed in fp64            s_j = x . e_j - h_j, formed in fp64 from the fp32 inputs
    code = argmax_j s_j: lowest index on equal scores, a NaN score never wins, code 0 when every score is NaN
    r_0 = x;  r_{q+1} = fl32(r_q - e_{c_q});  z = ((e_{c_0} + e_{c_1}) + ...) in fp32       (elementwise fp32 ops are correctly rounded:
                                                                                                identical on every device)
Decidability: an fp32 dot product of D terms, summed in ANY order, misses the exact one by at most gamma sum_d |r_d e_d| with
gamma = D u / (1 - D u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), so two codes whose fp64 scores
differ by more than  tau = 2 gamma max over the two of (sum_d |r_d e_d| + h)  cannot swap.  Nothing here is measured on the code under test.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def half_norms(embed: np.ndarray) -> np.ndarray:
    return (0.5 * (embed.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)


def gamma(D: int) -> float:
    return D * U / (1.0 - D * U)


def scores(r: np.ndarray, embed: np.ndarray) -> np.ndarray:
    """fp64 ``s (N, K)`` of frames ``r (N, D)`` against ``embed (K, D)``."""
    with np.errstate(invalid="ignore", over="ignore"):
        return r.astype(np.float64) @ embed.astype(np.float64).T - half_norms(embed).astype(np.float64)[None, :]


def magnitudes(r: np.ndarray, embed: np.ndarray) -> np.ndarray:
    """``sum_d |r_d e_d| + h`` per (frame, code): what the error bound scales with."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(r.astype(np.float64)) @ np.abs(embed.astype(np.float64)).T + half_norms(embed).astype(np.float64)[None, :]


def argmax_lowest(s: np.ndarray) -> np.ndarray:
    """Lowest index of the greatest non-NaN score per row; 0 where every score is NaN."""
    t = np.where(np.isnan(s), -np.inf, s)
    return np.argmax(t, axis=1)        # numpy returns the first occurrence of the maximum


def search(r: np.ndarray, embed: np.ndarray):
    """``(codes (N,), gap (N,), tau (N,))``: the fp64 gap between the best and the second-best score and the bound it must exceed for the
    frame to be decidable at this layer.  One code: gap = inf."""
    s = scores(r, embed)
    m = magnitudes(r, embed)
    n = np.arange(len(r))
    best = argmax_lowest(s)
    if embed.shape[0] == 1:
        return best, np.full(len(r), np.inf), 2 * gamma(r.shape[1]) * m[n, best]
    t = np.where(np.isnan(s), -np.inf, s)
    t2 = t.copy()
    t2[n, best] = -np.inf
    second = np.argmax(t2, axis=1)
    with np.errstate(invalid="ignore"):
        gap = t[n, best] - t[n, second]
    gap = np.where(np.isnan(gap), 0.0, gap)          # (-inf) - (-inf): not decidable
    tau = 2 * gamma(r.shape[1]) * np.maximum(m[n, best], m[n, second])
    return best, gap, tau


def gather_sum(codes: np.ndarray, embeds) -> np.ndarray:
    """``z (N, D)`` from ``codes (n_q, N)``: e_{c_0}, then + e_{c_1} ... in fp32, layer order; a negative code contributes nothing, a frame
    with none is exact zeros."""
    N, D = codes.shape[1], embeds[0].shape[1]
    z = np.zeros((N, D), np.float32)
    has = np.zeros(N, bool)
    for q, e in enumerate(embeds[: codes.shape[0]]):
        c = codes[q]
        ok = c >= 0
        rows = e[np.where(ok, c, 0)].astype(np.float32)
        z = np.where((ok & has)[:, None], (z + rows).astype(np.float32), np.where((ok & ~has)[:, None], rows, z))
        has |= ok
    return z


def encode(x: np.ndarray, embeds):
    """``x (N, D)`` fp32 -> ``(codes (n_q, N) int64, z (N, D) fp32, decidable (N,) bool)``."""
    r = x.astype(np.float32)
    codes, decidable = [], np.ones(len(x), bool)
    for e in embeds:
        c, gap, tau = search(r, e)
        decidable &= gap > tau
        codes.append(c)
        with np.errstate(invalid="ignore"):
            r = (r - e[c]).astype(np.float32)
    codes = np.stack(codes).astype(np.int64)
    return codes, gather_sum(codes, embeds), decidable


def path_excess(x: np.ndarray, embeds, codes: np.ndarray) -> np.ndarray:
    """Along the path the given ``codes (n_q, N)`` take (r_{q+1} = fl32(r_q - e_{codes_q})): per layer and frame, how far the chosen code's
    fp64 score lies below the best one, minus tau of the two.  <= 0 everywhere for a correct search.  ``(n_q, N)``."""
    r = x.astype(np.float32)
    n = np.arange(len(x))
    out = []
    for q, e in enumerate(embeds):
        s, m = scores(r, e), magnitudes(r, e)
        best = argmax_lowest(s)
        tau = 2 * gamma(r.shape[1]) * np.maximum(m[n, best], m[n, codes[q]])
        out.append((s[n, best] - s[n, codes[q]]) - tau)
        r = (r - e[codes[q]]).astype(np.float32)
    return np.stack(out)


def literal_codes(x: np.ndarray, embed: np.ndarray) -> np.ndarray:
    """encodec's literal form in fp64: argmax of -(|x|^2 - 2 x . e + |e|^2)."""
    x64, e64 = x.astype(np.float64), embed.astype(np.float64)
    dist = -((x64 ** 2).sum(1, keepdims=True) - 2 * x64 @ e64.T + (e64 ** 2).sum(1)[None, :])
    return np.argmax(dist, axis=1)


def make_case(D: int, K: int, n_q: int, N: int, seed: int = 0):
    """The tests' inputs: Gaussian frames; layer q's codebook Gaussian with sigma = 0.8 * 0.6^q."""
    rng = np.random.default_rng([seed, D, K, n_q, N])
    x = rng.standard_normal((N, D)).astype(np.float32)
    embeds = [(0.8 * 0.6 ** q * rng.standard_normal((K, D))).astype(np.float32) for q in range(n_q)]
    return x, embeds
