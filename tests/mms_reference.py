"""Float64 numpy restatements of the two steps around MMSEncoder's backbone (the checkers of the MMS tests, like w2v_reference.py for the
backbone itself).

``normalize``      HF's ``zero_mean_unit_var_norm`` (the processor's ``do_normalize``): ``(x - mean) / sqrt(var + 1e-7)``, population variance
``nearest_index``  the source frame of ``F.interpolate(mode="nearest")``, PyTorch's legacy rule, whose arithmetic is fp32 by definition:
                   ``scale = float32(F) / float32(N)``, ``src = min(int(floor(float32(j) * scale)), F - 1)`` with one rounded fp32 product
``interpolate``    ``x.transpose(0, 1)`` of a time-major (F, H) row, then that gather: (H, N)
"""
import numpy as np

EPS = 1e-7


def normalize(x) -> np.ndarray:
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return x.copy()
    return (x - x.mean()) / np.sqrt(x.var() + EPS)


def nearest_index(F: int, N: int) -> np.ndarray:
    """(N,) int64: the source frame of every output frame."""
    scale = np.float32(F) / np.float32(N)
    prod = np.arange(N, dtype=np.float32) * scale            # float32 x float32: one rounded product per element
    assert prod.dtype == np.float32
    return np.minimum(np.floor(prod).astype(np.int64), F - 1)


def interpolate(x, N: int) -> np.ndarray:
    """x: (F, H) time major -> (H, N) channel major."""
    x = np.asarray(x)
    return np.ascontiguousarray(x[nearest_index(x.shape[0], N)].T)
