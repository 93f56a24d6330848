"""Model weights as a pure function of (state-dict key order, shapes, seed) through numpy's PCG64 stream.

The wide-model fixtures (F8: d = 128 / 256) would otherwise carry megabytes of random weights; instead the fixture
generator loads THESE into the reference model before running it and the tests regenerate the same arrays
(``numpy.random.default_rng`` streams are stable across platforms and numpy versions by policy).  Scales follow the
reference's initialisers (uniform, bound 1/sqrt(fan_in) for matrices; N(0,1) item bias), so activations have
trained-model magnitudes.
"""
import numpy as np


def seeded_state(shapes, seed):
    """``{key: float32 array}`` for ``shapes = [(key, shape), ...]`` in that order."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, shape in shapes:
        shape = tuple(int(s) for s in shape)
        if key.endswith('items_bias'):
            a = rng.standard_normal(shape)
        elif len(shape) == 2:
            a = rng.uniform(-1.0, 1.0, shape) / np.sqrt(shape[1])
            if 'embedding' in key:
                a *= 4.0                                  # embedding rows of O(1/sqrt(d)) per element x 4: products stay well above fp32 noise
        else:
            a = rng.uniform(-0.1, 0.1, shape)
        out[key] = a.astype(np.float32)
    return out


def big_gradient_digest(g, limit=20_000):
    """What a fixture keeps of a parameter gradient: all of it up to ``limit`` elements, otherwise every 4th row plus
    float64 row and column sums (the interact-kernel tests compare the full matrix with the oracle)."""
    g = np.asarray(g)
    if g.size <= limit or g.ndim != 2:
        return {'full': g.astype(np.float32)}
    return {'rows4': g[::4].astype(np.float32), 'rowsum': g.astype(np.float64).sum(1), 'colsum': g.astype(np.float64).sum(0)}


def digest_sums_cancel(g, factor=100.0):
    """True when the largest row or column sum of a digested gradient is below 1 / ``factor`` of the largest sum of magnitudes: such a sum is
    left with the float32 rounding of the GEMM that produced the gradient (which moves with the host's BLAS code path), so a fixture keeps
    that gradient whole as well."""
    g = np.asarray(g, np.float64)
    if g.size <= 20_000 or g.ndim != 2:
        return False
    return any(np.abs(g).sum(a).max() > factor * np.abs(g.sum(a)).max() for a in (0, 1))
