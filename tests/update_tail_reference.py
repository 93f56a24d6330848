"""float64 references and rounding bounds for the loss-and-update end of a training step (``tests/test_update_tail.py`` on the GPU,
``tests/test_update_tail_host.py`` on the CPU): one Adam update element by element, its two step-dependent scalars, the inputs both
suites draw, and the operation-by-operation float32 evaluation of the rule that guards the bound itself.

The Adam rule as the library's ABI receives it (``ihg_adam_step`` takes ``float`` hyper-parameters): ``lr, beta1, beta2, eps, wd`` are rounded to
float32 first, the bias corrections ``1 - beta^t`` are formed in float64, ``step_size = float32(lr / bias1)``, ``bias2_sqrt = float32(sqrt(bias2))``;
then, per element and exactly (float64 here),

    g' = g + wd p;  m' = m + (g' - m)(1 - beta1);  v' = beta2 v + (1 - beta2) g'^2;  denom = sqrt(v') / bias2_sqrt + eps;  p' = p - step_size m' / denom

Rounding count of that rule evaluated operation by operation in float32 (every operation rounds once, relative error <= u = 2^-24; division and square root are
correctly rounded, there is no fast-math, a contraction to FMA only removes a rounding; first order in u), with G = |g| + wd |p|:

* ``g'``: the product and the sum round: ``|dg'| <= 2u G`` (exact when wd = 0).
* ``v'``, scale ``S_v = beta2 v + (1 - beta2) G^2``: the second term carries g' twice (4u) and three roundings (``1 - beta2``, two products): 7u (1 - beta2) G^2;
  the first term one product: 1u beta2 v; the sum one more on everything: ``|dv'| <= 8u S_v``.  **K_v = 8.**
* ``m'``, scale ``S_m = |m| + G``: ``g' - m`` inherits 2u G and rounds once (<= u S_m): 3u S_m; ``1 - beta1`` and the product round: 5u S_m (1 - beta1); the sum rounds
  once more (|m'| <= S_m): ``|dm'| <= 6u S_m``.  **K_m = 6** (4 without weight decay).
* ``p'``, scale ``S_p = |p| + |d| + step_size / denom S_m + |d| S_v / v'`` with ``d = step_size m' / denom``: m' brings 6u step_size / denom S_m; the square root halves
  v's relative error (4u S_v / v') and rounds, the division by bias2_sqrt and the sum with eps round (3u), on |d|; the quotient and the product by step_size round
  (2u |d|); the difference rounds (u (|p| + |d|)): ``|dp'| <= u (|p| + 6 |d| + 6 step_size / denom S_m + 4 |d| S_v / v')``.  **K_p = 6.**

The scales carry the rule's two cancellations (``g + wd p`` and ``m + (g - m)(1 - beta1)``), so the bounds count roundings; they are not measurements.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
K_V, K_M, K_P = 8.0, 6.0, 6.0
TINY_SCALE = 1e-30                 # a scale in (0, TINY_SCALE): products in float32's subnormal range, left out (at most MAX_TINY_SHARE of a case)
MAX_TINY_SHARE = 0.01

HYPERS = {                         # lr, beta1, beta2, eps, weight_decay
    'plain': (3e-3, 0.9, 0.999, 1e-8, 0.0),
    'decay': (3e-3, 0.9, 0.999, 1e-8, 1e-2),
    'driver': (1e-3, 0.9, 0.999, 1e-8, 0.0),              # Helpers/GlobalSettings.py + torch.optim.Adam's defaults (Main.py)
    'beta1_zero': (1e-2, 0.0, 0.3, 1e-3, 0.0),            # beta2 < 1/2: 1 - beta2 rounds
    'long_memory': (1e-3, 0.5, 0.9999, 1e-12, 0.1),
}
STEPS = (1, 2, 7, 1000, 2049, 10 ** 6)


def f32(x) -> float:
    return float(np.float32(x))


def step_scalars(lr, beta1, beta2, t):
    """``(step_size, bias2_sqrt)`` of step ``t`` as Python floats holding float32 values."""
    lr, beta1, beta2 = f32(lr), f32(beta1), f32(beta2)
    return f32(lr / (1.0 - beta1 ** t)), f32(math.sqrt(1.0 - beta2 ** t))


def draw_inputs(count, generator, device='cpu'):
    """``p, g, m, v`` (float32 ``[count]``) with the magnitudes and the exact zeros an update goes wrong at: p normal with a leading slice exactly 0 (there p' = -update);
    m and g normal x 10^k, k uniform in -6 .. 0 and -8 .. 3, each with a slice of exact zeros; v the square of such values with a zero slice that overlaps g's (denominator =
    eps alone).  |g| <= 10^4, so g^2 is finite in float32."""
    def scaled(lo, hi):
        k = torch.randint(lo, hi + 1, (count,), generator=generator, device=device).to(torch.float32)
        return torch.randn(count, generator=generator, device=device) * torch.pow(torch.tensor(10.0, device=device), k)
    p = torch.randn(count, generator=generator, device=device)
    m, g, r = scaled(-6, 0), scaled(-8, 3).clamp_(-1e4, 1e4), scaled(-8, 3).clamp_(-1e4, 1e4)
    v = r * r
    n = count
    p[:n // 5] = 0.0
    m[n // 10: n // 10 + n // 8] = 0.0
    g[n // 8: n // 8 + n // 8] = 0.0
    v[n // 16: n // 16 + n // 8] = 0.0                       # overlaps g's zeros on [n/8, 3n/16) and p's and m's zeros in part: every combination occurs
    return p, g, m, v


def adam_reference(p, g, m, v, hyper, t):
    """The exact update and the three error scales, float64 tensors on the inputs' device: ``dict(p, m, v, S_p, S_m, S_v)``."""
    lr, beta1, beta2, eps, wd = (f32(x) for x in hyper)
    step_size, bias2_sqrt = step_scalars(lr, beta1, beta2, t)
    p, g, m, v = (x.double() for x in (p, g, m, v))
    g1 = g + wd * p
    big_g = g.abs() + wd * p.abs()
    m1 = m + (g1 - m) * (1.0 - beta1)
    v1 = beta2 * v + (1.0 - beta2) * g1 * g1
    s_v = beta2 * v + (1.0 - beta2) * big_g * big_g
    s_m = m.abs() + big_g
    denom = v1.sqrt() / bias2_sqrt + eps
    d = step_size * m1 / denom
    ratio = torch.where(v1 > 0, s_v / torch.where(v1 > 0, v1, torch.ones_like(v1)), torch.zeros_like(v1))      # (the term is dropped where v' = 0)
    s_p = p.abs() + d.abs() + step_size / denom * s_m + d.abs() * ratio
    return dict(p=p - d, m=m1, v=v1, S_p=s_p, S_m=s_m, S_v=s_v)


def adam_float32(p, g, m, v, hyper, t):
    """The rule operation by operation in numpy float32 (what the bound is derived for): ``(p', m', v')`` as float32 arrays."""
    lr, beta1, beta2, eps, wd = (np.float32(x) for x in hyper)
    step_size, bias2_sqrt = (np.float32(x) for x in step_scalars(lr, beta1, beta2, t))
    p, g, m, v = (np.asarray(x, np.float32) for x in (p, g, m, v))
    one = np.float32(1.0)
    with np.errstate(under='ignore'):
        if wd != 0:
            g = g + wd * p
        m1 = m + (g - m) * (one - beta1)
        v1 = beta2 * v + (one - beta2) * g * g
        denom = np.sqrt(v1) / bias2_sqrt + eps
        p1 = p - step_size * (m1 / denom)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


def adam_errors(got_p, got_m, got_v, ref):
    """Worst ``|got - ref| / (u scale)`` of the three tensors over the elements whose scale is at least TINY_SCALE; elements of scale exactly 0 must be exactly equal.
    -> ``dict(p, m, v, tiny_share)`` of floats."""
    out, tiny, total = {}, 0, 0
    for name, got, scale in (('p', got_p, ref['S_p']), ('m', got_m, ref['S_m']), ('v', got_v, ref['S_v'])):
        got = torch.as_tensor(got).double()
        err = (got - ref[name]).abs()
        zero = scale == 0
        assert bool((err[zero] == 0).all()), f'{name}: an element whose error scale is 0 is not exact'
        keep = scale >= TINY_SCALE
        tiny += int((~keep & ~zero).sum())
        total += scale.numel()
        assert bool(torch.isfinite(got).all()), f'{name}: not finite'
        out[name] = float((err[keep] / (U * scale[keep])).max()) if bool(keep.any()) else 0.0
    out['tiny_share'] = tiny / max(total, 1)
    return out


def assert_adam_within_bounds(errors, what=''):
    assert errors['tiny_share'] <= MAX_TINY_SHARE, f'{what}: {errors["tiny_share"]:.4f} of the elements have a subnormal-range scale'
    assert errors['v'] <= K_V and errors['m'] <= K_M and errors['p'] <= K_P, f'{what}: errors in units of u x scale {errors} above K_v, K_m, K_p = {K_V}, {K_M}, {K_P}'


# ---------------------------------------------------------------------------------------------
# mean BCE with logits and its gradient, float64
# ---------------------------------------------------------------------------------------------
BCE_SIZES = (1, 2, 1023, 1024, 1025, 3300, 33000, 100000)
BCE_EDGES = (0.0, -0.0, 1e-8, -1e-8, 16.7, -16.7, 88.8, -88.8, 104.0, -104.0, 3e4, -3e4)


def bce_inputs(n, seed=0):
    """Scores normal x 3 with the first entries at the logits a BCE goes wrong at (as many as fit), labels 0 / 1 at 10 % positives with every seventh 0.25: float32 ``[n]``."""
    gen = torch.Generator().manual_seed(1000 + seed + n)
    scores = torch.randn(n, generator=gen) * 3.0
    edges = torch.tensor(BCE_EDGES, dtype=torch.float32)
    if n >= 12:
        scores[:12] = edges
    else:                                                  # n = 1, 2: the two ends of the range, where a missing branch of the stable form is off most
        scores[:n] = edges[10:10 + n]
    labels = (torch.rand(n, generator=gen) < 0.1).to(torch.float32)
    labels[::7] = 0.25
    return scores, labels


def bce_reference(scores, labels):
    """``(mean loss, dscores * n)`` in float64 numpy: ``max(s, 0) - s y + log1p(exp(-|s|))`` and ``sigmoid(s) - y``."""
    s, y = scores.double().numpy(), labels.double().numpy()
    e = np.exp(-np.abs(s))
    loss = float((np.maximum(s, 0.0) - s * y + np.log1p(e)).mean())
    sig = np.where(s >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return loss, sig - y


# ---------------------------------------------------------------------------------------------
# HEM scores of a batch and their three row gradients, float64
# ---------------------------------------------------------------------------------------------
def hem_reference(layers, rows, rows_upper, items, bias, lam, ds):
    """``layers``: float64 numpy ``[N_l, d]`` per layer (layer 0 addressed by ``rows``, the layers above by ``rows_upper`` where given; a negative row is a zero row).
    -> ``scores [B]``, ``abs_terms [B]`` (sum of |products| + |bias|), ``grads [3, B, L d]`` (user, query, item row) and ``grad_scales`` of the same shape: the magnitude
    each entry's rounding bound is relative to (user / query: |ds w X[i]|, item: |ds| (lam |X[q]| + (1 - lam) |X[u]|))."""
    lam = f32(lam)
    b = items.shape[0]
    n_layers, dim = len(layers), layers[0].shape[1]
    scores, abs_terms = bias[items].astype(np.float64).copy(), np.abs(bias[items]).astype(np.float64)
    grads, scales = np.zeros((3, b, n_layers * dim)), np.zeros((3, b, n_layers * dim))
    for l, x in enumerate(layers):
        rr = rows_upper if (l > 0 and rows_upper is not None) else rows
        xs = []
        for k in range(3):
            r = rr[k * b:(k + 1) * b]
            xs.append(np.where((r >= 0)[:, None], x[np.maximum(r, 0)], 0.0))
        xu, xq, xi = xs
        mix = lam * xq + (1.0 - lam) * xu
        scores += (xi * mix).sum(1)
        abs_terms += (np.abs(xi) * (lam * np.abs(xq) + (1.0 - lam) * np.abs(xu))).sum(1)
        cols = slice(l * dim, (l + 1) * dim)
        grads[0][:, cols] = ds[:, None] * (1.0 - lam) * xi
        grads[1][:, cols] = ds[:, None] * lam * xi
        grads[2][:, cols] = ds[:, None] * mix
        scales[0][:, cols], scales[1][:, cols] = np.abs(grads[0][:, cols]), np.abs(grads[1][:, cols])
        scales[2][:, cols] = np.abs(ds)[:, None] * (lam * np.abs(xq) + (1.0 - lam) * np.abs(xu))
    return scores, abs_terms, grads, scales
