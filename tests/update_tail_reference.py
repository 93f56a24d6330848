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


# ---------------------------------------------------------------------------------------------
# The cosine head of the batch tail (``hem_cosine_fwd_kernel`` / ``hem_cosine_bwd_kernel``, csrc/tail.hip), float64, with per-entry bounds from a rounding count of
# the kernels as written (u = 2^-24, n = L ceil(d / 64): the terms a lane adds in sequence; gamma(k) = k u / (1 - k u)):
#
#   m            lam x_q + (1 - lam) x_u: an addend passes 1 - lam, its product, the sum: |dm| <= 3 u mabs, mabs = lam |x_q| + (1 - lam) |x_u| (the mix can cancel)
#   aa           one product and n - 1 + 6 additions (the lane's sequence, six shuffle steps) of positive terms:       gamma(n + 6) aa
#   mm           the same sum of squares of the ROUNDED m: (m + dm)^2 - m^2 <= (2 * 3 + 1) u |m| mabs:                  gamma(n + 6) mm + gamma(7) sum |m| mabs
#   dot          m's three roundings, the product, n + 5 additions:                                                     gamma(n + 9) sum |a| mabs
#   1 / (na nm)  two square roots (each halves its sum's relative error e and adds u: h(e + 2u), h(e) = 1 / sqrt(1 - e) - 1 >= e / 2), the clamp, the
#                product, the division:                                                                                 e_cross = h(e_aa + 2u) + h(e_mm + 2u) + 2u
#                (the clamp itself does not round, but the kernels clamp at the float32 1e-8f, 6.1e-9 = 0.1 u below the float64 1e-8 this reference clamps at.  It
#                has no term of its own: where a norm is clamped the quotient no longer carries that norm's sum and square
#                root, and the h(e + 2u) >= u of that norm, which stays in e_cross, covers the 0.1 u.  The tiny-norm edge row spends its bound on this)
#   score        dot / (na nm) + bias:   (dot's bound) / (na nm) + |cos| e_cross + u |score|
#   bwd          ds = dscores x grad_scale (x the device scalar): 2 roundings; cross = 1 / (na nm): e_cross (from the forward's stats); cosv = dot cross: one more;
#                ka = cosv / na / ra: two divisions and two norms (2 u + 2 h(e_aa + 2u)); per column t1 = m cross, t2 = ka a, their difference and the product with ds:
#                |ds| (err t1 + err t2 + (1 + 2) u (|t1| + |t2|)); the user's and the query's rows carry (1 - lam) (two roundings) and lam (one) besides
#
# all of it to first order: the sums are multiplied by SECOND_ORDER = 1 + 2^-10, which covers the products of first-order terms (each below 2^-11: asserted).
# A term whose formula has a zero factor (a zero row, lam = 0 or 1) has bound 0: it must come out exactly 0.
# ---------------------------------------------------------------------------------------------
COSINE_EPS = 1e-8
SECOND_ORDER = 1 + 2.0 ** -10


def _gamma(k):
    return k * U / (1 - k * U)


def _h(e):
    assert (e < 2.0 ** -11).all(), 'a relative error of a sum of squares is beyond first order'
    return 1 / np.sqrt(1 - e) - 1


def hem_cosine_rows(layers, rows, rows_upper, batch):
    """``(x_u, x_q, a)`` [B, L d] of a batch: layer 0 addressed by ``rows``, the layers above by ``rows_upper`` where given; a negative row is a zero row."""
    out = [[], [], []]
    for l, x in enumerate(layers):
        rr = rows_upper if (l > 0 and rows_upper is not None) else rows
        for k in range(3):
            r = rr[k * batch:(k + 1) * batch]
            out[k].append(np.where((r >= 0)[:, None], x[np.maximum(r, 0)], np.zeros((), x.dtype)))
    return [np.concatenate(o, 1) for o in out]


def hem_cosine_reference(layers, rows, rows_upper, items, bias, lam, ds):
    """``layers``: float64 ``[N_l, d]`` per layer; ``ds`` [B] float64 = dscores x the scales.  -> dict of ``score`` [B], ``stats`` [B, 3] (a.m, |a|^2, |m|^2),
    ``grads`` [3, B, L d] (user, query, item row; the unclamped norm differentiated, as torch does) and the bounds ``score_bound``, ``stats_bound``, ``grad_bound``."""
    lam = f32(lam)
    b, n_layers, dim = items.shape[0], len(layers), layers[0].shape[1]
    n = n_layers * -(-dim // 64)
    xu, xq, a = hem_cosine_rows(layers, rows, rows_upper, b)
    m, mabs = lam * xq + (1 - lam) * xu, lam * np.abs(xq) + (1 - lam) * np.abs(xu)
    dot, aa, mm = (a * m).sum(1), (a * a).sum(1), (m * m).sum(1)
    ra, rm = np.sqrt(aa), np.sqrt(mm)
    na, nm = np.maximum(ra, COSINE_EPS), np.maximum(rm, COSINE_EPS)
    cross = 1 / (na * nm)
    cos = dot * cross
    score = cos + bias[items]
    dot_b = _gamma(n + 9) * (np.abs(a) * mabs).sum(1)
    aa_b = _gamma(n + 6) * aa
    mm_b = _gamma(n + 6) * mm + _gamma(7) * (np.abs(m) * mabs).sum(1)
    rel = lambda s_b, s: np.where(s > 0, s_b / np.where(s > 0, s, 1.0), 0.0)
    h_a, h_m = _h(rel(aa_b, aa) + 2 * U), _h(rel(mm_b, mm) + 2 * U)
    e_cross = h_a + h_m + 2 * U
    cos_b = dot_b * cross + np.abs(cos) * e_cross
    score_b = SECOND_ORDER * cos_b + U * np.abs(score)
    cosv_b = cos_b + U * np.abs(cos)
    safe = lambda r: np.where(r > 0, r, 1.0)
    ka, km = np.where(ra > 0, cos / na / safe(ra), 0.0), np.where(rm > 0, cos / nm / safe(rm), 0.0)
    ka_b = np.where(ra > 0, (cosv_b + np.abs(cos) * (2 * U + 2 * h_a)) / na / safe(ra), 0.0)
    km_b = np.where(rm > 0, (cosv_b + np.abs(cos) * (2 * U + 2 * h_m)) / nm / safe(rm), 0.0)
    col = lambda v: v[:, None]
    ds_, ads = col(ds), np.abs(col(ds))
    # the item row: ds (m cross - ka a)
    t1, t2 = m * col(cross), col(ka) * a
    e1 = col(cross) * (3 * U * mabs + np.abs(m) * col(e_cross + U))
    e2 = np.abs(a) * col(ka_b + np.abs(ka) * U)
    g_item = ds_ * (t1 - t2)
    b_item = SECOND_ORDER * ads * (e1 + e2 + 3 * U * (np.abs(t1) + np.abs(t2)))
    # dm = ds (a cross - km m), then (1 - lam) dm and lam dm
    s1, s2 = a * col(cross), col(km) * m
    f1 = np.abs(s1) * col(e_cross + U)
    f2 = np.abs(m) * col(km_b) + col(np.abs(km)) * (3 * U * mabs + U * np.abs(m))
    dm = ds_ * (s1 - s2)
    dm_b = ads * (f1 + f2 + 3 * U * (np.abs(s1) + np.abs(s2)))
    mag = ads * (np.abs(s1) + np.abs(s2))
    grads = np.stack([(1 - lam) * dm, lam * dm, g_item])
    bounds = np.stack([SECOND_ORDER * (1 - lam) * (dm_b + 2 * U * mag), SECOND_ORDER * lam * (dm_b + U * mag), b_item])
    return dict(score=score, stats=np.stack([dot, aa, mm], 1), grads=grads, score_bound=score_b, stats_bound=np.stack([dot_b, aa_b, mm_b], 1), grad_bound=bounds)


def hem_cosine_float32(layers, rows, rows_upper, items, bias, lam, dscores, grad_scale, device_scale=None):
    """The two kernels in float32 numpy, in their order: a lane adds its columns layer by layer, six shuffle steps, lane 0 finishes; the backward from the forward's
    stats.  -> ``(score [B], stats [B, 4], rowgrad [3, B, L d + 1])`` (the last column: d bias)."""
    one = np.float32(1)
    lam = np.float32(lam)
    b, dim = items.shape[0], layers[0].shape[1]
    xu, xq, a = hem_cosine_rows([np.asarray(x, np.float32) for x in layers], rows, rows_upper, b)
    m = lam * xq + (one - lam) * xu
    lanes = np.zeros((3, b, 64), np.float32)
    for c in range(a.shape[1]):
        lane = (c % dim) % 64
        for k, term in enumerate((a[:, c] * m[:, c], a[:, c] * a[:, c], m[:, c] * m[:, c])):
            lanes[k][:, lane] = lanes[k][:, lane] + term
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, :, np.arange(64) ^ off]
    dot, aa, mm = lanes[0][:, 0], lanes[1][:, 0], lanes[2][:, 0]
    eps = np.float32(COSINE_EPS)
    ra, rm = np.sqrt(aa), np.sqrt(mm)
    na, nm = np.maximum(ra, eps), np.maximum(rm, eps)
    score = dot / (na * nm) + np.asarray(bias, np.float32)[items]
    stats = np.stack([dot, aa, mm, np.zeros_like(dot)], 1)
    scale = np.float32(grad_scale) if device_scale is None else np.float32(grad_scale) * np.float32(device_scale)
    ds = np.asarray(dscores, np.float32) * scale
    cross = one / (na * nm)
    cosv = dot * cross
    with np.errstate(divide='ignore', invalid='ignore'):
        ka, km = np.where(ra > 0, cosv / na / ra, np.float32(0)), np.where(rm > 0, cosv / nm / rm, np.float32(0))
    col = lambda v: v[:, None]
    dm = col(ds) * (a * col(cross) - col(km) * m)
    g_item = col(ds) * (m * col(cross) - col(ka) * a)
    zero = np.zeros((b, 1), np.float32)
    rowgrad = np.stack([np.concatenate([(one - lam) * dm, zero], 1), np.concatenate([lam * dm, zero], 1), np.concatenate([g_item, col(ds)], 1)])
    return score, stats, rowgrad


COSINE_TAIL_NODES = (40, 15, 50, 70)        # users, queries, items, rows of the upper layers' own numbering
COSINE_TAIL_EDGES = ('zero_item', 'zero_mixed', 'tiny_item', 'item_isolated', 'user_and_query_isolated', 'user_isolated', 'query_isolated')


def cosine_tail_case(n_layers, dim, batch, form, seed):
    """Operands of one call in float32 numpy.  ``form``: 'one' (every layer in one numbering), 'upper' (the layers above layer 0 in a numbering of their own, -1 for
    isolated nodes), 'typed' (the same, layer 0 to be read from three typed tables).  User 0, query 0 and item 0 are zero rows, item 1 has a norm below 1e-8 (in every
    layer they reach); the first batch rows are ``COSINE_TAIL_EDGES`` in order (a batch of one row: the edge ``seed`` names)."""
    n_u, n_q, n_i, n_up = COSINE_TAIL_NODES
    n_nodes = n_u + n_q + n_i
    rng = np.random.default_rng([n_layers, dim, batch, seed, ('one', 'upper', 'typed').index(form)])
    layer0 = rng.standard_normal((n_nodes, dim)).astype(np.float32)
    above = [rng.standard_normal((n_nodes if form == 'one' else n_up, dim)).astype(np.float32) for _ in range(n_layers - 1)]
    special = {'user0': 0, 'query0': n_u, 'item0': n_u + n_q, 'item1': n_u + n_q + 1}
    for x in [layer0] + (above if form == 'one' else []):
        x[[special['user0'], special['query0'], special['item0']]] = 0
        x[special['item1']] = (1e-10 * rng.standard_normal(dim)).astype(np.float32)
    users, queries, items = rng.integers(1, n_u, batch), rng.integers(1, n_q, batch), rng.integers(2, n_i, batch)
    edges = list(COSINE_TAIL_EDGES) if batch >= len(COSINE_TAIL_EDGES) else [COSINE_TAIL_EDGES[(seed + k) % len(COSINE_TAIL_EDGES)] for k in range(batch)]
    for r, edge in enumerate(edges):
        if edge == 'zero_item':
            items[r] = 0
        elif edge == 'zero_mixed':
            users[r], queries[r] = 0, 0
        elif edge == 'tiny_item':
            items[r] = 1
    rows = np.concatenate([users, n_u + queries, n_u + n_q + items]).astype(np.int64)
    rows_upper = None
    if form != 'one':
        rows_upper = rng.integers(0, n_up, 3 * batch).astype(np.int64)
        rows_upper[rng.random(3 * batch) < 0.2] = -1
        for r, edge in enumerate(edges):
            mine = rows_upper[r::batch]
            mine[mine < 0] = 0
            blocks = {'zero_item': (2,), 'zero_mixed': (0, 1), 'tiny_item': (2,), 'item_isolated': (2,), 'user_and_query_isolated': (0, 1), 'user_isolated': (0,),
                      'query_isolated': (1,)}[edge]
            for k in blocks:
                rows_upper[k * batch + r] = -1
    return dict(layers=[layer0] + above, rows=rows, rows_upper=rows_upper, items=items.astype(np.int64), bias=rng.standard_normal(n_i).astype(np.float32),
                dscores=(rng.standard_normal(batch) / batch).astype(np.float32), edges=edges)


def assert_cosine_tail_within_bounds(score, stats, rowgrad, want, ds, what=''):
    """Every score, every entry of ``stats`` [B, >= 3] and of ``rowgrad`` [3, B, L d + 1] (float arrays) within its bound; an entry whose bound is 0 exactly equal.
    Returns the worst ``error / bound`` of (scores, stats, row gradients)."""
    worst = []
    width = want['grads'].shape[2]
    for name, got, ref, bound in (('score', score, want['score'], want['score_bound']), ('stats', stats[:, :3], want['stats'], want['stats_bound']),
                                  ('rowgrad', rowgrad[:, :, :width], want['grads'], want['grad_bound'])):
        got = np.asarray(got, np.float64)
        assert np.isfinite(got).all(), f'{what}: {name} is not finite'
        err = np.abs(got - ref)
        exact = bound == 0
        assert (err[exact] == 0).all(), f'{what}: {name}: an entry whose formula has a zero factor is not 0'
        ratio = np.where(exact, 0.0, err / np.where(exact, 1.0, bound))
        assert (ratio <= 1).all(), f'{what}: {name}: error / bound = {float(ratio.max()):.3g} at {np.unravel_index(int(ratio.argmax()), ratio.shape)}'
        worst.append(float(ratio.max()))
    col = np.asarray(rowgrad, np.float64)[:, :, width]
    assert (col[0] == 0).all() and (col[1] == 0).all() and (np.abs(col[2] - ds) <= 2 * U * np.abs(ds)).all(), f'{what}: the bias column'
    return worst
