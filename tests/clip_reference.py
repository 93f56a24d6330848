"""float64 reference, kernel-order emulation and rounding bounds of the clipped optimizer step (``ihg_grad_sqnorm`` -> ``ihg_clip_record`` -> ``ihg_adam_step_clipped``,
csrc/tail.hip; ``tests/test_grad_clip_host.py`` on the CPU, ``tests/test_grad_clip_kernels.py`` and ``tests/test_grad_clip_model.py`` on the GPU).

The step is ``torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False)`` followed by ``Adam.step()``:

    norm = sqrt(sum g^2) over every tensor;  coef = min(max_norm / (norm + 1e-6), 1)  (torch.clamp(max=1): a NaN stays a NaN);  Adam on coef g

``max_norm`` and ``1e-6`` reach the kernel as float32, so the reference takes their float32 values; everything else is float64 here.

Bounds, counted from the kernels' operations (u = 2^-24; first order, times ``SECOND_ORDER``):

* **norm.**  Every square is exact in double (24 x 24 bits), the sum of n non-negative doubles in any tree is within (log-depth + trips) 2^-53 relative - below 1e-12 for
  any tensor list - and the double square root adds 2^-53; the conversion to float32 rounds once.  So the float32 norm is the correctly rounded float64 norm unless the
  latter lies within 1e-12 relative of a rounding boundary: **within 1 ulp** of float32 at the reference (what is asserted; 1/2 ulp + 1e-12 is what is derived), and its
  relative error is <= u (1 + 2^-20).
* **coef.**  ``norm + 1e-6f`` rounds (u), the division rounds (u), the norm's own u passes through a quotient norm / (norm + eps) <= 1: **|coef - ref| <= E_COEF u |ref|,
  E_COEF = 3**, on the unclamped quotient; the clamp is a contraction, so the clamped values differ by no more.  max_norm = inf with a finite norm gives exactly 1.
* **Adam on g coef.**  The product rounds once more: the gradient Adam sees is ``g coef_ref (1 + d)``, |d| <= E_G u, **E_G = 4**.  ``update_tail_reference`` counts the
  unclipped rule with an exact g: K_v, K_m, K_p = 8, 6, 6 on its scales (G = |g coef| + wd |p|).  With the input off by E_G u: g' carries (2 + E_G) u G; v' takes g'
  twice - K_v = 8 + 2 E_G = **16**; m' once - K_m = 6 + E_G = **10**; p' = the larger of m's share (K_m) and half of v's (K_v / 2 = 8) beside the unchanged 6 |d|:
  K_p = **10**.  Same scales, same ``adam_errors``.
* **another chunking of the same gradient** (the sharded optimizer sums its flat shard, not the parameter list): another tree over the same squares, so the double sums
  agree to 1e-12 relative and the float32 norms are each within 1 ulp of float64 - within 1 ulp of each other unless equal.  Both coefficients are then within
  ``coef_bound`` of ONE float64 coefficient, and both updates within K_v, K_m, K_p of ONE float64 reference: that, per entry, is the tolerance a one-ulp coefficient
  allows, and what ``tests/test_grad_clip_model.py`` holds the sharded step to.
"""
import numpy as np
import torch

import update_tail_reference as R

U = R.U
CHUNK = 4096                              # kAdamChunk
THREADS = 256                             # kBlockThreads: 4 waves of 64
GRID = 256 * 16                           # workgroups of one partial launch; a launch takes 24 tensors
EPS32 = float(np.float32(1e-6))
SECOND_ORDER = 1 + 2.0 ** -20
E_COEF, E_G = 3.0, 4.0
K_V, K_M, K_P = R.K_V + 2 * E_G, R.K_M + E_G, max(R.K_P, R.K_M + E_G, R.K_V / 2 + E_G)
assert (K_V, K_M, K_P) == (16.0, 10.0, 10.0)


# ---------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------
def norm_reference(grads) -> float:
    """``sqrt(sum g^2)`` over a list of float arrays, float64 (numpy's pairwise sums: relative error far below 1e-12 at these sizes)."""
    with np.errstate(over='ignore', invalid='ignore'):
        return float(np.sqrt(sum(float(np.sum(np.square(np.asarray(g, np.float64)))) for g in grads)))


def coef_reference(norm: float, max_norm: float) -> float:
    """torch's rule on float64 values: ``clamp(max_norm / (norm + 1e-6), max=1)``; a NaN quotient (norm NaN, or inf / inf) stays NaN."""
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.float64(np.float32(max_norm)) / (np.float64(norm) + EPS32)
    return float(q) if np.isnan(q) else float(min(q, 1.0))


def coef_bound(norm: float, max_norm: float) -> float:
    """Largest |coef - coef_reference| the two float32 operations and the norm's rounding allow; 0 where the quotient is exact (inf / finite -> clamped to 1) or not finite."""
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.float64(np.float32(max_norm)) / (np.float64(norm) + EPS32)
    if not np.isfinite(q):
        return 0.0
    return float(E_COEF * U * SECOND_ORDER * abs(q))


def norm_within_one_ulp(got, norm: float) -> bool:
    """float32 ``got`` against the float64 norm: bitwise alike where the reference is inf / NaN, else within one float32 ulp at the reference."""
    got = np.float32(got)
    if not np.isfinite(norm):
        return bool(np.isnan(got)) if np.isnan(norm) else bool(got == np.float32(norm))
    if np.float32(norm) == np.float32(np.inf):               # finite in double, beyond float32: the conversion overflows
        return bool(got == np.float32(np.inf))
    return bool(abs(float(got) - norm) <= float(np.spacing(np.float32(norm))))


def adam_reference_clipped(p, g, m, v, hyper, t, coef: float):
    """``update_tail_reference.adam_reference`` on ``coef g`` (the product in float64): the exact update and the three error scales."""
    return R.adam_reference(p, torch.as_tensor(g).double() * coef, m, v, hyper, t)


def assert_clipped_adam_within_bounds(errors, what=''):
    assert errors['tiny_share'] <= R.MAX_TINY_SHARE, f'{what}: {errors["tiny_share"]:.4f} of the elements have a subnormal-range scale'
    assert errors['v'] <= K_V and errors['m'] <= K_M and errors['p'] <= K_P, f'{what}: errors in units of u x scale {errors} above K_v, K_m, K_p = {K_V}, {K_M}, {K_P}'


# ---------------------------------------------------------------------------------------------
# the kernels' scheme, operation by operation (float64 sums, float32 record and update)
# ---------------------------------------------------------------------------------------------
def _block_sum(acc):
    """``block_sum_fixed_order``: ``acc`` [..., 256] per-thread doubles -> [...]: six xor-shuffle steps inside each wave of 64, then the four waves added in order."""
    v = acc.reshape(acc.shape[:-1] + (THREADS // 64, 64))
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    total = np.zeros(v.shape[:-2], np.float64)
    for w in range(THREADS // 64):
        total = total + v[..., w, 0]
    return total


def emulate_partials(g, fp32_squares=False, skip_tail=False):
    """The partials of one tensor: thread t of a chunk adds the squares of elements (t + 256 k) 4 + c, k = 0 .. 3, c = 0 .. 3, in that order, then ``_block_sum``.
    Mutations: ``fp32_squares`` squares in float32 (overflows at 1e20), ``skip_tail`` drops the elements behind the last full chunk."""
    g = np.asarray(g, np.float32).reshape(-1)
    n = g.shape[0]
    chunks = -(-n // CHUNK)
    if chunks == 0:
        return np.zeros(0, np.float64)
    padded = np.zeros(chunks * CHUNK, np.float32)
    padded[:n] = g
    if skip_tail:
        padded[(n // CHUNK) * CHUNK:] = 0
    with np.errstate(over='ignore', invalid='ignore'):
        squares = (padded * padded).astype(np.float64) if fp32_squares else np.square(padded.astype(np.float64))
        squares = squares.reshape(chunks, CHUNK // (4 * THREADS), THREADS, 4)
        acc = np.zeros((chunks, THREADS), np.float64)
        for k in range(CHUNK // (4 * THREADS)):
            for c in range(4):
                acc = acc + squares[:, k, :, c]
        return _block_sum(acc)


def emulate_finish(partials):
    """``grad_sqnorm_finish_kernel``: thread t adds partials t, t + 256, ... in order, then ``_block_sum``."""
    n = partials.shape[0]
    trips = max(-(-n // THREADS), 1)
    padded = np.zeros(trips * THREADS, np.float64)
    padded[:n] = partials
    acc = np.zeros(THREADS, np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        for trip in padded.reshape(trips, THREADS):
            acc = acc + trip
        return float(_block_sum(acc))


def emulate_sqnorm(grads, drop_chunk=None, **mutations) -> float:
    """``ihg_grad_sqnorm``: the partials of every non-empty tensor in table order (the numbering goes on through the launches), one finish.  ``drop_chunk``: that
    partial is left out (a launch that loses a chunk)."""
    partials = np.concatenate([emulate_partials(g, **mutations) for g in grads] + [np.zeros(0, np.float64)])
    if drop_chunk is not None:
        partials = np.delete(partials, drop_chunk)
    return emulate_finish(partials)


def emulate_record(total: float, max_norm: float, fmin_clamp=False, no_eps=False):
    """``clip_record_kernel`` in float32: ``(norm, coef)``.  Mutations: ``fmin_clamp`` clamps with fminf (a NaN becomes 1), ``no_eps`` leaves the 1e-6 out."""
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        norm = np.float32(np.sqrt(np.float64(total)))
        coef = np.float32(max_norm) / (norm if no_eps else norm + np.float32(1e-6))
        if fmin_clamp:
            coef = np.float32(1) if np.isnan(coef) else min(coef, np.float32(1))
        else:
            coef = np.float32(1) if coef > np.float32(1) else coef
    assert norm.dtype == np.float32 and np.asarray(coef).dtype == np.float32
    return norm, np.float32(coef)


def emulate_update(p, g, m, v, hyper, t, coef, clip_after_decay=False):
    """``adam_update<true>`` in float32: ``g coef`` first, then ``update_tail_reference.adam_float32``.  Mutation ``clip_after_decay``: the coefficient on ``g + wd p``."""
    p, g = np.asarray(p, np.float32), np.asarray(g, np.float32)
    with np.errstate(under='ignore', over='ignore', invalid='ignore'):
        if not clip_after_decay:
            return R.adam_float32(p, g * np.float32(coef), m, v, hyper, t)
        wd = np.float32(hyper[4])
        g1 = (g + wd * p) * np.float32(coef) if wd != 0 else g * np.float32(coef)
        return R.adam_float32(p, g1, m, v, hyper[:4] + (0.0,), t)


def emulate_statistics(records):
    """The three floats after the listed ``(norm, coef)`` records, from zeros: largest norm (a NaN is passed over), steps with coef < 1, steps."""
    largest, clipped, steps = np.float32(0), np.float32(0), np.float32(0)
    for norm, coef in records:
        largest = norm if norm > largest else largest
        clipped = clipped + np.float32(1 if coef < 1 else 0)
        steps = steps + np.float32(1)
    return [float(largest), float(clipped), float(steps)]


# ---------------------------------------------------------------------------------------------
# the ladder both suites walk
# ---------------------------------------------------------------------------------------------
def _cycle(n):
    counts = (5, CHUNK, 1, CHUNK + 1, 100, CHUNK - 1, 33, 2 * CHUNK)
    return [counts[k % 8] for k in range(n)]


FINISH_TRIPS = (THREADS + 1) * CHUNK + 3                    # 258 partials: a second trip of the finish kernel's thread loop
GRID_TRIPS = GRID * CHUNK + 3 * CHUNK + 17                  # 4,100 chunks: a second trip of the partial kernel's grid, the last chunk partial

# name -> element counts of the tensors of one call (a count may be ``(count, offset)``: the gradient starts ``offset`` floats behind a 16-byte boundary)
GEOMETRY = {
    'n1': [1], 'n3': [3], 'n4095': [CHUNK - 1], 'n4096': [CHUNK], 'n4097': [CHUNK + 1], 'n8193': [2 * CHUNK + 1],
    'two': [CHUNK + 1, 7],
    'empties': [0, 7, 0, 0, CHUNK + 1, 0],
    'unaligned': [(3 * CHUNK + 5, 1), (CHUNK, 1), (9, 3)],
    'tensors24': _cycle(24), 'tensors25': _cycle(25), 'tensors49': _cycle(49),
    'finish_trips': [FINISH_TRIPS],
}
DESIGNS = ('zero', 'three_four', 'randn', 'huge', 'nan', 'inf')


def count_of(spec):
    return spec if isinstance(spec, int) else spec[0]


def offset_of(spec):
    return 0 if isinstance(spec, int) else spec[1]


def draw(specs, design, seed):
    """``[(p, g, m, v)]`` float32 torch tensors on the CPU, one quadruple per spec: ``update_tail_reference.draw_inputs`` with the gradient replaced per design -
    zero; 3 and 4 in the first and the last element of the list (norm exactly 5); randn (the drawn one); one 1e20 among entries of 1e-3 scale; one NaN; one inf."""
    gen = torch.Generator().manual_seed(seed)
    out = [list(R.draw_inputs(count_of(spec), gen)) for spec in specs]
    live = [k for k, spec in enumerate(specs) if count_of(spec) > 0]
    if design == 'randn':
        return [tuple(x) for x in out]
    for x in out:
        x[1] = torch.zeros_like(x[1]) if design in ('zero', 'three_four') else torch.randn(x[1].shape, generator=gen) * 1e-3
    first, last = out[live[0]][1], out[live[-1]][1]
    if design == 'three_four':
        if len(live) == 1 and first.numel() == 1:            # (a list of one element cannot hold both: it gets the 5 itself)
            first[0] = 5.0
        else:
            first[0], last[-1] = 3.0, 4.0
    elif design == 'huge':
        last[-1] = 1e20
    elif design == 'nan':
        last[-1] = float('nan')
    elif design == 'inf':
        first[0] = float('inf')
    return [tuple(x) for x in out]
