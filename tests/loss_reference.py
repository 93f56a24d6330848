"""Float64 restatement of the ranking losses (``ihg_ranking_loss``, ``csrc/tail.hip``), a float32 emulation of the kernel's scheme and the per-entry bounds, for
``tests/test_loss_host.py`` / ``test_loss_kernels.py`` / ``test_loss_model.py``.  Not a test module; numpy (and torch for the differentiable composition) on the CPU only.

LAYOUT.  ``scores [P (1 + k)]``: the P positives, then the k negatives of positive p at ``P + p k .. P + (p + 1) k - 1``.  ``s_p`` the positive, ``s_pj`` its j-th negative.

    bpr      x_pj = s_pj - s_p;  loss = (1 / (P k)) sum_p sum_j softplus(x_pj);  ds_pj = sigmoid(x_pj) / (P k);  ds_p = - sum_j ds_pj
    softmax  m_p = max(s_p, s_pj);  Z_p = exp(s_p - m_p) + sum_j exp(s_pj - m_p);  loss = (1 / P) sum_p (m_p + log Z_p - s_p);
             ds_pj = exp(s_pj - m_p) / (Z_p P);  ds_p = (exp(s_p - m_p) / Z_p - 1) / P

BOUNDS.  u = 2^-24 (one rounding of fp32); ``expf`` / ``log1pf`` / ``logf`` at K = 2 ulp = 2 K u relative (the figure ``attention_reference.py`` uses); first order in u;
every constant is counted from the kernel's operations, none is tuned to a measurement.  The reference is float64 on the float32 scores.  The compiler may fuse a product
into the addition that follows it: one rounding in place of two, so the counts below (every operation rounded on its own) hold either way.  ``1 / P`` and ``1 / (P k)``
are ``1.f / float(n)``: the conversion (exact below 2^24), the reciprocal and the product with it - 3 u on whatever is scaled.

bpr, with x = x_pj and the kernel's ``x^ = fl(s_pj - s_p)`` (u |x|), ``e = expf(-|x^|)`` (relative (|x| + 2 K) u: the argument's error moves the value by that much, relatively):
    sig      x >= 0: ``1 / (1 + e)``, x < 0: ``e / (1 + e)``.  Either is a function of e with relative sensitivity <= 1 -> (|x| + 2 K) u; the addition and the division 2 u
    ds_pj    = sig / (P k): 3 u more                                                -> relative (|x| + 2 K + 5) u          [c = 2 K + 5 = 9]
    ds_p     = - (the k rounded ds_pj added j ascending, k - 1 additions)           -> sum_j bound_pj + (k - 1) u sum_j |ds_pj|
    term     t = max(x^, 0) + log1pf(e):  max(x, 0) u;  log1p(e) moves by at most log1p(e) (|x| + 2 K) u for e's error (e / ((1 + e) log1p(e)) <= 1), log1pf's own
             2 K u log1p(e);  the addition u t                                      -> E_t = u (max(x, 0) + (|x| + 4 K) log1p(e) + t)
    loss     n = P k non-negative terms added in SOME order (a thread's chain, then the 10-level tree): at most n - 1 additions on a term; the scale 3 u
                                                                                    -> (sum E_t + (n + 2) u sum t) / n
softmax, with x_i = s_i - m_p over the group's 1 + k members (m_p is exact: comparisons), ``e_i = expf(fl(x_i))``: relative r_i = (|x_i| + 2 K) u:
    N = sum_j e_pj, j ascending (positive terms)                                    -> relative R_N = sum_j e_j r_j / N + (k - 1) u
    Z = e_p + N (the kernel's order: the negatives first, then the positive)        -> relative R_Z = (sum_i e_i r_i + (k - 1) u N) / Z + u
    ds_pj    = (e_pj / Z) / P: r_j, R_Z, the division, the scale 3 u                -> relative r_j + R_Z + 4 u
    ds_p     = - (N / Z) / P (= (e_p / Z - 1) / P without its cancellation)         -> relative R_N + R_Z + 4 u
    term     t = (m - s_p) + logf(Z): u (m - s_p);  log Z moves by R_Z; logf's own 2 K u log Z (Z >= 1);  the addition u t
                                                                                    -> E_t = u (m - s_p) + R_Z + 2 K u log Z + u t
    loss     P non-negative terms in some order, the scale 3 u                      -> (sum E_t + (P + 2) u sum t) / P
group sum.  bpr: the outputs of a group add up to the rounding of ds_p's own sum alone; softmax: ``sum_j e_j / Z`` against ``N / Z`` - N's k - 1 additions, and on either
side a division, a product with 1 / P (the same Z, the same 1 / P).  Either way ``|sum_group ds| <= (k + 4) u sum_group |ds|`` (added in float64 by the test).
all equal.  x = 0, e = 1: bpr ``sig = 1 / 2`` and softmax ``e / Z = 1 / (1 + k)``, ``N / Z = k / (1 + k)`` - with P k (bpr) or P and 1 + k (softmax) powers of two every
operation is exact and ``dscores`` must EQUAL the float64 values.

EMULATION.  ``emulate`` restates the kernel's scheme in numpy float32: a thread per group (group g on thread g % 1024, trip g // 1024), j ascending, the thread's partial
sum, the 1,024-wide 10-level tree.  numpy's ``exp`` / ``log1p`` / ``log`` need not match the device library's bits.  The host test holds it to every bound on every case
the GPU file runs and shows that each of ``MUTATIONS`` misses a named one.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
K_ULP = 2
KINDS = {'bpr': 1, 'softmax': 2}
THREADS = 1024                                              # kScatterThreads: the group loop's trip

# the shape ladder: every P at k = 10, every k at P in {1, 65}; for the exact verdict of the 'equal' design P in {1, 64} x k in {1, 15}
P_LADDER = (1, 2, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1)
K_LADDER = (1, 2, 10, 15, 16, 17, 33, 100)
SHAPES = tuple(dict.fromkeys([(p, 10) for p in P_LADDER] + [(p, k) for p in (1, 65) for k in K_LADDER]))
EXACT_SHAPES = ((1, 1), (1, 15), (64, 1), (64, 15))
DESIGNS = ('randn1', 'randn8', 'equal', 'ahead60', 'behind60', 'tie')
CASES = tuple((d, p, k) for d in DESIGNS for (p, k) in SHAPES) + tuple(('equal', p, k) for (p, k) in EXACT_SHAPES if (p, k) not in SHAPES)
HUGE_SHAPES = ((1, 1), (2, 10), (65, 17), (THREADS + 1, 10))


@functools.lru_cache(maxsize=None)
def scores_of(design: str, positives: int, k: int) -> np.ndarray:
    """float32 ``[P (1 + k)]``, seeded by the case.  ``ahead60`` / ``behind60``: the positive 60 ahead of its best / behind its worst negative, the groups centred at
    +40 (even p) and -40 (odd p) - both losses depend on a group's differences only; ``tie``: negative ``p % k`` of group p equals the positive; ``huge``: +-10^4."""
    P = positives
    rng = np.random.default_rng([DESIGNS.index(design) if design in DESIGNS else 99, P, k])
    s = rng.standard_normal(P * (1 + k)).astype(np.float32)
    neg = s[P:].reshape(P, k)                               # (a view: written through below)
    if design == 'randn8':
        s *= np.float32(8)
    elif design == 'equal':
        s[:] = np.float32(0.75)
    elif design in ('ahead60', 'behind60'):
        neg += np.where(np.arange(P) % 2 == 0, 40, -40).astype(np.float32)[:, None]
        s[:P] = neg.max(1) + np.float32(60) if design == 'ahead60' else neg.min(1) - np.float32(60)
    elif design == 'tie':
        neg[np.arange(P), np.arange(P) % k] = s[:P]
    elif design == 'huge':
        s[:] = np.where(rng.random(s.shape[0]) < 0.5, -1e4, 1e4).astype(np.float32)
    elif design != 'randn1':
        raise ValueError(design)
    return s


def reference(kind: str, scores, positives: int, k: int) -> dict:
    """Float64 values and bounds: ``dict(loss, ds, bound_loss, bound_ds)`` (``ds`` / ``bound_ds`` ``[P (1 + k)]``; the bounds absolute)."""
    P, c = positives, 2 * K_ULP
    s = np.asarray(scores, np.float64)
    sp, neg = s[:P], s[P:].reshape(P, k)
    ds, bound = np.empty_like(s), np.empty_like(s)
    if kind == 'bpr':
        n = P * k
        x = neg - sp[:, None]
        e = np.exp(-np.abs(x))
        sig = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
        d = sig / n
        bd = (np.abs(x) + c + 5) * U * d
        ds[P:], bound[P:] = d.reshape(-1), bd.reshape(-1)
        ds[:P] = -d.sum(1)
        bound[:P] = bd.sum(1) + (k - 1) * U * d.sum(1)
        soft = np.log1p(e)
        t = np.maximum(x, 0) + soft
        err = U * (np.maximum(x, 0) + (np.abs(x) + 2 * c) * soft + t)
        return dict(loss=t.sum() / n, ds=ds, bound_loss=(err.sum() + (n + 2) * U * t.sum()) / n, bound_ds=bound)
    if kind == 'softmax':
        m = np.maximum(sp, neg.max(1))
        xp, xn = sp - m, neg - m[:, None]
        ep, en = np.exp(xp), np.exp(xn)
        rp, rn = (np.abs(xp) + c) * U, (np.abs(xn) + c) * U
        N = en.sum(1)
        Z = ep + N
        rel_n = (en * rn).sum(1) / N + (k - 1) * U
        rel_z = (ep * rp + (en * rn).sum(1) + (k - 1) * U * N) / Z + U
        d = en / Z[:, None] / P
        ds[P:], bound[P:] = d.reshape(-1), ((rn + rel_z[:, None] + 4 * U) * d).reshape(-1)
        ds[:P] = -(N / Z) / P                               # (= (ep / Z - 1) / P, which cancels in float64 as well where the positive is far ahead)
        bound[:P] = (rel_n + rel_z + 4 * U) * (N / Z / P)
        t = (m - sp) + np.log(Z)
        err = U * (m - sp) + rel_z + c * U * np.log(Z) + U * t
        return dict(loss=t.sum() / P, ds=ds, bound_loss=(err.sum() + (P + 2) * U * t.sum()) / P, bound_ds=bound)
    raise ValueError(kind)


def torch_loss(kind: str, scores: torch.Tensor, positives: int) -> torch.Tensor:
    """The same formulas as a differentiable torch composition, in the dtype of ``scores`` (float64 for the model tests, float32 for the timing tool)."""
    P = positives
    sp, neg = scores[:P], scores[P:].view(P, -1)
    if kind == 'bpr':
        x = neg - sp[:, None]
        return torch.logaddexp(x, torch.zeros_like(x)).mean()
    if kind == 'softmax':
        return (torch.logsumexp(torch.cat([sp[:, None], neg], 1), 1) - sp).mean()
    raise ValueError(kind)


MUTATIONS = ('drop_last_negative', 'ds_p_sign', 'bpr_mean_over_p', 'softmax_no_max_shift', 'softmax_positive_not_in_z', 'second_trip_ignored')
# the (kind, design, P, k) each mutation must miss a verdict on
MUTATION_CASES = {
    'drop_last_negative': [('bpr', 'randn1', 65, 10), ('softmax', 'randn1', 65, 10)],
    'ds_p_sign': [('bpr', 'randn1', 2, 10), ('softmax', 'randn1', 2, 10)],
    'bpr_mean_over_p': [('bpr', 'randn1', 65, 10)],
    'softmax_no_max_shift': [('softmax', 'ahead60', 65, 10), ('softmax', 'ahead60', 1, 10)],      # (exp(100) overflows without the shift)
    'softmax_positive_not_in_z': [('softmax', 'randn1', 65, 10), ('softmax', 'ahead60', 1, 1)],
    'second_trip_ignored': [('bpr', 'randn1', THREADS + 1, 10), ('softmax', 'randn1', THREADS + 1, 10)],
}


def emulate(kind: str, scores, positives: int, k: int, mutation=None):
    """-> ``(loss float32, dscores float32 [P (1 + k)])`` by the kernel's scheme in numpy float32 (see the module's head).  ``dscores`` starts as NaN, as the tests' buffers do."""
    assert mutation is None or mutation in MUTATIONS
    f = np.float32
    P = positives
    s = np.asarray(scores, f)
    ds = np.full(s.shape, np.nan, f)
    part = np.zeros(THREADS, f)
    inv_p = f(1) / f(P)
    inv_n = inv_p if mutation == 'bpr_mean_over_p' else f(1) / f(P * k)
    last = k - 1 if mutation == 'drop_last_negative' else k
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for first in range(0, P, THREADS):                  # one trip of the group loop: groups first .. first + 1023 on threads 0 .. 1023
            if first > 0 and mutation == 'second_trip_ignored':
                break
            g = np.arange(first, min(P, first + THREADS))
            acc = part[:g.shape[0]]                         # (a view: the threads' running sums)
            sp = s[g]
            col = lambda j: s[P + g * k + j]
            if kind == 'bpr':
                dsum = np.zeros(g.shape[0], f)
                for j in range(last):
                    x = col(j) - sp
                    e = np.exp(-np.abs(x)).astype(f)
                    acc += np.maximum(x, f(0)) + np.log1p(e).astype(f)
                    sig = np.where(x >= 0, f(1) / (f(1) + e), e / (f(1) + e)).astype(f)
                    d = sig * inv_n
                    ds[P + g * k + j] = d
                    dsum += d
                ds[g] = dsum if mutation == 'ds_p_sign' else -dsum
            else:
                m = sp.copy()
                for j in range(last):
                    m = np.maximum(m, col(j))
                if mutation == 'softmax_no_max_shift':
                    m = np.zeros_like(m)
                negatives = np.zeros(g.shape[0], f)
                for j in range(last):
                    negatives += np.exp(col(j) - m).astype(f)
                z = negatives if mutation == 'softmax_positive_not_in_z' else np.exp(sp - m).astype(f) + negatives
                acc += (m - sp) + np.log(z).astype(f)
                for j in range(last):
                    ds[P + g * k + j] = np.exp(col(j) - m).astype(f) / z * inv_p
                head = (negatives / z) * inv_p
                ds[g] = head if mutation == 'ds_p_sign' else -head
        if mutation == 'drop_last_negative':
            ds[P + np.arange(P) * k + k - 1] = f(0)
        off = THREADS // 2
        while off > 0:
            part[:off] += part[off:2 * off]
            off //= 2
        loss = part[0] * (inv_n if kind == 'bpr' else inv_p)
    return f(loss), ds


def power_of_two(n: int) -> bool:
    return n >= 1 and n & (n - 1) == 0


def verdicts(kind: str, design: str, scores, positives: int, k: int, loss, ds) -> dict:
    """Hold ``(loss, ds)`` - the kernel's or the emulation's, as numpy float32 - to the verdicts of the case; -> the worst ``error / bound`` per output
    (``dict(loss, ds_neg, ds_pos)``).  Raises AssertionError with the first entry that misses."""
    P = positives
    ds = np.asarray(ds, np.float64)
    loss = float(loss)
    assert np.isfinite(ds).all() and np.isfinite(loss), f'{kind} {design} P={P} k={k}: not finite'
    groups = np.concatenate([ds[:P, None], ds[P:].reshape(P, k)], 1)
    total, size = np.abs(groups.sum(1)), np.abs(groups).sum(1)
    assert (total <= (k + 4) * U * size).all(), f'{kind} {design} P={P} k={k}: a group of dscores sums to {total.max():.3e}'
    if design == 'huge':
        cap = 1.0 / (P * k) if kind == 'bpr' else 1.0 / P
        assert (ds[P:] >= 0).all() and (ds[P:] <= cap * (1 + 2 * U)).all(), f'{kind} huge P={P} k={k}: a negative\'s gradient outside [0, {cap}]'
        return {}
    ref = reference(kind, scores, P, k)
    err = np.abs(ds - ref['ds'])
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / ref['bound_ds'])
    worst = int(ratio.argmax())
    assert ratio[worst] <= 1, f'{kind} {design} P={P} k={k}: dscores[{worst}] = {ds[worst]!r}, float64 {ref["ds"][worst]!r}, error / bound {ratio[worst]:.3f}'
    loss_ratio = abs(loss - ref['loss']) / ref['bound_loss']
    assert loss_ratio <= 1, f'{kind} {design} P={P} k={k}: loss {loss!r}, float64 {ref["loss"]!r}, error / bound {loss_ratio:.3f}'
    if design == 'equal' and (power_of_two(P * k) if kind == 'bpr' else power_of_two(P) and power_of_two(1 + k)):
        assert (ds == ref['ds']).all(), f'{kind} equal P={P} k={k}: dscores must be exact'
    if design == 'ahead60' and kind == 'bpr':
        assert loss < 1e-20
    if design == 'behind60' and kind == 'bpr':
        assert 60 <= loss < 70
    return dict(loss=loss_ratio, ds_neg=float(ratio[P:].max()), ds_pos=float(ratio[:P].max()))
