"""Hard negatives (``ihg_sample_pool``, ``ihg_hard_negative_loss``; ``csrc/tail.hip``, contracts in ``include/ihgnn_hip.h``) restated for ``tests/test_hard_negatives_host.py`` /
``test_hard_negatives_kernels.py`` / ``test_hard_negatives_model.py``.  Not a test module; numpy on the CPU only.

POOL.  ``pool_draw`` is the sequential definition - row r's stream ``row_keys(seed, counter)[r]``, attempts from 0, attempt a yields ``mulhi(mix64(key + a C), n_items)``,
accepted iff it differs from everything accepted before, the first m accepted values in attempt order - in ``uint64`` numpy, exact to the bit: the device is held to it
with ``torch.equal``.  ``pool_draw_chunked`` is the kernel's scheme (64 attempts at a time; fresh = not in the list and not held by an earlier lane of the chunk).

SELECTION.  ``score_keys``: the monotone ``uint32`` key of a float's bits (sign bit set: ``~bits``, otherwise ``bits | 0x80000000``); ``select``: per group the first k of
the M candidates by (key descending, pool position ascending); ``compact``: ``[s_p ..] ++ [the selected scores, rank order]`` - a ``[P (1 + k)]`` batch in ``collate_fn``'s
layout, on which the loss is the existing objective.

BOUNDS.  On the compacted scores ``bpr`` / ``softmax`` are ``loss_reference.reference``'s values and bounds: that derivation counts at most k - 1 additions on a term of a
group sum and at most n - 1 on a term of the loss "in SOME order", which covers the kernel's orders here (lane chains, the xor butterfly, the trip chain, the 16-wide tree)
as it covers ``ihg_ranking_loss``'s.  ``bce`` is counted the same way (u = 2^-24, ``expf`` / ``log1pf`` at K = 2 ulp = 2 K u relative, c = 2 K; first order in u), from
``update_tail_reference.bce_reference``'s formulas with labels 1 on the P positives and 0 on the P k negatives, n = P (1 + k):
    e = expf(-|s|)   the argument is exact                                          -> relative c u
    sig              s >= 0: 1 / (1 + e), s < 0: e / (1 + e): relative sensitivity to e <= 1 -> c u; the addition and the division 2 u  -> relative (c + 2) u
    ds (label 0)     sig / n: the scale 3 u (conversion, reciprocal, product)       -> relative (c + 5) u
    ds (label 1)     (sig - 1) / n: sig's error stays ABSOLUTE through the difference, the difference rounds once, the scale 3 u
                                                                                    -> ((c + 2) u sig + 4 u |sig - 1|) / n
    term             label 0: max(s, 0) + log1pf(e), label 1: (max(s, 0) - s) + log1pf(e); the first summand is exact (0, s or -s); log1p(e) moves by at most
                     c u log1p(e) for e's error (e / ((1 + e) log1p(e)) <= 1), log1pf's own c u log1p(e); the addition u t  -> E_t = u (2 c log1p(e) + t)
    loss             n non-negative terms in some order: at most n - 1 additions on a term; the scale 3 u      -> (sum E_t + (n + 2) u sum t) / n
No constant is tuned to a measurement.

EMULATION.  ``emulate`` restates the kernel's scheme in numpy float32: the rank of a candidate counted over the group's M keys, ``selected[p][rank] = position`` and the
score into slot ``rank`` where rank < k, sums over the slots in rank order (lane l takes slots l, l + 64, .. ascending, then the xor butterfly 32 .. 1), group g on wave
g % 16 at trip g // 16, the 16 partial sums through a four-level tree.  ``MUTATIONS`` each miss a named verdict (``tests/test_hard_negatives_host.py``)."""
import functools

import numpy as np

import loss_reference as R
from logged_negatives_reference import _ATTEMPT, mix64, mulhi, row_keys

U, K_ULP = R.U, R.K_ULP
KINDS = {'bce': 0, 'bpr': 1, 'softmax': 2}
WAVE, WAVES, POOL_MAX = 64, 16, 256

# ---------------------------------------------------------------------------------------------
# the pool stream
# ---------------------------------------------------------------------------------------------
POOL_ROWS = (1, 65, 300)
POOL_M = (1, 16, 17, 64, 65, 256)


def pool_items(m):
    return tuple(dict.fromkeys((m, m + 1, 1000, 2 ** 40)))


POOL_CASES = tuple((rows, m, n_items) for rows in POOL_ROWS for m in POOL_M for n_items in pool_items(m) if m <= n_items)


@functools.lru_cache(maxsize=None)
def pool_draw(seed, counter, n_rows, n_items, m):
    """``ihg_sample_pool`` by its sequential definition -> ``[n_rows, m]`` int64 (all rows at once under a mask of the rows that still wait for a fresh value)."""
    assert 1 <= m <= min(POOL_MAX, n_items)
    keys = row_keys(seed, counter, n_rows)
    below = np.uint64(n_items)
    picked = np.full((n_rows, m), -1, np.int64)
    attempt = np.zeros(n_rows, np.uint64)
    for slot in range(m):
        waiting = np.arange(n_rows)
        while len(waiting):
            with np.errstate(over='ignore'):
                r = mix64(keys[waiting] + attempt[waiting] * _ATTEMPT)
            attempt[waiting] += np.uint64(1)
            value = mulhi(r, below).astype(np.int64)
            fresh = ~(picked[waiting, :slot] == value[:, None]).any(axis=1)
            picked[waiting[fresh], slot] = value[fresh]
            waiting = waiting[~fresh]
    picked.setflags(write=False)
    return picked


def pool_draw_chunked(seed, counter, n_rows, n_items, m, mutation=None):
    """The kernel's scheme, row by row: attempts 64 at a time, lane j taking attempt ``base + j``; fresh = not in the accepted list and not held by an earlier lane of the
    chunk; slots by the prefix count over the fresh lanes, cut at m.  ``mutation='chunk_duplicate_accepted'`` drops the earlier-lane check."""
    assert mutation in (None, 'chunk_duplicate_accepted')
    keys = row_keys(seed, counter, n_rows)
    out = np.full((n_rows, m), -1, np.int64)
    lanes = np.arange(WAVE, dtype=np.uint64)
    for row in range(n_rows):
        accepted, base = [], 0
        while len(accepted) < m:
            with np.errstate(over='ignore'):
                value = mulhi(mix64(keys[row] + (np.uint64(base) + lanes) * _ATTEMPT), np.uint64(n_items)).astype(np.int64)
            fresh = ~np.isin(value, np.asarray(accepted, np.int64))
            if mutation is None:
                first = np.unique(value, return_index=True)[1]              # the first lane that holds each value
                fresh &= np.isin(np.arange(WAVE), first)
            accepted.extend(value[fresh].tolist())
            base += WAVE
        out[row] = accepted[:m]
    return out


# ---------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------
def score_keys(scores):
    bits = np.ascontiguousarray(scores, np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def select(scores, positives, pool, keep):
    """-> ``[P, keep]`` int32: per group the pool positions of the first ``keep`` candidates by (key descending, position ascending)."""
    keys = score_keys(scores)[positives:].reshape(positives, pool).astype(np.int64)
    order = np.argsort(-keys, axis=1, kind='stable')                        # (stable: equal keys stay in position order)
    return order[:, :keep].astype(np.int32)


def compact(values, positives, pool, selected):
    """``[v_p ..] ++ [v at the selected candidates, rank order]`` -> ``[P (1 + keep)]`` (``values``: the scores, or ``dscores``)."""
    values = np.asarray(values)
    cand = values[positives:].reshape(positives, pool)
    return np.concatenate([values[:positives], np.take_along_axis(cand, selected.astype(np.int64), 1).reshape(-1)])


def selection_mask(positives, pool, selected):
    """bool ``[P (1 + pool)]``: True on the positives and on the selected candidates."""
    mask = np.zeros((positives, pool), bool)
    np.put_along_axis(mask, selected.astype(np.int64), True, 1)
    return np.concatenate([np.ones(positives, bool), mask.reshape(-1)])


# ---------------------------------------------------------------------------------------------
# float64 values and bounds
# ---------------------------------------------------------------------------------------------
def bce_reference(scores, positives, keep):
    """Float64 values and bounds of the BCE over compacted scores ``[P (1 + keep)]`` with labels 1 / 0: ``dict(loss, ds, bound_loss, bound_ds)`` (bounds absolute)."""
    P, c = positives, 2 * K_ULP
    s = np.asarray(scores, np.float64)
    n = s.shape[0]
    assert n == P * (1 + keep)
    y = np.concatenate([np.ones(P), np.zeros(n - P)])
    e = np.exp(-np.abs(s))
    sig = np.where(s >= 0, 1 / (1 + e), e / (1 + e))
    ds = (sig - y) / n
    bound = np.where(y == 0, (c + 5) * U * sig, (c + 2) * U * sig + 4 * U * np.abs(sig - 1)) / n
    soft = np.log1p(e)
    t = np.maximum(s, 0) - s * y + soft
    err = U * (2 * c * soft + t)
    return dict(loss=t.sum() / n, ds=ds, bound_loss=(err.sum() + (n + 2) * U * t.sum()) / n, bound_ds=bound)


def reference(kind, scores, positives, keep):
    return bce_reference(scores, positives, keep) if kind == 'bce' else R.reference(kind, scores, positives, keep)


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
P_LADDER = (1, 2, 15, 16, 17, 33, 1025)
M_LADDER = (2, 11, 63, 64, 65, 128, 255, 256)


def keeps_of(pool):
    return tuple(k for k in dict.fromkeys((1, 10, pool - 1, pool)) if 1 <= k <= pool)


# every P at (M, k) = (11, 10), the wave / trip edges of P at a pool beyond one chunk, every M with each of its k at P = 17
SHAPES = tuple(dict.fromkeys([(p, 11, 10) for p in P_LADDER] + [(p, 65, 10) for p in (1, 16, 17, 1025)] + [(17, m, k) for m in M_LADDER for k in keeps_of(m)]))
CORE_SHAPES = ((2, 11, 10), (17, 65, 10), (33, 128, 127), (16, 256, 256))
# 'tie' is loss_reference's (a candidate equals the positive); 'tiek': whole groups equal, and equal pairs / triples straddling the k-th place;
# 'bits': NaNs of both signs, +-inf, +-0 among the candidates
NEW_DESIGNS = ('tiek', 'bits')
DESIGNS = R.DESIGNS + NEW_DESIGNS
CASES = tuple((d, *shape) for d in ('randn1',) + NEW_DESIGNS for shape in SHAPES) + tuple((d, *shape) for d in R.DESIGNS[1:] for shape in CORE_SHAPES)
SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def scores_of(design, positives, pool, keep):
    """float32 ``[P (1 + M)]`` (read-only), seeded by the case.  ``loss_reference``'s designs are its ``scores_of`` with M in place of k."""
    P, M, k = positives, pool, keep
    if design in R.DESIGNS:
        s = R.scores_of(design, P, M).copy()
    else:
        rng = np.random.default_rng([50 + NEW_DESIGNS.index(design), P, M, k])
        s = rng.standard_normal(P * (1 + M)).astype(np.float32)
        cand = s[P:].reshape(P, M)                                          # (a view: written through below)
        if design == 'tiek':
            for p in range(P):
                if p % 3 == 0:
                    cand[p] = cand[p, 0]                                    # the whole group equal: positions 0 .. k-1 win
                elif k < M:
                    order = np.argsort(-cand[p], kind='stable')
                    width = 2 if p % 3 == 1 or k < 2 or k + 1 >= M else 3   # ranks k-1, k (and k+1) hold one value: the k-th place goes to the lowest position
                    cand[p, order[k:k - 1 + width]] = cand[p, order[k - 1]]
        else:
            n_special = max(1, (P * M) // 3)
            where = rng.choice(P * M, n_special, replace=False)
            s[P:][where] = SPECIALS[rng.integers(0, len(SPECIALS), n_special)]
    s.setflags(write=False)
    return s


# ---------------------------------------------------------------------------------------------
# the kernel's scheme in float32
# ---------------------------------------------------------------------------------------------
MUTATIONS = ('tie_higher_position', 'keep_k_plus_1', 'unselected_not_zeroed', 'nan_compared_with_gt')
# per mutation: ((kind, design, P, M, k), the verdict it must miss there - the word its AssertionError carries)
MUTATION_CASES = {
    'tie_higher_position': [(('bpr', 'tiek', 17, 65, 10), 'selected'), (('bce', 'tiek', 17, 11, 10), 'selected')],
    'keep_k_plus_1': [(('bce', 'randn1', 17, 65, 10), 'off the selection'), (('softmax', 'randn1', 2, 11, 10), 'off the selection')],
    'unselected_not_zeroed': [(('bpr', 'randn1', 17, 65, 10), 'not written'), (('bce', 'randn1', 1, 11, 10), 'not written')],
    # (a NaN is never greater and never beaten: the NaNs all land on rank 0 and the finite candidates move up - the wrong k; with k = M - 1 slots stay unwritten)
    'nan_compared_with_gt': [(('bce', 'bits', 17, 65, 10), 'selected'), (('softmax', 'bits', 17, 256, 255), 'distinct')],
}


def _softplus(x):
    f = np.float32
    return (np.maximum(x, f(0)) + np.log1p(np.exp(-np.abs(x)).astype(f)).astype(f)).astype(f)


def _sigmoid(x):
    f = np.float32
    e = np.exp(-np.abs(x)).astype(f)
    return np.where(x >= 0, f(1) / (f(1) + e), e / (f(1) + e)).astype(f)


def _wave_sum(slots, fn):
    """``[G, k]`` slots in rank order -> ``[G]``: lane l adds ``fn`` of slots l, l + 64, .. ascending, then the xor butterfly 32, 16, .. 1 (every lane ends with the same sum)."""
    f = np.float32
    G, k = slots.shape
    v = np.zeros((G, WAVE), f)
    for first in range(0, k, WAVE):
        width = min(WAVE, k - first)
        v[:, :width] += fn(slots[:, first:first + width])
    lanes = np.arange(WAVE)
    o = WAVE // 2
    while o >= 1:
        v = (v + v[:, lanes ^ o]).astype(f)
        o //= 2
    return v[:, 0]


def emulate(kind, scores, positives, pool, keep, mutation=None):
    """-> ``(loss float32, dscores float32 [P (1 + M)], selected int32 [P, keep])`` by the kernel's scheme.  ``dscores`` starts as NaN and ``selected`` as -1, as the tests'
    buffers do."""
    assert mutation is None or mutation in MUTATIONS
    f = np.float32
    P, M, k = positives, pool, keep
    s = np.asarray(scores, f)
    cand = s[P:].reshape(P, M)
    pos = np.arange(M)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        if mutation == 'nan_compared_with_gt':
            mine, other = cand[:, :, None], cand[:, None, :]
        else:
            keys = score_keys(s)[P:].reshape(P, M)
            mine, other = keys[:, :, None], keys[:, None, :]
        earlier = pos[None, None, :] > pos[None, :, None] if mutation == 'tie_higher_position' else pos[None, None, :] < pos[None, :, None]
        rank = ((other > mine) | ((other == mine) & earlier)).sum(2)       # [P, M]: how many of the group come before candidate c
        used = k + 1 if mutation == 'keep_k_plus_1' else k
        chosen = rank < used
        selected = np.full((P, k), -1, np.int32)
        kept = np.zeros((P, used), f)
        for p, c in zip(*np.nonzero(chosen)):                              # (position order, as the lanes' stores land; a later store overwrites an earlier one)
            if rank[p, c] < k:
                selected[p, rank[p, c]] = c
            kept[p, rank[p, c]] = cand[p, c]
        sp = s[:P]
        ds = np.full(s.shape, np.nan, f)
        dcand = ds[P:].reshape(P, M)                                        # (a view)
        inv_p = f(1) / f(P)
        inv_n = f(1) / f(P * (k + 1 if kind == 'bce' else k))
        if kind == 'softmax':
            m = np.fmax(sp, np.fmax.reduce(kept, 1))                       # (fmaxf: a NaN operand is passed over)
            negatives = _wave_sum(kept, lambda x: np.exp(x - m[:, None]).astype(f))
            z = (np.exp(sp - m).astype(f) + negatives).astype(f)
            terms = ((m - sp) + np.log(z).astype(f)).astype(f)
            dcand[chosen] = (np.exp(cand - m[:, None]).astype(f) / z[:, None] * inv_p)[chosen]
            ds[:P] = -(negatives / z) * inv_p
        elif kind == 'bpr':
            terms = _wave_sum(kept, lambda x: _softplus(x - sp[:, None]))
            dsum = _wave_sum(kept, lambda x: _sigmoid(x - sp[:, None]) * inv_n)
            dcand[chosen] = (_sigmoid(cand - sp[:, None]) * inv_n)[chosen]
            ds[:P] = -dsum
        else:
            e = np.exp(-np.abs(sp)).astype(f)
            terms = (_wave_sum(kept, _softplus) + ((np.maximum(sp, f(0)) - sp) + np.log1p(e).astype(f))).astype(f)
            dcand[chosen] = (_sigmoid(cand) * inv_n)[chosen]
            ds[:P] = (_sigmoid(sp) - f(1)) * inv_n
        if mutation != 'unselected_not_zeroed':
            dcand[~chosen] = f(0)
        part = np.zeros(WAVES, f)
        for first in range(0, P, WAVES):                                    # one trip: groups first .. first + 15 on waves 0 .. 15
            width = min(WAVES, P - first)
            part[:width] += terms[first:first + width]
        off = WAVES // 2
        while off > 0:
            part[:off] += part[off:2 * off]
            off //= 2
        loss = part[0] * (inv_p if kind == 'softmax' else inv_n)
    return f(loss), ds, selected


# ---------------------------------------------------------------------------------------------
# verdicts
# ---------------------------------------------------------------------------------------------
def verdicts(kind, design, scores, positives, pool, keep, loss, ds, selected):
    """Hold ``(loss, dscores, selected)`` - the kernel's or the emulation's - to the verdicts of the case; -> the worst ``error / bound`` per output.  Raises AssertionError
    with the first verdict that misses."""
    P, M, k = positives, pool, keep
    what = f'{kind} {design} P={P} M={M} k={k}'
    ds = np.asarray(ds, np.float32)
    selected = np.asarray(selected)
    assert selected.shape == (P, k)
    # exactly k distinct in-range positions per group, whatever the scores are
    in_range = (selected >= 0) & (selected < M)
    distinct = np.array([len(set(row.tolist())) for row in selected]) == k
    assert in_range.all() and distinct.all(), f'{what}: a group without {k} distinct in-range positions (first: group {int(np.argmin(in_range.all(1) & distinct))})'
    want = select(scores, P, M, k)
    assert (selected == want).all(), f'{what}: selected differs from the reference, first in group {int(np.argmax((selected != want).any(1)))}'
    mask = selection_mask(P, M, want)
    off = ds[~mask]
    if design != 'bits':
        assert not np.isnan(ds).any(), f'{what}: dscores not written at {int(np.isnan(ds).sum())} entries'
    assert not np.isnan(off).any(), f'{what}: dscores not written at {int(np.isnan(off).sum())} unselected entries'
    assert (off.view(np.uint32) == 0).all(), f'{what}: dscores is not +0.0 off the selection at {int((off.view(np.uint32) != 0).sum())} entries'
    if design == 'bits':
        return {}
    small, small_ds = compact(scores, P, M, want), compact(ds, P, M, want)
    if kind != 'bce':
        return R.verdicts(kind, design, small, P, k, loss, small_ds)
    ref = bce_reference(small, P, k)
    assert np.isfinite(small_ds).all() and np.isfinite(loss), f'{what}: not finite'
    err = np.abs(small_ds.astype(np.float64) - ref['ds'])
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / ref['bound_ds'])
    worst = int(ratio.argmax())
    assert ratio[worst] <= 1, f'{what}: compacted dscores[{worst}] = {small_ds[worst]!r}, float64 {ref["ds"][worst]!r}, error / bound {ratio[worst]:.3f}'
    loss_ratio = abs(float(loss) - ref['loss']) / ref['bound_loss']
    assert loss_ratio <= 1, f'{what}: loss {float(loss)!r}, float64 {ref["loss"]!r}, error / bound {loss_ratio:.3f}'
    return dict(loss=loss_ratio, ds_neg=float(ratio[P:].max()), ds_pos=float(ratio[:P].max()))
