"""Popularity-weighted negatives (``ihg_sample_pool_weighted``; ``csrc/tail.hip``, contract in ``include/ihgnn_hip.h``) restated for
``tests/test_popularity_negatives_host.py`` / ``test_popularity_negatives_kernels.py`` / ``test_popularity_negatives_model.py``.  Not a test module; numpy on the CPU only.

``pool_draw_weighted`` is the sequential definition - row r's stream ``row_keys(seed, counter)[r]``, attempts from 0, attempt a yields the threshold
``t = mulhi(mix64(key + a C), total)`` and the value ``i`` with ``cum[i] <= t < cum[i + 1]``, accepted iff it is not in list ``list_of_row[r]`` and differs from everything
accepted before, the first m accepted values in attempt order - in ``uint64`` numpy, exact to the bit: the device is held to it with ``torch.equal``.  It counts every row's
attempts.  ``pool_draw_weighted_chunked`` is the kernel's scheme (64 attempts at a time) with two mutations: ``'threshold_truncated_to_32_bits'`` keeps the low half of t,
``'search_takes_the_first_not_less'`` searches ``cum`` for the lower bound instead of the upper one (so a threshold that equals ``cum[i]`` lands on item ``i - 1``).

The weight tables (each a ``cum`` int64 ``[n + 1]``): ``unit`` (``cum[i] = i``: the uniform draw's own bits), ``equal`` (every weight 2^32: the same bits again),
``squares`` (weights ``((i mod 8) + 1)^2 << 29``, a ratio of 64 between neighbours of a run of eight) and ``powerlaw`` (the dataset's formula at alpha = 0.75 on the counts
``floor(1000 / (i + 1))``).  All but ``unit`` have sums beyond 2^32, so the high half of a threshold matters.

Inputs respect the launch's promises - a strictly ascending ``cum`` and ``m + longest list <= n_items`` - because a broken promise is a loop that does not end; ``GPU_CASES``
are further chosen so that no row needs more than ``MAX_ATTEMPTS`` attempts (asserted on the host).  The catalogue of 2^40 items of ``POOL_CASES`` is left out here: its
table would be 8 TB.  What it stood for there - values beyond 32 bits - is a matter of the thresholds here, which pass 2^32 at every size."""
import functools

import numpy as np

from filter_negatives_reference import LONGEST, POOL_CASES, POOL_M, POOL_ROWS, WAVE, POOL_MAX, _run, make_lists, rows_to_lists   # noqa: F401 (re-exported)
from logged_negatives_reference import _ATTEMPT, mix64, mulhi, row_keys

MUTATIONS = ('threshold_truncated_to_32_bits', 'search_takes_the_first_not_less')
MAX_ATTEMPTS = 2 ** 16
MUTATION_CHUNKS = 64                                                        # the chunks a mutated emulation is given before it is cut off
ALPHA = 0.75
N_LISTS = 13


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------
def cum_of(weights):
    weights = np.asarray(weights, np.int64)
    assert (weights >= 1).all() and float(weights.astype(np.float64).sum()) < 2.0 ** 62
    cum = np.zeros(len(weights) + 1, np.int64)
    np.cumsum(weights, out=cum[1:])
    cum.setflags(write=False)
    return cum


def dataset_weights(counts, alpha):
    """``GraphDataset.item_sampling_weights``' formula: ``max(1, rint(2^32 ((c + 1) / (c_max + 1))^alpha))`` in float64 -> int64."""
    counts = np.asarray(counts, np.float64)
    return np.maximum(1, np.rint(2.0 ** 32 * ((counts + 1.0) / (counts.max() + 1.0)) ** alpha)).astype(np.int64)


def unit_weights(n):
    return np.ones(n, np.int64)


def equal_weights(n):
    return np.full(n, 2 ** 32, np.int64)


def squares_weights(n):
    return ((np.arange(n, dtype=np.int64) % 8 + 1) ** 2) << 29


def powerlaw_weights(n):
    return dataset_weights(1000 // (np.arange(n, dtype=np.int64) + 1), ALPHA)


WEIGHTS = {'unit': unit_weights, 'equal': equal_weights, 'squares': squares_weights, 'powerlaw': powerlaw_weights}


@functools.lru_cache(maxsize=None)
def table(name, n):
    """``cum`` int64 ``[n + 1]`` of the named table over ``n`` items (read-only, made once)."""
    return cum_of(WEIGHTS[name](n))


# ---------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------
def _no_lists(n_rows):
    return np.full(n_rows, -1, np.int64), np.zeros(2, np.int64), np.zeros(0, np.int64)      # one empty list that no row names


def values_of(r, cum, mutation=None):
    """64 random bits -> the item: the threshold ``mulhi(r, total)``, then the last index with ``cum[i] <= t``."""
    t = mulhi(r, np.uint64(cum[-1]))
    if mutation == 'threshold_truncated_to_32_bits':
        t = t & np.uint64(0xFFFFFFFF)
    side = 'left' if mutation == 'search_takes_the_first_not_less' else 'right'
    return np.searchsorted(cum, t.astype(np.int64), side=side).astype(np.int64) - 1


def pool_draw_weighted(seed, counter, n_rows, n_items, m, cum, list_of_row=None, ptr=None, items=None, attempts=None):
    """``ihg_sample_pool_weighted`` by its sequential definition -> ``[n_rows, m]`` int64, row by row, every attempt judged in order.
    ``list_of_row is None``: no row has a list.  ``attempts`` (a list) receives the int64 ``[n_rows]`` number of attempts every row took."""
    cum = np.asarray(cum, np.int64)
    if list_of_row is None:
        list_of_row, ptr, items = _no_lists(n_rows)
    list_of_row, ptr, items = np.asarray(list_of_row, np.int64), np.asarray(ptr, np.int64), np.asarray(items, np.int64)
    assert 1 <= m <= min(POOL_MAX, n_items) and len(list_of_row) == n_rows and len(cum) == n_items + 1
    assert cum[0] == 0 and (np.diff(cum) >= 1).all() and n_items <= cum[-1] < 2 ** 63               # the promises: no launch, and no loop here, sees a broken one
    keys = row_keys(seed, counter, n_rows)
    picked = np.full((n_rows, m), -1, np.int64)
    attempt = np.zeros(n_rows, np.int64)
    for row in range(n_rows):
        taken = set(_run(list_of_row, ptr, items, row).tolist())           # the row's list, then also what it has accepted
        assert m + len(taken) <= n_items
        slot, start, size = 0, 0, max(WAVE, 2 * m)                          # (the block size is of no consequence: attempts are judged one by one, in order)
        while slot < m:
            with np.errstate(over='ignore'):
                value = values_of(mix64(keys[row] + np.arange(start, start + size, dtype=np.uint64) * _ATTEMPT), cum)
            for a in np.sort(np.unique(value, return_index=True)[1]).tolist():      # a later repeat inside the block is never fresh: the first occurrences, in attempt order
                if int(value[a]) not in taken:
                    taken.add(int(value[a]))
                    picked[row, slot] = value[a]
                    slot += 1
                    if slot == m:
                        attempt[row] = start + a + 1
                        break
            start, size = start + size, min(4 * size, MAX_ATTEMPTS)
    if attempts is not None:
        attempts.append(attempt)
    picked.setflags(write=False)
    return picked


def pool_draw_weighted_chunked(seed, counter, n_rows, n_items, m, cum, list_of_row=None, ptr=None, items=None, mutation=None, only=None):
    """The kernel's scheme, row by row: attempts 64 at a time, lane j taking attempt ``base + j`` and turning its threshold into a value by the search over ``cum``; fresh =
    not on the row's list, not in the accepted list and not held by an earlier lane of the chunk; slots by the prefix count over the fresh lanes, cut at m.  ``only``: the rows to draw (every row is drawn on its own; the others stay -1)."""
    assert mutation is None or mutation in MUTATIONS
    cum = np.asarray(cum, np.int64)
    if list_of_row is None:
        list_of_row, ptr, items = _no_lists(n_rows)
    list_of_row, ptr, items = np.asarray(list_of_row, np.int64), np.asarray(ptr, np.int64), np.asarray(items, np.int64)
    keys = row_keys(seed, counter, n_rows)
    out = np.full((n_rows, m), -1, np.int64)
    lanes = np.arange(WAVE, dtype=np.uint64)
    for row in (range(n_rows) if only is None else np.asarray(only).tolist()):
        run = _run(list_of_row, ptr, items, row)
        accepted, base = [], 0
        while len(accepted) < m:
            with np.errstate(over='ignore'):
                value = values_of(mix64(keys[row] + (np.uint64(base) + lanes) * _ATTEMPT), cum, mutation)
            fresh = ~np.isin(value, run) & ~np.isin(value, np.asarray(accepted, np.int64))
            first = np.unique(value, return_index=True)[1]                  # the first lane that holds each value
            fresh &= np.isin(np.arange(WAVE), first)
            accepted.extend(value[fresh].tolist())
            base += WAVE
            if mutation is not None and base >= MUTATION_CHUNKS * WAVE and len(accepted) < m:
                accepted.extend([-1] * (m - len(accepted)))          # (a mutated draw may have lost the values it needs: cut off, the rest of the row left at -1)
        out[row] = accepted[:m]
    return out


# ---------------------------------------------------------------------------------------------
# the cases of the GPU tests
# ---------------------------------------------------------------------------------------------
SEED, COUNTER = 7919 * 5 + 2, (3 << 32) + 41
STORABLE = 2 ** 24                                                          # catalogue sizes whose table a test may build (POOL_CASES' 2^40 items are not among them)
CORNER = (65, 156, 256)                                                     # rows, m, n_items with m + LONGEST = n_items: the whole complement (squares only)
GPU_CASES = tuple((rows, m, n, 'squares') for rows, m, n in POOL_CASES + (CORNER,) if n <= STORABLE) + \
    tuple((rows, m, n, 'powerlaw') for rows, m, n in POOL_CASES if n == 1000)
EQUIVALENCE_M = (1, 10, 16, 17, 100, 256)                                   # unit / equal tables against the three uniform launches, 300 rows of 1000 items


@functools.lru_cache(maxsize=None)
def lists_of(n_items):
    """The case's lists (lengths 0, 1, 63, 64, 65, 100 in turn), read-only, made once per catalogue size."""
    ptr, items = make_lists(N_LISTS, n_items)
    ptr.setflags(write=False), items.setflags(write=False)
    return ptr, items


@functools.lru_cache(maxsize=None)
def expected(rows, m, n_items, name):
    """``(want [rows, m], attempts [rows])`` of a GPU case: the sequential definition with the case's lists, computed once and left unchanged."""
    ptr, items = lists_of(n_items)
    counted = []
    want = pool_draw_weighted(SEED, COUNTER, rows, n_items, m, table(name, n_items), rows_to_lists(rows, N_LISTS), ptr, items, attempts=counted)
    counted[0].setflags(write=False)
    return want, counted[0]


# ---------------------------------------------------------------------------------------------
# distribution: the first accepted column follows the weights renormalised over the complement of the list
# ---------------------------------------------------------------------------------------------
STREAMS = ((1, 7), (39597, (3 << 32) + 41))
SQUARES_LAW = dict(table='squares', n_items=40, listed=(0, 3, 4, 9, 17, 18, 25, 31, 38, 39), rows=20000, critical=58.30)    # 29 degrees of freedom, 99.9 %
POWERLAW_LAW = dict(table='powerlaw', n_items=64, listed=(), rows=200000, critical=103.44)                                   # 63 degrees of freedom, 99.9 %


def first_draw_weighted(seed, counter, n_rows, cum, listed=()):
    """Column 0 of ``pool_draw_weighted`` with the one list ``listed`` on every row -> ``(values [n_rows], attempts [n_rows])``: the same rule for all rows at once under a
    mask of the rows that still wait (the laws need 200,000 rows; the host test holds this to ``pool_draw_weighted`` on the leading rows)."""
    cum, listed = np.asarray(cum, np.int64), np.asarray(listed, np.int64)
    keys = row_keys(seed, counter, n_rows)
    picked, attempt = np.full(n_rows, -1, np.int64), np.zeros(n_rows, np.uint64)
    waiting = np.arange(n_rows)
    while len(waiting):
        with np.errstate(over='ignore'):
            value = values_of(mix64(keys[waiting] + attempt[waiting] * _ATTEMPT), cum)
        attempt[waiting] += np.uint64(1)
        fresh = ~np.isin(value, listed)
        picked[waiting[fresh]] = value[fresh]
        waiting = waiting[~fresh]
    return picked, attempt.astype(np.int64)


def chi_square_weighted(first_column, cum, listed):
    """Pearson's chi-square of the counts of the allowed items in ``first_column`` against the weights renormalised over them -> ``(chi2, smallest expected count)``; no
    draw may be a listed item."""
    n_items = len(cum) - 1
    counts = np.bincount(np.asarray(first_column).reshape(-1), minlength=n_items)
    allowed = np.setdiff1d(np.arange(n_items), np.asarray(listed, np.int64))
    assert counts.sum() == counts[allowed].sum()
    weights = np.diff(np.asarray(cum, np.int64)).astype(np.float64)[allowed]
    want = counts.sum() * weights / weights.sum()
    return float(((counts[allowed] - want) ** 2 / want).sum()), float(want.min())
