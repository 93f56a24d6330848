"""Filtered negatives (``ihg_sample_pool_excluding``; ``csrc/tail.hip``, contract in ``include/ihgnn_hip.h``) restated for ``tests/test_filter_negatives_host.py`` /
``test_filter_negatives_kernels.py`` / ``test_filter_negatives_model.py``.  Not a test module; numpy on the CPU only.

``pool_draw_excluding`` is the sequential definition - row r's stream ``row_keys(seed, counter)[r]``, attempts from 0, attempt a yields ``mulhi(mix64(key + a C), n_items)``,
accepted iff it is not in list ``list_of_row[r]`` (a row id outside ``[0, n_lists)``: an empty list) and differs from everything accepted before, the first m accepted
values in attempt order - in ``uint64`` numpy, exact to the bit: the device is held to it with ``torch.equal``.  ``pool_draw_excluding_chunked`` is the kernel's scheme (64
attempts at a time; fresh = not on the list, not in the accepted list, not held by an earlier lane of the chunk); its mutation ``'list_checked_on_first_lane_only'`` looks
at the list for lane 0 of a chunk only.  ``delete_listed`` is the third statement of the same thing: the unfiltered stream with the listed values taken out."""
import numpy as np

from logged_negatives_reference import _ATTEMPT, mix64, mulhi, row_keys

WAVE, POOL_MAX = 64, 256
MUTATIONS = ('list_checked_on_first_lane_only',)

POOL_ROWS = (1, 65, 300)
POOL_M = (1, 16, 17, 64, 65, 256)
LIST_LENGTHS = (0, 1, 63, 64, 65, 100)
LONGEST = max(LIST_LENGTHS)


def pool_items(m):
    """The catalogue sizes of a case: the corner m + L = n_items only where it stays within 256 items (the draw then needs a few dozen chunks at most)."""
    sizes = (m + LONGEST, 1000, 2 ** 40)
    return tuple(dict.fromkeys(n for n in sizes if n >= m + LONGEST and (n != m + LONGEST or n <= 256)))


POOL_CASES = tuple((rows, m, n_items) for rows in POOL_ROWS for m in POOL_M for n_items in pool_items(m))


def make_lists(n_lists, n_items, lengths=LIST_LENGTHS, seed=0):
    """``n_lists`` lists in the layout of ``ops.exclusion_lists``: ``(ptr int64 [n_lists + 1], items int32)``, list l of length ``lengths[l % len(lengths)]``, ascending
    and distinct, uniform over ``[0, n_items)`` (over the first 2^31 - 1 values where the catalogue is larger: the ids are int32)."""
    rng = np.random.default_rng([seed, n_lists, min(n_items, 2 ** 62)])
    sizes = np.array([lengths[l % len(lengths)] for l in range(n_lists)], np.int64)
    ptr = np.zeros(n_lists + 1, np.int64)
    np.cumsum(sizes, out=ptr[1:])
    below = min(n_items, 2 ** 31 - 1)
    runs = []
    for size in sizes.tolist():
        if below <= 4096:
            run = np.sort(rng.choice(below, size, replace=False))
        else:
            run = np.unique(rng.integers(0, below, size))
            while len(run) < size:                                          # (a repeat among a hundred draws from 1000 or more: top up)
                run = np.unique(np.concatenate([run, rng.integers(0, below, size - len(run))]))
        runs.append(run.astype(np.int32))
    items = np.concatenate(runs) if runs else np.zeros(0, np.int32)
    return ptr, np.ascontiguousarray(items, np.int32)


def rows_to_lists(n_rows, n_lists, outside=True):
    """``list_of_row`` int64 ``[n_rows]``: row r reads list ``r % n_lists``; with ``outside`` one row (the middle one) carries an id outside ``[0, n_lists)`` - -1 or,
    with at least three rows, ``n_lists`` on the last one as well."""
    rows = np.arange(n_rows, dtype=np.int64) % n_lists
    if outside:
        rows[n_rows // 2] = -1
        if n_rows >= 3:
            rows[-1] = n_lists
    return rows


def _run(list_of_row, ptr, items, row):
    l = int(list_of_row[row])
    if l < 0 or l >= len(ptr) - 1:
        return np.zeros(0, np.int64)
    return np.asarray(items[ptr[l]:ptr[l + 1]], np.int64)


def _padded_runs(list_of_row, ptr, items):
    """``[n_rows, longest]`` int64: every row's list, padded with -1 (no value is -1)."""
    n_rows = len(list_of_row)
    n_lists = len(ptr) - 1
    ok = (list_of_row >= 0) & (list_of_row < n_lists)
    safe = np.where(ok, list_of_row, 0)
    first = np.where(ok, ptr[safe], 0)
    length = np.where(ok, ptr[safe + 1] - ptr[safe], 0)
    width = int(length.max(initial=0))
    padded = np.full((n_rows, max(width, 1)), -1, np.int64)
    for j in range(width):
        has = length > j
        padded[has, j] = items[first[has] + j]
    return padded


def pool_draw_excluding(seed, counter, n_rows, n_items, m, list_of_row, ptr, items):
    """``ihg_sample_pool_excluding`` by its sequential definition -> ``[n_rows, m]`` int64 (all rows at once under a mask of the rows that still wait for a fresh value)."""
    list_of_row, ptr, items = np.asarray(list_of_row, np.int64), np.asarray(ptr, np.int64), np.asarray(items, np.int64)
    assert 1 <= m <= min(POOL_MAX, n_items) and len(list_of_row) == n_rows
    listed = _padded_runs(list_of_row, ptr, items)
    assert m + int((listed >= 0).sum(1).max(initial=0)) <= n_items
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
            fresh = ~(picked[waiting, :slot] == value[:, None]).any(axis=1) & ~(listed[waiting] == value[:, None]).any(axis=1)
            picked[waiting[fresh], slot] = value[fresh]
            waiting = waiting[~fresh]
    picked.setflags(write=False)
    return picked


def pool_draw_excluding_chunked(seed, counter, n_rows, n_items, m, list_of_row, ptr, items, mutation=None, chunks=None):
    """The kernel's scheme, row by row: attempts 64 at a time, lane j taking attempt ``base + j``; fresh = not on the row's list, not in the accepted list and not held by an
    earlier lane of the chunk; slots by the prefix count over the fresh lanes, cut at m.  ``mutation='list_checked_on_first_lane_only'`` skips the list check for the lanes
    after the first of a chunk.  ``chunks`` (a list) receives the number of chunks every row took."""
    assert mutation is None or mutation in MUTATIONS
    list_of_row, ptr, items = np.asarray(list_of_row, np.int64), np.asarray(ptr, np.int64), np.asarray(items, np.int64)
    keys = row_keys(seed, counter, n_rows)
    out = np.full((n_rows, m), -1, np.int64)
    lanes = np.arange(WAVE, dtype=np.uint64)
    for row in range(n_rows):
        run = _run(list_of_row, ptr, items, row)
        accepted, base = [], 0
        while len(accepted) < m:
            with np.errstate(over='ignore'):
                value = mulhi(mix64(keys[row] + (np.uint64(base) + lanes) * _ATTEMPT), np.uint64(n_items)).astype(np.int64)
            on_list = np.isin(value, run)
            if mutation == 'list_checked_on_first_lane_only':
                on_list[1:] = False
            fresh = ~on_list & ~np.isin(value, np.asarray(accepted, np.int64))
            first = np.unique(value, return_index=True)[1]                  # the first lane that holds each value
            fresh &= np.isin(np.arange(WAVE), first)
            accepted.extend(value[fresh].tolist())
            base += WAVE
        if chunks is not None:
            chunks.append(base // WAVE)
        out[row] = accepted[:m]
    return out


def delete_listed(unfiltered, list_of_row, ptr, items, m):
    """Row r of ``unfiltered`` (rows of the plain pool stream, long enough) without the values of its list, cut at m -> ``[n_rows, m]`` int64."""
    list_of_row, ptr, items = np.asarray(list_of_row, np.int64), np.asarray(ptr, np.int64), np.asarray(items, np.int64)
    out = np.empty((len(unfiltered), m), np.int64)
    for row, draws in enumerate(np.asarray(unfiltered)):
        kept = draws[~np.isin(draws, _run(list_of_row, ptr, items, row))]
        assert len(kept) >= m, (row, len(kept))
        out[row] = kept[:m]
    return out


# uniformity over the complement: one list over a catalogue of 40, five draws per row
UNIFORM = dict(n_items=40, listed=(0, 3, 4, 9, 17, 18, 25, 31, 38, 39), m=5, rows=20000, seed=1, counter=7)
CHI2_CRITICAL = 58.30                                                       # the 99.9 % point of chi-square at 29 degrees of freedom


def chi_square(draws, n_items, listed):
    """Pearson's chi-square of the counts of the allowed items in ``draws`` against the uniform expectation; no draw may be a listed item."""
    counts = np.bincount(np.asarray(draws).reshape(-1), minlength=n_items)
    allowed = np.setdiff1d(np.arange(n_items), np.asarray(listed))
    assert counts[np.asarray(listed)].sum() == 0
    expected = counts.sum() / len(allowed)
    return float(((counts[allowed] - expected) ** 2 / expected).sum())
