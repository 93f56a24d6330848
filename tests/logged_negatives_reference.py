"""A numpy emulation of ``ihg_device_batch`` and ``ihg_sample_negatives`` (``csrc/tail.hip``; contract in ``include/ihgnn_hip.h``), exact to the bit: the kernels'
generator is integer arithmetic, so the device is held to this with ``torch.equal`` (``tests/test_logged_negatives_kernel.py``) and every statistical property is
checked here on the CPU (``tests/test_logged_negatives_host.py``).

``mix64`` is the splitmix64 finaliser in ``uint64`` with wrap-around; the high half of a 64 x 64 product is put together from 32-bit halves; the reject-and-redraw
loop runs over all rows at once under a mask of the rows that still wait for a fresh value.  No test functions."""
import numpy as np

SAMPLE_MAX = 16
POSITION_STREAM = np.uint64(0xA0761D6478BD642F)
_GOLDEN, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_ROW, _ATTEMPT = np.uint64(0xD1B54A32D192ED03), np.uint64(0x2545F4914F6CDD1D)
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def mix64(x):
    x = np.atleast_1d(np.asarray(x)).astype(np.uint64)
    with np.errstate(over='ignore'):
        x = x + _GOLDEN
        x = (x ^ (x >> np.uint64(30))) * _M1
        x = (x ^ (x >> np.uint64(27))) * _M2
    return x ^ (x >> np.uint64(31))


def mulhi(a, b):
    """The high 64 bits of the 128-bit product of two ``uint64`` arrays (``__umul64hi``)."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    a_lo, a_hi, b_lo, b_hi = a & _LOW, a >> _S32, b & _LOW, b >> _S32
    lo_lo, hi_lo, lo_hi, hi_hi = a_lo * b_lo, a_hi * b_lo, a_lo * b_hi, a_hi * b_hi            # each < 2^64
    carry = (lo_lo >> _S32) + (hi_lo & _LOW) + (lo_hi & _LOW)                                    # < 3 * 2^32
    return hi_hi + (hi_lo >> _S32) + (lo_hi >> _S32) + (carry >> _S32)


def row_keys(seed, counter, n_rows):
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    base = mix64(np.uint64(seed) ^ mix64(np.uint64(counter))[0])[0]
    with np.errstate(over='ignore'):
        return base ^ mix64(np.arange(n_rows, dtype=np.uint64) * _ROW)


def draw_distinct(keys, below, count):
    """Per row ``r``: ``count[r]`` distinct values below ``below[r]`` from the stream ``keys[r]``, attempts counted from 0 -> ``[R, max count]`` int64, -1 where a
    row draws fewer.  The kernels' ``draw_distinct``."""
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    below = np.broadcast_to(np.asarray(below, np.uint64), (n,))
    count = np.broadcast_to(np.asarray(count, np.int64), (n,))
    assert bool((count <= np.minimum(below, SAMPLE_MAX).astype(np.int64)).all())
    width = int(count.max(initial=0))
    picked = np.full((n, width), -1, np.int64)
    attempt = np.zeros(n, np.uint64)
    for slot in range(width):
        waiting = np.flatnonzero(count > slot)
        while len(waiting):
            with np.errstate(over='ignore'):
                r = mix64(keys[waiting] + attempt[waiting] * _ATTEMPT)
            attempt[waiting] += np.uint64(1)
            value = mulhi(r, below[waiting]).astype(np.int64)
            fresh = ~(picked[waiting, :slot] == value[:, None]).any(axis=1)
            picked[waiting[fresh], slot] = value[fresh]
            waiting = waiting[~fresh]
    return picked


def corpus(lengths, k_logged, n_items=50, seed=0, repeats=True):
    """Test corpus: one positive per pair, pair ``p`` with a list of ``lengths[p]`` items (from five distinct values where ``repeats``: every longer list repeats
    an item) -> ``(pos_triples [P, 3], (pair_of_edge, neg_ptr, neg_items))``."""
    rng = np.random.default_rng([seed, k_logged, len(lengths)])
    n = len(lengths)
    pos = np.stack([np.arange(n), rng.integers(0, 7, n), rng.integers(0, n_items, n)], 1).astype(np.int64)
    neg_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lengths, out=neg_ptr[1:])
    neg_items = rng.integers(0, min(n_items, 5) if repeats else n_items, int(neg_ptr[-1])).astype(np.int32)
    return pos, (np.arange(n, dtype=np.int32), neg_ptr, neg_items)


def list_lengths(k_logged, n_pairs):
    """``n_pairs`` list lengths cycling through {0, 1, k_logged - 1, k_logged, k_logged + 1, 17, 1000}: both branches of the rule and their border, in one launch."""
    ladder = sorted({x for x in (0, 1, k_logged - 1, k_logged, k_logged + 1, 17, 1000) if x >= 0})
    return np.array([ladder[p % len(ladder)] for p in range(n_pairs)], np.int64)


def sample_negatives(seed, counter, n_rows, n_items, k):
    """``ihg_sample_negatives`` -> ``[n_rows, k]`` int64."""
    assert 1 <= k <= min(SAMPLE_MAX, n_items)
    return draw_distinct(row_keys(seed, counter, n_rows), n_items, k)


def device_batch(seed, counter, pos_triples, edge_ids, tables, n_items, k_rand, k_logged):
    """``ihg_device_batch`` -> pack ``[4, n (1 + k)]`` int64; ``tables`` = ``(pair_of_edge, neg_ptr, neg_items)`` or ``None`` with ``k_logged == 0``."""
    k = k_rand + k_logged
    assert k_rand >= 0 and k_logged >= 0 and 1 <= k <= min(SAMPLE_MAX, n_items) and (tables is not None or k_logged == 0)
    pos_triples, edge_ids = np.asarray(pos_triples, np.int64).reshape(-1, 3), np.asarray(edge_ids, np.int64)
    n = len(edge_ids)
    pos = pos_triples[edge_ids]
    if k_logged:
        pair_of_edge, neg_ptr, neg_items = (np.asarray(t) for t in tables)
        pair = pair_of_edge[edge_ids].astype(np.int64)
        start, length = neg_ptr[pair], neg_ptr[pair + 1] - neg_ptr[pair]
    else:
        neg_items = np.zeros(0, np.int32)
        start = length = np.zeros(n, np.int64)
    enough = length >= k_logged
    n_random = np.where(enough, k_rand, k - length)
    n_listed = k - n_random
    keys = row_keys(seed, counter, n)
    random_items = draw_distinct(keys, n_items, n_random)
    positions = draw_distinct(keys ^ POSITION_STREAM, np.where(enough, length, SAMPLE_MAX), np.where(enough, n_listed, 0))      # (a short list is not drawn from)
    # slot by slot: a row with enough logged negatives is [drawn list entries | random items], a row with a short list [random items | the list]
    slot = np.broadcast_to(np.arange(k)[None, :], (n, k))
    full, first_listed = enough[:, None], np.where(enough, 0, n_random)[:, None]
    is_listed = np.where(full, slot < k_logged, slot >= first_listed)
    positions = np.pad(positions, ((0, 0), (0, k - positions.shape[1])))
    random_items = np.pad(random_items, ((0, 0), (0, k - random_items.shape[1])))
    in_list = np.where(full, positions, slot - first_listed)
    listed = np.append(neg_items, 0).astype(np.int64)[np.where(is_listed, start[:, None] + in_list, len(neg_items))]
    drawn = np.take_along_axis(random_items, np.where(full & ~is_listed, slot - k_logged, np.where(is_listed, 0, slot)), 1)
    negatives = np.where(is_listed, listed, drawn)
    pack = np.zeros((4, n * (1 + k)), np.int64)
    pack[:3, :n] = pos.T
    pack[3, :n] = 1
    pack[0, n:] = np.repeat(pos[:, 0], k)
    pack[1, n:] = np.repeat(pos[:, 1], k)
    pack[2, n:] = negatives.reshape(-1)
    return pack
