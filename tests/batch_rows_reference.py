"""Cases, references, verdicts and a numpy emulation for the kernels at the batch end of a training step - test infrastructure (CPU, numpy / torch only):
``ihg_batch_scatter_add``, ``ihg_batch_combine``, ``ihg_batch_rows_add``, ``ihg_batch_rows_put``, ``ihg_batch_node_rows``, ``ihg_zero_rows``, ``ihg_mark_rows``,
``ihg_zero_floats`` (``csrc/tail.hip``, ``csrc/common.hpp``) and ``ihg_compose_first_order_fwd`` / ``_bwd`` (``csrc/dense.hip``).  ``tests/test_batch_rows_kernels.py``
(GPU) and ``tests/test_batch_rows_host.py`` (CPU) read it; the product imports nothing from it.

* **References** are the operations' definitions from ``include/ihgnn_hip.h`` in float64 / int64 (``np.add.at`` over the first occurrence of every destination, plain
  matrix products for the compose pair); ``*_loops`` are the same definitions as plain Python loops, for the host test.
* **Exact cases**: integer payloads in [-8, 8] (compose: [-2, 2]); ``sum |terms|`` of every output element is asserted below 2^24 where the case is built
  (``ensure_exact``), so every summation order gives the same float32 value and the verdict is ``torch.equal`` (``aggregate_reference.assert_exact``).
* **Float cases**: normal draws whose magnitude rises with the row.  Two verdicts for the sums: (a) per element ``(m + 4) 2^-24 sum |terms|`` with m the members of
  that destination (``aggregate_reference.assert_within_float_bound``); (b) the BATCH-ORDER verdict: the header promises "duplicates summed in batch order", and
  as ``batch_scatter_kernel`` reads, a leader adds its members in ascending batch position to a float32 accumulator that starts at +0 (absent slots add an exact
  +0), then adds the accumulator once to the destination (scatter, rows_add) or stores it (combine).  ``ordered_sums`` is that sequential float32 sum; the
  comparison is on bit patterns (``assert_same_bits``).
* **Ladders** are built from the kernels' loop bounds, each builder names its constant: ``WAVE`` (``kWave``: the ballot window of the follower scan and of the
  leader's walk), ``MEMBERS`` (rows loaded per trip), ``CHUNK_COLS`` (4 x 64 columns per column chunk), ``SCATTER_MAX`` / ``SCATTER_MAX_WIDE`` (ids in 64 KiB / 128 KiB
  of LDS), ``GRID_WAVES`` (``grid_for_waves``: 2,048 workgroups of four waves before the grid-stride loop takes a second trip), ``GRID_THREADS``.
* **Emulation** (``emu_*``): the kernels' scheme in numpy float32 - follower scan, the leader's walk over absolute 64-windows in trips of 16, column chunks, the three
  destination forms; ``strided_dot``'s four partial sums and the wave butterfly for the compose pair.  Each takes a ``mutation`` that breaks it in one named way
  (``MUTATIONS``); the host test shows that the emulation passes both verdicts and every mutation fails one, on the cases the GPU file runs.
"""
from collections import namedtuple

import numpy as np
import torch

import aggregate_reference as AR

WAVE = 64                                 # kWave
MEMBERS = 16                              # batch_scatter_kernel: member rows in flight per trip
CHUNK_COLS = 4 * WAVE                     # batch_scatter_kernel: columns per column chunk (four per lane)
SCATTER_MAX = 16384                       # kScatterMax: the 64 KiB instance
SCATTER_MAX_WIDE = 32768                  # kScatterMaxWide: the 128 KiB instance; more rows are refused
GRID_WAVES = 2048 * 4                     # grid_for_waves: kMaxBlocks workgroups x kWavesPerBlock
GRID_THREADS = 2048 * 256                 # the thread-per-element kernels: kMaxBlocks x kBlockThreads
COMPOSE_WAVES = 256 * 16 * 4              # ihg_compose_first_order_bwd's grid: 4,096 workgroups of four waves
SENTINEL = np.float32(12345.678)          # the value of tests/test_aggregate_kernels.py's guards (the GPU file asserts they agree)
CAP = 1 << 24

Ref = namedtuple('Ref', 'want mag n')     # what aggregate_reference's verdicts read: float64 value, sum |terms|, number of addends (broadcastable)

MUTATIONS = ('drop_17th_member', 'drop_next_window', 'walk_from_k_plus_1', 'followers_walk_from_lo', 'merge_across_blocks', 'negative_leader', 'drop_second_chunk',
             'tail_per_lane', 'tail_low_edge', 'tail_high_edge', 'block_mod_width', 'typed_gt', 'assign_zero_fill', 'follower_overwritten', 'reverse_order',
             'compose_c_every_type', 'compose_da_without_bias_term', 'compose_tail_skipped', 'compose_second_wave_trip_skipped')


def _gen(*key):
    return np.random.default_rng([sum(ord(c) for c in k) if isinstance(k, str) else int(k) for k in key])


def ensure_exact(mag, what):
    """``sum |terms|`` of every output element of an exact case, an integer below 2^24: raises otherwise (a case beyond the cap is a broken case)."""
    mag = np.asarray(mag, np.float64)
    if mag.size and not (np.all(mag == np.round(mag)) and float(mag.max()) < CAP):
        raise ValueError(f'{what}: sum |terms| reaches {float(mag.max())}: not exact in float32')
    return float(mag.max()) if mag.size else 0.0


# =============================================================================================
# id lists.  Every builder returns [(name, rows int64 [n])]; ``listed`` puts one destination (HOT) at the given batch positions among rows of their own.
# =============================================================================================
HOT = 7


def listed(n, positions, extra=()):
    """``n`` rows with destinations of their own (100 + k), ``HOT`` at ``positions``; ``extra``: further (id, positions) groups."""
    rows = 100 + np.arange(n, dtype=np.int64)
    rows[list(positions)] = HOT
    for ident, pos in extra:
        rows[list(pos)] = ident
    return rows


def member_count_lists():
    """Members of one destination INSIDE one 64-window (``WAVE``; trips of ``MEMBERS`` = 16: one trip short, full, one more; two trips short, full, one more; the
    whole window): 1, 2, 15, 16, 17, 31, 32, 33, 63, 64 in the second of three windows; ACROSS windows: 65 and 129 (a window, the next, one more member), and
    'hundreds': one hot destination owning every other row of 700."""
    out = [(f'{m} members in one window', listed(3 * WAVE, range(WAVE, WAVE + m))) for m in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64)]
    out += [(f'{m} members across windows', listed(m + 70, range(3, 3 + m))) for m in (65, 129)]
    out.append(('hundreds of members', listed(700, range(0, 700, 2))))
    return out


def position_lists():
    """Positions inside the windows (``WAVE``; the leader's walk starts at ``k & ~63``): first occurrence at ``k % 64`` = 0, 1, 63; the last member at n - 1; members
    at ``64 m - 1`` and ``64 m``; a destination whose only later member sits in the last, partial window.  n = 150: windows [0, 64), [64, 128), [128, 150)."""
    n = 150
    return [('window positions', listed(n, (0, 64, n - 1), extra=[(8, (1, 127, 128)), (9, (63, 130)), (10, (65, 66))]))]


def random_rows(n, rng, hot=False):
    """Random destinations with many duplicates (about three rows each); ``hot``: one destination owns every other row as well."""
    rows = rng.integers(0, max(2, n // 3), n).astype(np.int64)
    if hot:
        rows[::2] = HOT
    return rows


N_LADDER = (1, 2, 63, 64, 65, GRID_WAVES, GRID_WAVES + 1, SCATTER_MAX, SCATTER_MAX + 1, SCATTER_MAX_WIDE)
WIDTH_LADDER = (1, 3, 4, 63, 64, 65, CHUNK_COLS - 1, CHUNK_COLS, CHUNK_COLS + 1, 2 * CHUNK_COLS + 1)
ROWS_N_LADDER = (1, GRID_WAVES, GRID_WAVES + 1, 20000)


def n_ladder_lists():
    """``n`` around one window (``WAVE``), around one grid of waves (``GRID_WAVES`` = 8,192: the grid-stride loop's second trip), around the 64 KiB instance
    (``SCATTER_MAX``) and at the largest launch (``SCATTER_MAX_WIDE``); from 8,192 on a hot destination owns every other row."""
    return [(f'n = {n}', random_rows(n, _gen('n ladder', n), hot=n >= GRID_WAVES)) for n in N_LADDER]


def negative_lists():
    """Negative ids (rows that take no part): alone, between two members of one destination, in the first row, in the last row."""
    return [('a negative id alone', np.array([-1], np.int64)),
            ('negative ids first, between members and last', np.array([-1, 5, -1, 5, 6, -3, 6, 7, 5, -1], np.int64)),
            ('negative ids across windows', np.where(np.arange(200) % 7 == 3, -2, np.arange(200) % 11).astype(np.int64))]


COMBINE_N = 3307                          # three blocks of 1,100 and a short one of 7; lo = 1,100 is no multiple of 64
COMBINE_N_WIDE = SCATTER_MAX + 1 + 300


def combine_block_cases():
    """``(name, rows, disjoint_block_rows)``: blocks of 0 (= n), 1, 63, 64, 65, 1,100, n and n + 1 rows over 3,307 rows (short last blocks, block starts off the
    64-windows); 16,384 (``SCATTER_MAX``: the 64 KiB instance at its capacity, a second block of 301 rows) and 16,385 (the 128 KiB instance, a second block of 300)
    over 16,685 rows.  The ids of every block are drawn from ONE range: the same id sits in several blocks, where each first occurrence is a leader of its own."""
    rows = random_rows(COMBINE_N, _gen('combine blocks'))
    wide = random_rows(COMBINE_N_WIDE, _gen('combine wide'), hot=True)
    out = [(f'blocks of {b}', rows, b) for b in (0, 1, 63, 64, 65, 1100, COMBINE_N, COMBINE_N + 1)]
    out += [(f'blocks of {b} (n = {COMBINE_N_WIDE})', wide, b) for b in (SCATTER_MAX, SCATTER_MAX + 1)]
    return out


def effective_block(n, block_rows):
    return n if block_rows <= 0 or block_rows > n else block_rows


# =============================================================================================
# cases
# =============================================================================================
class RowCase:
    """``rowgrad`` [n, ld] float32 with NaN beyond ``width``, ``rows`` [n] int64.  Exact: integers in [-8, 8]; float: normal draws times 2^(0 .. 11) rising along the rows."""

    def __init__(self, name, rows, width, exact=True, pad=5, values=None):
        self.name, self.rows, self.width, self.exact = name, np.asarray(rows, np.int64), int(width), exact
        n = len(self.rows)
        rng = _gen(name, n, width, int(exact))
        self.rowgrad = np.full((n, width + pad), np.nan, np.float32)
        if values is not None:
            self.rowgrad[:, :width] = values
        elif exact:
            self.rowgrad[:, :width] = rng.integers(-8, 9, (n, width))
        else:
            self.rowgrad[:, :width] = rng.standard_normal((n, width)) * np.ldexp(1.0, np.arange(n) * 12 // max(n, 1))[:, None]
        self.what = f'{name}, width {width}, {"exact" if exact else "float"}'

    @property
    def n(self):
        return len(self.rows)

    @property
    def values(self):
        return self.rowgrad[:, :self.width]


def order_visible_case():
    """Five members 2^24, 1, 1, 1, 1 of one destination (between rows of other destinations): in batch order every 1 is rounded away (2^24), in reverse order the
    ones add up first (2^24 + 4).  Both are within verdict (a) - its bound is 9 x 2^-24 x (2^24 + 4) - and differ in verdict (b)."""
    rows = listed(12, (1, 3, 4, 8, 11))
    values = np.full((12, 3), 0.5, np.float32)
    values[[3, 4, 8, 11]] = 1.0
    values[1] = 2.0 ** 24
    return RowCase('order made visible', rows, 3, exact=False, values=values)


def first_occurrence(rows, block_rows=0):
    """``first[k]``: the first batch position of ``rows[k]`` inside k's block, -1 for a negative id (vectorised; ``first_occurrence_loops`` is the plain form)."""
    rows = np.asarray(rows, np.int64)
    n = len(rows)
    first = np.full(n, -1, np.int64)
    if n == 0:
        return first
    k = np.arange(n)
    valid = rows >= 0
    key = (k // effective_block(n, block_rows))[valid] * (1 << 40) + rows[valid]
    _, idx, inv = np.unique(key, return_index=True, return_inverse=True)
    first[valid] = k[valid][idx[inv.reshape(-1)]]
    return first


def first_occurrence_loops(rows, block_rows=0):
    n = len(rows)
    b = effective_block(n, block_rows) if n else 1
    first, seen = [-1] * n, {}
    for k in range(n):
        if rows[k] < 0:
            continue
        first[k] = seen.setdefault((k // b, int(rows[k])), k)
    return np.asarray(first, np.int64)


def ordered_sums(values, first, reverse=False):
    """The float32 accumulator of every leader: +0, then its members added one by one in ascending (``reverse``: descending) batch position.  [n, width] float32;
    rows that lead nothing stay 0.  Members of equal rank in their groups are added together: every group has one member of each rank."""
    values = np.asarray(values, np.float32)
    acc = np.zeros_like(values)
    valid = np.nonzero(first >= 0)[0]
    if reverse:
        valid = valid[::-1]
    if len(valid) == 0:
        return acc
    order = np.argsort(first[valid], kind='stable')
    members, groups = valid[order], first[valid][order]
    starts = np.concatenate([[0], np.nonzero(np.diff(groups))[0] + 1])
    rank = np.arange(len(groups)) - np.repeat(starts, np.diff(np.concatenate([starts, [len(groups)]])))
    by_rank = np.argsort(rank, kind='stable')
    members, rank = members[by_rank], rank[by_rank]
    cuts = np.concatenate([[0], np.nonzero(np.diff(rank))[0] + 1, [len(rank)]])
    for a, b in zip(cuts[:-1], cuts[1:]):
        m = members[a:b]
        acc[first[m]] = acc[first[m]] + values[m]
    return acc


Sums = namedtuple('Sums', 'first leader want mag count seq')


def group_sums(case, block_rows=0):
    """Per leader row: the float64 sum of its destination's rows inside its block, ``sum |terms|``, the member count, and the batch-order float32 sum."""
    first = first_occurrence(case.rows, block_rows)
    valid = first >= 0
    v = case.values.astype(np.float64)
    want, mag = np.zeros_like(v), np.zeros_like(v)
    np.add.at(want, first[valid], v[valid])
    np.add.at(mag, first[valid], np.abs(v[valid]))
    count = np.bincount(first[valid], minlength=case.n).astype(np.int64)
    if case.exact:
        ensure_exact(mag, case.what)
    return Sums(first, (first == np.arange(case.n)).astype(np.int32), want, mag, count, ordered_sums(case.values, first))


def group_sums_loops(case, block_rows=0):
    first = first_occurrence_loops(case.rows, block_rows)
    want = np.zeros((case.n, case.width), np.float64)
    for k in range(case.n):
        if first[k] >= 0:
            for c in range(case.width):
                want[first[k], c] += float(case.values[k, c])
    return first, want


# ---- destinations of the scatter ----
class Dest:
    """The destination of ``ihg_batch_scatter_add`` / ``ihg_batch_rows_add`` as ONE flat float32 arena: column c of row r lies at
    ``(c // block_width) * block_stride + r * ld_dense + c % block_width``; everything that is no payload element - the columns beyond ``block_width``, the gap between two
    blocks - holds ``SENTINEL``; the payload holds integers in [-8, 8] (float cases: normal draws): the kernels ADD.  ``tail`` = (tail_row_offset, tail_rows): the last of
    the ``width`` columns goes to ``tail[row - offset]`` and ``body = width - 1`` columns to the arena."""

    def __init__(self, n_nodes, width, ld_pad=3, block_width=None, gap=0, tail=None, exact=True, seed=0):
        self.n_nodes, self.width, self.tail = n_nodes, width, tail
        self.body = width - 1 if tail is not None else width
        self.block_width = block_width or max(self.body, 1)
        self.ld_dense = self.block_width + ld_pad
        self.n_blocks = max(-(-self.body // self.block_width), 1)
        self.block_stride = n_nodes * self.ld_dense + gap if (self.n_blocks > 1 or gap) else 0
        rng = _gen('dest', n_nodes, width, seed)
        self.arena = np.full((self.n_blocks - 1) * self.block_stride + n_nodes * self.ld_dense, SENTINEL, np.float32)
        self.payload = np.zeros(len(self.arena), bool)
        if self.body:
            idx = self.index(np.arange(n_nodes)[:, None], np.arange(self.body)[None, :]).reshape(-1)
            assert len(np.unique(idx)) == len(idx) and idx.max() < len(self.arena)
            self.payload[idx] = True
            self.arena[idx] = rng.integers(-8, 9, len(idx)) if exact else rng.standard_normal(len(idx))
        if tail is not None:
            self.tail_arena = (rng.integers(-8, 9, tail[1]) if exact else rng.standard_normal(tail[1])).astype(np.float32)

    def index(self, row, c, wrong_width=None):
        """The flat position of column c of row ``row`` (``wrong_width``: the column inside the block taken modulo that width instead - a mutation of the host test)."""
        return (c // self.block_width) * self.block_stride + row * self.ld_dense + c % (wrong_width or self.block_width)


Scattered = namedtuple('Scattered', 'dense tail dense_seq tail_seq')     # dense / tail: Ref over the flat arenas; *_seq: the batch-order float32 arenas


def _add_leaders(arena, idx, sums, leaders, cols):
    """(Ref, seq) of a flat arena after ``arena[idx[l, c]] += sums[leaders[l], cols[c]]`` over distinct positions ``idx`` [leaders, columns]."""
    want, mag, count, seq = arena.astype(np.float64), np.zeros(len(arena)), np.zeros(len(arena)), arena.copy()
    assert len(np.unique(idx)) == idx.size
    mag[idx] = np.abs(arena[idx]).astype(np.float64) + sums.mag[leaders][:, cols]
    want[idx] += sums.want[leaders][:, cols]
    count[idx] = np.broadcast_to(sums.count[leaders][:, None], idx.shape)
    seq[idx] = arena[idx] + sums.seq[leaders][:, cols]
    return Ref(torch.from_numpy(want), torch.from_numpy(mag), torch.from_numpy(count)), seq


def scatter_reference(case, dest):
    """``dense[rows[k], c] += rowgrad[k, c]`` over every k with ``rows[k] >= 0``, the last column to ``tail[rows[k] - offset]`` where that is inside [0, tail_rows)."""
    sums = group_sums(case)
    leaders = np.nonzero(sums.leader)[0]
    assert len(np.unique(case.rows[leaders])) == len(leaders) and (len(leaders) == 0 or case.rows[leaders].max() < dest.n_nodes)
    idx = dest.index(case.rows[leaders][:, None], np.arange(dest.body)[None, :]).astype(np.int64)
    dense, dense_seq = _add_leaders(dest.arena, idx, sums, leaders, slice(0, dest.body))
    tail = tail_seq = None
    if dest.tail is not None:
        tr = case.rows[leaders] - dest.tail[0]
        inside = (tr >= 0) & (tr < dest.tail[1])
        tail, tail_seq = _add_leaders(dest.tail_arena, tr[inside][:, None], sums, leaders[inside], slice(case.width - 1, case.width))
    if case.exact:
        ensure_exact(dense.mag.numpy(), case.what)
    return Scattered(dense, tail, dense_seq, tail_seq)


def scatter_reference_loops(case, dest):
    want = dest.arena.astype(np.float64)
    tail = None if dest.tail is None else dest.tail_arena.astype(np.float64)
    for k in range(case.n):
        r = int(case.rows[k])
        if r < 0:
            continue
        for c in range(case.width):
            if dest.tail is not None and c == case.width - 1:
                if 0 <= r - dest.tail[0] < dest.tail[1]:
                    tail[r - dest.tail[0]] += float(case.values[k, c])
            else:
                want[(c // dest.block_width) * dest.block_stride + r * dest.ld_dense + c % dest.block_width] += float(case.values[k, c])
    return want, tail


def dest_form_cases():
    """``(name, rows, width, Dest kwargs)`` over the three destination forms: a plain matrix with ``ld_dense > width``; L = 1, 2, 4 blocks of ``block_width`` = 1, 32, 65
    columns, ``block_stride`` 11 floats more than a block (a sentinel gap between the blocks); the tail column with destinations at ``tr`` = -1, 0, tail_rows - 1 and
    tail_rows (offset 5, 9 rows: destinations 4, 5, 13, 14), alone (width 1) and behind a body."""
    rows = np.concatenate([[4, 5, 13, 14, 5, 14, 4, 0, 39], _gen('dest forms').integers(0, 40, 80)]).astype(np.int64)
    out = [('plain matrix', rows, 37, dict(ld_pad=6))]
    for blocks in (1, 2, 4):
        for bw in (1, 32, 65):
            out.append((f'{blocks} blocks of {bw} columns', rows, blocks * bw, dict(block_width=bw, gap=11, ld_pad=blocks % 2)))
            out.append((f'{blocks} blocks of {bw} columns and a tail', rows, blocks * bw + 1, dict(block_width=bw, gap=11, ld_pad=1, tail=(5, 9))))
    out.append(('a tail alone', rows, 1, dict(tail=(5, 9))))
    return out


# ---- rows_add / rows_put ----
class LeaderCase:
    """``src`` [n, ld] with NaN beyond ``width`` AND in every row the contract never reads (leader = 0), ``rows`` with duplicates where only the first occurrence leads,
    negative rows with leader = 1 (skipped)."""

    def __init__(self, name, rows, width, exact=True, negative=()):
        base = RowCase(name, rows, width, exact)
        self.name, self.what, self.width, self.exact, self.n = name, base.what, width, exact, base.n
        self.rows = base.rows.copy()
        self.leader = (first_occurrence(self.rows) == np.arange(self.n)).astype(np.int32)
        for k in negative:
            if k < self.n and self.leader[k]:
                self.rows[k] = -1 - k
        self.src = base.rowgrad
        self.src[self.leader == 0] = np.nan

    def live(self):
        return np.nonzero((self.leader == 1) & (self.rows >= 0))[0]


def rows_add_reference(case, dest):
    """``dense[rows[k], 0:width] += src[k, 0:width]`` over the leader rows with ``rows[k] >= 0``; with a tail: ``tail[rows[k] - offset] += src[k, 0]``."""
    live = case.live()
    vals = np.nan_to_num(case.src[:, :case.width])
    sums = Sums(None, None, vals.astype(np.float64), np.abs(vals).astype(np.float64), np.ones(case.n, np.int64), vals)
    if dest.tail is not None:
        tr = case.rows[live] - dest.tail[0]
        inside = (tr >= 0) & (tr < dest.tail[1])
        ref, seq = _add_leaders(dest.tail_arena, tr[inside][:, None], sums, live[inside], slice(0, 1))
    else:
        idx = dest.index(case.rows[live][:, None], np.arange(case.width)[None, :]).astype(np.int64)
        ref, seq = _add_leaders(dest.arena, idx, sums, live, slice(0, case.width))
    if case.exact:
        ensure_exact(ref.mag.numpy(), case.what)
    return ref, seq


class TypedDest:
    """Three allocations, one per node type, rows ``type_begin[t] .. type_begin[t + 1]`` of the destination's numbering in allocation t; ``fill``: 'ints' or 'sentinel'."""

    def __init__(self, type_begin, width, ld_pad=2, fill='ints'):
        self.type_begin, self.width, self.ld = tuple(type_begin), width, width + ld_pad
        rng = _gen('typed', *type_begin, width)
        self.arenas = []
        for t in range(3):
            a = np.full((type_begin[t + 1] - type_begin[t], self.ld), SENTINEL, np.float32)
            if fill == 'ints':
                a[:, :width] = rng.integers(-8, 9, (len(a), width))
            self.arenas.append(a)

    def type_of(self, row, gt=False):
        tb = self.type_begin
        return np.where((row > tb[2]) if gt else (row >= tb[2]), 2, np.where((row > tb[1]) if gt else (row >= tb[1]), 1, 0))


def typed_rows_for(type_begin, rng, extra=40):
    """Rows at begin1 - 1, begin1, begin2 - 1, begin2, the first row and the last row of every type (empty types: none), and random ones; some twice."""
    tb = type_begin
    edge = [r for t in range(3) if tb[t + 1] > tb[t] for r in (tb[t], tb[t + 1] - 1)]
    edge += [r for r in (tb[1] - 1, tb[1], tb[2] - 1, tb[2]) if tb[0] <= r < tb[3]]
    rows = np.concatenate([edge, rng.integers(tb[0], tb[3], extra), edge[:3]]).astype(np.int64)
    return rows


TYPED_BEGINS = ((2, 12, 17, 30), (0, 6, 6, 15), (3, 3, 9, 20), (1, 8, 14, 14))      # a numbering that starts at 2; no queries; no users; no items


def rows_put_reference(case, typed, assign):
    """``dense_rows[t][rows[k] - type_begin[t]] (+)= src[k]`` over the live leader rows, t the type whose range holds ``rows[k]``.  [(Ref, seq)] per type."""
    live = case.live()
    out = []
    types = typed.type_of(case.rows[live])
    for t in range(3):
        a = typed.arenas[t]
        want, mag, seq = a.astype(np.float64), np.zeros(a.shape), a.copy()
        ks = live[types == t]
        local = case.rows[ks] - typed.type_begin[t]
        assert len(np.unique(local)) == len(local) and (len(local) == 0 or (local.min() >= 0 and local.max() < len(a)))
        v = case.src[ks, :case.width]
        if assign:
            want[local, :case.width], seq[local, :case.width] = v.astype(np.float64), v
            mag[local, :case.width] = 0.0                                     # a copy: exact in either kind of case
        else:
            mag[local, :case.width] = np.abs(a[local, :case.width]) + np.abs(v)
            want[local, :case.width] += v.astype(np.float64)
            seq[local, :case.width] = a[local, :case.width] + v
        out.append((Ref(torch.from_numpy(want), torch.from_numpy(mag), 1.0), seq))
    return out


# =============================================================================================
# verdicts
# =============================================================================================
def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f'{what}: shape {got.shape} for {want.shape}'
    bad = got.view(np.int32) != want.view(np.int32)
    if bad.any():
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements differ in their bits; first at {first}: got {got[first]!r}, want {want[first]!r}')


def hold(got, ref, seq, exact, what, order=True):
    """Both verdicts on one output (numpy float32 of the reference's shape): exact cases ``torch.equal``, float cases the per-element bound (returns the worst
    error / bound); then, ``order``, the batch-order verdict on bit patterns."""
    got_t = torch.from_numpy(np.ascontiguousarray(got, np.float32))
    worst = 0.0
    if exact:
        AR.assert_exact(got_t, ref, what)
    else:
        worst = AR.assert_within_float_bound(got_t, ref, what)
    if order:
        assert_same_bits(got, seq, what + ' (batch order)')
    return worst


def check_scatter(case, dest, got_dense, got_tail, order=True):
    ref = scatter_reference(case, dest)
    worst = hold(got_dense, ref.dense, ref.dense_seq, case.exact, f'scatter {case.what}', order)
    if dest.tail is not None:
        worst = max(worst, hold(got_tail, ref.tail, ref.tail_seq, case.exact, f'scatter tail {case.what}', order))
    return worst


def check_combine(case, block_rows, got_rowgrad, got_leader, order=True):
    """After ``ihg_batch_combine``: ``leader`` exactly the first occurrences inside their blocks (0 for a negative id); every row that leads nothing, and every column
    >= width, unchanged bit for bit; the leaders' sums by both verdicts."""
    what = f'combine {case.what}, blocks of {block_rows}'
    sums = group_sums(case, block_rows)
    got_leader = np.asarray(got_leader)
    assert got_leader.dtype == np.int32 and np.array_equal(got_leader, sums.leader), \
        f'{what}: leader differs at rows {np.nonzero(got_leader != sums.leader)[0][:8].tolist()} (got {got_leader[got_leader != sums.leader][:8].tolist()})'
    lead = sums.leader == 1
    assert_same_bits(got_rowgrad[:, case.width:], case.rowgrad[:, case.width:], what + ': columns beyond width')
    assert_same_bits(got_rowgrad[~lead], case.rowgrad[~lead], what + ': a row that leads nothing was written')
    ref = Ref(torch.from_numpy(sums.want[lead]), torch.from_numpy(sums.mag[lead]), torch.from_numpy(sums.count[lead].astype(np.float64))[:, None])
    return hold(got_rowgrad[lead][:, :case.width], ref, sums.seq[lead], case.exact, what, order)


# =============================================================================================
# emulation of batch_scatter_kernel and batch_rows_add_kernel
# =============================================================================================
def emu_leader_sums(case, block_rows=0, mutation=None):
    """``(leader [n] int32, acc [n, width] float32)`` as the kernel forms them: per block a wave per row; a negative id retires; the follower scan looks for an earlier
    equal id in the block; a leader walks the absolute 64-windows from ``k & ~63`` to the block's end, takes the members of a window in trips of 16, adds them in
    order, per chunk of 256 columns."""
    n, width = case.n, case.width
    rows = case.rows.astype(np.int64)
    b = n if mutation == 'merge_across_blocks' else effective_block(n, block_rows)
    leader, acc, walked = np.zeros(n, np.int32), np.zeros((n, width), np.float32), []
    vals = case.values
    for lo in range(0, n, max(b, 1)):
        hi = min(lo + b, n)
        where = {}
        for k in range(lo, hi):
            where.setdefault(int(rows[k]), []).append(k)
        for ident, ks in where.items():
            if ident < 0 and mutation != 'negative_leader':
                continue
            walkers = ks if mutation == 'followers_walk_from_lo' else ks[:1]
            leader[ks[0]] = 1
            for k in walkers:
                members = [j for j in ks if (j > k if mutation == 'walk_from_k_plus_1' else (True if mutation == 'followers_walk_from_lo' else j >= k))]
                if mutation == 'reverse_order':
                    members = members[::-1]
                kept, in_window = [], {}
                for j in members:
                    w = j // WAVE
                    if mutation == 'drop_next_window' and w != k // WAVE:
                        continue
                    in_window[w] = in_window.get(w, 0) + 1
                    if mutation == 'drop_17th_member' and in_window[w] > MEMBERS:
                        continue
                    kept.append(j)
                a = np.zeros(width, np.float32)
                for j in kept:
                    a = a + vals[j]
                if mutation == 'drop_second_chunk':
                    a[CHUNK_COLS:] = 0.0
                acc[k] = a
                walked.append(k)
    return leader, acc, walked


def emu_scatter(case, dest, mutation=None):
    leader, acc, walked = emu_leader_sums(case, 0, mutation)
    dense = dest.arena.copy()
    tail = None if dest.tail is None else dest.tail_arena.copy()
    lo_edge, hi_edge = (-1 if mutation == 'tail_low_edge' else 0), (1 if mutation == 'tail_high_edge' else 0)
    for k in walked:
        r = int(case.rows[k])
        if r < 0:
            raise IndexError('a negative row was written')
        for c in range(case.width):
            if dest.tail is not None and c == case.width - 1:
                tr = r - dest.tail[0]
                if lo_edge <= tr < dest.tail[1] + hi_edge and 0 <= tr < len(tail):
                    tail[tr] = tail[tr] + acc[k, c] * np.float32(WAVE if mutation == 'tail_per_lane' else 1)
                elif lo_edge <= tr < dest.tail[1] + hi_edge:
                    raise IndexError('the tail was written outside its rows')
            else:
                i = dest.index(r, c, wrong_width=case.width if mutation == 'block_mod_width' else None)
                dense[i] = dense[i] + acc[k, c]
    return dense, tail


def emu_combine(case, block_rows, mutation=None):
    leader, acc, _ = emu_leader_sums(case, block_rows, mutation)
    out = case.rowgrad.copy()
    lead = leader == 1
    out[lead, :case.width] = acc[lead]
    if mutation == 'follower_overwritten':
        out[~lead, :case.width] = acc[~lead]
    return out, leader


def emu_rows_add(case, dest, mutation=None):
    """Flat arena (or tail) after ``batch_rows_add_kernel<false>`` on a plain matrix."""
    out = (dest.tail_arena if dest.tail is not None else dest.arena).copy()
    lo_edge, hi_edge = (-1 if mutation == 'tail_low_edge' else 0), (1 if mutation == 'tail_high_edge' else 0)
    for k in range(case.n):
        r = int(case.rows[k])
        if case.leader[k] == 0 or r < 0:
            continue
        if dest.tail is not None:
            tr = r - dest.tail[0]
            if lo_edge <= tr < dest.tail[1] + hi_edge:
                if not 0 <= tr < len(out):
                    raise IndexError('the tail was written outside its rows')
                for _ in range(WAVE if mutation == 'tail_per_lane' else 1):
                    out[tr] = out[tr] + case.src[k, 0]
            continue
        for c in range(case.width):
            i = dest.index(r, c)
            out[i] = out[i] + case.src[k, c]
    return out


def emu_rows_put(case, typed, assign, mutation=None):
    outs = [a.copy() for a in typed.arenas]
    if mutation == 'assign_zero_fill' and assign:
        for a in outs:
            a[:, :case.width] = 0.0
    for k in range(case.n):
        r = int(case.rows[k])
        if case.leader[k] == 0 or r < 0:
            continue
        t = int(typed.type_of(np.int64(r), gt=mutation == 'typed_gt'))
        local = r - typed.type_begin[t]
        if not 0 <= local < len(outs[t]):
            raise IndexError('a typed row landed outside its allocation')
        v = case.src[k, :case.width]
        outs[t][local, :case.width] = v if assign else outs[t][local, :case.width] + v
    return outs


# =============================================================================================
# the small kernels
# =============================================================================================
NODE_ROWS_B = (0, 1, 85, 86, 174762, 174763)         # 3 b around 256 threads (one workgroup) and around GRID_THREADS = 524,288 (the grid-stride loop's second trip)
ZERO_ROWS_DIMS = (1, 63, 64, 65, 257)
ZERO_FLOATS_N = (0, 1, 255, 256, 257, GRID_THREADS + 1)
MARK_ROWS_N = (1, 300, GRID_THREADS + 5)


def node_rows_reference(users, queries, items, query_row0, item_row0):
    """rows[0 .. 3 b) = users | queries + query_row0 | items + item_row0."""
    return np.concatenate([users, queries + query_row0, items + item_row0]).astype(np.int64)


def zero_rows_reference(base, dim, rows):
    want = base.copy()
    want[np.asarray(rows, np.int64), :dim] = 0.0
    return want


def mark_rows_reference(mask, rows, value):
    want = mask.copy()
    want[np.asarray(rows, np.int64)] = value
    return want


# =============================================================================================
# compose: w_eff[i][t d + j] = sum_k A[i][t d + k] W[k][j], b_eff[t][i] = sum_k A[i][t d + k] b[k] + (t == 0 ? c[i] : 0) and its backward
# =============================================================================================
COMPOSE_DIMS = (1, 3, 7, 8, 9, 12, 32, 63, 64, 65, 96, 128, 129, 256)
# strided_dot: an unrolled body of 8 and a tail (d = 7 / 8 / 9: tail only, body only, both);  part 1 of the backward: lanes over j, a second trip at d > 64
# (63 / 64 / 65; 128 / 129: a third);  part 1's grid-stride loop: a second trip where 3 d^2 > COMPOSE_WAVES = 16,384, d >= 74 (65 / 96)
COMPOSE_ROUNDINGS = 3.0
COMPOSE_PADS = dict(a=3, w=2, w_eff=5, dw_eff=1, da=4, dw=6)


class ComposeCase:
    def __init__(self, dim, exact, with_c=True):
        self.dim, self.exact, self.with_c = dim, exact, with_c
        rng = _gen('compose', dim, int(exact))
        draw = (lambda *s: rng.integers(-2, 3, s).astype(np.float32)) if exact else (lambda *s: rng.standard_normal(s).astype(np.float32))
        self.a, self.w, self.b, self.c = draw(dim, 3 * dim), draw(dim, dim), draw(dim), draw(dim)
        self.dw_eff, self.db_eff = draw(dim, 3 * dim), draw(3, dim)
        self.what = f'compose d = {dim}, {"exact" if exact else "float"}, c {"given" if with_c else "NULL"}'


def compose_fwd_reference(case):
    """``dict(w_eff, b_eff)`` of ``Ref``: float64 from the header's formulas.  K = d."""
    d = case.dim
    a, w, b, c = (x.astype(np.float64) for x in (case.a, case.w, case.b, case.c))
    blocks = a.reshape(d, 3, d)                                                # [i, t, k]
    w_eff = np.einsum('itk,kj->itj', blocks, w).reshape(d, 3 * d)
    w_mag = np.einsum('itk,kj->itj', np.abs(blocks), np.abs(w)).reshape(d, 3 * d)
    b_eff, b_mag = np.einsum('itk,k->ti', blocks, b), np.einsum('itk,k->ti', np.abs(blocks), np.abs(b))
    if case.with_c:
        b_eff[0] += c
        b_mag[0] += np.abs(c)
    if case.exact:
        ensure_exact(w_mag, case.what), ensure_exact(b_mag, case.what)
    t = torch.from_numpy
    return dict(w_eff=Ref(t(w_eff), t(w_mag), float(d)), b_eff=Ref(t(b_eff), t(b_mag), float(d)))


def compose_bwd_reference(case):
    """``dict(da, dc, dw, db)``: dA[i][t d + k] = sum_j dWe[i][t d + j] W[k][j] + dbe[t][i] b[k] (K = d), dW[k][j] = sum_t sum_i A[i][t d + k] dWe[i][t d + j]
    (K = 3 d), db[k] = sum_t sum_i A[i][t d + k] dbe[t][i] (K = 3 d), dc = dbe[0] (a copy)."""
    d = case.dim
    a, w, b, g, gb = (x.astype(np.float64) for x in (case.a, case.w, case.b, case.dw_eff, case.db_eff))
    ab, gblocks = a.reshape(d, 3, d), g.reshape(d, 3, d)
    da = (np.einsum('itj,kj->itk', gblocks, w) + np.einsum('ti,k->itk', gb, b)).reshape(d, 3 * d)
    da_mag = (np.einsum('itj,kj->itk', np.abs(gblocks), np.abs(w)) + np.einsum('ti,k->itk', np.abs(gb), np.abs(b))).reshape(d, 3 * d)
    dw, dw_mag = np.einsum('itk,itj->kj', ab, gblocks), np.einsum('itk,itj->kj', np.abs(ab), np.abs(gblocks))
    db, db_mag = np.einsum('itk,ti->k', ab, gb), np.einsum('itk,ti->k', np.abs(ab), np.abs(gb))
    if case.exact:
        for m in (da_mag, dw_mag, db_mag):
            ensure_exact(m, case.what)
    t = torch.from_numpy
    return dict(da=Ref(t(da), t(da_mag), float(d)), dw=Ref(t(dw), t(dw_mag), float(3 * d)), db=Ref(t(db), t(db_mag), float(3 * d)),
                dc=Ref(t(gb[0].copy()), torch.zeros(d, dtype=torch.float64), 1.0))


def compose_reference_loops(case):
    """The forward and ``da`` / ``dw`` / ``db`` as plain loops (small d only)."""
    d = case.dim
    a, w, b, c, g, gb = (x.astype(np.float64).tolist() for x in (case.a, case.w, case.b, case.c, case.dw_eff, case.db_eff))
    w_eff = [[sum(a[i][t * d + k] * w[k][j] for k in range(d)) for t in range(3) for j in range(d)] for i in range(d)]
    b_eff = [[sum(a[i][t * d + k] * b[k] for k in range(d)) + (c[i] if t == 0 and case.with_c else 0.0) for i in range(d)] for t in range(3)]
    da = [[sum(g[i][t * d + j] * w[k][j] for j in range(d)) + gb[t][i] * b[k] for t in range(3) for k in range(d)] for i in range(d)]
    dw = [[sum(a[i][t * d + k] * g[i][t * d + j] for t in range(3) for i in range(d)) for j in range(d)] for k in range(d)]
    db = [sum(a[i][t * d + k] * gb[t][i] for t in range(3) for i in range(d)) for k in range(d)]
    return tuple(np.asarray(x, np.float64) for x in (w_eff, b_eff, da, dw, db))


def compose_bound(ref):
    """``(K + c) 2^-24 sum |terms|`` in the form of ``contraction_reference.float_bound``: K the contraction length (d; 3 d for dw / db), c = 3 other roundings per
    element: the product of every term, and for the one addend outside the contraction (``dbe b`` of da, ``c`` of b_eff) its product and its addition."""
    return (ref.n + COMPOSE_ROUNDINGS) * AR.U * ref.mag


def hold_compose(got, ref, exact, what):
    """Exact: ``torch.equal``.  Float: per element within ``compose_bound``; returns the worst error / bound."""
    got_t = torch.from_numpy(np.ascontiguousarray(got, np.float32))
    if exact:
        AR.assert_exact(got_t, ref, what)
        return 0.0
    assert bool(torch.isfinite(got_t).all()), f'{what}: a value is not finite'
    err, bound = (got_t.double() - ref.want).abs(), compose_bound(ref)
    assert bool((err[bound == 0] == 0).all()), f'{what}: an element without terms differs'
    ratio = err / torch.where(bound > 0, bound, torch.ones_like(bound))
    worst = float(ratio.max())
    assert worst <= 1.0, f'{what}: error / bound = {worst:.3g} at {tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0])}'
    return worst


def emu_strided_dot(x, y, mutation=None):
    """``strided_dot`` over the LAST axis of two broadcastable float32 arrays: four partial sums, index k into partial k & 3, the unrolled body and the tail in index
    order, ``(acc0 + acc1) + (acc2 + acc3)``.  'compose_tail_skipped': the tail is left out."""
    n = x.shape[-1]
    stop = n - n % 8 if mutation == 'compose_tail_skipped' else n
    acc = [np.zeros(np.broadcast_shapes(x.shape[:-1], y.shape[:-1]), np.float32) for _ in range(4)]
    for k in range(stop):
        acc[k & 3] = acc[k & 3] + x[..., k] * y[..., k]
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def emu_compose_fwd(case, mutation=None):
    d = case.dim
    blocks = case.a.reshape(d, 3, d)
    w_eff = emu_strided_dot(blocks[:, :, None, :], case.w.T[None, None, :, :], mutation).reshape(d, 3 * d)
    b_eff = emu_strided_dot(blocks.transpose(1, 0, 2), case.b[None, None, :], mutation)
    if case.with_c:
        b_eff[0 if mutation != 'compose_c_every_type' else slice(None)] += case.c
    return w_eff, b_eff


def emu_compose_bwd(case, mutation=None):
    d = case.dim
    g, ab = case.dw_eff.reshape(d, 3, d), case.a.reshape(d, 3, d)
    lanes = np.zeros((d, 3, d, WAVE), np.float32)                              # part 1: lane partials over j = lane, lane + 64, ...; then the xor butterfly
    for j0 in range(0, d, WAVE):
        if mutation == 'compose_second_wave_trip_skipped' and j0 > 0:
            break
        width = min(WAVE, d - j0)
        lanes[..., :width] = lanes[..., :width] + g[:, :, None, j0:j0 + width] * case.w[None, None, :, j0:j0 + width]
    o = WAVE // 2
    while o >= 1:
        lanes = lanes + lanes[..., np.arange(WAVE) ^ o]
        o //= 2
    da = lanes[..., 0]
    if mutation != 'compose_da_without_bias_term':
        da = da + case.db_eff.T[:, :, None] * case.b[None, None, :]
    dw, db = np.zeros((d, d), np.float32), np.zeros(d, np.float32)
    for t in range(3):                                                         # part 2: per type a strided_dot over i, the three added in order
        dw = dw + emu_strided_dot(ab[:, t, :].T[:, None, :], g[:, t, :].T[None, :, :], mutation)
        db = db + emu_strided_dot(ab[:, t, :].T, case.db_eff[t][None, :], mutation)
    return dict(da=da.reshape(d, 3 * d), dw=dw, db=db, dc=case.db_eff[0].copy())


# =============================================================================================
# the catalogue: the cases both test files run, by group
# =============================================================================================
def _id_lists():
    return member_count_lists() + position_lists() + negative_lists()


def _plain(rows, width, exact=True, seed=0):
    return Dest(int(max(np.max(rows, initial=0), 0)) + 2, width, exact=exact, seed=seed)


def scatter_cases(group):
    """``[(RowCase, Dest)]`` of one group: 'members' (the id lists, width 5), 'n' (``N_LADDER``, width 3), 'widths' (``WIDTH_LADDER`` over 70 rows), 'forms' (the
    destination forms), 'float' (float payloads on non-zero float contents: the hot destination, a second grid trip at width 8, two column chunks, a blocked form with
    a tail, and the case that makes the order visible)."""
    if group == 'members':
        return [(RowCase(name, rows, 5), _plain(rows, 5)) for name, rows in _id_lists()]
    if group == 'n':
        return [(RowCase(name, rows, 3), _plain(rows, 3)) for name, rows in n_ladder_lists()]
    if group == 'widths':
        rows = random_rows(70, _gen('widths'))
        return [(RowCase(f'width ladder {w}', rows, w), _plain(rows, w)) for w in WIDTH_LADDER]
    if group == 'forms':
        return [(RowCase(name, rows, width), Dest(40, width, seed=1, **kw)) for name, rows, width, kw in dest_form_cases()]
    assert group == 'float'
    hot, big, wide = member_count_lists()[-1][1], n_ladder_lists()[6][1], random_rows(70, _gen('widths'))
    name, rows, width, kw = dest_form_cases()[4]
    visible = order_visible_case()
    return [(RowCase('hundreds of members', hot, 5, exact=False), _plain(hot, 5, exact=False)),
            (RowCase('n = 8193', big, 8, exact=False), _plain(big, 8, exact=False)),
            (RowCase('two column chunks', wide, 2 * CHUNK_COLS + 1, exact=False), _plain(wide, 2 * CHUNK_COLS + 1, exact=False)),
            (RowCase(name, rows, width, exact=False), Dest(40, width, exact=False, seed=1, **kw)),
            (visible, Dest(120, 3, exact=True))]


def combine_cases(group):
    """``[(RowCase, disjoint_block_rows)]``: 'members', 'n', 'widths' as for the scatter (one block); 'blocks' (``combine_block_cases``, width 3); 'float'."""
    if group == 'blocks':
        return [(RowCase(name, rows, 3), b) for name, rows, b in combine_block_cases()]
    if group == 'float':
        name, rows, b = combine_block_cases()[5]
        return [(c, 0) for c, _ in scatter_cases('float')] + [(RowCase(name, rows, 7, exact=False), b)]
    return [(c, 0) for c, _ in scatter_cases(group)]


def rows_add_cases(group):
    """``[(LeaderCase, Dest)]``: 'widths' (``WIDTH_LADDER`` over 70 rows, some negative leader rows), 'n' (``ROWS_N_LADDER`` = 1, 8,192, 8,193, 20,000 rows: the
    grid-stride loop's second and third trips; width 3), 'tail' (the tail mode over the range edges of ``dest_form_cases``), 'float'."""
    if group == 'widths':
        rows = random_rows(70, _gen('rows add'))
        return [(LeaderCase(f'rows_add width {w}', rows, w, negative=(0, 5, 69)), _plain(rows, w, seed=2)) for w in WIDTH_LADDER]
    if group == 'n':
        return [(LeaderCase(f'rows_add n = {n}', random_rows(n, _gen('rows add', n)), 3, negative=(0, n - 1, n // 2)), Dest(n // 3 + 3, 3, seed=2)) for n in ROWS_N_LADDER]
    if group == 'tail':
        rows = dest_form_cases()[0][1]
        return [(LeaderCase('rows_add tail', rows, 1, negative=(8,)), Dest(40, 1, tail=(5, 9))),
                (LeaderCase('rows_add tail, float', rows, 1, exact=False), Dest(40, 1, tail=(5, 9), exact=False))]
    assert group == 'float'
    rows = random_rows(300, _gen('rows add float'))
    return [(LeaderCase('rows_add float', rows, w, exact=False, negative=(3,)), _plain(rows, w, exact=False)) for w in (5, CHUNK_COLS + 1)]


def rows_put_cases():
    """``[(LeaderCase, TypedDest, assign)]``: every ``TYPED_BEGINS`` numbering, assign = 1 into sentinel-filled allocations and assign = 0 onto integer contents;
    ``WIDTH_LADDER`` on the first numbering; 8,193 rows (a second grid trip) on a wide numbering."""
    out = []
    for tb in TYPED_BEGINS:
        rows = typed_rows_for(tb, _gen('typed', *tb))
        for assign in (1, 0):
            out.append((LeaderCase(f'rows_put types {tb} assign {assign}', rows, 5, negative=(7,)), TypedDest(tb, 5, fill='sentinel' if assign else 'ints'), assign))
    tb = TYPED_BEGINS[0]
    rows = typed_rows_for(tb, _gen('typed widths'))
    for w in WIDTH_LADDER:
        out.append((LeaderCase(f'rows_put width {w}', rows, w), TypedDest(tb, w, fill='ints'), w % 2))
    tb = (5, 2005, 2300, 4000)
    rows = typed_rows_for(tb, _gen('typed many'), extra=GRID_WAVES + 1 - 13)
    out.append((LeaderCase('rows_put 8193 rows', rows, 3), TypedDest(tb, 3, fill='ints'), 0))
    out.append((LeaderCase('rows_put float', typed_rows_for(TYPED_BEGINS[0], _gen('typed float')), 9, exact=False), TypedDest(TYPED_BEGINS[0], 9), 0))
    return out


def check_rows_add(case, dest, got):
    ref, seq = rows_add_reference(case, dest)
    return hold(got, ref, seq, case.exact, case.what)


def check_rows_put(case, typed, assign, got):
    worst = 0.0
    for t, (ref, seq) in enumerate(rows_put_reference(case, typed, assign)):
        worst = max(worst, hold(got[t], ref, seq, case.exact, f'{case.what}, type {t}'))
    return worst


def compose_cases():
    """Every ``COMPOSE_DIMS`` width exact, with ``c`` given and NULL alternating - both at the widths on the two sides of a boundary pair -; float cases at 9, 65, 96, 129."""
    exact = [ComposeCase(d, True, with_c=(k % 2 == 0)) for k, d in enumerate(COMPOSE_DIMS)] + [ComposeCase(d, True, with_c=False) for d in (1, 8, 64)]
    return exact + [ComposeCase(d, False, with_c=(d != 96)) for d in (9, 65, 96, 129)]
