"""Reference for the evaluation ranking of ``csrc/eval.hip`` (``ihg_score_topk``, ``ihg_score_topk_cosine``, ``ihg_score_topk_deep``), for
``tests/test_ranking_host.py`` (CPU) and ``tests/test_ranking_kernels.py`` (GPU).  Not a test module; numpy and torch on the CPU only.

    geometry    ``eval_ksteps`` / ``eval_pair_tiles`` / ``eval_slices`` restated, the waves' tile ranges and ``list_of(item)``: which of the up to 1,024 partial
                lists of ten an item lands in (run x lane half); ``test_ranking_host.py`` pins it to ``ihg_score_topk_workspace_bytes``
    cases       *exact* designs - integer operands, power-of-two row scales, for the cosine head rows of power-of-two norm - whose every score is exact in the
                kernels' arithmetic (``ensure_exact``), placed list by list with ``list_of``; *float* designs with a per-score bound
    verdicts    exact: items EQUAL the stable ranking, scores EQUAL float32(float64 scores); float: ``float_verdict``
    emulation   the whole call in numpy - split, float32 accumulation, the lists of ten with ``ranks_before``, the merge, the deep passes - with ``mutation``
                naming ONE way of being wrong

The per-score bound (u = 2^-24, ``T = sum_c |a_c| (lam |q_c| + (1 - lam) |u_c|)``: the UNMIXED magnitudes, because the mix can cancel):

    |s - s64| <= (C_MIX + 48 ksteps + C_FIN) u T + 3 * 2^-22 T + N + u |s64|

    (the count n times u: first order.  The remainder, below n u / 2 < 2^-12 of the term at 79 k-steps, is not added: n counts the LONGEST chain of roundings, which
    only the first addends of a row pass through - the last pass through C_MIX + 1 + C_FIN)
    C_MIX = 3   an addend of the mix passes through at most: 1.f - lam, its product with the row, the sum (lam itself is the float32 both sides use)
    48 ksteps    three MFMAs of 16 columns per k-step into one float32 accumulator: an addend passes through at most 48 ksteps additions (the products of
                 two fp16 values are exact in float32; the scales are powers of two)
    C_FIN = 3    the product of the two inverse scales, its product with the accumulator, and one unit for the difference between u |s| and u |s64|
    3 * 2^-22    what the two-fp16 split loses per product (``split_common.hpp``; ``test_host_logic.py`` holds it)
    N            2^-36 (|a|_inf |m|_1 + |m|_inf |a|_1): entries below 2^-17 of their row's largest have a subnormal ``lo`` (same test)
    u |s64|      the final addition of the bias

The cosine head divides the accumulator by both norms: with ``na``, ``nm`` the float64 norms clamped at the float64 1e-8 (the kernels clamp at the float32
``1e-8f``, 0.1 u below it: a clamped norm has no sum and no square root behind it, so its C_NORM u, which stays in the bound, covers that)

    |s - s64| <= (the dot product's bound) / (na nm) + |s64 - bias| (2 C_NORM u + C_MIX u |mm|_2 / nm) + u |s64 - bias| + u |s64|

    C_NORM = (ceil(d / 64) + 7) / 2 + 2   the sum of squares: one product, ceil(d / 64) - 1 additions in a lane and six shuffle steps, all terms positive - halved by
                 the square root, which adds one rounding, and the division of the inverse scale by the norm another
    C_MIX u |mm|_2 / nm   the mixed row the norm is taken of carries the mix's roundings, relative to the unmixed magnitudes ``mm``
    u |s64 - bias|   the product of the two inverse factors is no longer exact
"""
import math

import numpy as np
import torch

import split_emulation as se
import topk_reference as tref
from contraction_reference import CAP, U

FLT_MAX = float(np.finfo(np.float32).max)
TOP = 10                                 # kTopMax: entries per partial list
DEEP_MAX = 128                           # kDeepMax
WAVES = 8                                # kEvalThreads / kWave
LDS_BYTES = 160 * 1024
EPS = 1e-8
SPLIT_LOSS = 3 * 2.0 ** -22
C_MIX, C_FIN = 3, 3


# =============================================================================================
# launch geometry (csrc/eval.hip, restated)
# =============================================================================================
def eval_ksteps(dim):
    return (dim + 15) // 16


def eval_lds_bytes(dim, pb):
    return 32 * pb * (4 * 16 * eval_ksteps(dim) + 16) + 32 * pb * 4


def eval_pair_tiles(dim):
    return 2 if eval_lds_bytes(dim, 2) <= LDS_BYTES else 1


def eval_slices(n_pairs, n_items, dim):
    per = 32 * eval_pair_tiles(dim)
    blocks = (n_pairs + per - 1) // per
    tiles = (n_items + 31) // 32
    slices = (512 + blocks - 1) // blocks
    most = max(1, tiles // (WAVES * 4))
    return max(1, min(slices, most, 64))


def n_lists(n_pairs, n_items, dim):
    return eval_slices(n_pairs, n_items, dim) * WAVES * 2


def workspace_bytes(n_pairs, n_items, dim):
    tiles = (n_items + 31) // 32
    frag = tiles * eval_ksteps(dim) * 2 * 64 * 16
    aux = tiles * 32 * 8
    return frag + aux + n_pairs * n_lists(n_pairs, n_items, dim) * TOP * 8


def deep_workspace_bytes(n_pairs, n_items, dim):
    return workspace_bytes(n_pairs, n_items, dim) + 16 * n_pairs


def tile_ranges(n_pairs, n_items, dim):
    """``[(tile_begin, tile_end)]`` per run (= item slice x wave)."""
    n_tiles = (n_items + 31) // 32
    n_runs = eval_slices(n_pairs, n_items, dim) * WAVES
    return [(n_tiles * r // n_runs, n_tiles * (r + 1) // n_runs) for r in range(n_runs)]


def half_of(position, mapping=None):
    """The lane half that holds position ``j`` of a 32-item tile: ``(j >> 2) & 1`` (the accumulator rows of v_mfma_f32_32x32: 8 r4 + 4 half + x).  ``mapping`` names a
    misstatement: 'swap_lane_halves' (a relabelling of the same two sets), 'halves_by_sixteen' (the halves as the tile's two runs of sixteen)."""
    half = (position >> 2) & 1
    return {None: half, 'swap_lane_halves': 1 - half, 'halves_by_sixteen': (position >> 4) & 1}[mapping]


def list_of(n_pairs, n_items, dim, mapping=None):
    """int64 ``[n_items]``: the partial list every item lands in, ``run * 2 + lane half``; position ``j`` of a 32-item tile belongs to half ``(j >> 2) & 1``."""
    ranges = tile_ranges(n_pairs, n_items, dim)
    run_of_tile = np.zeros((n_items + 31) // 32, np.int64)
    for r, (b, e) in enumerate(ranges):
        run_of_tile[b:e] = r
    item = np.arange(n_items)
    return run_of_tile[item >> 5] * 2 + half_of(item & 31, mapping)


def max_passes(k, n_items):
    return (min(k, n_items) + TOP - 1) // TOP


# =============================================================================================
# cases
# =============================================================================================
def _gen(*key):
    return np.random.default_rng([ord(c) for k in key for c in str(k)])


class RankCase:
    """One call: ``features`` [N, dim] float32 (users' rows, then the queries', then the items'), ``users`` / ``queries`` [C] int64, ``bias`` [I] float32, ``lam``.
    Exact cases carry what ``ensure_exact`` needs: ``quantum`` (every term is a multiple of ``quantum * 2^(item_exp + pair_exp)``)."""

    def __init__(self, name, dim, n_items, n_pairs, u_rows, q_rows, a_rows, users, queries, bias, lam, exact, quantum=None, item_exp=None, pair_exp=None):
        self.name, self.dim, self.n_items, self.n_pairs, self.lam, self.exact = name, dim, n_items, n_pairs, float(np.float32(lam)), exact
        self.query_row0, self.item_row0 = len(u_rows) + 2, len(u_rows) + 2 + len(q_rows) + 3            # (rows between the blocks belong to nobody)
        f = np.full((self.item_row0 + n_items, dim), 77.0, np.float64)
        f[:len(u_rows)], f[self.query_row0:self.query_row0 + len(q_rows)], f[self.item_row0:] = u_rows, q_rows, a_rows
        assert np.array_equal(f.astype(np.float32).astype(np.float64), f), f'{name}: an operand is not a float32'
        self.features = torch.from_numpy(f.astype(np.float32))
        self.users, self.queries = torch.from_numpy(np.asarray(users, np.int64)), torch.from_numpy(np.asarray(queries, np.int64))
        self.bias = torch.from_numpy(np.asarray(bias, np.float64).astype(np.float32))
        self.quantum = quantum
        self.item_exp = np.zeros(n_items, np.int64) if item_exp is None else item_exp
        self.pair_exp = np.zeros(n_pairs, np.int64) if pair_exp is None else pair_exp
        self._scores = {}

    def scores64(self, cosine):
        """[C, I] float64 scores (computed once per head and shared)."""
        if cosine not in self._scores:
            self._scores[cosine] = tref.all_item_scores(self.features, self.users, self.queries, self.query_row0, self.item_row0, self.bias, self.lam, cosine)
        return self._scores[cosine]

    def rows(self):
        """float64 numpy ``(u, q, a)``: the pairs' user and query rows [C, d] and the item rows [I, d]."""
        f = self.features.double().numpy()
        return f[self.users.numpy()], f[self.queries.numpy() + self.query_row0], f[self.item_row0:]

    def magnitudes(self):
        """``(mm [C, d], T [C, I])``: the unmixed magnitudes ``lam |q| + (1 - lam) |u|`` and ``sum_c |a_c| mm_c``."""
        u, q, a = self.rows()
        mm = self.lam * np.abs(q) + (1 - self.lam) * np.abs(u)
        return mm, mm @ np.abs(a).T


EXACT_DESIGNS = ('random', 'mixed_bits', 'row_scales', 'all_equal', 'ascending', 'descending', 'last_tile', 'tile0', 'identity', 'one_list_dec', 'one_list_inc',
                 'one_per_list', 'tied_across', 'tie_at_boundary')
COSINE_EXACT_DESIGNS = tuple(d for d in EXACT_DESIGNS if d not in ('random', 'mixed_bits', 'identity'))    # (rows of power-of-two norm: no free integers)
FLOAT_DESIGNS = ('randn', 'worst', 'wide_range')
LAMS_EXACT = (0.5, 0.25)
LAMS_FLOAT = (0.0, 0.3, 1.0)


def _pairs(n_pairs, matched):
    nu = min(n_pairs, 13)
    nq = nu if matched else min(n_pairs, 11)
    c = np.arange(n_pairs)
    users = c % nu
    return nu, nq, users, (users if matched else (3 * c + 1) % nq)


def _sparse_rows(rng, n, dim, log2_mag, onto=None):
    """Rows with 1, 4 or 16 nonzeros (as the width allows) of magnitude ``2^log2_mag``: their norm is a power of two.  ``onto``: rows whose supports these rows
    share - row ``r`` takes its columns from the support of ``onto[r % len(onto)]`` first and from the other rows' next, so that the dot products are not all 0."""
    rows = np.zeros((n, dim))
    counts = [z for z in (1, 4, 16) if z <= dim]
    shared = None if onto is None else np.flatnonzero(np.any(onto != 0, 0))
    for r in range(n):
        nnz = counts[r % len(counts)]
        cols = rng.permutation(dim)
        if onto is not None:
            cols = np.concatenate([rng.permutation(np.flatnonzero(onto[r % len(onto)])), rng.permutation(shared), cols])
            cols = cols[np.sort(np.unique(cols, return_index=True)[1])]      # (each column once, in the order of its first appearance)
        rows[r, cols[:nnz]] = rng.choice([-1.0, 1.0], nnz) * 2.0 ** log2_mag
    return rows


def rank_values(design, n_pairs, n_items, dim, rng):
    """``(v [I] int, classes [I] int)`` of a structural design: item ``i`` scores ``pool[classes[i]] . m + v[i] * step`` with ``step`` beyond the spread of the
    dot products, so ``v`` decides the order and equal ``v`` of one class is a bit-equal score.  Every placement is derived from ``list_of``."""
    lists = list_of(n_pairs, n_items, dim)
    v = np.zeros(n_items, np.int64)
    classes = (np.arange(n_items) * 7 + 3) % 4
    ids = np.arange(n_items)
    top = DEEP_MAX + 12
    if design == 'all_equal':
        classes[:] = 0
    elif design == 'ascending':
        v = np.clip(ids - (n_items - 1 - top), 0, None)
    elif design == 'descending':
        v = np.clip(top - ids, 0, None)
    elif design in ('last_tile', 'tile0'):
        members = ids[(ids >> 5) == ((n_items - 1) >> 5 if design == 'last_tile' else 0)]
        v[members] = rng.permutation(len(members)) + 1
    elif design in ('one_list_dec', 'one_list_inc'):
        sizes = np.bincount(lists)
        members = ids[lists == int(np.argmax(sizes))][:top]
        v[members] = np.arange(len(members), 0, -1) if design == 'one_list_dec' else np.arange(1, len(members) + 1)
    elif design == 'one_per_list':
        first = np.array([ids[lists == l][0] for l in np.unique(lists)])[:top]
        v[first] = rng.permutation(len(first)) + 1
    elif design == 'tied_across':
        ranges = [r for r in tile_ranges(n_pairs, n_items, dim) if r[1] > r[0]]
        spots = set()
        for b, e in (ranges[0], ranges[len(ranges) // 2], ranges[-1]):       # (the last run lies in the last item slice)
            for tile in (b, e - 1):
                for j in (0, 4, 3, 31):
                    if tile * 32 + j < n_items:
                        spots.add(tile * 32 + j)
        spots = np.array(sorted(spots))
        v[spots], classes[spots] = 5, 1
    elif design == 'tie_at_boundary':                                      # the winners in ONE list, as one_list, in a shuffled id order: a pass ranks exactly ten of them
        sizes = np.bincount(lists)
        where = rng.permutation(ids[lists == int(np.argmax(sizes))][:top])
        vals = np.arange(len(where), 0, -1)
        for r in range(TOP, len(where), TOP):                              # ranks r and r + 1 (1-based) tie, r = 10, 20, ...: every pass ends inside a tie
            vals[r] = vals[r - 1]
        v[where], classes[where] = vals, 2
    else:
        raise KeyError(design)
    return v, classes


def exact_case(design, n_pairs, n_items, dim, cosine=False, lam=0.5, seed=0):
    """An exact case of ``design``; 'identity' sets ``n_items = dim`` itself."""
    rng = _gen('exact', design, n_pairs, n_items, dim, cosine, seed)
    quantum = min(lam, 1 - lam)
    name = f'{design} C={n_pairs} I={n_items} d={dim} lam={lam}' + (' cosine' if cosine else '')
    ints = lambda shape, m: rng.integers(-m, m + 1, shape).astype(np.float64)
    if cosine:
        assert design in COSINE_EXACT_DESIGNS, design
        nu, nq, users, queries = _pairs(n_pairs, True)
        s = _sparse_rows(rng, nu, dim, 0)
        u_rows, q_rows = s * 2.0, s * (6.0 if lam == 0.5 else 10.0)        # lam q + (1 - lam) u = 4 s (0.5: 3 + 1; 0.25: 2.5 + 1.5), and u != q
        pair_exp = np.zeros(n_pairs, np.int64)
        item_exp = np.zeros(n_items, np.int64)
        if design == 'row_scales':
            eu = np.linspace(-20, 20, nu).round().astype(np.int64)
            u_rows, q_rows = u_rows * 2.0 ** eu[:, None], q_rows * 2.0 ** eu[:, None]
            item_exp = np.linspace(-20, 20, n_items).round().astype(np.int64)[rng.permutation(n_items)]
            a_rows = _sparse_rows(rng, n_items, dim, 0, s) * 2.0 ** item_exp[:, None]
            bias = ints(n_items, 3) / 16
        else:
            v, classes = rank_values(design, n_pairs, n_items, dim, rng)
            a_rows = _sparse_rows(rng, 4, dim, 1, s)[classes]                # (the pool rows on the mixed rows' supports: the cosines are not all 0)
            bias = v * 4.0                                                 # |cosine| <= 1: a step of 4 decides
        return RankCase(name, dim, n_items, n_pairs, u_rows, q_rows, a_rows, users, queries, bias, lam, True, 1.0 / 16, item_exp, pair_exp)
    matched = design == 'row_scales'
    nu, nq, users, queries = _pairs(n_pairs, matched)
    if design == 'identity':
        assert n_items == dim
        pi = np.stack([rng.permutation(dim) + 1 for _ in range(nq)]).astype(np.float64)
        q_rows, u_rows = 4 * pi * rng.choice([-1.0, 1.0], (nq, dim)), ints((nu, dim), 1)
        return RankCase(name, dim, dim, n_pairs, u_rows, q_rows, np.eye(dim), users, queries, ints(dim, 2) * quantum, lam, True, quantum)
    if design in ('random', 'mixed_bits', 'row_scales'):
        m = 255 if dim <= 64 and design == 'random' else 15
        if design == 'mixed_bits':                                          # the queries 2^8 above the users: the mixed rows have 12 bits, so their lo plane is not 0
            ma = 7 if dim <= 256 else 3
            u_rows, q_rows, a_rows = ints((nu, dim), 15), ints((nq, dim), 15) * 256, ints((n_items, dim), ma)
        else:
            u_rows, q_rows, a_rows = ints((nu, dim), m), ints((nq, dim), m), ints((n_items, dim), m)
        item_exp, pair_exp = np.zeros(n_items, np.int64), np.zeros(n_pairs, np.int64)
        bias = ints(n_items, 40) * quantum
        if design == 'row_scales':
            eu = np.linspace(-20, 20, nu).round().astype(np.int64)[rng.permutation(nu)]
            u_rows, q_rows, pair_exp = u_rows * 2.0 ** eu[:, None], q_rows * 2.0 ** eu[:, None], eu[users]
            item_exp = np.linspace(-20, 20, n_items).round().astype(np.int64)[rng.permutation(n_items)]
            a_rows, bias = a_rows * 2.0 ** item_exp[:, None], np.zeros(n_items)
        return RankCase(name, dim, n_items, n_pairs, u_rows, q_rows, a_rows, users, queries, bias, lam, True, quantum, item_exp, pair_exp)
    v, classes = rank_values(design, n_pairs, n_items, dim, rng)
    m = 7 if dim <= 64 else (3 if dim <= 300 else 1)
    step = 2.0 ** math.ceil(math.log2(2 * dim * m * m + 1))
    pool = ints((4, dim), m)
    return RankCase(name, dim, n_items, n_pairs, ints((nu, dim), m), ints((nq, dim), m), pool[classes], users, queries, v * step, lam, True, quantum)


def float_case(design, n_pairs, n_items, dim, lam=0.3, seed=0):
    rng = _gen('float', design, n_pairs, n_items, dim, seed)
    nu, nq, users, queries = _pairs(n_pairs, False)
    shapes = ((nu, dim), (nq, dim), (n_items, dim))
    if design == 'randn':
        u_rows, q_rows, a_rows = (rng.standard_normal(s).astype(np.float32) for s in shapes)
    elif design == 'worst':                                                # the significand the split loses most on, all positive: the loss is one-sided
        x = np.float32(se.worst_two_fp16_significand()[0])
        u_rows, q_rows, a_rows = (x * np.exp2(rng.integers(-2, 3, s)).astype(np.float32) for s in shapes)
    elif design == 'wide_range':                                           # entries down to 2^-17 of their row's largest
        u_rows, q_rows, a_rows = ((rng.standard_normal(s) * np.exp2(rng.integers(-17, 1, s))).astype(np.float32) for s in shapes)
        for r in (u_rows, q_rows, a_rows):
            r[:, 0] = np.where(np.abs(r[:, 0]) < 1, 1.5, r[:, 0])
    else:
        raise KeyError(design)
    bias = (0.1 * rng.standard_normal(n_items)).astype(np.float32)
    name = f'{design} C={n_pairs} I={n_items} d={dim} lam={lam}'
    return RankCase(name, dim, n_items, n_pairs, u_rows.astype(np.float64), q_rows.astype(np.float64), a_rows.astype(np.float64), users, queries, bias, lam, False)


# =============================================================================================
# verdicts
# =============================================================================================
def _pow2_norm_rows(x):
    """True when every row of ``x`` has 1, 4 or 16 nonzeros, all of one power-of-two magnitude (so its norm is a power of two)."""
    ax = np.abs(x)
    mx = ax.max(1, keepdims=True)
    nnz = (ax > 0).sum(1)
    return bool(np.all((ax == 0) | (ax == mx))) and bool(np.all(np.isin(nnz, (1, 4, 16)))) and bool(np.all(np.log2(mx) == np.round(np.log2(mx))))


def ensure_exact(case, cosine=False):
    """Raises unless every score of the case is exact in the kernels' arithmetic.  Item rows have at most 11 significant bits (their ``lo`` plane is 0, so the omitted
    ``lo lo`` term is 0); for every (pair, item) ``sum_c |a_c m_c|`` and ``|score|`` are integers below 2^24 in units of the case's quantum times the two rows'
    powers of two.  Cosine: item rows and mixed rows of power-of-two norm besides, and the bias a multiple of 2^-4."""
    u, q, a = case.rows()
    _, e = np.frexp(a)
    lsb = np.where(a != 0, np.abs(a) / np.exp2(e - 11), 0.0)
    if not np.array_equal(lsb, np.round(lsb)):
        raise ValueError(f'{case.name}: an item entry has more than 11 significant bits')
    m = case.lam * q + (1 - case.lam) * u
    if not np.array_equal(m.astype(np.float32).astype(np.float64), m):
        raise ValueError(f'{case.name}: a mixed entry is not a float32')
    if cosine:
        if not (_pow2_norm_rows(a) and _pow2_norm_rows(m)):
            raise ValueError(f'{case.name}: a row has no power-of-two norm')
        b = case.bias.double().numpy() * 16
        if not (np.array_equal(b, np.round(b)) and np.abs(b).max() < 2 ** 20):
            raise ValueError(f'{case.name}: the bias is not a small multiple of 2^-4')
        return 16
    unit = case.quantum * np.exp2((case.pair_exp[:, None] + case.item_exp[None, :]).astype(np.float64))
    t = (np.abs(m) @ np.abs(a).T) / unit
    s = np.abs(case.scores64(False).numpy()) / unit
    b = case.bias.double().numpy()[None, :] / unit
    for name, x in (('sum |a m|', t), ('|score|', s), ('bias', b)):
        if not np.array_equal(x, np.round(x)):
            raise ValueError(f'{case.name}: {name} is not a multiple of the unit')
    worst = max(float(t.max()) * (1 + 2.0 ** -10), float(s.max()))         # (hi and lo of a mixed entry are accumulated apart: |hi| + |lo| <= (1 + 2^-10) |m|)
    if worst >= CAP:
        raise ValueError(f'{case.name}: {worst} >= 2^24 units - the case is not exact in float32')
    return worst


def expected(case, k, cosine):
    """``(top_scores [C, k] float32, top_items [C, k] int32)`` of the stable ranking of the float64 scores, the tail past ``min(k, I)`` ``(-FLT_MAX, -1)``."""
    s = case.scores64(cosine)
    n = min(k, case.n_items)
    order = tref.ranking(s, n)
    scores = torch.full((case.n_pairs, k), -FLT_MAX, dtype=torch.float32)
    items = torch.full((case.n_pairs, k), -1, dtype=torch.int32)
    scores[:, :n], items[:, :n] = torch.gather(s, 1, order).float(), order.int()
    return scores, items


def assert_exact(got_scores, got_items, case, k, cosine, what):
    want_scores, want_items = expected(case, k, cosine)
    got_scores, got_items = got_scores.cpu(), got_items.cpu()
    if not torch.equal(got_items, want_items):
        bad = (got_items != want_items).nonzero()[0].tolist()
        raise AssertionError(f'{what}: items differ from the stable ranking, first at (pair, rank) {bad}: got {int(got_items[tuple(bad)])}, want {int(want_items[tuple(bad)])}')
    if not torch.equal(got_scores, want_scores):
        bad = ((got_scores != want_scores) | torch.isnan(got_scores)).nonzero()[0].tolist()
        raise AssertionError(f'{what}: scores differ, first at (pair, rank) {bad}: got {float(got_scores[tuple(bad)])}, want {float(want_scores[tuple(bad)])}')


def score_bound(case, cosine):
    """[C, I] float64: the bound of the module docstring on ``|s - s64|`` of every (pair, item)."""
    u, q, a = case.rows()
    mm, t = case.magnitudes()
    s64 = case.scores64(cosine).numpy()
    n = 2.0 ** -36 * (np.abs(a).max(1)[None, :] * mm.sum(1)[:, None] + mm.max(1)[:, None] * np.abs(a).sum(1)[None, :])
    dot = (C_MIX + 48 * eval_ksteps(case.dim) + C_FIN) * U * t + SPLIT_LOSS * t + n
    if not cosine:
        return dot + U * np.abs(s64)
    m = case.lam * q + (1 - case.lam) * u
    na, nm = np.maximum(np.linalg.norm(a, axis=1), EPS), np.maximum(np.linalg.norm(m, axis=1), EPS)
    c_norm = ((case.dim + 63) // 64 + 7) / 2 + 2
    cos = np.abs(s64 - case.bias.double().numpy()[None, :])
    rel = 2 * c_norm * U + (C_MIX * U * np.linalg.norm(mm, axis=1) / nm)[:, None] + U
    return dot / (na[None, :] * nm[:, None]) + cos * rel + U * np.abs(s64)


def float_verdict(got_scores, got_items, case, k, cosine, what):
    """The ranking verdict of a float case, nothing left out: the returned scores do not increase, equal neighbours are in ascending id, the items are distinct and in
    range, every returned score is within its bound of ``s64[item]``, and no omitted item ``j`` has ``s64[j] - bound_j > s64[last] + bound_last``.  Returns the worst
    ``|s - s64| / bound``."""
    s64, bound = case.scores64(cosine).numpy(), score_bound(case, cosine)
    gs, gi = got_scores.cpu().numpy().astype(np.float64), got_items.cpu().numpy().astype(np.int64)
    n = min(k, case.n_items)
    assert gs.shape == gi.shape == (case.n_pairs, k), f'{what}: shape'
    assert np.all(gi[:, n:] == -1) and np.all(gs[:, n:] == -FLT_MAX), f'{what}: the tail past min(k, items) is not (-FLT_MAX, -1)'
    gs, gi = gs[:, :n], gi[:, :n]
    assert np.all(np.isfinite(gs)), f'{what}: a score is not finite'
    assert np.all((gi >= 0) & (gi < case.n_items)), f'{what}: an item id is out of range'
    assert all(len(set(row)) == n for row in gi.tolist()), f'{what}: an item is returned twice'
    assert np.all(gs[:, 1:] <= gs[:, :-1]), f'{what}: the scores increase somewhere'
    assert np.all((gs[:, 1:] < gs[:, :-1]) | (gi[:, 1:] > gi[:, :-1])), f'{what}: equal scores are not in ascending id'
    rows = np.arange(case.n_pairs)[:, None]
    ratio = np.abs(gs - s64[rows, gi]) / bound[rows, gi]
    worst = float(ratio.max())
    assert worst <= 1.0, f'{what}: |s - s64| / bound = {worst:.3g} at (pair, rank) {np.unravel_index(int(ratio.argmax()), ratio.shape)}'
    omitted = np.ones_like(s64, bool)
    omitted[rows, gi] = False
    floor = (s64[rows, gi[:, -1:]] + bound[rows, gi[:, -1:]])
    beats = omitted & (s64 - bound > floor)
    assert not beats.any(), f'{what}: an omitted item beats the last returned one beyond both bounds, (pair, item) {np.argwhere(beats)[0].tolist()}'
    return worst


# =============================================================================================
# emulation
# =============================================================================================
MUTATIONS = ('drop_hi_lo', 'read_column_tail', 'padded_item_competes', 'swap_lane_halves', 'ties_by_higher_id', 'worst_last_entry_for_t', 'boundary_not_advanced',
             'drop_tenth_entry', 'score_pair_past_end', 'halves_by_sixteen')
LIST_MAPPINGS = ('swap_lane_halves', 'halves_by_sixteen')


def _f32(x):
    return np.asarray(x, np.float32)


def _prepare(x, dp, cosine, mutation):
    """Rows -> (hi, lo) float32 planes [n, dp] under each row's scale, and the row's inverse factor (float32): ``score_prepare_kernel`` / the mixed rows' loop."""
    x = _f32(x)
    n, dim = x.shape
    mx = np.abs(x).max(1) if dim else np.zeros(n, np.float32)
    sc = se.scale_up_for(mx)
    inv = _f32(1.0 / sc)
    xs = np.zeros((n, dp), np.float32)
    xs[:, :dim] = _f32(x * _f32(sc)[:, None])
    if mutation == 'read_column_tail':                                     # what lies behind the row, read as if it belonged to it
        xs[:, dim:] = _f32(mx * _f32(sc))[:, None]
    hi, lo = se.split_two_fp16(xs)
    if cosine:
        lanes = np.zeros((n, 64), np.float32)
        for c in range(dim):
            lanes[:, c % 64] = lanes[:, c % 64] + x[:, c] * x[:, c]
        for off in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, np.arange(64) ^ off]
        inv = _f32(inv / np.maximum(np.sqrt(lanes[:, 0]), np.float32(EPS)))
    return _f32(hi), _f32(lo), inv


def emu_scores(case, cosine=False, mutation=None):
    """[C, I] float32 (``padded_item_competes``: [C, 32 tiles]): the kernels' scores - the mix in float32, both splits, three products per column accumulated in
    float32 k-step by k-step, the two inverse factors and the bias."""
    f = case.features.numpy()
    lam = np.float32(case.lam)
    per = 32 * eval_pair_tiles(case.dim)
    pr = np.arange((case.n_pairs + per - 1) // per * per)
    if mutation != 'score_pair_past_end':
        pr = np.minimum(pr, case.n_pairs - 1)                               # pairs past the end repeat the last one
    users, queries = case.users.numpy()[pr], case.queries.numpy()[pr]       # (IndexError: a pair past n_pairs was read)
    m = _f32(_f32(lam * f[queries + case.query_row0]) + _f32(_f32(np.float32(1) - lam) * f[users]))[:case.n_pairs]
    a = f[case.item_row0:]
    bias = case.bias.numpy()
    if mutation == 'padded_item_competes':
        pad = (-case.n_items) % 32
        a = np.concatenate([a, np.ones((pad, case.dim), np.float32)])
        bias = np.concatenate([bias, np.zeros(pad, np.float32)])
    ksteps = eval_ksteps(case.dim)
    ah, al, ainv = _prepare(a, 16 * ksteps, cosine, mutation)
    mh, ml, minv = _prepare(m, 16 * ksteps, cosine, mutation)
    acc = np.zeros((len(m), len(a)), np.float32)
    for ks in range(ksteps):
        for pa, pm in ((ah, ml), (al, mh), (ah, mh)):
            if mutation == 'drop_hi_lo' and pm is ml:
                continue
            for c in range(16 * ks, 16 * ks + 16):
                acc = acc + pm[:, c, None] * pa[None, :, c]
    return _f32(_f32(acc * _f32(ainv[None, :] * minv[:, None])) + bias[None, :])


def emulate(case, k, cosine=False, deep=False, mutation=None, scores=None):
    """The whole call: ``(top_scores [C, k] float32, top_items [C, k] int32, passes [C] or None)``.  ``scores``: the [C, I] float32 scores, where the caller has them
    (an exact case: float32 of the float64 scores)."""
    s = emu_scores(case, cosine, mutation) if scores is None else _f32(scores)
    n_pairs, n_all = s.shape
    mapping = mutation if mutation in LIST_MAPPINGS else None
    lists = list_of(n_pairs, case.n_items, case.dim, mapping)
    if n_all > case.n_items:                                               # padded items of the last tile: the lists of its run
        ids = np.arange(case.n_items, n_all)
        lists = np.concatenate([lists, lists[-1] // 2 * 2 + half_of(ids & 31, mapping)])
    keep = TOP - 1 if mutation == 'drop_tenth_entry' else TOP
    out_s = np.full((n_pairs, k), -FLT_MAX, np.float32)
    out_i = np.full((n_pairs, k), -1, np.int32)
    passes = np.zeros(n_pairs, np.int32)
    target = min(k, case.n_items)
    ids = np.arange(n_all)
    for c in range(n_pairs):
        order = np.lexsort((-ids if mutation == 'ties_by_higher_id' else ids, -s[c].astype(np.float64)))    # ranks_before: a strict total order
        lists_ranked = lists[order]

        def partial_lists(after):
            """Per list the global positions of its first ten candidates that rank after position ``after``: (positions, a mask of those that close a full list)."""
            pos = np.arange(after + 1, n_all)
            by_list = np.argsort(lists_ranked[pos], kind='stable')
            l_sorted = lists_ranked[pos][by_list]
            start = np.searchsorted(l_sorted, l_sorted, 'left')
            nth = np.arange(len(pos)) - start
            full = np.zeros(len(pos), bool)
            count = np.bincount(l_sorted, minlength=int(lists.max()) + 1)[l_sorted]
            if keep < TOP:
                full_last = (nth == keep - 1) & (count >= TOP)
                held = (nth < keep) | ((count < TOP) & (nth < TOP))
            else:
                full_last = (nth == TOP - 1)
                held = nth < TOP
            return pos[by_list][held], pos[by_list][full_last]

        if not deep:
            held, _ = partial_lists(-1)
            best = np.sort(held)[:k]
            out_s[c, :len(best)], out_i[c, :len(best)] = s[c, order[best]], order[best]
            continue
        count, boundary = 0, -1
        for _ in range(max_passes(k, case.n_items)):
            if count >= target:
                break
            held, lasts = partial_lists(boundary)
            t = n_all if len(lasts) == 0 else int(lasts.max() if mutation == 'worst_last_entry_for_t' else lasts.min())
            emit = np.sort(held[held <= t])[:k - count]
            out_s[c, count:count + len(emit)], out_i[c, count:count + len(emit)] = s[c, order[emit]], order[emit]
            count += len(emit)
            if mutation != 'boundary_not_advanced' and len(emit):
                boundary = int(emit[-1])
            passes[c] += 1
    return out_s, out_i, (passes if deep else None)
