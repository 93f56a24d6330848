"""Cases, float64 references, bounds and a numpy emulation for the matrix-core contractions - the interactive layer in its hyperedge form (``ihg_interact_fwd``,
``ihg_interact_bwd``, ``_user_reduced``, ``_user_reduced_planes``, ``_gathered``), its node-level form (``ihg_node_interact_fwd``, ``ihg_node_interact_bwd_weight``) and
the node-level linear maps (``ihg_node_linear_*``).  Test infrastructure: ``tests/test_contraction_kernels.py`` (GPU) and ``tests/test_contraction_host.py`` (CPU) read
it, the product imports nothing from it.

* **Launch table** (``edge_launch``, ``node_launch``, ``node_weight_plan``, ``node_linear_accumulates``): for each (entry, d, order, arithmetic mode) which arithmetic takes the call, the tile size
  and the number of tile ranges of every kernel behind it, whether the call is refused.  It is the tests' own statement of ``csrc/interact.hip``'s dispatch: the
  GPU tests assert the ``*_supported`` answers against it, the ladders below are derived from it.
* **Exact cases**: every operand an integer in [-m, m] (m <= 4), every scale a power of two, degrees small non-negative integers.  Integers of this size are exact
  under the two-fp16 split (``lo = 0``), the three-bf16 split, the fp32 MFMA and the scalar kernels, and every partial sum in any order is a float32 value as long as
  ``sum |terms|`` of the output element stays below 2^24 units.  ``ensure_exact`` checks that in int64 for EVERY output element and raises: a case beyond the cap
  is a broken case.  The verdict is ``torch.equal`` with the float64 reference cast to float32 (``assert_equal``).
* **Float cases**: ``|got - want| <= ((K + c) 2^-24 + L) sum |terms|`` per element (``float_bound``; K, c and L derived next to it).
* **Emulation** (``emu_*``): numpy float32 accumulation in a fixed order over the kernels' tiles and ranges with the same operand split and the same kept
  partial products; each takes a ``mutation`` that breaks it in one named way - the host test shows that every mutation fails a named case.
"""
import functools

import numpy as np
import torch

import split_emulation as SE

U = 2.0 ** -24                       # unit roundoff of float32
CAP = 1 << 24                        # sum |terms| of an exact case stays below this many units
SPLIT_LOSS = 2.0 ** -21              # what either operand split loses per product, relative (tests/test_host_logic.py holds both emulations to it)
MFMA_DIMS = (32, 64, 128, 256)
SCALAR_DIMS = (8, 12)
ARITHS = ('split', 'f32')            # IHG_INTERACT_ARITH unset / 'f32'
ORDERS = (2, 3)
ENTRIES = ('fwd', 'bwd', 'user_reduced', 'planes', 'gathered')


def product_blocks(order):
    return 4 if order == 3 else 3


def weight_columns(order):
    return (7 if order == 3 else 6)


# =============================================================================================
# the launch table
# =============================================================================================
class Kernel:
    """One tiled kernel of a launch: ``te`` rows per tile, ``ranges`` workgroups (waves at d = 32) that share the tiles - ``'contiguous'``: range r takes tiles
    [r per, (r + 1) per) with per = ceil(tiles / ranges); ``'strided'``: tiles r, r + ranges, ...  ``per`` below is the largest number of tiles one range takes.
    ``arithmetic``: how the kernel multiplies - 'two_fp16' (operands under a power of two, two fp16 terms, three products), 'three_bf16' (three bf16 terms, six
    products), 'f32' (fp32 MFMA)."""

    def __init__(self, name, te, ranges, deal, arithmetic='f32'):
        self.name, self.te, self.ranges, self.deal, self.arithmetic = name, te, ranges, deal, arithmetic

    def per(self, n_rows):
        tiles = -(-n_rows // self.te)
        return -(-tiles // self.ranges)

    def used_ranges(self, n_rows):
        tiles = -(-n_rows // self.te)
        if self.deal == 'strided':
            return min(tiles, self.ranges)
        return -(-tiles // max(self.per(n_rows), 1)) if tiles else 0

    def last_fill(self, n_rows):
        return n_rows - (-(-n_rows // self.te) - 1) * self.te if n_rows else 0

    def ladder(self):
        """1, TE - 1, TE, TE + 1 rows; RANGES TE - 1, RANGES TE, RANGES TE + 1 (``per`` becomes 2); (2 RANGES + 1) TE + 5 (``per`` = 3, whole empty ranges at the end
        under the contiguous deal, a partial last tile)."""
        te, r = self.te, self.ranges
        return [1, te - 1, te, te + 1, r * te - 1, r * te, r * te + 1, (2 * r + 1) * te + 5]


_SPLIT_RANGES = {64: 256, 128: 128, 256: 32}     # 256 workgroups / column parts (1, 2, 8) of the split member-gradient and weight-gradient kernels


def _members(dim, arith, user_reduced):
    if dim == 32:
        return Kernel('members_narrow', 16, 2048, 'contiguous') if user_reduced else Kernel('members_ws', 128, 256, 'strided')
    if arith == 'split':
        return Kernel('members_split', 32, _SPLIT_RANGES[dim], 'contiguous', 'two_fp16')
    if user_reduced:
        return Kernel('members_strip_ur', 32, 256, 'contiguous') if dim == 128 else None
    return {64: Kernel('members_ws', 64, 256, 'strided'), 128: Kernel('members_strip', 32, 256, 'strided'), 256: Kernel('members_strip256', 16, 64, 'strided')}[dim]


def _weights(dim, arith):
    if dim == 32:
        return Kernel('weight_mfma32', 64, 512, 'strided')
    if arith == 'split':
        return Kernel('weight_split', 32, _SPLIT_RANGES[dim], 'contiguous', 'three_bf16')
    return {64: Kernel('weight_ws', 64, 256, 'strided'), 128: Kernel('weight_strip', 32, 256, 'strided'), 256: Kernel('weight_ws', 64, 16, 'strided')}[dim]


def edge_launch(entry, dim, order, arith):
    """``dict(supported, arithmetic, kernels)`` of one entry point of the hyperedge form on 16-byte aligned operands with ``ld % 4 == 0``.  ``arithmetic``: the
    family that takes the call - 'split' (the 16-bit matrix pipe: L = 2^-21 in the bound), 'f32' (fp32 MFMA) or 'scalar'; ``kernels``: the tiled kernels in launch
    order (``[]`` for the scalar ones), each with the operand split IT uses: in the split family the forward and the weight gradient take three bf16 terms, the
    member gradients two fp16 terms - a backward launch runs one kernel of each (``launch_splits``).  A launch that is not ``supported`` must return
    ``IHG_ERR_INVALID`` and write nothing."""
    assert entry in ENTRIES and order in ORDERS and arith in ARITHS
    if dim not in MFMA_DIMS:
        return dict(supported=entry in ('fwd', 'bwd'), arithmetic='scalar', kernels=[])
    takes = 'split' if arith == 'split' and dim != 32 else 'f32'
    if entry == 'fwd':
        kernel = {('split', 64): Kernel('fwd_split_ws', 16, 256, 'strided', 'three_bf16'), ('split', 128): Kernel('fwd_kpass', 32, 256, 'contiguous', 'three_bf16'),
                  ('split', 256): Kernel('fwd_kpass', 16, 128, 'contiguous', 'three_bf16'), ('f32', 32): Kernel('fwd_ws', 128, 256, 'strided'),
                  ('f32', 64): Kernel('fwd_ws', 64, 256, 'strided'), ('f32', 128): Kernel('fwd_strip', 32, 256, 'strided'),
                  ('f32', 256): Kernel('fwd_strip256', 16, 64, 'strided')}[(takes, dim)]
        return dict(supported=True, arithmetic=takes, kernels=[kernel])
    if entry == 'bwd':
        return dict(supported=True, arithmetic=takes, kernels=[_members(dim, arith, False), _weights(dim, arith)])
    if entry == 'user_reduced':
        ok = dim in (32, 128) or arith == 'split'
    elif entry == 'planes':
        ok = dim == 256 and arith == 'split'
    else:
        ok = dim == 32 or (dim in (64, 128) and arith == 'split')
    if not ok:
        return dict(supported=False, arithmetic=takes, kernels=[])
    return dict(supported=True, arithmetic=takes, kernels=[_members(dim, arith, True)] + ([] if entry == 'planes' else [_weights(dim, arith)]))


def launch_splits(launch):
    """The operand splits among a launch's kernels, in launch order: each gets a float case built from ITS adversarial significand."""
    return [a for a in dict.fromkeys(k.arithmetic for k in launch['kernels']) if a != 'f32']


def worst_significand(arithmetic):
    """``split_emulation.worst_*`` for a split; for the fp32-MFMA and scalar kernels, which have none, the significand with every low bit set."""
    return _worst(arithmetic if arithmetic == 'two_fp16' else 'three_bf16')


@functools.lru_cache(maxsize=None)
def _worst(split):
    return (SE.worst_two_fp16_significand if split == 'two_fp16' else SE.worst_three_bf16_significand)()[0]


def edge_ladder(entry, dim, order, arith):
    """The hyperedge counts of the exact ladder of one launch: the union of its kernels' ladders (members, then weights); the scalar kernels: around one workgroup of
    256 threads' worth of elements."""
    launch = edge_launch(entry, dim, order, arith)
    counts = set()
    for k in launch['kernels']:
        counts.update(k.ladder())
    if not launch['kernels']:
        counts.update([1, 2, 256 // dim, 256 // dim + 1, 3 * 256 // dim + 2, 1027])
    return sorted(counts)


def node_launch(entry, dim, arith):
    """The node-level form: ``entry`` 'fwd' (``ihg_node_interact_fwd``) or 'weight' (``ihg_node_interact_bwd_weight``).  ``tile``: rows per tile (tiles never cross a
    node type), ``group``: tiles per workgroup visit of the forward."""
    if dim == 32:
        return dict(supported=True, arithmetic='f32', split='f32', tile=16, group=8, ranges=512)
    ok = arith == 'split' and dim in (64, 128, 256)
    return dict(supported=ok, arithmetic='split', split='two_fp16', tile=16 if dim == 64 and entry == 'fwd' else 32, group=4 if dim == 256 else 8, ranges=_SPLIT_RANGES.get(dim, 0))


def node_weight_plan(type_begin, dim):
    """``[(ranges of type t, tiles per range)]`` as the host code of ``ihg_node_interact_bwd_weight`` deals them: tiles of 32 rows (d = 32: blocks of 64 rows, 512
    ranges), ranges by type in proportion to the tiles (d = 32: the rows) out of ``ranges - 2``, every non-empty type at least one and at most one per tile."""
    ranges, unit = (512, 64) if dim == 32 else (_SPLIT_RANGES[dim], 32)
    rows = [type_begin[t + 1] - type_begin[t] for t in range(3)]
    tiles = [-(-r // unit) for r in rows]
    weight = rows if dim == 32 else tiles
    total = max(sum(weight), 1)
    plan = []
    for t in range(3):
        n = 0 if tiles[t] == 0 else min(max(1, weight[t] * (ranges - 2) // total), tiles[t])
        per = 0 if n == 0 else (-(-(-(-rows[t] // n)) // unit) if dim == 32 else -(-tiles[t] // n))
        plan.append((n, per))
    return plan


def rows_for_tiles_per_range(dim, per):
    """Rows of one type, beside two types of at most two tiles each, at which ``node_weight_plan`` gives that type ``per`` tiles per range: per (ranges - 6) tiles, the
    last one of 3 rows (tiles of 32 rows; d = 32: blocks of 64 rows)."""
    ranges, unit = (512, 64) if dim == 32 else (_SPLIT_RANGES[dim], 32)
    return (per * (ranges - 6) - 1) * unit + 3


def node_linear_accumulates(dim, arith):
    """``ihg_node_linear_bwd_accumulates`` on aligned rows: d = 32 / 64 always, d = 128 / 256 on the split kernels."""
    return dim in (32, 64) or (dim in (128, 256) and arith == 'split')


def type_ladder(tile, group):
    """Row counts of one node type: 0, 1, TILE - 1, TILE, TILE + 1, GROUP TILE - 1, GROUP TILE + 1."""
    return [0, 1, tile - 1, tile, tile + 1, group * tile - 1, group * tile + 1]


def type_cases(dim):
    """``type_begin`` tuples: every rung of the type ladder (tiles of 16 and of 32, this width's group) in each of the three positions beside types of 5 and 37 rows;
    an empty first type, an empty last type, two empty types (each of the three ways)."""
    group = 4 if dim == 256 else 8
    sizes = sorted(set(type_ladder(16, group)) | set(type_ladder(32, group)))
    cases = []
    for pos in range(3):
        for n in sizes:
            rows = [5, 37, 21]
            rows[pos] = n
            cases.append(rows)
    cases += [[0, 33, 17], [33, 17, 0], [0, 0, 33], [0, 33, 0], [33, 0, 0]]
    return [tuple(int(x) for x in np.concatenate([[0], np.cumsum(c)])) for c in cases]


# =============================================================================================
# operands
# =============================================================================================
def _gen(*key):
    return np.random.default_rng([int(k) if not isinstance(k, str) else sum(ord(c) for c in k) for k in key])


def ints(rng, shape, m):
    return torch.from_numpy(rng.integers(-m, m + 1, shape).astype(np.float64))


def pow2(rng, n, exps=(-1, 0, 1, 2)):
    return torch.from_numpy(np.ldexp(1.0, rng.choice(np.asarray(exps), n)).astype(np.float64))


def floats(rng, shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32).astype(np.float64))


def scales(rng, n):
    return torch.from_numpy((0.5 + rng.random(n)).astype(np.float32).astype(np.float64))


class EdgeCase:
    """Operands of the hyperedge form, float64 tensors whose values are float32 values: ``h`` [n_nodes, d], ``p`` [n_nodes, d], ``w`` [d, k d], ``dout`` [E, d],
    ``dy`` [n_nodes, d] with ``dy_scale`` [n_nodes] (the gathering form), ``i3`` [E, 3] int32 with ``i3[:, 0]`` non-decreasing and ``< n_users``."""

    def __init__(self, i3, n_users, n_nodes, dim, order, rng, exact, m=4):
        self.i3, self.n_users, self.n_nodes, self.dim, self.order, self.exact, self.m = i3, n_users, n_nodes, dim, order, exact, m
        self.reference = {}          # the float64 reference of the case, computed once by the test that runs it and shared by the entry's call forms
        k = weight_columns(order)
        e = len(i3)
        if exact:
            self.h, self.p, self.w = ints(rng, (n_nodes, dim), m), ints(rng, (n_nodes, dim), m), ints(rng, (dim, k * dim), m)
            self.dout, self.dy, self.dy_scale = ints(rng, (e, dim), m), ints(rng, (n_nodes, dim), m), pow2(rng, n_nodes)
        else:
            self.h, self.p, self.w = floats(rng, (n_nodes, dim)), floats(rng, (n_nodes, dim)), floats(rng, (dim, k * dim)) / np.sqrt(dim)
            self.w = self.w.float().double()
            self.dout, self.dy, self.dy_scale = floats(rng, (e, dim)), floats(rng, (n_nodes, dim)), scales(rng, n_nodes)

    def to(self, device):
        for name in ('i3', 'h', 'p', 'w', 'dout', 'dy', 'dy_scale'):
            setattr(self, name, getattr(self, name).to(device))
        return self


def random_i3(rng, n_edges, n_users, n_q=37, n_i=29, user_of=None):
    """[E, 3] int32 global ids (u, U + q, U + Q + i) with the users non-decreasing; few queries and items, so neighbouring hyperedges often gather the same row."""
    users = np.sort(rng.integers(0, n_users, n_edges)) if user_of is None else np.asarray(user_of)
    i3 = np.stack([users, n_users + rng.integers(0, n_q, n_edges), n_users + n_q + rng.integers(0, n_i, n_edges)], 1).astype(np.int32)
    return torch.from_numpy(i3), n_users + n_q + n_i


def edge_case(n_edges, dim, order, key, exact=True, m=4, layout=None):
    """The case of a test, from its key: random users (about three hyperedges each, two users without any) or ``layout = (users [E], n_users)``."""
    rng = _gen(*key)
    if layout is None:
        n_users = max(1, n_edges // 3) + 2
        i3, n_nodes = random_i3(rng, n_edges, n_users)
    else:
        users, n_users = layout
        i3, n_nodes = random_i3(rng, n_edges, n_users, user_of=users)
    return EdgeCase(i3, n_users, n_nodes, dim, order, rng, exact, m)


def float_case(entry, dim, order, arith, design):
    """The float case of one kernel instance, as the GPU test and the host test both build it: 9 TE + 5 hyperedges of the launch's first kernel; ``design``
    'randn', or 'worst two_fp16' / 'worst three_bf16' / 'worst f32': every operand the adversarial significand of that split (``worst_significand``) under a
    power of two in {1/2, 1, 2} (w: also 2^-floor(log2(d) / 2)), ALL POSITIVE - the products of a sum share a sign, so what the split leaves out adds up."""
    launch = edge_launch(entry, dim, order, arith)
    te = launch['kernels'][0].te if launch['kernels'] else 8
    case = edge_case(9 * te + 5, dim, order, ('float', entry, dim, order, design), exact=False)
    if design != 'randn':
        make_worst(case, ('h', 'w', 'dout', 'dy', 'p'), design.split()[1], dim + order)
    return case


def make_worst(case, names, arithmetic, seed):
    """Every element of the named operands becomes ``worst_significand(arithmetic)`` times a power of two in {1/2, 1, 2} (``w``: times 2^-floor(log2(d) / 2) as
    well), all positive."""
    s = worst_significand(arithmetic)
    gen = torch.Generator().manual_seed(seed)
    for name in names:
        t = getattr(case, name)
        exp = torch.randint(-1, 2, t.shape, generator=gen).double() - (int(np.log2(case.dim)) // 2 if name == 'w' else 0)
        setattr(case, name, (s * torch.pow(2.0, exp)).float().double().to(t.device))


def float_designs(launch):
    return ['randn'] + [f'worst {a}' for a in (launch_splits(launch) or ['f32'])]


def user_runs(kernel, rng=None):
    """The user-run ladder of one user-reduced member-gradient kernel (``te`` hyperedges per tile, ``ranges`` contiguous tile ranges): (1.5 ranges) te + 5 hyperedges,
    so ``per`` = 2, a quarter of the ranges is empty and the last tile is partial.  With P = per te hyperedges per range, in hyperedge order:
    run [0, P): range 0 is one run;  short runs up to 2 P (a run ends on range 1's last hyperedge, the next starts on range 2's first);  a run of 1.5 te;  a run of
    3 P + 1 starting mid-tile (ranges 3 and 4 lie wholly inside it);  runs of te - 1, te, te + 1;  a run of 5 for hyperedges that all gather the same rows (``same_rows``);
    2 te + 3 users with one hyperedge each;  runs of 1 .. 2 te up to the last te + 5 hyperedges, which are one run.  Users without hyperedges: two at the start, one
    after every third run, three at the end.  Returns ``dict(users [E], n_users, runs [(user, begin, end)], named {name: run index}, same_rows (begin, end))``."""
    rng = rng or _gen('runs', kernel.te, kernel.ranges)
    te, n_edges = kernel.te, (kernel.ranges + kernel.ranges // 2) * kernel.te + 5
    per = kernel.per(n_edges)
    assert per == 2
    p = per * te
    lengths, named = [p], {'one_range': 0}
    pos = p
    while pos < 2 * p:
        n = min(int(rng.integers(1, 6)), 2 * p - pos)
        lengths.append(n)
        pos += n
    named['ends_on_range_end'] = len(lengths) - 1
    named['starts_on_range_begin'] = len(lengths)
    lengths.append(te + te // 2)
    named['through_ranges'] = len(lengths)
    lengths.append(3 * p + 1)
    for n in (te - 1, te, te + 1):
        named[f'run_{n - te:+d}'] = len(lengths)
        lengths.append(n)
    named['same_rows'] = len(lengths)
    lengths.append(5)
    named['singles'] = len(lengths)
    lengths += [1] * (2 * te + 3)
    pos = sum(lengths)
    while pos < n_edges - (te + 5):
        n = min(int(rng.integers(1, 2 * te + 1)), n_edges - (te + 5) - pos)
        lengths.append(n)
        pos += n
    named['last'] = len(lengths)
    lengths.append(te + 5)
    assert sum(lengths) == n_edges
    users, runs, user, begin = np.empty(n_edges, np.int64), [], 2, 0
    for k, n in enumerate(lengths):
        users[begin:begin + n] = user
        runs.append((user, begin, begin + n))
        begin += n
        user += 2 if k % 3 == 2 else 1
    same = runs[named['same_rows']]
    return dict(users=users, n_users=user + 3, runs=runs, named=named, same_rows=(same[1], same[2]), per=per)


def run_layout(kind, n_edges):
    """``(users [E], n_users)``: 'singles' - every user one hyperedge; 'one' - one user (of three) owns everything."""
    if kind == 'singles':
        return np.arange(n_edges, dtype=np.int64), n_edges
    return np.full(n_edges, 1, np.int64), 3


# =============================================================================================
# float64 references.  Every function returns ``(value, magnitude)``: the magnitude is the same expression over the operands' absolute values - sum |terms| of
# the output element, which bounds every partial sum in any order.
# =============================================================================================
def _tn(a, b, chunk=512):
    """``a^T b`` for tall operands [n, .]: chunks of rows as one batched product, then their sum (a library GEMM with two small dimensions and a long contraction
    runs in one workgroup on the GPU; on integers every order of the float64 additions gives the same value)."""
    n = a.shape[0]
    if n <= 2 * chunk:
        return a.T @ b
    pad = (-n) % chunk
    if pad:
        a, b = torch.cat([a, a.new_zeros(pad, a.shape[1])]), torch.cat([b, b.new_zeros(pad, b.shape[1])])
    return torch.bmm(a.view(-1, chunk, a.shape[1]).transpose(1, 2), b.view(-1, chunk, b.shape[1])).sum(0)


def _run_sums(rows, counts):
    """Sums of consecutive runs of ``rows`` [E, d] (``counts[u]`` rows for user u, users in order) as differences of the float64 running sum: exact on the integer
    cases (every running sum is an integer below 2^53), and within 2^-52 of the running total - nothing beside the float bounds - otherwise.  (An ``index_add_`` of
    50 k rows into one row is half a second of colliding atomics on the GPU.)"""
    running = torch.cat([rows.new_zeros(1, rows.shape[1]), rows.cumsum(0)])
    ends = counts.cumsum(0)
    return running[ends] - running[ends - counts]


def _members_of(c):
    i3 = c.i3.long()
    return c.h[i3[:, 0]], c.h[i3[:, 1]], c.h[i3[:, 2]]


def _blocks(c, w=None):
    w = c.w if w is None else w
    d = c.dim
    return [w[:, (3 + b) * d:(4 + b) * d] for b in range(product_blocks(c.order))]


def _products(hu, hq, hi, order):
    z = [hu * hq, hq * hi, hi * hu]
    return z + [hu * hq * hi] if order == 3 else z


def fwd64(c):
    """out[e] = p[u] + p[q] + p[i] + sum_b W_b z_b(e)."""
    i3 = c.i3.long()
    out = c.p[i3[:, 0]] + c.p[i3[:, 1]] + c.p[i3[:, 2]]
    mag = c.p.abs()[i3[:, 0]] + c.p.abs()[i3[:, 1]] + c.p.abs()[i3[:, 2]]
    hu, hq, hi = _members_of(c)
    for z, wb in zip(_products(hu, hq, hi, c.order), _blocks(c)):
        out = out + z @ wb.T
        mag = mag + z.abs() @ wb.abs().T
    return out, mag


def gathered_dout64(c):
    """dout[e] = sum over the three members m of dy_scale[m] dy[m]."""
    rows = c.dy * c.dy_scale[:, None]
    i3 = c.i3.long()
    return rows[i3[:, 0]] + rows[i3[:, 1]] + rows[i3[:, 2]], rows.abs()[i3[:, 0]] + rows.abs()[i3[:, 1]] + rows.abs()[i3[:, 2]]


def bwd64(c, dout=None, dout_mag=None):
    """``dict(g [E, 3, d], dw [d, nblk d], g2, dh [n_users, d], has_edges [n_users])`` with magnitudes under ``'<name>_mag'``: the member gradients through the product
    terms, the product blocks' weight gradient, the user slot summed per user."""
    dout = c.dout if dout is None else dout
    dmag = dout.abs() if dout_mag is None else dout_mag
    hu, hq, hi = _members_of(c)
    dz = [dout @ wb for wb in _blocks(c)]
    dza = [dmag @ wb.abs() for wb in _blocks(c)]

    def slots(dz, hu, hq, hi):
        gu, gq, gi = dz[0] * hq + dz[2] * hi, dz[0] * hu + dz[1] * hi, dz[1] * hq + dz[2] * hu
        if c.order == 3:
            gu, gq, gi = gu + dz[3] * hq * hi, gq + dz[3] * hu * hi, gi + dz[3] * hu * hq
        return torch.stack([gu, gq, gi], 1)
    g, g_mag = slots(dz, hu, hq, hi), slots(dza, hu.abs(), hq.abs(), hi.abs())
    z = _products(hu, hq, hi, c.order)
    dw = torch.cat([_tn(dout, zb) for zb in z], 1)
    dw_mag = torch.cat([_tn(dmag, zb.abs()) for zb in z], 1)
    users = c.i3[:, 0].long()
    counts = torch.bincount(users, minlength=c.n_users)
    dh, dh_mag, has = _run_sums(g[:, 0], counts), _run_sums(g_mag[:, 0], counts), counts > 0
    return dict(g=g, g_mag=g_mag, dw=dw, dw_mag=dw_mag, g2=g[:, 1:], g2_mag=g_mag[:, 1:], dh=dh, dh_mag=dh_mag, has_edges=has)


# ---- the node-level form ----
# X blocks of a node v with the sums S_a, S_b, S_ab over the OTHER two members (a, b) of its hyperedges - (query, item) for a user, (user, item) for a query,
# (user, query) for an item - and the block of w = [A_u | A_q | A_i | W_uq | W_qi | W_iu | W_uqi] each meets.  From the hyperedge form: a user's hyperedge feature is
# A_u h + A_q h_a + A_i h_b + W_uq (h h_a) + W_qi (h_a h_b) + W_iu (h_b h) + W_uqi (h h_a h_b), summed over its hyperedges; likewise for the other two types.
X_BLOCKS = ('deg h', 'S_a', 'h S_a', 'S_b', 'h S_b', 'S_ab', 'h S_ab')
W_BLOCK_OF = {0: (0, 1, 3, 2, 5, 4, 6), 1: (1, 0, 3, 2, 4, 5, 6), 2: (2, 0, 5, 1, 4, 3, 6)}
PRODUCT_X = (2, 4, 5, 6)             # the X blocks that meet the product blocks of w (the weight gradient's)


class NodeCase:
    """Operands of the node-level form with ARBITRARY sums: ``h`` [N, d], ``sums`` [N, 3 d], ``degree`` [N] (isolated nodes: degree 0 and zero sums), ``scale`` [N]
    (``out_scale`` / ``dy_scale``), ``bias`` [d], ``w`` [d, k d], ``dy`` [N, d].  ``row_exp``: per-row exponents (h, dy) of the running-scale cases."""

    def __init__(self, type_begin, dim, order, rng, exact, m=4, row_exp=None, zero_rows=None):
        n = type_begin[3]
        self.type_begin, self.dim, self.order, self.exact, self.n = tuple(type_begin), dim, order, exact, n
        k = weight_columns(order)
        if exact:
            self.h, self.sums, self.dy = ints(rng, (n, dim), m), ints(rng, (n, 3 * dim), m), ints(rng, (n, dim), m)
            self.w, self.bias, self.scale = ints(rng, (dim, k * dim), m), ints(rng, (dim,), m), pow2(rng, n)
            self.degree = torch.from_numpy(rng.integers(0, 6, n).astype(np.float64))
        else:
            self.h, self.sums, self.dy = floats(rng, (n, dim)), floats(rng, (n, 3 * dim)), floats(rng, (n, dim))
            self.w, self.bias, self.scale = (floats(rng, (dim, k * dim)) / np.sqrt(dim)).float().double(), floats(rng, (dim,)), scales(rng, n)
            self.degree = torch.from_numpy(rng.integers(1, 6, n).astype(np.float64))
        self.isolated = torch.from_numpy(rng.random(n) < 0.1)
        self.degree[self.isolated] = 0
        self.sums[self.isolated] = 0
        if row_exp is not None:
            self.h = self.h * torch.from_numpy(np.ldexp(1.0, row_exp[0]))[:, None]
            self.dy = self.dy * torch.from_numpy(np.ldexp(1.0, row_exp[1]))[:, None]
        if zero_rows is not None:
            self.h[torch.from_numpy(zero_rows[0])] = 0
            self.sums[torch.from_numpy(zero_rows[0])] = 0
            self.dy[torch.from_numpy(zero_rows[1])] = 0

    def to(self, device):
        for name in ('h', 'sums', 'dy', 'w', 'bias', 'scale', 'degree'):
            setattr(self, name, getattr(self, name).to(device))
        return self


def x_blocks(c, absolute=False):
    d = c.dim
    h, s = (c.h.abs(), c.sums.abs()) if absolute else (c.h, c.sums)
    sa, sb, sab = s[:, :d], s[:, d:2 * d], s[:, 2 * d:]
    x = [c.degree[:, None] * h, sa, h * sa, sb, h * sb, sab, h * sab]
    return x if c.order == 3 else x[:6]


def node_fwd64(c, use_scale=True, use_bias=True, w_block_of=W_BLOCK_OF, bias_scale_twice=False):
    """out[v] = out_scale[v] (sum_xb W_block(type, xb) X_xb[v] + degree[v] bias).  (``w_block_of`` / ``bias_scale_twice``: the mutations of the host test.)"""
    d, tb = c.dim, c.type_begin
    out = torch.zeros(c.n, d, dtype=torch.float64, device=c.h.device)
    mag = torch.zeros_like(out)
    for t in range(3):
        lo, hi = tb[t], tb[t + 1]
        for xb, (x, xa) in enumerate(zip(x_blocks(c), x_blocks(c, True))):
            wb = c.w[:, w_block_of[t][xb] * d:(w_block_of[t][xb] + 1) * d]
            out[lo:hi] += x[lo:hi] @ wb.T
            mag[lo:hi] += xa[lo:hi] @ wb.abs().T
    if use_bias:
        bias = c.degree[:, None] * c.bias[None, :]
        out, mag = out + (bias * c.scale[:, None] if bias_scale_twice else bias), mag + bias.abs()
    if use_scale:
        out, mag = out * c.scale[:, None], mag * c.scale[:, None]
    return out, mag


def node_weight64(c, use_scale=True):
    """dw[:, (3 + b) d ...] = sum over the nodes of (dy_scale[v] dy[v]) x X_block[v]^T, the X blocks h S_a, h S_b, S_ab (, h S_ab) routed by node type."""
    d, tb = c.dim, c.type_begin
    nb = product_blocks(c.order)
    dw = torch.zeros(d, nb * d, dtype=torch.float64, device=c.h.device)
    mag = torch.zeros_like(dw)
    dy = c.dy * c.scale[:, None] if use_scale else c.dy
    x, xa = x_blocks(c), x_blocks(c, True)
    for t in range(3):
        lo, hi = tb[t], tb[t + 1]
        for xb in PRODUCT_X[:nb]:
            b = W_BLOCK_OF[t][xb] - 3
            dw[:, b * d:(b + 1) * d] += _tn(dy[lo:hi], x[xb][lo:hi])
            mag[:, b * d:(b + 1) * d] += _tn(dy[lo:hi].abs(), xa[xb][lo:hi])
    return dw, mag


# ---- the node-level linear maps ----
class LinearCase:
    """x, g [N, d], w [d, 3 d] (typed) or [d, d], bias [d] (typed: the users' only), an integer ``prefill`` for ``dx_accumulate``."""

    def __init__(self, type_begin, dim, typed, rng, m=4, row_exp=None, zero_rows=None):
        n = type_begin[3]
        self.type_begin, self.dim, self.typed, self.n = tuple(type_begin), dim, typed, n
        self.x, self.g, self.prefill = ints(rng, (n, dim), m), ints(rng, (n, dim), m), ints(rng, (n, dim), 8)
        self.w, self.bias = ints(rng, (dim, 3 * dim if typed else dim), m), ints(rng, (dim,), m)
        if row_exp is not None:
            self.x = self.x * torch.from_numpy(np.ldexp(1.0, row_exp[0]))[:, None]
            self.g = self.g * torch.from_numpy(np.ldexp(1.0, row_exp[1]))[:, None]
        if zero_rows is not None:
            self.x[torch.from_numpy(zero_rows[0])] = 0
            self.g[torch.from_numpy(zero_rows[1])] = 0
        self.stride, self.mask = (dim, 0b001) if typed else (0, 0b111)


def linear64(c):
    """``dict(out, dx, dw, db)`` and magnitudes: out = x W_t^T + b, dx = g W_t, dW_t = g_t^T x_t, db = column sums of g over the rows that have the bias."""
    d, tb = c.dim, c.type_begin
    out, dx = torch.zeros(c.n, d, dtype=torch.float64), torch.zeros(c.n, d, dtype=torch.float64)
    out_mag, dx_mag, dw, dw_mag = torch.zeros_like(out), torch.zeros_like(out), torch.zeros_like(c.w), torch.zeros_like(c.w)
    for t in range(3):
        lo, hi = tb[t], tb[t + 1]
        cols = slice(t * d, (t + 1) * d) if c.typed else slice(0, d)
        wt = c.w[:, cols]
        has_bias = t == 0 or not c.typed
        out[lo:hi] = c.x[lo:hi] @ wt.T + (c.bias if has_bias else 0)
        out_mag[lo:hi] = c.x[lo:hi].abs() @ wt.abs().T + (c.bias.abs() if has_bias else 0)
        dx[lo:hi], dx_mag[lo:hi] = c.g[lo:hi] @ wt, c.g[lo:hi].abs() @ wt.abs()
        dw[:, cols] += c.g[lo:hi].T @ c.x[lo:hi]
        dw_mag[:, cols] += c.g[lo:hi].abs().T @ c.x[lo:hi].abs()
    rows = slice(0, tb[1]) if c.typed else slice(0, c.n)
    return dict(out=out, out_mag=out_mag, dx=dx, dx_mag=dx_mag, dw=dw, dw_mag=dw_mag, db=c.g[rows].sum(0), db_mag=c.g[rows].abs().sum(0))


def rising_exponents(n, tile, top, place):
    """Per-row exponents 0 ... ``top`` rising along the rows (the running scale of the weight-gradient kernels is raised again and again), the largest row placed
    'last' (last row of the last tile), 'first_of_tile' (first row of the last tile) - ``n`` chosen by the caller so that 'alone' makes it the only row of a partial
    last tile."""
    e = (np.arange(n) * (top + 1) // max(n, 1)).astype(np.int64)
    e = np.minimum(e, top - 1)
    last_tile = (n - 1) // tile * tile
    e[{'last': n - 1, 'first_of_tile': last_tile, 'alone': n - 1}[place]] = top
    return e


# =============================================================================================
# verdicts
# =============================================================================================
def ensure_exact(mag, unit=1.0, what=''):
    """The cap of an exact case, in int64, over every output element: ``sum |terms|`` in units of ``unit`` (the smallest power of two any term is a multiple of)
    is an integer below 2^24.  Raises: a case beyond the cap is a broken case."""
    units = mag.double() / unit
    as_int = units.round().to(torch.int64)
    if not bool((as_int.double() == units).all()):
        raise ValueError(f'{what}: a term is not a multiple of the unit {unit}')
    worst = int(as_int.max()) if as_int.numel() else 0
    if worst >= CAP:
        raise ValueError(f'{what}: sum |terms| reaches {worst} >= 2^24 units - the case is not exact in float32')
    return worst


def assert_equal(got, want64, what):
    """``torch.equal`` against the float64 reference cast to float32, with the first differing element in the message."""
    want = want64.float().to(got.device)
    if torch.equal(got, want):
        return
    assert got.shape == want.shape, f'{what}: shape {tuple(got.shape)} != {tuple(want.shape)}'
    bad = (got != want) | torch.isnan(got)
    idx = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: got {float(got[idx])}, want {float(want[idx])}')


# Roundings besides the K - 1 additions, per output element - the ``c`` of the bound.  To first order an addend passes through at most K - 1 additions whatever the
# order (tiles, ranges, slabs, boundary entries: all additions), and through these multiplications:
ROUNDINGS = {
    'fwd': 3,          # h h (and (h h) h at order 3): 2, the product with w: 1; the three first-order rows are addends
    'gathered_dout': 1,  # dy_scale dy; three addends
    'members': 3,      # dout w: 1, the product of the other members' values: 1, times dz: 1
    'dh': 3,           # the same addends, summed over the user's run as well
    'dw': 3,           # h h (h): 2, dout z: 1
    'node_fwd': 3,     # deg h or h S: 1, the product with w (deg bias for the bias): 1, out_scale: 1
    'node_weight': 3,  # dy_scale dy: 1, h S: 1, their product: 1
}
GATHERED_EXTRA = 3     # a cotangent formed on chip carries (3 - 1) + 1 roundings of its own into everything computed from it


def float_bound(kind, n_addends, mag, arithmetic, gathered=False):
    """``((K + c) 2^-24 + L) sum |terms|``: K addends, c other roundings (above), L the split's loss per product (0 for the fp32-MFMA, narrow and scalar kernels)."""
    c = ROUNDINGS[kind] + (GATHERED_EXTRA if gathered else 0)
    return ((n_addends + c) * U + (SPLIT_LOSS if arithmetic == 'split' else 0.0)) * mag


def assert_within(got, want64, bound, what):
    """Per element; returns the worst ``error / bound`` (elements whose bound is 0 must be equal)."""
    want, bound = want64.to(got.device), bound.to(got.device)
    assert bool(torch.isfinite(got).all()), f'{what}: a value is not finite'
    err = (got.double() - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        idx = tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError(f'{what}: error / bound = {worst:.3g} at {idx}: got {float(got[idx])}, want {float(want[idx])}, bound {float(bound[idx]):.3g}')
    return worst


# =============================================================================================
# numpy emulation: the operand split, the kept partial products, float32 accumulation in a fixed order.  ``mutation`` names ONE way of being wrong.
# =============================================================================================
MUTATIONS = ('drop_edge_of_last_partial_tile', 'count_padded_row', 'wrong_weight_block', 'drop_boundary_entry', 'close_run_early', 'omit_hi_lo',
             'no_rescale', 'bias_scaled_twice', 'fp16_partial')


def _f32(x):
    return np.asarray(x, np.float32)


def emu_dot(a, b, arithmetic, mutation=None, k_step=32):
    """Rows of ``a`` [n, K] against rows of ``b`` [m, K] -> [n, m] float32: operands split per row (two fp16 terms under the row's power of two; three bf16 terms;
    none), the kept partial products of ``k_step`` contraction values formed exactly (float64) and added to a float32 accumulator step by step, the row scales
    taken out at the end (powers of two: exact).  'omit_hi_lo': the two-fp16 product without its hi lo term; 'fp16_partial': every step's partial kept in fp16."""
    a, b = _f32(a), _f32(b)
    n, m, kk = a.shape[0], b.shape[0], a.shape[1]
    if arithmetic == 'two_fp16':
        sa = SE.scale_up_for(np.abs(a).max(1, initial=0.0)) if n else np.ones(0)
        sb = SE.scale_up_for(np.abs(b).max(1, initial=0.0)) if m else np.ones(0)
        parts_a = SE.split_two_fp16((a.astype(np.float64) * sa[:, None]).astype(np.float32))
        parts_b = SE.split_two_fp16((b.astype(np.float64) * sb[:, None]).astype(np.float32))
        kept = [(0, 1), (1, 0), (0, 0)]
        if mutation == 'omit_hi_lo':
            kept = [(1, 0), (0, 0)]
    elif arithmetic == 'three_bf16':
        sa, sb = np.ones(n), np.ones(m)
        parts_a, parts_b = SE.split_three_bf16(a), SE.split_three_bf16(b)
        kept = [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)]
    else:
        sa, sb = np.ones(n), np.ones(m)
        parts_a, parts_b = (a.astype(np.float64),), (b.astype(np.float64),)
        kept = [(0, 0)]
    acc = np.zeros((n, m), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        return _emu_accumulate(acc, parts_a, parts_b, kept, kk, k_step, mutation, sa, sb)


def _emu_accumulate(acc, parts_a, parts_b, kept, kk, k_step, mutation, sa, sb):
    for k0 in range(0, kk, k_step):
        for i, j in kept:
            part = parts_a[i][:, k0:k0 + k_step] @ parts_b[j][:, k0:k0 + k_step].T
            if mutation == 'fp16_partial':
                with np.errstate(over='ignore'):
                    part = part.astype(np.float16).astype(np.float64)
            acc = (acc.astype(np.float64) + part).astype(np.float32)
    return (acc.astype(np.float64) / sa[:, None] / sb[None, :]).astype(np.float32)


def _np(t):
    return t.cpu().numpy()


def emu_fwd(c, arithmetic, mutation=None, te=16):
    """The hyperedge forward: per tile, the products formed in float32, the four blocks contracted one after the other onto one accumulator, the first-order rows
    added u, q, i.  'drop_edge_of_last_partial_tile': the last hyperedge of a partial last tile keeps its prefill (NaN)."""
    i3, h, p = _np(c.i3).astype(np.int64), _f32(_np(c.h)), _f32(_np(c.p))
    blocks = [_f32(_np(wb)) for wb in _blocks(c)]
    e = len(i3)
    out = np.full((e, c.dim), np.nan, np.float32)
    for e0 in range(0, e, te):
        e1 = min(e0 + te, e)
        if mutation == 'drop_edge_of_last_partial_tile' and e1 == e and (e1 - e0) < te:
            e1 -= 1
        hu, hq, hi = (h[i3[e0:e1, s]] for s in range(3))
        z = [hu * hq, hq * hi, hi * hu] + ([(hu * hq) * hi] if c.order == 3 else [])
        acc = np.zeros((e1 - e0, c.dim), np.float32)
        for zb, wb in zip(z, blocks):
            acc = acc + emu_dot(zb, wb, arithmetic, mutation)
        out[e0:e1] = ((p[i3[e0:e1, 0]] + p[i3[e0:e1, 1]]) + p[i3[e0:e1, 2]]) + acc
    return out


def emu_members(c, arithmetic, mutation=None, dout=None):
    """[E, 3, d] member gradients: dz_b = dout W_b by ``emu_dot``, then the product rule in float32."""
    i3, h = _np(c.i3).astype(np.int64), _f32(_np(c.h))
    dout = _f32(_np(c.dout)) if dout is None else dout
    hu, hq, hi = (h[i3[:, s]] for s in range(3))
    dz = [emu_dot(dout, _f32(_np(wb)).T.copy(), arithmetic, mutation) for wb in _blocks(c)]
    gu, gq, gi = dz[0] * hq + dz[2] * hi, dz[0] * hu + dz[1] * hi, dz[1] * hq + dz[2] * hu
    if c.order == 3:
        gu, gq, gi = gu + dz[3] * (hq * hi), gq + dz[3] * (hu * hi), gi + dz[3] * (hu * hq)
    return np.stack([gu, gq, gi], 1).astype(np.float32)


def emu_user_reduce(gu, users, n_users, kernel, mutation=None, prefill=np.nan):
    """``dh`` [n_users, d] from the user-slot gradients as the user-reduced kernels form it: contiguous tile ranges; inside a range the rows of a run are added in
    hyperedge order; a run that neither opens nor closes its range is stored at once; the range's first run goes to boundary entry 2 r, its last open run - unless
    the range is one run - to entry 2 r + 1; the boundary pass adds the consecutive entries of one user in table order and stores.  Rows of users without
    hyperedges keep ``prefill``.  'drop_boundary_entry': the second entry of the first run that crosses ranges is lost; 'close_run_early': the boundary pass stops
    after two entries."""
    e, d = gu.shape
    te, per = kernel.te, kernel.per(e)
    dh = np.full((n_users, d), prefill, np.float32)
    table = []                                                           # (user, value) in table order
    for r in range(kernel.used_ranges(e)):
        b, end = r * per * te, min((r + 1) * per * te, e)
        starts = [b] + [k for k in range(b + 1, end) if users[k] != users[k - 1]]
        for n, s in enumerate(starts):
            stop = starts[n + 1] if n + 1 < len(starts) else end
            acc = np.zeros(d, np.float32)
            for k in range(s, stop):
                acc = acc + gu[k]
            if n == 0 or n == len(starts) - 1:
                table.append((int(users[s]), acc))
            else:
                dh[users[s]] = acc
    dropped = False
    k = 0
    while k < len(table):
        user, acc = table[k]
        n = 1
        while k + n < len(table) and table[k + n][0] == user:
            if mutation == 'close_run_early' and n == 2:
                break
            if mutation == 'drop_boundary_entry' and not dropped:
                dropped = True
            else:
                acc = acc + table[k + n][1]
            n += 1
        while k + n < len(table) and table[k + n][0] == user:            # (entries a run closed early leaves behind)
            n += 1
        dh[user] = acc
        k += n
    return dh


def emu_weight(dout, z, kernel, arithmetic, mutation=None):
    """One block of the weight gradient, dw[c, j] = sum_e dout[e, c] z[e, j]: per tile the contraction over the tile's rows (``emu_dot`` with the rows as the
    contraction index; under the two-fp16 split every column of the tile under a power of two of its own - the kernels scale the ROWS and carry a running scale
    instead, ``emu_running_scale_weight`` - which loses the same 2^-21 per product), per range a slab that adds its tiles in order, the slabs added in range order.  'count_padded_row': the rows past the end of a partial last
    tile repeat the last row instead of being zero; 'drop_edge_of_last_partial_tile'."""
    e, d = dout.shape
    te = kernel.te
    tiles = -(-e // te)
    slabs = np.zeros((kernel.ranges, d, z.shape[1]), np.float32)
    per = kernel.per(e)
    for t in range(tiles):
        e0, e1 = t * te, min((t + 1) * te, e)
        a, b = dout[e0:e1], z[e0:e1]
        if e1 - e0 < te:
            if mutation == 'count_padded_row':
                a, b = np.concatenate([a, a[-1:]]), np.concatenate([b, b[-1:]])
            if mutation == 'drop_edge_of_last_partial_tile':
                a, b = a[:-1], b[:-1]
        r = t // per if kernel.deal == 'contiguous' else t % kernel.ranges
        slabs[r] = slabs[r] + emu_dot(a.T.copy(), b.T.copy(), arithmetic, mutation, k_step=min(te, 32))
    acc = np.zeros_like(slabs[0])
    for r in range(kernel.ranges):
        acc = acc + slabs[r]
    return acc


def emu_node_fwd(c, arithmetic, mutation=None):
    """The node-level forward per node type: the X blocks formed in float32, contracted block after block onto one accumulator, ``degree bias`` added, the sum
    scaled.  'wrong_weight_block': the items' h S_a block meets the block of the users' table; 'bias_scaled_twice'."""
    d, tb = c.dim, c.type_begin
    h, s, deg, scale = _f32(_np(c.h)), _f32(_np(c.sums)), _f32(_np(c.degree)), _f32(_np(c.scale))
    w, bias = _f32(_np(c.w)), _f32(_np(c.bias))
    sa, sb, sab = s[:, :d], s[:, d:2 * d], s[:, 2 * d:]
    x = [deg[:, None] * h, sa, h * sa, sb, h * sb, sab, h * sab][:7 if c.order == 3 else 6]
    out = np.zeros((c.n, d), np.float32)
    for t in range(3):
        lo, hi = tb[t], tb[t + 1]
        table = W_BLOCK_OF[0] if (mutation == 'wrong_weight_block' and t == 2) else W_BLOCK_OF[t]
        for xb, xv in enumerate(x):
            out[lo:hi] = out[lo:hi] + emu_dot(xv[lo:hi], w[:, table[xb] * d:(table[xb] + 1) * d], arithmetic, mutation)
    db = deg[:, None] * bias[None, :]
    if mutation == 'bias_scaled_twice':
        db = db * scale[:, None]
    return (out + db) * scale[:, None]


def emu_running_scale_weight(a, b, tile, mutation=None):
    """dW = a^T b over the rows (the contraction index) as the split weight-gradient kernels keep it: every row pair is brought to a common magnitude by a power of
    two of its own, so a tile's products carry the tile's scale; the accumulators carry a running power-of-two scale, the largest so far, and are rescaled when a
    later tile raises it; the scale is taken out at the end.  'no_rescale': the accumulators are left as they are when the scale rises."""
    a, b = _f32(a), _f32(b)
    acc = np.zeros((a.shape[1], b.shape[1]), np.float32)
    running = None
    for r0 in range(0, a.shape[0], tile):
        at, bt = a[r0:r0 + tile], b[r0:r0 + tile]
        top = float(np.abs(at).max(initial=0.0) * np.abs(bt).max(initial=0.0))
        if top == 0.0:
            continue
        scale = 2.0 ** np.floor(np.log2(top))
        if running is None:
            running = scale
        elif scale > running:
            if mutation != 'no_rescale':
                acc = (acc.astype(np.float64) * (running / scale)).astype(np.float32)
            running = scale
        part = emu_dot(at.T.copy(), bt.T.copy(), 'two_fp16', mutation, k_step=min(tile, 32))
        acc = (acc.astype(np.float64) + part.astype(np.float64) / running).astype(np.float32)
    return acc if running is None else (acc.astype(np.float64) * running).astype(np.float32)
