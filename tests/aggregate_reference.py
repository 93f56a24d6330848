"""Case generators and references for the aggregation kernels of ``ihgnn_amd/csrc/aggregate.hip`` - test infrastructure (CPU, numpy / torch only).

Two kinds of input, two kinds of verdict:

* EXACT cases.  Features are integers in [-8, 8]; ``node_scale``, ``src_scale``, ``out_scale``, ``alpha`` and ``edge_scale`` are powers of two in {1/2, 1, 2, 4}
  (``out_scale`` may also be 0 in divide mode); ``entry_scale``, ``self_weight`` and ``pair_weight`` are integers in [1, 4]; the bias and an accumulated-onto output
  are integers.  Every term of every sum is then a multiple of ``2^-QUANTUM_BITS`` (one halving by a source scale, up to two more by the output scale: 3 bits), and
  ``assert_exact_condition`` checks, in int64 units of that quantum, that ``sum |terms|`` of every output element - before and after the output scale - stays below
  2^24.  Under that condition every partial sum taken in any order, fused or not, is a float32 value: the kernel's result must EQUAL the float64 reference
  (``torch.equal``), no tolerance.  This is what catches a dropped, doubled, misplaced or mis-weighted entry.
* FLOAT cases.  ``randn`` features, scales in [0.5, 1.5).  Per element ``|got - want| <= (n + 4) 2^-24 sum |terms|`` with ``n`` the element's number of addends and
  ``sum |terms|`` the float64 sum of the magnitudes of its scaled terms: the first-order bound for n terms summed in ANY order (an addend passes through at most n - 1
  additions), one rounding for each product, one for a product of two weights, two for the output scale and the bias / accumulated value.  It does not depend on the
  kernel's order of summation; its job is to catch a loss of precision CLASS (an accumulator or a partial kept in 16 bits).  ``tests/test_aggregate_host.py`` holds a
  sequential float32 sum in numpy to the same bound, so a failing kernel case is a wrong kernel and not a tight bar.

The references take torch tensors on any device (the second-grid-stride-trip cases build them on the GPU) and compute in float64 with ``index_add_``: on exact inputs
every float64 partial sum is exact as well, whatever order a device's atomics take.  ``*_loops`` are the same sums as plain Python loops, for the host test.
"""
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24                             # float32 unit roundoff
EXACT_LIMIT = 1 << 24
QUANTUM_BITS = 3

# --- the test's own table of the kernels' launch geometry.  These mirror aggregate.hip as it is today (group_lanes, the K5 launch table, IHG_K5_UPLANES, agg_grid,
# heavy_finish_kernel's FLY = 16 / 4 loops, accumulate_list's UNR = 8 / 16).  If the kernels' constants change the cases stay valid: they only become less pointed.
WAVE = 64
BLOCK_THREADS = 256
MAX_WAVES = 256 * 64 * (BLOCK_THREADS // WAVE)              # agg_grid: 16,384 workgroups of four waves; beyond that a wave takes a second trip
K5_U = {4: 1, 8: 2, 16: 3, 32: 3, 64: 3}                    # consecutive hyperedges per lane group
K5_UPLANES = 4
FINISH_DEPTHS = (16, 4)                                     # partials in flight per lane group in the split-row finish: a 16-deep loop, a 4-deep loop, a tail
GATHER_DEPTHS = (8, 16)                                     # row gathers in flight per lane in K7 / the pair sums

WIDE_DIMS = (16, 32, 64, 128, 256, 320, 8)                  # 16-byte path: G = 4, 8, 16, 32, 64, 64 (two column passes), 4 (idle lanes)
NARROW_DIMS = (3, 7, 13, 30, 50, 100)                       # 4-byte path: G = 4, 8, 16, 32, 64, 64 (two passes; 100 is on this path in an unaligned geometry)
ALL_DIMS = WIDE_DIMS + NARROW_DIMS
GEOMETRIES = ('a', 'b', 'c', 'd')


def geometry_of(dim, geometry):
    """``(ld, col0)`` of a ``[rows, dim]`` view into a ``[rows, ld]`` buffer: (a) contiguous, 16-byte aligned; (b) a column slice of a wider matrix, ``ld % 4 == 0``,
    16-byte aligned; (c) ``ld`` not a multiple of 4; (d) the base pointer one float past a 16-byte boundary (``ld % 4 == 0``)."""
    up = (dim + 3) // 4 * 4
    return {'a': (dim, 0), 'b': (up + 8, 4), 'c': (up + 5, 0), 'd': (up + 8, 1)}[geometry]


def vec_of(dim, geometry):
    """Floats per lane and load: 4 when the width and the geometry allow 16-byte accesses, else 1."""
    return 4 if dim % 4 == 0 and geometry in ('a', 'b') else 1


def group_lanes(dim, vec):
    """Lanes that own one row: the smallest power of two >= dim / vec, clamped to [4, 64]."""
    g = 4
    while g < dim // vec and g < WAVE:
        g *= 2
    return g


def finish_groups(g):
    return BLOCK_THREADS // g


def k5_epw(g):
    """Hyperedges a wave takes per trip of K5's loop."""
    return (WAVE // g) * K5_U[g]


def k5_edge_counts(g):
    epw = k5_epw(g)
    return sorted({0, 1, epw - 1, epw, epw + 1, 3 * epw + 2})


def finish_trips(segments, groups):
    """The test's model of the split-row finish: for every lane group of the workgroup, how many trips it takes through the 16-deep loop, the 4-deep loop and the
    tail when a row has ``segments`` partials.  ``[(t16, t4, tail)] * groups``."""
    out = []
    for grp in range(groups):
        s, trips = grp, []
        for depth in FINISH_DEPTHS + (1,):
            t = 0
            while s + (depth - 1) * groups < segments:
                s += depth * groups
                t += 1
            trips.append(t)
        out.append(tuple(trips))
    return out


def ladder_segment_counts(g):
    """Segment counts of the split rows of one ladder: around one, four, sixteen partials per lane group, one with a 16-deep trip followed by a 4-deep one, one with
    two 16-deep trips.  The largest is 33 x 64 + 3 = 2,115 segments (4,230 entries at two entries per segment)."""
    gr = finish_groups(g)
    return [gr - 1, gr, gr + 1, 4 * gr - 1, 4 * gr, 4 * gr + 1, 16 * gr - 1, 16 * gr, 16 * gr + 1, 21 * gr + 2, 33 * gr + 3]


def ladder_lengths(g, rng):
    """Row lengths of a ladder CSR for ``heavy_threshold = 2, heavy_chunk = 2`` (a row of 2 k entries: k segments): the ladder's rows, one odd row (11 entries: the last
    of its six segments holds one), light rows of 0, 1 and 2 entries, shuffled."""
    lengths = [2 * k for k in ladder_segment_counts(g)] + [11] + [0, 1, 2, 2, 1, 0, 2]
    return [int(x) for x in rng.permutation(lengths)]


def pair_ladder_lengths(g, rng):
    """The ladder for the pair sums (ids per row; one pair per segment at threshold 2, chunk 2): its rows, and light rows of no pair and one pair."""
    lengths = [2 * k for k in ladder_segment_counts(g)] + [0, 2, 2, 0, 2]
    return [int(x) for x in rng.permutation(lengths)]


def light_lengths(g, rng):
    """Row lengths at the lane-group and unroll boundaries, every length twice, shuffled; in front a 200-entry row between empty ones (they share a wave at G < 64)."""
    base = sorted({0, 1, g - 1, g, g + 1, 7, 8, 9, 15, 16, 17, 2 * g + 3, 200})
    return [0, 200, 0, 0] + [int(x) for x in rng.permutation(base + base)]


def csr_from_lengths(lengths, n_src, rng):
    """``(ptr, ids)`` int32 numpy arrays: rows of the given lengths with ids drawn uniformly from ``[0, n_src)``."""
    ptr = np.zeros(len(lengths) + 1, np.int32)
    np.cumsum(np.asarray(lengths, np.int64), out=ptr[1:])
    return ptr, rng.integers(0, n_src, int(ptr[-1])).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------
def features(rng, rows, dim, exact):
    x = rng.integers(-8, 9, (rows, dim)) if exact else rng.standard_normal((rows, dim))
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


def scales(rng, n, exact, zeros=False):
    """Powers of two in {1/2, 1, 2, 4} (``zeros``: about one in six is 0 - divide mode) or uniform in [0.5, 1.5)."""
    x = rng.choice(np.array([0.5, 1.0, 2.0, 4.0]), n) if exact else rng.random(n) + 0.5
    if zeros and n:
        x[rng.random(n) < 1 / 6] = 0.0
        x[0] = 0.0
    return torch.from_numpy(x.astype(np.float32))


def weights(rng, n, exact):
    """``entry_scale``, ``self_weight``, ``pair_weight``: integers in [1, 4], or uniform in [0.5, 1.5)."""
    x = rng.integers(1, 5, n) if exact else rng.random(n) + 0.5
    return torch.from_numpy(x.astype(np.float32))


def integers(rng, shape):
    """A bias or an accumulated-onto output: integers in [-8, 8] (used for the float cases too - any float32 values would do)."""
    return torch.from_numpy(rng.integers(-8, 9, shape).astype(np.float32))


def reuse_i3(n_nodes, n_blocks=24):
    """Member ids whose column 0 runs in blocks of equal ids of lengths 1, 2, 3, 4, 7 (K5's "same user as the previous hyperedge" reuse fires inside a lane group and
    must stop at its boundary); columns 1 and 2 differ inside a block; neighbouring blocks differ in column 0; the last hyperedge's three ids are equal."""
    rows, k = [], 0
    for b in range(n_blocks):
        for _ in range((1, 2, 3, 4, 7)[b % 5]):
            rows.append(((7 * b + 3) % n_nodes, (5 * k + 1) % n_nodes, (11 * k + 2) % n_nodes))
            k += 1
    rows.append((9 % n_nodes,) * 3)
    return torch.tensor(rows, dtype=torch.int32)


def k5_case(dim, i3, on, exact, rng, n_nodes=41):
    """``(src, keyword arguments of edge_gather_reference)``: ``on`` gives a ``node_scale`` per node, an integer ``bias``, ``alpha != 1`` and an ``edge_scale``."""
    src = features(rng, n_nodes, dim, exact)
    if not on:
        return src, {}
    return src, dict(node_scale=scales(rng, n_nodes, exact), bias=integers(rng, dim), alpha=0.5 if exact else 0.37, edge_scale=scales(rng, i3.shape[0], exact))


K7_ALL_ON = ('src_scale', 'entry_scale', 'mode2', 'self_weight', 'accumulate', 'src_mask')


def k7_case(ptr, ids, n_src, dim, options, exact, rng, listed=0.5, dead_row=None):
    """``(src, keyword arguments of segment_sum_reference)`` for a CSR ``ptr, ids`` (numpy) over ``n_src >= n_rows`` source rows.  ``options``: any of ``src_scale``,
    ``entry_scale``, ``mode1`` (multiply), ``mode2`` (divide; some scales 0), ``self_weight``, ``accumulate`` (an integer ``acc_in``), ``src_mask`` (a share ``listed``
    of the source rows has a 1; ``dead_row``: every id of that row is unlisted)."""
    n_rows = len(ptr) - 1
    assert n_src >= n_rows
    src = features(rng, n_src, dim, exact)
    kw = {}
    if 'src_scale' in options:
        kw['src_scale'] = scales(rng, n_src, exact)
    if 'entry_scale' in options:
        kw['entry_scale'] = weights(rng, len(ids), exact)
    for mode in (1, 2):
        if f'mode{mode}' in options:
            kw.update(mode=mode, out_scale=scales(rng, n_rows, exact, zeros=mode == 2))
    if 'self_weight' in options:
        kw['self_weight'] = weights(rng, n_rows, exact)
    if 'accumulate' in options:
        kw['acc_in'] = integers(rng, (n_rows, dim))
    if 'src_mask' in options:
        mask = (rng.random(n_src) < listed).astype(np.uint8)
        if len(ids):
            mask[ids[len(ids) // 2]] = 1
        if dead_row is not None:
            mask[ids[ptr[dead_row]:ptr[dead_row + 1]]] = 0
        kw['src_mask'] = torch.from_numpy(mask)
    return src, kw


# ---------------------------------------------------------------------------------------------
# references (float64, any device)
# ---------------------------------------------------------------------------------------------
# want: the result; mag: sum |terms| of each element of the result (the float bound's scale); peak: the larger of mag and the same sum before the output scale (the
# exact condition: every intermediate must be a float32 value too); n: addends per element (a [rows] or [rows, 1] tensor, or a number)
Ref = namedtuple('Ref', 'want mag peak n')


def _f64(t):
    return None if t is None else t.double()


def edge_gather_reference(src, i3, node_scale=None, bias=None, alpha=1.0, edge_scale=None):
    """K5: ``out[e] = alpha edge_scale[e] sum_m node_scale[i3[e, m]] src[i3[e, m]] + bias``."""
    src, i3 = src.double(), i3.long()
    rows = src[i3]                                                                       # [E, 3, d]
    w = node_scale.double()[i3] if node_scale is not None else torch.ones(i3.shape, dtype=torch.float64, device=src.device)
    inner = (rows * w[:, :, None]).sum(1)
    inner_mag = (rows.abs() * w.abs()[:, :, None]).sum(1)
    f = torch.full((i3.shape[0],), float(np.float32(alpha)), dtype=torch.float64, device=src.device)
    if edge_scale is not None:
        f = f * edge_scale.double()
    want, mag, n = inner * f[:, None], inner_mag * f.abs()[:, None], 3
    if bias is not None:
        want, mag, n = want + bias.double(), mag + bias.double().abs(), 4
    return Ref(want, mag, torch.maximum(mag, inner_mag), n)


def segment_sum_reference(src, ptr, ids, src_scale=None, entry_scale=None, out_scale=None, mode=0, self_weight=None, src_mask=None, acc_in=None):
    """K7: ``out[r] = op(out_scale[r]) (sum_{k in row r} src_scale[ids[k]] entry_scale[k] src[ids[k]] + self_weight[r] src_scale[r] src[r]) (+ acc_in[r])``; ``op``:
    mode 0 none, 1 multiply, 2 divide unless the scale is 0.  ``src_mask``: source rows with a 0 are taken as zero WHATEVER they hold (ids and the row's own term)."""
    src64, ptr, ids = src.double(), ptr.long(), ids.long()
    dev, n_rows, dim = src.device, ptr.shape[0] - 1, src.shape[1]
    row_of = torch.repeat_interleave(torch.arange(n_rows, device=dev), ptr[1:] - ptr[:-1])
    w = torch.ones(ids.shape[0], dtype=torch.float64, device=dev)
    if src_scale is not None:
        w = w * src_scale.double()[ids]
    if entry_scale is not None:
        w = w * entry_scale.double()
    live = src_mask[ids] != 0 if src_mask is not None else torch.ones(ids.shape[0], dtype=torch.bool, device=dev)
    terms = torch.where(live[:, None], src64[ids] * w[:, None], torch.zeros((), dtype=torch.float64, device=dev))
    inner = torch.zeros(n_rows, dim, dtype=torch.float64, device=dev).index_add_(0, row_of, terms)
    inner_mag = torch.zeros(n_rows, dim, dtype=torch.float64, device=dev).index_add_(0, row_of, terms.abs())
    n = torch.zeros(n_rows, dtype=torch.float64, device=dev).index_add_(0, row_of, live.double())
    if self_weight is not None:
        own = src_mask[:n_rows] != 0 if src_mask is not None else torch.ones(n_rows, dtype=torch.bool, device=dev)
        sw = self_weight.double() * (src_scale.double()[:n_rows] if src_scale is not None else 1.0)
        own_terms = torch.where(own[:, None], src64[:n_rows] * sw[:, None], torch.zeros((), dtype=torch.float64, device=dev))
        inner, inner_mag, n = inner + own_terms, inner_mag + own_terms.abs(), n + own.double()
    f = torch.ones(n_rows, dtype=torch.float64, device=dev)
    if mode == 1:
        f = out_scale.double()
    elif mode == 2:
        s = out_scale.double()
        f = torch.where(s != 0, 1.0 / torch.where(s != 0, s, torch.ones_like(s)), torch.ones_like(s))
    want, mag = inner * f[:, None], inner_mag * f.abs()[:, None]
    if acc_in is not None:
        want, mag, n = want + acc_in.double(), mag + acc_in.double().abs(), n + 1
    return Ref(want, mag, torch.maximum(mag, inner_mag), n[:, None])


def pair_sums_reference(h, ptr, ids, pair_weight=None):
    """``[rows, 3 d]``: ``S_a | S_b | S_ab`` over the id pairs ``(ids[2 p], ids[2 p + 1])`` of every row (``ptr`` counts ids: even offsets), pair ``p`` taken
    ``pair_weight[p]`` times."""
    h64, ptr, ids = h.double(), ptr.long(), ids.long()
    dev, n_rows, dim = h.device, ptr.shape[0] - 1, h.shape[1]
    pairs = (ptr[1:] - ptr[:-1]) // 2
    row_of = torch.repeat_interleave(torch.arange(n_rows, device=dev), pairs)
    a, b = h64[ids[0::2]], h64[ids[1::2]]
    w = pair_weight.double()[:, None] if pair_weight is not None else torch.ones(a.shape[0], 1, dtype=torch.float64, device=dev)
    terms = torch.cat([a * w, b * w, a * b * w], 1)
    want = torch.zeros(n_rows, 3 * dim, dtype=torch.float64, device=dev).index_add_(0, row_of, terms)
    mag = torch.zeros(n_rows, 3 * dim, dtype=torch.float64, device=dev).index_add_(0, row_of, terms.abs())
    return Ref(want, mag, mag, pairs.double()[:, None])


def bag_mean_backward_reference(dout, ptr, words, table_rows):
    """``dtable[w] = sum over the occurrences of word w in a bag b of dout[b] / len(b)`` - from the bags themselves, not from the library's transposed list."""
    ptr, words = ptr.long(), words.long()
    n_bags, lens = ptr.shape[0] - 1, (ptr[1:] - ptr[:-1])
    bag_of = torch.repeat_interleave(torch.arange(n_bags), lens)
    inv = (1.0 / lens.double().clamp(min=1)).float().double()                            # the layout's float32 1 / len
    terms = dout.double()[bag_of] * inv[bag_of, None]
    want = torch.zeros(table_rows, dout.shape[1], dtype=torch.float64).index_add_(0, words, terms)
    mag = torch.zeros(table_rows, dout.shape[1], dtype=torch.float64).index_add_(0, words, terms.abs())
    n = torch.zeros(table_rows, dtype=torch.float64).index_add_(0, words, torch.ones(words.shape[0], dtype=torch.float64))
    return Ref(want, mag, mag, n[:, None])


# ---------------------------------------------------------------------------------------------
# the same sums as plain loops (host test, small cases)
# ---------------------------------------------------------------------------------------------
def edge_gather_loops(src, i3, node_scale=None, bias=None, alpha=1.0, edge_scale=None):
    dim = src.shape[1]
    src, i3 = src.double().tolist(), i3.tolist()
    ns = node_scale.double().tolist() if node_scale is not None else None
    out = []
    for e, members in enumerate(i3):
        row = []
        for c in range(dim):
            s = 0.0
            for v in members:
                s += (ns[v] if ns is not None else 1.0) * src[v][c]
            s *= float(np.float32(alpha)) * (float(edge_scale[e]) if edge_scale is not None else 1.0)
            row.append(s + (float(bias[c]) if bias is not None else 0.0))
        out.append(row)
    return torch.tensor(out, dtype=torch.float64).reshape(len(i3), dim)


def segment_sum_loops(src, ptr, ids, src_scale=None, entry_scale=None, out_scale=None, mode=0, self_weight=None, src_mask=None, acc_in=None):
    x, ptr, ids = src.double().tolist(), ptr.tolist(), ids.tolist()
    dim = src.shape[1]
    out = []
    for r in range(len(ptr) - 1):
        row = []
        for c in range(dim):
            s = 0.0
            for k in range(ptr[r], ptr[r + 1]):
                v = ids[k]
                if src_mask is not None and int(src_mask[v]) == 0:
                    continue
                s += (float(src_scale[v]) if src_scale is not None else 1.0) * (float(entry_scale[k]) if entry_scale is not None else 1.0) * x[v][c]
            if self_weight is not None and (src_mask is None or int(src_mask[r]) != 0):
                s += float(self_weight[r]) * (float(src_scale[r]) if src_scale is not None else 1.0) * x[r][c]
            if mode == 1:
                s *= float(out_scale[r])
            elif mode == 2 and float(out_scale[r]) != 0:
                s /= float(out_scale[r])
            row.append(s + (float(acc_in[r][c]) if acc_in is not None else 0.0))
        out.append(row)
    return torch.tensor(out, dtype=torch.float64).reshape(len(ptr) - 1, dim)


def pair_sums_loops(h, ptr, ids, pair_weight=None):
    x, ptr, ids = h.double().tolist(), ptr.tolist(), ids.tolist()
    dim = h.shape[1]
    out = []
    for r in range(len(ptr) - 1):
        sa, sb, sab = [0.0] * dim, [0.0] * dim, [0.0] * dim
        for k in range(ptr[r], ptr[r + 1], 2):
            m = float(pair_weight[k // 2]) if pair_weight is not None else 1.0
            for c in range(dim):
                sa[c] += m * x[ids[k]][c]
                sb[c] += m * x[ids[k + 1]][c]
                sab[c] += m * x[ids[k]][c] * x[ids[k + 1]][c]
        out.append(sa + sb + sab)
    return torch.tensor(out, dtype=torch.float64).reshape(len(ptr) - 1, 3 * dim)


# ---------------------------------------------------------------------------------------------
# verdicts
# ---------------------------------------------------------------------------------------------
def assert_exact_condition(ref, what='', bits=QUANTUM_BITS):
    """The condition on an exact case's INPUTS: in int64 units of ``2^-bits`` every element's ``sum |terms|`` (before and after the output scale) is an integer below
    2^24, and the reference itself is a whole number of units.  Returns the largest sum in units."""
    if ref.peak.numel() == 0:
        return 0
    units = ref.peak * float(1 << bits)
    as_int = units.round().to(torch.int64)
    assert bool((as_int.double() == units).all()), f'{what}: a term is not a multiple of 2^-{bits}'
    want_units = ref.want * float(1 << bits)
    assert bool((want_units == want_units.round()).all()), f'{what}: the reference is not a multiple of 2^-{bits}'
    worst = int(as_int.max())
    assert worst < EXACT_LIMIT, f'{what}: sum |terms| = {worst} x 2^-{bits} is not below 2^24: the case is not exact'
    return worst


def assert_exact(got, ref, what):
    """Bit for bit (as values: ``-0.0 == 0.0``): ``got`` (float32) equals the float64 reference."""
    want = ref.want.to(torch.float32)
    assert got.shape == want.shape, f'{what}: shape {tuple(got.shape)} for {tuple(want.shape)}'
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f'{what}: {bad.shape[0]} of {got.numel()} elements differ from the exact sum; first at {first}: got {float(got[first])!r}, '
                             f'want {float(want[first])!r}; rows {sorted({int(i) for i in bad[:64, 0]})[:16]}')


def float_bound(ref):
    n = ref.n if torch.is_tensor(ref.n) else float(ref.n)
    return (n + 4.0) * U * ref.mag


def assert_within_float_bound(got, ref, what):
    """Per element ``|got - want| <= (n + 4) 2^-24 sum |terms|``; an element without terms must be exactly 0.  Prints and returns the largest ``error / bound``."""
    err = (got.double() - ref.want).abs()
    bound = float_bound(ref)
    assert bool(torch.isfinite(got).all()), f'{what}: the result is not finite'
    assert bool((err[bound == 0] == 0).all()), f'{what}: an element without terms is not zero'
    ratio = err / torch.where(bound > 0, bound, torch.ones_like(bound))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f'aggregate float case {what}: worst error / bound = {worst:.4f}')
    if worst > 1.0:
        first = tuple(int(i) for i in torch.nonzero(ratio > 1.0)[0])
        raise AssertionError(f'{what}: element {first} is off by {float(err[first]):.3e}, bound {float(bound[first]):.3e} (n = {float(ref.n if not torch.is_tensor(ref.n) else ref.n[first[0]])})')
    return worst


def assert_mean_of_exact_sum(got, total, lens, what):
    """Bag-mean forward on exact inputs: every element is ``float32(exact_sum / len)`` or a neighbouring float (an IEEE division of the exact sum gives the former; the
    neighbour is room for a doubled rounding).  ``total``: the exact sums (float64), ``lens``: the bag lengths; an empty bag gives 0."""
    lens = lens.double()[:, None]
    q = torch.where(lens > 0, total / lens.clamp(min=1), torch.zeros_like(total)).to(torch.float32)
    lo = torch.nextafter(q, torch.full_like(q, -float('inf')))
    hi = torch.nextafter(q, torch.full_like(q, float('inf')))
    ok = (got >= lo) & (got <= hi)
    assert bool(ok.all()), f'{what}: {int((~ok).sum())} elements are more than one float away from exact_sum / len; first at {tuple(int(i) for i in torch.nonzero(~ok)[0])}'
    assert bool((got[(lens == 0).expand_as(got)] == 0).all()), f'{what}: an empty bag is not zero'


def sequential_float32_sum(terms_by_element):
    """A plain float32 evaluation for the host test: ``terms_by_element`` is ``[n, elements]`` float64 terms (already scaled); every term is rounded to float32 and the
    column is added up in index order in float32."""
    t = np.asarray(terms_by_element, np.float64).astype(np.float32)
    acc = np.zeros(t.shape[1], np.float32)
    for k in range(t.shape[0]):
        acc = (acc + t[k]).astype(np.float32)
    return acc
