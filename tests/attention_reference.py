"""Ladders, score designs, float64 references, derived bounds and a float32 emulation for the attention launches of ``csrc/attention.hpp``, ``csrc/gat.hip`` and
``csrc/phase2.hip`` - test infrastructure (CPU, numpy / torch only; ``tests/test_attention_host.py`` guards it, ``tests/test_attention_kernels.py`` uses it).

GRAPHS.  A ``Graph`` is one real layout (``PairLayout`` under completeness ``'ui'`` for GAT, ``IncidenceLayout`` for phase 2) seen as what the kernels walk: a CSR
whose row v lists the SOURCES of v's entries, a second table (``mirror`` / ``pos``) and, under phase 2 with repeated triples kept once, a multiplicity per source.
The main ladder is cut at ``heavy_threshold = 2`` with chunk 2 (a hub row of 2 k entries has k segments), the short one at threshold and chunk 34.  The chunk is
``layout.HEAVY_CHUNK``, set for the time of the construction only (``heavy_chunk``).  Hub rows: hub USERS under GAT (their items come from two shared pools, so
the item rows have mixed small lengths, some of them split, and ``mirror`` crosses split rows; three items of every hub user are its own - its first entry, its
last entry and one entry of a segment with index >= 256 where the row has one - so that a score set on a source can single out one entry of one row); hub QUERIES
under phase 2 (every hyperedge is in exactly one hub row, so the scores of a hub row are free per entry).  The builders assert that the hub rows' differences of
``csr.heavy_segptr`` are exactly the ladder's counts, in row order; the other split rows (items; users and items under phase 2) have a handful of segments each.

DESIGNS.  Under the concatenation head ``x[u] = (s_u, g_u, 0, ...)`` for a source, ``h[v] = (., ., t_v, 0)`` for a destination, ``w_src = e_0``, ``w_dst = e_2``:
``z[p] = act(s_ids[p] + t_v + c)`` and, with ``dout[v] = r_v e_1``, ``d alpha[p] = r_v g_ids[p]``.  s, g, t, r and (but for ``equal`` at 0.3) c are small integers.

VERDICTS.  eps = 2^-24 (float32 unit roundoff); every bound is first order in eps and is derived here, none is tuned against the kernels.

* EXACT.  Integer features in [-4, 4], integer weights in [-2, 2], integer c: every product and partial sum of a score before the activation is an integer, and
  when ``sum |terms| < 2^24`` (``assert_exact_condition``) each is a float32 value whatever the order or fusing of the additions.  ReLU is then exact; LeakyReLU
  is ONE rounding of ``float32(0.01) x``, which the float64 reference reproduces (the 48-bit product is exact in float64, the cast rounds it once).  So ``z`` must
  EQUAL the reference under ReLU and LeakyReLU.  ``d alpha`` (a dot of integers), ``ihg_gat_symmetrize`` on integers and ``ihg_phase2_edges_bwd`` on power-of-two
  ``alpha_edge`` / ``ds_edge`` and integer rows are exact in the same way.
* z, float inputs.  A dot of d terms added in any order: at most d roundings on a term (its product, d - 1 additions).  The concatenation head adds its two dots
  and c (2 more), the product head multiplies three numbers per term (1 more) and adds c (1 more):
  ``|pre - pre64| <= (d + 4) eps sum |terms|`` (|c| among the terms).  The activations are 1-Lipschitz; LeakyReLU rounds once more (eps |z|); ``tanhf`` is taken at
  5 ulp = 10 eps |z| - the OpenCL accuracy figure its device library is written to; no figure for it was found in the ROCm headers next to the compiler.
* alpha, ``equal`` design.  All scores of a row are equal, so every ``z - max`` is 0, ``expf(0) = 1``, the denominator is the integer ``sum m`` (exact in any order
  below 2^24), every merge multiplies by ``expf(0) = 1``: the division is the only rounding and ``alpha[p]`` is ``float32(m_p / sum m)`` or a neighbouring float
  (room for a division that is not correctly rounded).  Where ``sum m`` is a power of two ``alpha`` is exact.
* alpha, ``one_hot`` design.  A row of n <= 2,050 entries whose runner-up is 40 below its maximum: the denominator is within ``n e^-40 < 2^-25`` of 1, which rounds to
  1, so the winner's ``alpha`` is exactly 1.0f.
* alpha, general, per entry RELATIVE to the entry's own ``alpha64`` (the float64 softmax of the float32 ``z`` the kernel stored, times the multiplicity).  n: the
  row's entries, M its maximum, D = M - min z, K = EXPF_ULP (``expf`` at K ulp = 2 K eps; the ROCm headers next to the compiler state no figure, so 2 ulp is
  allowed).  The maximum is exact (a comparison).
    numerator    ``m_p expf(z_p - M)``: the subtraction moves the exponent by eps |z_p - M| (hence the value by that, relatively); expf 2 K eps; the product with
                 m_p eps; the division eps                                                          -> eps (|z_p - M| + 2 K + 2)
    denominator  every term like the numerator but relative to ITS segment's maximum, <= eps (D + 2 K + 1); at most n - 1 additions on any term in any order
                 (c - 1 inside a segment of c entries, one per merge that has a partner: a row of S segments has at most S - 1 of those on a path)
                                                                                                     -> eps (D + 2 K + 1 + n - 1)
    merges       a split row's (max, sum) pairs pass through ``trips + 8`` merge levels (trips = ceil(S / 256) in the thread loop, 8 in the tree).  A level
                 multiplies the running sum by ``expf(m - mx)``: eps |m - mx| <= eps D on the exponent, expf 2 K eps, the product eps (the addition is counted
                 above)                                                                              -> eps (trips + 8) (D + 2 K + 1)
  The relative bound of ``alpha64`` is the sum of the three.
* ds, per entry.  The reference is shift invariant: ``ds64 = alpha (g - C) act'(z)`` with ``C = sum alpha g / sum alpha`` in float64, from the float32 ``alpha`` and
  ``z`` the forward stored (the stored alphas sum to 1 only up to rounding; the kernel's ``(g - g0) - sum alpha (g - g0)`` differs from the normalised form by
  ``sum alpha (g - g0) (1 - 1 / sum alpha)``, the last term below).  With u = g - g0, A = sum_q alpha_q |u_q|, exact g:
    ``u_q``: eps |u_q|;  ``c = sum alpha u`` in any order: one more for each product, n - 1 additions -> eps (n + 1) A;  ``w = u_p - c``: eps (|u_p| + A);
    ``t = alpha w`` and ``ds = t a``: 2 eps (|u_p| + A);  ``a = 1 - z^2`` under tanh: two roundings, absolutely 2 eps -> 2 eps (|u_p| + A) more (a <= 1)
    -> ``|ds - ds64| <= alpha_p [(n + 6) eps (|u_p| + A) + A |1 - sum alpha|]``   (|act'| <= 1 under all three activations)
  With float inputs ``g = d alpha`` itself carries ``E_q = (d + 2) eps sum_k |dout[v, k] x[u, k]|`` (a dot of d terms), which reaches ds as ``alpha_p (E_p + sum alpha E)``.
* node_sums.  ``S[v] = sum_row ds`` is formed as ``sum t a`` or as ``- sum t (1 - a)`` (equal in exact arithmetic because the normalised t sum to 0): the entries'
  bounds add up (they bound t as well, |a| <= 1), and the sum of n terms ``t a`` or ``t (1 - a)`` in any order adds ``(n + 2) eps sum |t|``.  A row whose activation
  slopes are all 1 (positive scores under LeakyReLU / ReLU) must give +-0: ``sum t (1 - a)`` is a sum of zeros.  GAT's ``node_sums[2 v] = sum_row ds[mirror]``: the
  bounds of the entries it adds, plus ``n eps sum |ds64[mirror]|``.
* ``alpha_mirror[mirror[p]] == alpha[p]``, ``alpha_edge[pos[p]] == alpha[p]``, ``ds_edge[pos[p]] == ds[p]``: bitwise, every entry.
* ``ihg_phase2_edges_bwd``, float: an element is 3 (concatenation: 4; product: 6 and the product with w) terms: ``8 eps sum |terms|``.

EMULATION.  ``emulate_forward`` / ``emulate_backward`` restate the kernels' scheme in numpy float32 (16 lanes per unit, butterfly, 256-thread loop, 8-level tree);
they need not match the kernels' bits.  The host test holds them to every bound on every case the GPU file runs and shows that each ``mutation`` misses one.
"""
import contextlib
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

EPS = 2.0 ** -24
EXACT_LIMIT = 1 << 24
EXPF_ULP = 2
TANHF_ULP = 5
LANES = 16                               # lanes per unit of the scalar passes (attention.hpp: kScalarLanes)
BLOCK = 256                              # threads of a finish workgroup (kBlockThreads)
TREE_LEVELS = 8
MAX_SCALAR_UNITS = 8192 * 4 * 4          # scalar passes: 8,192 workgroups x 4 waves x 4 units before a second grid-stride trip
MAX_ROWDOT_UNITS_G64 = 8192 * 4          # row gather-dot at G = 64: one unit per wave
MAX_FINISH_ROWS = 8192                   # finish kernels: one split row per workgroup
MAX_FLAT = 8192 * BLOCK                  # the flat passes (symmetrize, edge-slot copy): 2,097,152 entries
ACTS = ('leaky_relu', 'relu', 'tanh')
HEADS = ('concatenation', 'product')
SLOPE = float(np.float32(0.01))
CPU = torch.device('cpu')


def attention_segment_counts():
    """Around one lane group, one wave and one workgroup of partials; two and four trips of the finish kernels' thread loop and one beyond."""
    return [2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]


SHORT_LADDER = [255, 256, 257]           # at chunk 34: segments longer than a unit's 16 lanes (two trips per lane and a remainder)
LADDERS = {2: attention_segment_counts(), 34: SHORT_LADDER}


def ladder_lengths(chunk):
    """Hub row lengths (threshold = chunk): the ladder's rows, one odd row whose last segment holds one entry, light rows of 0, 1 and 2 (and, at chunk 34, 20) entries."""
    odd = [11] if chunk == 2 else [3 * chunk + 1, 20]
    lengths = [chunk * k for k in LADDERS[chunk]] + odd + [0, 1, 2]
    return [int(x) for x in np.random.default_rng(chunk).permutation(lengths)]


@contextlib.contextmanager
def heavy_chunk(chunk):
    """``monkeypatch.setattr(layout, 'HEAVY_CHUNK', chunk)`` for the time of a construction (``split_row_plan_for`` reads it at call time)."""
    from ihgnn_amd import layout
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(layout, 'HEAVY_CHUNK', chunk)
        yield


# kind: 'gat' | 'phase2'; ptr, ids, table: int64 numpy (table: mirror / pos); mult: float64 numpy per source or None; hub_rows / hub_lens: the ladder's rows
Graph = namedtuple('Graph', 'kind layout csr n_rows n_src ptr ids table mult hub_rows hub_lens chunk')


def graph_of(kind, lay, hub_rows=(), hub_lens=(), chunk=None):
    csr = lay.csr if kind == 'gat' else lay.node_csr
    table = lay.mirror_host if kind == 'gat' else lay.member_csr.ids_host
    mult = None if kind == 'gat' or lay.edge_weight_host is None else lay.edge_weight_host.astype(np.float64)
    n_src = lay.node_count if kind == 'gat' else lay.edge_count
    return Graph(kind, lay, csr, lay.node_count, n_src, csr.ptr_host.astype(np.int64), csr.ids_host.astype(np.int64), np.asarray(table, np.int64), mult,
                 np.asarray(hub_rows, np.int64), np.asarray(hub_lens, np.int64), chunk)


def row_of(g):
    return np.repeat(np.arange(g.n_rows), np.diff(g.ptr))


def segment_counts(csr):
    """{row: segments} of the split rows of a ``Csr``."""
    if csr.n_heavy == 0:
        return {}
    return dict(zip(csr.heavy_rows.cpu().numpy().tolist(), np.diff(csr.heavy_segptr.cpu().numpy()).tolist()))


def assert_ladder(g):
    """The hub rows have the wanted lengths and - the point of the ladder - exactly the wanted segment counts, in row order."""
    lens = np.diff(g.ptr)
    np.testing.assert_array_equal(lens[g.hub_rows], g.hub_lens)
    counts = segment_counts(g.csr)
    got = [counts[int(r)] for r in g.hub_rows if int(r) in counts]
    want = [-(-int(n) // g.chunk) for n in g.hub_lens if n > g.chunk]
    assert got == want, (got, want)
    assert set(LADDERS[g.chunk]) <= set(got) <= set(np.diff(g.csr.heavy_segptr.cpu().numpy()).tolist())
    return got


def deep_position(length, chunk):
    """Position, inside a hub row, of the entry that lies in a segment with index >= 256 where the row has one (else: its last entry but one)."""
    return 1 + min(length - 3, chunk * BLOCK + 1) if length >= 3 else 0


def gat_ladder_triples(chunk):
    """``(triples, U, Q, I)``: hub user r pairs with ``lengths[r]`` distinct items - its own first / deep / last item (ids below, between and above the two shared
    pools) and items drawn from the pools."""
    rng = np.random.default_rng([71, chunk])
    lengths = ladder_lengths(chunk)
    H = len(lengths)
    n_low = [min(n - 3, chunk * BLOCK + 1) if n >= 3 else 0 for n in lengths]
    n_high = [max(n - 3 - lo, 0) for n, lo in zip(lengths, n_low)]
    PL, PH = 2 * max(n_low) + 8, 2 * max(n_high) + 8
    low0, mid0, high0, last0 = H, H + PL, H + PL + H, H + PL + H + PH
    rows = []
    for r, n in enumerate(lengths):
        items = [r][:n] + ([last0 + r] if n >= 2 else []) + ([mid0 + r] if n >= 3 else [])
        items += (low0 + rng.choice(PL, n_low[r], replace=False)).tolist() + (high0 + rng.choice(PH, n_high[r], replace=False)).tolist()
        assert len(items) == n == len(set(items))
        rows += [(r, 0, i) for i in items]
    triples = np.asarray(rows, np.int64).reshape(-1, 3)
    return triples[rng.permutation(len(triples))], H, 1, last0 + H, lengths


@functools.lru_cache(maxsize=None)
def gat_ladder(chunk=2, device=CPU):
    from ihgnn_amd.layout import PairLayout
    triples, U, Q, I, lengths = gat_ladder_triples(chunk)
    with heavy_chunk(chunk):
        lay = PairLayout(triples, U, Q, I, device, completeness='ui', heavy_threshold=chunk)
    g = graph_of('gat', lay, np.arange(U), lengths, chunk)
    assert_ladder(g)
    lens = np.diff(g.ptr)
    assert lens[U] == 0 and (lens[U + Q:] <= chunk).any()                                               # the query is isolated; item rows are light ...
    assert chunk != 2 or (lens[U + Q:] > chunk).any()                                                   # ... and, on the main ladder, split as well
    return g


def phase2_ladder_triples(chunk, repeated):
    """Hub query q sits in ``lengths[q]`` DISTINCT (user, q, item) triples, users and items from shared pools; ``repeated``: every triple 1 ... 4 times."""
    rng = np.random.default_rng([72, chunk, int(repeated)])
    lengths = ladder_lengths(chunk)
    U = I = 1500
    rows = []
    for q, n in enumerate(lengths):
        code = rng.choice(U * I, n, replace=False)
        rows += [(int(c) // I, q, int(c) % I) for c in code]
    triples = np.asarray(rows, np.int64).reshape(-1, 3)
    if repeated:
        triples = np.repeat(triples, rng.integers(1, 5, len(triples)), axis=0)
    return triples[rng.permutation(len(triples))], U, len(lengths), I, lengths


@functools.lru_cache(maxsize=None)
def phase2_ladder(chunk=2, repeated=False, device=CPU):
    from ihgnn_amd.layout import IncidenceLayout
    triples, U, Q, I, lengths = phase2_ladder_triples(chunk, repeated)
    with heavy_chunk(chunk):
        lay = IncidenceLayout(triples, U, Q, I, device, heavy_threshold=chunk, edge_multiplicity='1' if repeated else '0', compact_nodes='0')
    g = graph_of('phase2', lay, U + np.arange(Q), lengths, chunk)
    assert_ladder(g)
    assert lay.edge_count == sum(lengths)
    if repeated:
        assert set(np.unique(g.mult).tolist()) == {1.0, 2.0, 3.0, 4.0}
    else:
        assert g.mult is None
    return g


def ladder(kind, chunk=2, repeated=False, device=CPU):
    return gat_ladder(chunk, device) if kind == 'gat' else phase2_ladder(chunk, repeated, device)


def graph_from_lengths(kind, lengths, threshold, chunk=2, device=CPU, seed=0):
    """A small real layout whose hub rows (users under GAT, queries under phase 2) have the given lengths, other rows short; ``threshold`` 0: no split rows."""
    from ihgnn_amd.layout import IncidenceLayout, PairLayout
    rng = np.random.default_rng([73, seed, len(lengths)])
    H, pool = len(lengths), max(max(lengths, default=0), 1) * 2 + 3
    rows = []
    for r, n in enumerate(lengths):
        if kind == 'gat':
            rows += [(r, 0, int(i)) for i in rng.choice(pool, n, replace=False)]
        else:
            rows += [(int(c) // pool, r, int(c) % pool) for c in rng.choice(pool * pool, n, replace=False)]
    triples = np.asarray(rows, np.int64).reshape(-1, 3)
    big = 1 << 30
    with heavy_chunk(chunk):
        if kind == 'gat':
            lay = PairLayout(triples, H, 1, pool, device, completeness='ui', heavy_threshold=threshold or big)
            return graph_of('gat', lay, np.arange(H), lengths, chunk)
        lay = IncidenceLayout(triples, pool, H, pool, device, heavy_threshold=threshold or big, edge_multiplicity='0', compact_nodes='0')
        return graph_of('phase2', lay, pool + np.arange(H), lengths, chunk)


# ---------------------------------------------------------------------------------------------
# cases: the inputs of the launches (float32 torch, CPU)
# ---------------------------------------------------------------------------------------------
# x: the source table ([n, d] node rows under GAT - the same tensor as h -, [E, d] hyperedge rows under phase 2); h: the destination rows; w: [2 d] | [d]; c: [1]
Case = namedtuple('Case', 'x h w c dout head exact')

DESIGNS = ('equal', 'equal100', 'equal_neg', 'one_hot_first', 'one_hot_last', 'one_hot_deep', 'staircase', 'ascending', 'descending', 'float')
BACKWARD_DESIGNS = ('equal', 'equal100', 'staircase', 'float')
TANH_DESIGNS = ('equal', 'equal100', 'equal_neg', 'float')     # tanh saturates the integer designs: only these make sense under it


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def concat_case(g, s, gsrc, t, c, r=None, d=4):
    """The concatenation head with free scores: ``z[p] = act(s[ids[p]] + t[v] + c)``, ``d alpha[p] = r[v] gsrc[ids[p]]``."""
    x = np.zeros((g.n_src, d))
    x[:, 0], x[:, 1] = s, gsrc
    if g.kind == 'gat':
        x[:, 2] = t
        h = x
    else:
        h = np.zeros((g.n_rows, d))
        h[:, 2] = t
    w = np.zeros(2 * d)
    w[0] = w[d + 2] = 1.0
    dout = np.zeros((g.n_rows, d))
    dout[:, 1] = 1.0 if r is None else r
    x = _f32(x)
    return Case(x, x if g.kind == 'gat' else _f32(h), _f32(w), _f32([c]), _f32(dout), 'concatenation', float(c) == int(c))


def winners(g, where):
    """One entry per hub row: ``(entries, their sources)``; under GAT the source must be the hub's own item."""
    lens = g.hub_lens
    keep = lens > 0
    rows, lens = g.hub_rows[keep], lens[keep]
    at = {'first': np.zeros_like(lens), 'last': lens - 1, 'deep': np.asarray([deep_position(int(n), g.chunk) for n in lens])}[where]
    p = g.ptr[rows] + at
    src = g.ids[p]
    if g.kind == 'gat':
        assert (np.diff(g.ptr)[src] == 1).all(), 'a winner is shared between hub rows'
    assert len(set(src.tolist())) == len(src)
    if where == 'deep':
        seg = at // g.chunk
        assert (seg[lens > g.chunk * BLOCK] >= BLOCK).all() and (lens > g.chunk * BLOCK).any()
    return p, src


def design_scores(g, design, rng):
    """``(s per source, c)`` of a score design (integers, but for c = 0.3)."""
    s, c = np.zeros(g.n_src), 0.0
    if design == 'equal':
        c = 0.3
    elif design == 'equal100':
        c = 100.0                                                          # expf overflows unless the row's maximum is subtracted
    elif design == 'equal_neg':
        c = -5.0                                                           # all-negative scores: under ReLU every z is 0
    elif design.startswith('one_hot'):
        s[winners(g, design[len('one_hot_'):])[1]] = 40.0
    elif design == 'staircase':
        s, c = rng.integers(-30, 1, g.n_src).astype(np.float64), 33.0          # (c lifts the scores above 0: the activations leave the staircase as it is)
    elif design in ('ascending', 'descending'):
        if g.kind == 'gat':
            # a source is shared between rows, so the score rises with the source's id: every row holds ascending ids, hence ascending scores
            first = g.layout.user_count + g.layout.query_count
            s[first:] = np.floor(60.0 * np.arange(g.n_src - first) / max(g.n_src - first - 1, 1))
        else:
            # a hyperedge is in one hub row: 3 per segment of that row, clipped so that max - min <= 60
            for r in g.hub_rows:
                p = np.arange(g.ptr[r], g.ptr[r + 1])
                s[g.ids[p]] = np.minimum(3.0 * ((p - g.ptr[r]) // g.chunk), 60.0)
        if design == 'descending':
            s = 60.0 - s if g.kind != 'gat' else np.where(np.arange(g.n_src) >= g.layout.user_count + g.layout.query_count, 60.0 - s, 0.0)
    else:
        raise ValueError(design)
    return s, c


def float_case(g, head, d, rng, scale=1.0):
    """``randn`` features at width d, the attention vector at ``scale / sqrt(d)``."""
    x = _f32(rng.standard_normal((g.n_src, d)))
    h = x if g.kind == 'gat' else _f32(rng.standard_normal((g.n_rows, d)))
    w = _f32(rng.standard_normal(2 * d if head == 'concatenation' else d) * scale / np.sqrt(d))
    return Case(x, h, w, _f32([rng.standard_normal()]), _f32(rng.standard_normal((g.n_rows, d))), head, False)


def integer_case(g, head, d, rng):
    """Integer features in [-4, 4], integer weights in [-2, 2], an integer c, an integer cotangent: every score before the activation and every ``d alpha`` is exact."""
    x = _f32(rng.integers(-4, 5, (g.n_src, d)))
    h = x if g.kind == 'gat' else _f32(rng.integers(-4, 5, (g.n_rows, d)))
    w = _f32(rng.integers(-2, 3, 2 * d if head == 'concatenation' else d))
    return Case(x, h, w, _f32([rng.integers(-3, 4)]), _f32(rng.integers(-4, 5, (g.n_rows, d))), head, True)


def design_case(g, design, head='concatenation', seed=0):
    """The case of a ladder and a design.  ``float``: width 32, scores spread over a few tens (asserted <= 60 by the callers through ``row_spread``)."""
    rng = np.random.default_rng([74, seed, DESIGNS.index(design)])
    if design == 'float':
        return float_case(g, head, 32, rng, scale=4.0)
    assert head == 'concatenation'
    s, c = design_scores(g, design, rng)
    # (one_hot: t >= 0, so that the winner stays 40 above act(t) under every activation)
    t = rng.integers(0, 3, g.n_rows) if design.startswith('one_hot') else rng.integers(-2, 3, g.n_rows)
    return concat_case(g, s, rng.integers(-3, 4, g.n_src), t, c, rng.integers(1, 3, g.n_rows))


# ---------------------------------------------------------------------------------------------
# float64 references (torch, any device: index tensors are made on the device of the features)
# ---------------------------------------------------------------------------------------------
def _index(g, dev):
    cache = g.layout.__dict__.setdefault('_attention_reference_index', {})       # (kept on the layout: it lives as long as the layout does)
    got = cache.get(str(dev))
    if got is None:
        got = cache[str(dev)] = tuple(torch.from_numpy(a).to(dev) for a in (g.ids, row_of(g), g.table, g.ptr))
    return got


def act64(pre, act):
    if act == 'leaky_relu':
        return torch.where(pre > 0, pre, pre * SLOPE)
    return torch.relu(pre) if act == 'relu' else torch.tanh(pre)


def act_grad64(z, act):
    """The derivative from the OUTPUT, as the kernels and torch take it (slope at 0 under LeakyReLU, 0 at 0 under ReLU)."""
    z = z.double()
    if act == 'leaky_relu':
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, SLOPE))
    return (z > 0).double() if act == 'relu' else 1.0 - z * z


ZRef = namedtuple('ZRef', 'want bound peak')


def z64(g, case, act):
    """``z`` from the features: ``(float64 value, per-entry bound for float inputs, sum |terms| before the activation)``."""
    ids, rows, _, _ = _index(g, case.x.device)
    x, h, w, d = case.x.double(), case.h.double(), case.w.double(), case.x.shape[1]
    c = case.c.double().reshape(())
    if case.head == 'concatenation':
        a, b = x @ w[:d], h @ w[d:]
        a_mag, b_mag = x.abs() @ w[:d].abs(), h.abs() @ w[d:].abs()
        pre, mag = a[ids] + b[rows] + c, a_mag[ids] + b_mag[rows] + c.abs()
    else:
        hw = h * w
        pre = (x[ids] * hw[rows]).sum(1) + c
        mag = (x[ids].abs() * hw[rows].abs()).sum(1) + c.abs()
    want = act64(pre, act)
    bound = (d + 4) * EPS * mag + {'leaky_relu': 1.0, 'relu': 0.0, 'tanh': 2.0 * TANHF_ULP}[act] * EPS * want.abs()
    return ZRef(want, bound, mag)


def assert_exact_condition(peak, what=''):
    """The condition on an exact case's inputs: the sum of the magnitudes of the terms of every element is an integer below 2^24.  Returns the largest."""
    if peak.numel() == 0:
        return 0
    assert bool((peak == peak.round()).all()), f'{what}: a term is not an integer'
    worst = int(peak.max())
    assert worst < EXACT_LIMIT, f'{what}: sum |terms| = {worst} is not below 2^24: the case is not exact'
    return worst


def assert_equal(got, want64, what):
    want = want64.to(torch.float32)
    assert got.shape == want.shape, f'{what}: shape {tuple(got.shape)} for {tuple(want.shape)}'
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f'{what}: {bad.shape[0]} of {got.numel()} elements differ from the exact value; first at {first}: got {float(got[first])!r}, want {float(want[first])!r}')


def assert_within(got, want64, bound, what, label):
    """Per element ``|got - want| <= bound`` (an element whose bound is 0 must be equal); prints and returns the worst ``error / bound``."""
    assert bool(torch.isfinite(got).all()), f'{what}: {label} is not finite'
    err = (got.double() - want64).abs()
    assert bool((err[bound == 0] == 0).all()), f'{what}: an element of {label} with a zero bound differs'
    ratio = err / torch.where(bound > 0, bound, torch.ones_like(bound))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f'attention {what}: {label} worst error / bound = {worst:.4f}')
    if worst > 1.0:
        first = tuple(int(i) for i in torch.nonzero(ratio > 1.0)[0])
        raise AssertionError(f'{what}: {label} {first} is off by {float(err[first]):.3e}, bound {float(bound[first]):.3e} ({int((ratio > 1).sum())} elements over)')
    return worst


def _row_sum(rows, n, v):
    return torch.zeros(n, dtype=torch.float64, device=v.device).index_add_(0, rows, v)


def _row_max(rows, n, v):
    return torch.full((n,), -float('inf'), dtype=torch.float64, device=v.device).scatter_reduce(0, rows, v, 'amax', include_self=True)


AlphaRef = namedtuple('AlphaRef', 'want rel_bound spread')


def finish_levels(g, dev):
    """Per row: the merge levels a split row's partials pass through (thread-loop trips + 8), 0 for a light row."""
    lv = np.zeros(g.n_rows)
    for r, s in segment_counts(g.csr).items():
        lv[r] = -(-s // BLOCK) + TREE_LEVELS
    return torch.from_numpy(lv).to(dev)


def alpha64(g, z32):
    """The softmax of the float32 ``z`` the kernel stored, times the multiplicity, in float64; the per-entry RELATIVE bound; the rows' spreads D."""
    ids, rows, _, ptr = _index(g, z32.device)
    z = z32.double()
    top = _row_max(rows, g.n_rows, z)
    low = -_row_max(rows, g.n_rows, -z)
    e = torch.exp(z - top[rows])
    if g.mult is not None:
        e = e * torch.from_numpy(g.mult).to(z.device)[ids]
    want = e / _row_sum(rows, g.n_rows, e)[rows]
    n = (ptr[1:] - ptr[:-1]).double()
    D = torch.where(n > 0, top - low, torch.zeros_like(top))
    k = 2.0 * EXPF_ULP
    per_row = (D + k + 1 + n - 1) + finish_levels(g, z.device) * (D + k + 1)
    return AlphaRef(want, EPS * ((top[rows] - z) + k + 2 + per_row[rows]), D)


def assert_alpha_equal_design(g, alpha, what):
    """``equal`` design: within one float of ``float32(m_p / sum m)``; exact where ``sum m`` is a power of two.  Prints whether the whole tensor was bit-equal."""
    ids, rows, _, _ = _index(g, alpha.device)
    m = torch.ones(ids.shape[0], dtype=torch.float64, device=alpha.device) if g.mult is None else torch.from_numpy(g.mult).to(alpha.device)[ids]
    total = _row_sum(rows, g.n_rows, m)[rows]
    q = (m / total).to(torch.float32)
    lo, hi = torch.nextafter(q, torch.full_like(q, -1.0)), torch.nextafter(q, torch.full_like(q, 2.0))
    ok = (alpha >= lo) & (alpha <= hi)
    assert bool(ok.all()), f'{what}: {int((~ok).sum())} alphas are more than one float from m / sum m; first at {int(torch.nonzero(~ok)[0])}'
    pow2 = torch.frexp(total)[0] == 0.5
    assert bool((alpha[pow2] == q[pow2]).all()), f'{what}: alpha is not exact on a row whose sum of multiplicities is a power of two'
    bit_equal = bool(torch.equal(alpha, q))
    print(f'attention {what}: alpha bit-equal to float32(m / sum m): {bit_equal}')
    return bit_equal


def assert_alpha_one_hot(g, z32, alpha, what):
    """Rows whose runner-up is at least 40 below the maximum: the winner's alpha is exactly 1."""
    ids, rows, _, ptr = _index(g, z32.device)
    z = z32.double()
    top = _row_max(rows, g.n_rows, z)
    is_top = z == top[rows]
    second = _row_max(rows, g.n_rows, torch.where(is_top, torch.full_like(z, -float('inf')), z))
    single = (_row_sum(rows, g.n_rows, is_top.double()) == 1) & (second <= top - 40) & ((ptr[1:] - ptr[:-1]) <= 2050)
    pick = is_top & single[rows]
    assert int(pick.sum()) >= len(g.hub_rows) - 1, f'{what}: the design has no winners'
    assert bool((alpha[pick] == 1.0).all()), f'{what}: a winner 40 above its row is not exactly 1'


DsRef = namedtuple('DsRef', 'ds ds_bound S S_bound src src_bound t_is_zero')


def dalpha64(g, case):
    """``d alpha[p] = dout[v] . x[ids[p]]``: ``(float64 value, sum |terms|)``."""
    ids, rows, _, _ = _index(g, case.x.device)
    x, dout = case.x.double(), case.dout.double()
    return (dout[rows] * x[ids]).sum(1), (dout[rows].abs() * x[ids].abs()).sum(1)


def ds64(g, z32, alpha32, galpha, act, g_err=None):
    """The softmax backward from the float32 ``alpha`` and ``z`` the forward stored and a float64 ``d alpha`` (``g_err``: its per-entry error bound when it comes
    from float inputs): ds, S = sum_row ds, GAT's sum_row ds[mirror], and their bounds."""
    ids, rows, table, ptr = _index(g, z32.device)
    al, a = alpha32.double(), act_grad64(z32, act)
    n = (ptr[1:] - ptr[:-1]).double()
    first = ptr[:-1].clamp(max=max(ids.shape[0] - 1, 0))
    g0 = torch.where(n > 0, galpha[first] if ids.shape[0] else torch.zeros_like(n), torch.zeros_like(n))
    mass = _row_sum(rows, g.n_rows, al)
    safe = torch.where(mass > 0, mass, torch.ones_like(mass))
    # (normalised, the value does not depend on the shift; taken about g0 so that float64's own cancellation stays below the bound where one alpha is 1 - 1e-12)
    shifted = galpha - g0[rows]
    C = _row_sum(rows, g.n_rows, al * shifted) / safe
    t = al * (shifted - C[rows])
    ds = t * a
    u = shifted.abs()
    A = _row_sum(rows, g.n_rows, al * u)
    bound = al * ((n[rows] + 6) * EPS * (u + A[rows]) + A[rows] * (1 - mass).abs()[rows])
    if g_err is not None:
        bound = bound + al * (g_err + _row_sum(rows, g.n_rows, al * g_err)[rows])
    S = _row_sum(rows, g.n_rows, ds)
    S_bound = _row_sum(rows, g.n_rows, bound) + (n + 2) * EPS * _row_sum(rows, g.n_rows, t.abs())
    all_one = _row_sum(rows, g.n_rows, (a != 1).double()) == 0
    src = src_bound = None
    if g.kind == 'gat':
        src = _row_sum(rows, g.n_rows, ds[table])
        src_bound = _row_sum(rows, g.n_rows, bound[table]) + n * EPS * _row_sum(rows, g.n_rows, ds[table].abs())
    return DsRef(ds, bound, S, S_bound, src, src_bound, all_one)


def symmetrize64(g, ds32):
    _, _, table, _ = _index(g, ds32.device)
    return ds32.double() + ds32.double()[table]


def edges_bwd64(dout, h, i3, alpha_edge, ds_edge, w, head):
    """``ihg_phase2_edges_bwd``: ``def[e] = sum_k alpha_edge[e, k] dout[i3[e, k]] + (sum_k ds_edge[e, k]) w_src`` (concatenation) or
    ``+ w * sum_k ds_edge[e, k] h[i3[e, k]]`` (product): ``(value, sum |terms|)``."""
    i3 = i3.long()
    al, s = alpha_edge.double().view(-1, 3), ds_edge.double().view(-1, 3)
    rows = dout.double()[i3]                                             # [E, 3, d]
    want = (rows * al[:, :, None]).sum(1)
    mag = (rows.abs() * al.abs()[:, :, None]).sum(1)
    d = dout.shape[1]
    if head == 'concatenation':
        ws = w.double()[:d]
        want, mag = want + s.sum(1)[:, None] * ws, mag + s.abs().sum(1)[:, None] * ws.abs()
    else:
        hr = h.double()[i3] * w.double()
        want, mag = want + (hr * s[:, :, None]).sum(1), mag + (hr.abs() * s.abs()[:, :, None]).sum(1)
    return want, mag


EDGES_BWD_ROUNDINGS = 8


# ---------------------------------------------------------------------------------------------
# float32 emulation of the kernels' scheme (numpy)
# ---------------------------------------------------------------------------------------------
MUTATIONS = ('drop_segment', 'first_trip_only', 'max_without_rescale', 'mult_not_in_denominator', 'fp16_partial', 'no_g0_shift')
F = np.float32


def _units(g):
    """``(begin, length, row, seg)`` of every work unit: the segments of the split rows, then every row (a split row: length 0 here)."""
    csr, lens = g.csr, np.diff(g.ptr)
    if csr.n_heavy:
        sb, se, sr = (t.cpu().numpy().astype(np.int64) for t in (csr.seg_begin, csr.seg_end, csr.seg_row))
        heavy = np.zeros(g.n_rows, bool)
        heavy[csr.heavy_rows.cpu().numpy()] = True
    else:
        sb = se = sr = np.zeros(0, np.int64)
        heavy = np.zeros(g.n_rows, bool)
    rows = np.arange(g.n_rows)
    begin = np.concatenate([sb, g.ptr[:-1]])
    length = np.concatenate([se - sb, np.where(heavy, 0, lens)])
    return begin, length, np.concatenate([sr, rows]), np.concatenate([np.arange(len(sb)), np.full(g.n_rows, -1)]), heavy


def _lane_table(begin, length):
    """Entry index of (unit, trip, lane), -1 where there is none: ``[units, trips, 16]``."""
    trips = max(int(-(-length.max(initial=0) // LANES)), 1)
    i = np.arange(trips * LANES).reshape(1, trips, LANES)
    return np.where(i < length[:, None, None], begin[:, None, None] + i, -1)


def _butterfly(v, op):
    """The 16-lane xor butterfly: every lane ends with the same value; returns lane 0's."""
    lanes = np.arange(LANES)
    for o in (8, 4, 2, 1):
        v = op(v, v[:, lanes ^ o])
    return v[:, 0]


def _lane_sum(table, values):
    """Per unit: every lane adds its entries trip by trip (float32), then the butterfly."""
    acc = np.zeros((table.shape[0], LANES), F)
    for k in range(table.shape[1]):
        idx = table[:, k]
        acc = np.where(idx >= 0, acc + values[np.maximum(idx, 0)], acc).astype(F)
    return _butterfly(acc, lambda a, b: (a + b).astype(F))


def _merge(m, l, m2, l2, mutation):
    with np.errstate(invalid='ignore', over='ignore'):
        mx = np.maximum(m, m2)
        if mutation == 'max_without_rescale':
            merged = (l + l2).astype(F)
        else:
            merged = (l * np.exp((m - mx).astype(F)).astype(F) + l2 * np.exp((m2 - mx).astype(F)).astype(F)).astype(F)
    skip = np.isneginf(m2)
    return np.where(skip, m, mx).astype(F), np.where(skip, l, np.where(np.isneginf(m), l2, merged)).astype(F)


def _heavy_table(g):
    """Segment index of (split row, trip, thread), -1 where there is none: ``[n_heavy, trips, 256]``."""
    segptr = g.csr.heavy_segptr.cpu().numpy().astype(np.int64)
    counts = np.diff(segptr)
    trips = int(-(-counts.max() // BLOCK))
    i = np.arange(trips * BLOCK).reshape(1, trips, BLOCK)
    return np.where(i < counts[:, None, None], segptr[:-1, None, None] + i, -1)


def _block_sum(v):
    """The 256-thread tree of ``block_sum``: ``[rows, 256]`` float32 -> ``[rows]``."""
    v = v.astype(F)
    o = BLOCK // 2
    while o > 0:
        v = np.concatenate([(v[:, :o] + v[:, o:2 * o]).astype(F), v[:, 2 * o:]], 1)[:, :o]
        o //= 2
    return v[:, 0]


def emulate_forward(g, z32, mutation=None):
    """``alpha`` (float32 numpy) from the stored ``z`` by the kernels' scheme: per unit a lane-strided maximum and sum over 16 lanes, a butterfly; light rows are
    finished there; a split row's (max, sum) pairs are merged per thread over trips of 256 and then in an 8-level tree."""
    z = np.asarray(z32, F)
    if z.shape[0] == 0:
        return np.zeros(0, F)
    mult = np.ones(g.n_src, F) if g.mult is None else g.mult.astype(F)
    me = mult[g.ids]
    begin, length, urow, useg, heavy = _units(g)
    table = _lane_table(begin, length)
    zt = np.where(table >= 0, z[np.maximum(table, 0)], -np.inf).astype(F)
    m = zt.max((1, 2))
    m_entry = np.full(z.shape[0], 0, F)
    valid = table >= 0
    m_entry[table[valid]] = np.broadcast_to(m[:, None, None], table.shape)[valid]
    with np.errstate(invalid='ignore'):
        e = np.exp((z - m_entry).astype(F)).astype(F)
    weighted = e if mutation == 'mult_not_in_denominator' else (me * e).astype(F)
    l = _lane_sum(table, weighted)
    alpha = np.zeros(z.shape[0], F)
    light = (useg < 0) & (length > 0)
    l_entry = np.zeros(z.shape[0], F)
    l_entry[table[valid]] = np.broadcast_to(l[:, None, None], table.shape)[valid]
    is_light = ~heavy[row_of(g)]
    alpha[is_light] = ((me * e).astype(F)[is_light] / l_entry[is_light]).astype(F)
    if g.csr.n_heavy:
        n_seg = int((useg >= 0).sum())
        pm, pl_ = m[:n_seg].copy(), l[:n_seg].copy()
        if mutation == 'fp16_partial':
            pl_ = pl_.astype(np.float16).astype(F)
        ht = _heavy_table(g)
        if mutation == 'drop_segment':
            big = int(np.argmax((ht >= 0).sum((1, 2))))
            victim = ht[big, 0, 5]
            pm[victim], pl_[victim] = -np.inf, 0
        if mutation == 'first_trip_only':
            ht = ht[:, :1]
        rm = np.full((ht.shape[0], BLOCK), -np.inf, F)
        rl = np.zeros((ht.shape[0], BLOCK), F)
        for k in range(ht.shape[1]):
            idx = ht[:, k]
            m2 = np.where(idx >= 0, pm[np.maximum(idx, 0)], -np.inf).astype(F)
            l2 = np.where(idx >= 0, pl_[np.maximum(idx, 0)], 0).astype(F)
            rm, rl = _merge(rm, rl, m2, l2, mutation)
        o = BLOCK // 2
        while o > 0:
            a, b = _merge(rm[:, :o], rl[:, :o], rm[:, o:2 * o], rl[:, o:2 * o], mutation)
            rm, rl = a, b
            o //= 2
        hrows = g.csr.heavy_rows.cpu().numpy()
        mx, den = np.zeros(g.n_rows, F), np.ones(g.n_rows, F)
        mx[hrows], den[hrows] = rm[:, 0], rl[:, 0]
        r = row_of(g)
        hv = heavy[r]
        alpha[hv] = ((me[hv] * np.exp((z[hv] - mx[r[hv]]).astype(F)).astype(F)).astype(F) / den[r[hv]]).astype(F)
    return alpha


def emulate_backward(g, z32, alpha32, galpha32, act, mutation=None):
    """``(ds, S)`` (float32 numpy) by the kernels' scheme: ``c = sum alpha (g - g0)`` per unit (lanes, butterfly), per split row over the thread loop and the block
    tree; ``ds = alpha ((g - g0) - c) a``; the row sum as ``sum t a`` or ``- sum t (1 - a)``, whichever has the smaller alpha-mass."""
    z, al, gg = np.asarray(z32, F), np.asarray(alpha32, F), np.asarray(galpha32, F)
    if z.shape[0] == 0:
        return np.zeros(0, F), np.zeros(g.n_rows, F)
    a = act_grad64(torch.from_numpy(z), act).numpy().astype(F) if act != 'tanh' else (F(1) - (z * z).astype(F)).astype(F)
    r = row_of(g)
    lens = np.diff(g.ptr)
    g0 = np.zeros(g.n_rows, F)
    g0[lens > 0] = gg[g.ptr[:-1][lens > 0]]
    if mutation == 'no_g0_shift':
        g0[:] = 0
    u = (gg - g0[r]).astype(F)
    begin, length, urow, useg, heavy = _units(g)
    table = _lane_table(begin, length)
    c_unit = _lane_sum(table, (al * u).astype(F))
    c_row = np.zeros(g.n_rows, F)
    n_seg = int((useg >= 0).sum())
    c_row[urow[n_seg:]] = c_unit[n_seg:]
    if g.csr.n_heavy:
        ht = _heavy_table(g)
        acc = np.zeros((ht.shape[0], BLOCK), F)
        for k in range(ht.shape[1]):
            idx = ht[:, k]
            acc = np.where(idx >= 0, acc + c_unit[np.maximum(idx, 0)], acc).astype(F)
        c_row[g.csr.heavy_rows.cpu().numpy()] = _block_sum(acc)
    t = (al * (u - c_row[r]).astype(F)).astype(F)
    ds = (t * a).astype(F)
    one_minus = (F(1) - a).astype(F)
    parts = [(al * a).astype(F), (al * one_minus).astype(F), ds, (t * one_minus).astype(F)]
    # rows as units of their own for the four row sums (a light row: lanes + butterfly; a split row: 256 threads strided over the row + four block sums)
    sums = []
    lt = _lane_table(g.ptr[:-1], np.where(heavy, 0, lens))
    for v in parts:
        s = _lane_sum(lt, v)
        if g.csr.n_heavy:
            hrows = g.csr.heavy_rows.cpu().numpy()
            hl = lens[hrows]
            trips = int(-(-hl.max() // BLOCK))
            i = np.arange(trips * BLOCK).reshape(1, trips, BLOCK)
            tab = np.where(i < hl[:, None, None], g.ptr[hrows][:, None, None] + i, -1)
            acc = np.zeros((len(hrows), BLOCK), F)
            for k in range(trips):
                idx = tab[:, k]
                acc = np.where(idx >= 0, acc + v[np.maximum(idx, 0)], acc).astype(F)
            s[hrows] = _block_sum(acc)
        sums.append(s)
    ma, mb, sa, sb = sums
    S = np.where(mb < ma, -sb, sa).astype(F)
    return ds, S


# ---------------------------------------------------------------------------------------------
# the cases and the verdicts that the host test (on the emulation) and the GPU test (on the launches) share
# ---------------------------------------------------------------------------------------------
LADDER_GRAPHS = [('gat', 2, False), ('phase2', 2, False), ('phase2', 2, True), ('gat', 34, False), ('phase2', 34, False)]


def ladder_designs(head, act, backward=False):
    """The designs that make sense for a head and an activation: the free-score designs need the concatenation head; tanh saturates the integer staircases."""
    names = BACKWARD_DESIGNS if backward else DESIGNS
    if head == 'product':
        return ('float',)
    return tuple(d for d in names if act != 'tanh' or d in TANH_DESIGNS)


def near_equal_dalpha_case(g):
    """Equal scores and ``d alpha = 4096 + (-3 ... 3)``: the row's spread is 1e-3 of its level - what the shift by the row's first entry is for."""
    rng = np.random.default_rng(75)
    return concat_case(g, np.zeros(g.n_src), 4096 + rng.integers(-3, 4, g.n_src), rng.integers(-2, 3, g.n_rows), 1.0)


def check_forward(g, case, act, design, z, alpha, what, hold_alpha=True):
    """Every verdict on ``z`` and ``alpha`` (float32 torch tensors on one device).  Returns ``{'z': ratio or 'equal', 'alpha': ratio, 'bit_equal': bool or None}``."""
    out = {'bit_equal': None}
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(alpha).all()), f'{what}: an entry was not written'
    zr = z64(g, case, act)
    if case.exact and act != 'tanh':
        assert_exact_condition(zr.peak, what)
        assert_equal(z, zr.want, f'{what}: z')
        out['z'] = 'equal'
    else:
        out['z'] = assert_within(z, zr.want, zr.bound, what, 'z')
    if not hold_alpha:                                                   # (integer scores at a real width spread over hundreds: only z is held there)
        return out
    ar = alpha64(g, z)
    assert ar.spread.numel() == 0 or float(ar.spread.max()) <= 60.0, f'{what}: a row spreads over more than 60'
    if design.startswith('equal'):
        out['bit_equal'] = assert_alpha_equal_design(g, alpha, what)
    if design.startswith('one_hot'):
        assert_alpha_one_hot(g, z, alpha, what)
    out['alpha'] = assert_within(alpha, ar.want, ar.rel_bound * ar.want, what, 'alpha')
    return out


def check_backward(g, case, act, design, z, alpha, ds, S, src_sums, what):
    """Every verdict on ``ds``, ``S = node_sums[:, 1]`` and (GAT, concatenation head) ``node_sums[:, 0]``."""
    out = {}
    assert bool(torch.isfinite(ds).all()) and bool(torch.isfinite(S).all()), f'{what}: an entry was not written'
    ga, gmag = dalpha64(g, case)
    g_err = None
    if case.exact or design != 'float':
        assert_exact_condition(gmag, what)
    else:
        g_err = (case.x.shape[1] + 2) * EPS * gmag
    ref = ds64(g, z, alpha, ga, act, g_err)
    out['ds'] = assert_within(ds, ref.ds, ref.ds_bound, what, 'ds')
    out['S'] = assert_within(S, ref.S, ref.S_bound, what, 'node_sums[:, 1]')
    assert bool((S[ref.t_is_zero] == 0).all()), f'{what}: the row sum of a row whose slopes are all 1 is not +-0'
    if design.startswith('equal') and act == 'leaky_relu' and design != 'equal_neg' and g_err is None:
        # rows whose multiplicities sum to a power of two: alpha = m / 2^k is exact, u and c are multiples of 2^-k far below 2^24 of them: ds is exact
        ids, rows, _, _ = _index(g, z.device)
        m = torch.ones(ids.shape[0], dtype=torch.float64, device=z.device) if g.mult is None else torch.from_numpy(g.mult).to(z.device)[ids]
        pow2 = (torch.frexp(_row_sum(rows, g.n_rows, m))[0] == 0.5)[rows] & ref.t_is_zero[rows]
        assert int(pow2.sum()) > 0
        assert_equal(ds[pow2], ref.ds[pow2], f'{what}: ds on the rows of power-of-two length')
    if src_sums is not None:
        out['src'] = assert_within(src_sums, ref.src, ref.src_bound, what, 'node_sums[:, 0]')
    return out


@functools.lru_cache(maxsize=None)
def small_graph(kind, which, device=CPU):
    """The degenerate plans and the light-row graph of the host test (the GPU file builds the same ones on its device): ``light`` - no split rows, lengths at the
    boundaries of the 16 lanes of a scalar unit; ``no_edges``; ``only_split`` - every row that has entries is split (GAT keeps its one, isolated, query row);
    ``split_among_isolated`` - one split row between rows without entries."""
    from ihgnn_amd.layout import IncidenceLayout, PairLayout
    if which == 'light':
        return graph_from_lengths(kind, [0, 200, 0, 0, 1, 15, 16, 17, 31, 32, 33, 35, 7, 2], 0, device=device)
    if which == 'split_among_isolated':
        return graph_from_lengths(kind, [0, 0, 9, 0, 0], 2, device=device)
    if which == 'no_edges':
        triples = np.zeros((0, 3), np.int64)
    else:
        k = 4 if kind == 'gat' else 3
        triples = np.asarray([(u, 0 if kind == 'gat' else q, i) for u in range(k) for q in range(1 if kind == 'gat' else k) for i in range(k)], np.int64)
    U, Q, I = (4, 1, 4) if kind == 'gat' else (3, 3, 3)
    with heavy_chunk(2):
        if kind == 'gat':
            g = graph_of('gat', PairLayout(triples, U, Q, I, device, completeness='ui', heavy_threshold=2), chunk=2)
        else:
            g = graph_of('phase2', IncidenceLayout(triples, U, Q, I, device, heavy_threshold=2, edge_multiplicity='0', compact_nodes='0'), chunk=2)
    lens = np.diff(g.ptr)
    if which == 'only_split':
        assert g.csr.n_heavy == int((lens > 0).sum()) > 0
    else:
        assert len(g.ids) == 0 and g.csr.n_heavy == 0
    return g


def on_device(case, device):
    return Case(*[t.to(device) if torch.is_tensor(t) else t for t in case])


def zero_weight_case(g, head, d, rng):
    """Integer features and cotangent at width d, a zero attention vector and c = 1: every score is act(1) = 1 (the ``equal`` design at a real width) and
    ``d alpha`` is an exact dot of integers."""
    case = integer_case(g, head, d, rng)
    return case._replace(w=torch.zeros_like(case.w), c=_f32([1.0]))


def short_rows_graph(kind, n_hubs, per_row, threshold, device=CPU, pool=1000):
    """``n_hubs`` hub rows of ``per_row(r)`` (1 ... 4) entries each, built without a Python loop: the graphs of the second grid-stride trips."""
    from ihgnn_amd.layout import IncidenceLayout, PairLayout
    lens = np.asarray(per_row(np.arange(n_hubs)), np.int64)
    r = np.repeat(np.arange(n_hubs), lens)
    j = np.arange(len(r)) - np.repeat(np.cumsum(lens) - lens, lens)
    big = 1 << 30
    with heavy_chunk(2):
        if kind == 'gat':
            triples = np.stack([r, np.zeros_like(r), (7 * r + j) % pool], 1)             # (consecutive residues: distinct inside a row)
            lay = PairLayout(triples, n_hubs, 1, pool, device, completeness='ui', heavy_threshold=threshold or big)
            return graph_of('gat', lay, np.arange(n_hubs), lens, 2)
        triples = np.stack([(5 * r + j) % pool, r, (3 * r + 2 * j) % pool], 1)
        lay = IncidenceLayout(triples, pool, n_hubs, pool, device, heavy_threshold=threshold or big, edge_multiplicity='0', compact_nodes='0')
        return graph_of('phase2', lay, pool + np.arange(n_hubs), lens, 2)
