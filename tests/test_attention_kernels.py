"""The attention launches of ``csrc/gat.hip`` and ``csrc/phase2.hip`` (kernels of ``csrc/attention.hpp``), each on its own through the C ABI:
``ihg_gat_attention_fwd``, ``ihg_phase2_attention_fwd``, ``ihg_gat_scores_bwd``, ``ihg_phase2_scores_bwd``, ``ihg_gat_symmetrize``, ``ihg_phase2_edges_bwd``.

Their outputs - ``z``, ``alpha``, ``alpha_mirror`` / ``alpha_edge``, ``ds``, ``ds_edge``, ``node_sums``, the hyperedge gradient, ``ds + ds[mirror]`` - are held PER ENTRY
over ladders of split rows (2 ... 1,025 segments: around one lane group, one wave and one workgroup of partials, up to five trips of the finish kernels' thread
loop), over light rows at the lane boundaries of the row gather-dot at every width and geometry, over the second grid-stride trip of every pass, and over the
degenerate plans.  The graphs, the score designs, the float64 references and every bound are in ``tests/attention_reference.py``, where each bound is derived;
``tests/test_attention_host.py`` holds a float32 emulation of the kernels' scheme to the same verdicts on the same cases, so a failing case here is a wrong kernel.
Every written tensor is a view into a sentinel-filled buffer with guards in front and behind, pre-filled with NaN where every entry must be written; every source
is compared with its copy after the launch; the workspace is exactly as long as the library asks, with a guard behind it."""
import numpy as np
import pytest
import torch

import aggregate_reference as AR
import attention_reference as R
from test_aggregate_kernels import SENTINEL, Padded
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

GUARD = 64                               # sentinel floats in front of and behind every 1-D payload (a multiple of 4: the payload stays 16-byte aligned)
NAN = float('nan')


def _rng(*key):
    return np.random.default_rng([ord(k) if isinstance(k, str) else int(k) for k in key])


class Guarded:
    """An ``[n]`` float32 view into a sentinel-filled buffer; the payload pre-filled with ``fill`` (NaN: every entry must come back written)."""

    def __init__(self, n, fill=NAN):
        self.n = int(n)
        self.buf = torch.full((GUARD + max(self.n, 1) + GUARD,), SENTINEL, dtype=torch.float32, device=dev())
        self.view = self.buf[GUARD:GUARD + self.n]
        self.view.fill_(fill)
        self.arg = self.buf[GUARD:]                                        # the payload's address (an empty view of torch's has a null pointer)
        self.before = self.buf.clone()

    def assert_guards(self, what):
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all()), f'{what}: memory around an output was written'

    def assert_untouched(self, what):
        assert torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32)), f'{what}: written where nothing should be'


class Source:
    """A small device tensor (weights, bias, indices, a previous launch's output) and its copy."""

    def __init__(self, t):
        if t.numel() == 0:                                                 # (a graph without edges: something to point at)
            t = torch.zeros(4, dtype=t.dtype)
        self.t = t.to(dev()).contiguous()
        self.before = self.t.clone()

    def assert_unchanged(self, what):
        a, b = (x.view(torch.int32) if x.dtype == torch.float32 else x for x in (self.t, self.before))
        assert torch.equal(a, b), f'{what}: a source was written'


def _tables(g):
    """(rowptr, ids, mirror / pos, row_order) of the layout, on the device."""
    lay = g.layout
    if len(g.ids) == 0:                                                    # (an empty torch tensor has a null pointer: the entry points ask for a real one)
        nothing = torch.zeros(4, dtype=torch.int32, device=dev())
        return g.csr.ptr, nothing, nothing, g.csr.row_order
    return g.csr.ptr, g.csr.ids, (lay.mirror if g.kind == 'gat' else lay.member_csr.ids), g.csr.row_order


def _workspace(g, dim, head):
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    if g.kind == 'gat':
        n_bytes = int(lib.ihg_gat_workspace_bytes(g.n_rows, g.csr.n_segments, dim, ops.GAT_HEADS[head]))
    else:
        n_bytes = int(lib.ihg_phase2_workspace_bytes(g.n_rows, g.n_src, g.csr.n_segments, dim, ops.GAT_HEADS[head]))
    assert n_bytes > 0 and n_bytes % 4 == 0
    return Guarded(n_bytes // 4, fill=-7.0), n_bytes


class Forward:
    """One forward launch of ``case`` on ``g``: ``z``, ``alpha`` and the second table's copy, with every guard and source checked."""

    def __init__(self, g, case, act, geometry='a', what=''):
        from ihgnn_amd import _lib, ops
        lib = _lib.load()
        self.g, self.case, self.act, self.what = g, case, act, what
        nnz, dim = len(g.ids), case.x.shape[1]
        self.x = Padded(case.x, geometry)
        self.h = self.x if g.kind == 'gat' else Padded(case.h, geometry)
        self.w, self.c = Source(case.w), Source(case.c)
        self.z, self.alpha, self.copy = Guarded(nnz), Guarded(nnz), Guarded(nnz)
        ws, ws_bytes = _workspace(g, dim, case.head)
        ptr, ids, table, order = _tables(g)
        head, code = ops.GAT_HEADS[case.head], ops.GAT_ACTIVATIONS[act]
        outs = (ops._ptr(self.z.arg), ops._ptr(self.alpha.arg), ops._ptr(self.copy.arg), ops._ptr(ws.arg), ws_bytes, ops._stream())
        if g.kind == 'gat':
            rc = lib.ihg_gat_attention_fwd(ops._ptr(self.x.view), int(self.x.view.stride(0)), ops._ptr(ptr), ops._ptr(ids), ops._ptr(table), ops._ptr(order), g.n_rows, dim,
                                           ops._ptr(self.w.t), ops._ptr(self.c.t), head, code, *ops._split_row_args(g.csr), *outs)
        else:
            rc = lib.ihg_phase2_attention_fwd(ops._ptr(self.h.view), int(self.h.view.stride(0)), ops._ptr(self.x.view), int(self.x.view.stride(0)), ops._ptr(ptr),
                                              ops._ptr(ids), ops._ptr(table), ops._ptr(order), g.n_rows, g.n_src, dim, ops._ptr(self.w.t), ops._ptr(self.c.t),
                                              ops._ptr(g.layout.edge_weight), head, code, *ops._split_row_args(g.csr), *outs)
        torch.cuda.synchronize()
        assert rc == _lib.OK, f'{what}: forward launch returned {rc}'
        for out in (self.z, self.alpha, self.copy, ws):
            out.assert_guards(what)
        for src in (self.x, self.h, self.w, self.c):
            src.assert_unchanged(what)
        if nnz == 0:
            return
        assert bool(torch.isfinite(self.z.view).all()) and bool(torch.isfinite(self.alpha.view).all()) and bool(torch.isfinite(self.copy.view).all()), \
            f'{what}: an entry of z, alpha or the second table was not written'
        assert torch.equal(self.copy.view[table.long()].view(torch.int32), self.alpha.view.view(torch.int32)), f'{what}: the second table is not alpha at its slots'

    def outputs(self, device=None):
        return tuple(t.view.to(device or 'cpu') for t in (self.z, self.alpha))

    def check(self, design, hold_alpha=True, device=None):
        case = self.case if device is None else R.on_device(self.case, device)
        z, alpha = self.outputs(device)
        return R.check_forward(self.g, case, self.act, design, z, alpha, self.what, hold_alpha)


class Backward:
    """``ihg_gat_scores_bwd`` / ``ihg_phase2_scores_bwd`` on the ``z`` and ``alpha`` a forward launch stored."""

    def __init__(self, fwd, geometry='a'):
        from ihgnn_amd import _lib, ops
        lib = _lib.load()
        g, case, what = fwd.g, fwd.case, fwd.what
        self.fwd = fwd
        nnz, dim = len(g.ids), case.x.shape[1]
        self.dout = Padded(case.dout, geometry)
        z, alpha = Source(fwd.z.view), Source(fwd.alpha.view)
        self.ds, self.ds_edge, self.node_sums = Guarded(nnz), Guarded(nnz), Guarded(2 * g.n_rows, fill=SENTINEL)
        ws, ws_bytes = _workspace(g, dim, case.head)
        ptr, ids, table, order = _tables(g)
        head, code = ops.GAT_HEADS[case.head], ops.GAT_ACTIVATIONS[fwd.act]
        x = fwd.x
        if g.kind == 'gat':
            rc = lib.ihg_gat_scores_bwd(ops._ptr(x.view), int(x.view.stride(0)), ops._ptr(self.dout.view), int(self.dout.view.stride(0)), ops._ptr(ptr), ops._ptr(ids),
                                        ops._ptr(table), ops._ptr(order), g.n_rows, dim, head, code, *ops._split_row_args(g.csr), ops._ptr(z.t), ops._ptr(alpha.t),
                                        ops._ptr(self.ds.arg), ops._ptr(self.node_sums.arg), ops._ptr(ws.arg), ws_bytes, ops._stream())
        else:
            rc = lib.ihg_phase2_scores_bwd(ops._ptr(x.view), int(x.view.stride(0)), ops._ptr(self.dout.view), int(self.dout.view.stride(0)), ops._ptr(ptr), ops._ptr(ids),
                                           ops._ptr(table), ops._ptr(order), g.n_rows, g.n_src, dim, head, code, *ops._split_row_args(g.csr), ops._ptr(z.t),
                                           ops._ptr(alpha.t), ops._ptr(self.ds.arg), ops._ptr(self.ds_edge.arg), ops._ptr(self.node_sums.arg), ops._ptr(ws.arg),
                                           ws_bytes, ops._stream())
        torch.cuda.synchronize()
        assert rc == _lib.OK, f'{what}: backward launch returned {rc}'
        for out in (self.ds, self.ds_edge, self.node_sums, ws):
            out.assert_guards(what)
        for src in (x, self.dout, z, alpha):
            src.assert_unchanged(what)
        sums = self.node_sums.view.view(g.n_rows, 2)
        self.S = sums[:, 1]
        self.src_sums = sums[:, 0] if g.kind == 'gat' and case.head == 'concatenation' else None
        if self.src_sums is None:
            assert bool((sums[:, 0] == SENTINEL).all()), f'{what}: node_sums[:, 0] was written'
        if g.kind == 'gat':
            self.ds_edge.assert_untouched(what)
        elif nnz:
            assert torch.equal(self.ds_edge.view[table.long()].view(torch.int32), self.ds.view.view(torch.int32)), f'{what}: ds_edge is not ds at its slots'

    def check(self, design, device=None):
        fwd = self.fwd
        device = device or 'cpu'
        case = fwd.case if device == 'cpu' else R.on_device(fwd.case, device)
        z, alpha = fwd.outputs(device)
        src = None if self.src_sums is None else self.src_sums.to(device)
        return R.check_backward(fwd.g, case, fwd.act, design, z, alpha, self.ds.view.to(device), self.S.to(device), src, fwd.what)


def _same(a, b, what):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f'{what}: two launches differ'


def _symmetrize(g, ds):
    """``ihg_gat_symmetrize`` on its own: ``(ds + ds[mirror])`` from the launch."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    src, out = Source(ds), Guarded(len(g.ids))
    mirror = Source(g.layout.mirror)
    assert lib.ihg_gat_symmetrize(ops._ptr(src.t), ops._ptr(mirror.t), len(g.ids), ops._ptr(out.arg), ops._stream()) == _lib.OK
    torch.cuda.synchronize()
    out.assert_guards('symmetrize')
    src.assert_unchanged('symmetrize')
    mirror.assert_unchanged('symmetrize')
    return out.view


def _edges_bwd(g, dim, head, geometry, exact, rng, what):
    """``ihg_phase2_edges_bwd`` on its own: integer rows and weights with power-of-two ``alpha_edge`` / ``ds_edge`` (exact), or ``randn`` (held to the bound)."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    n, e = g.n_rows, g.n_src
    if exact:
        dout_cpu, h_cpu = R._f32(rng.integers(-4, 5, (n, dim))), R._f32(rng.integers(-4, 5, (n, dim)))
        w_cpu = R._f32(rng.integers(-2, 3, 2 * dim if head == 'concatenation' else dim))
        al_cpu = R._f32(rng.choice([1.0, 2.0, 4.0], 3 * e))
        s_cpu = R._f32(rng.choice([-2.0, -1.0, 1.0, 2.0], 3 * e))
    else:
        dout_cpu, h_cpu = R._f32(rng.standard_normal((n, dim))), R._f32(rng.standard_normal((n, dim)))
        w_cpu = R._f32(rng.standard_normal(2 * dim if head == 'concatenation' else dim))
        al_cpu, s_cpu = R._f32(rng.random(3 * e)), R._f32(rng.standard_normal(3 * e))
    i3_cpu = torch.from_numpy(g.layout.i3_host.astype(np.int32)).reshape(-1, 3)
    want, mag = R.edges_bwd64(dout_cpu, h_cpu, i3_cpu, al_cpu, s_cpu, w_cpu, head)
    dout, h, out = Padded(dout_cpu, geometry), Padded(h_cpu, geometry), Padded((e, dim), geometry)
    out.view.fill_(NAN)
    out.before = out.buf.clone()
    w, al, s, i3 = Source(w_cpu), Source(al_cpu), Source(s_cpu), Source(i3_cpu)
    rc = lib.ihg_phase2_edges_bwd(ops._ptr(dout.view), int(dout.view.stride(0)), ops._ptr(h.view), int(h.view.stride(0)), ops._ptr(i3.t), ops._ptr(al.t), ops._ptr(s.t),
                                  ops._ptr(w.t), ops.GAT_HEADS[head], e, dim, ops._ptr(out.view), int(out.view.stride(0)) if e else dim, ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.OK, what
    out.assert_guards(what)
    for src in (dout, h, w, al, s, i3):
        src.assert_unchanged(what)
    got = out.view.cpu()
    if exact:
        R.assert_exact_condition(mag, what)
        R.assert_equal(got, want, f'{what}: hyperedge gradient')
        return 0.0
    return R.assert_within(got, want, R.EDGES_BWD_ROUNDINGS * R.EPS * mag, what, 'hyperedge gradient')


# =============================================================================================
# ladders of split rows
# =============================================================================================
@pytest.mark.parametrize('kind,chunk,repeated', R.LADDER_GRAPHS)
@pytest.mark.parametrize('head', R.HEADS)
@pytest.mark.parametrize('act', R.ACTS)
def test_ladder_forward(kind, chunk, repeated, head, act):
    """Every score design on a ladder: ``z`` equal to (integer designs) or within its bound of the float64 scores, ``alpha`` per entry within its relative bound of
    the float64 softmax of the stored ``z``; ``equal``: one float from m / sum m; ``one_hot``: exactly 1; two launches bitwise equal."""
    g = R.ladder(kind, chunk, repeated, dev())
    counts = R.assert_ladder(g)
    assert set(R.LADDERS[chunk]) <= set(counts)
    for design in R.ladder_designs(head, act):
        what = f'{kind} chunk {chunk} repeated {repeated} {head} {act} {design} forward'
        case = R.design_case(g, design, head)
        first, second = Forward(g, case, act, what=what), Forward(g, case, act, what=what)
        _same((first.z.view, first.alpha.view, first.copy.view), (second.z.view, second.alpha.view, second.copy.view), what)
        first.check(design)


@pytest.mark.parametrize('kind,chunk,repeated', R.LADDER_GRAPHS)
@pytest.mark.parametrize('head', R.HEADS)
@pytest.mark.parametrize('act', R.ACTS)
def test_ladder_backward(kind, chunk, repeated, head, act):
    """``ds`` per entry, ``node_sums`` per row within their bounds of the float64 softmax backward of the stored ``alpha`` and ``z``; ``equal``: ds exact on the rows of
    power-of-two length and the row sums +-0; ``ds_edge`` bitwise ``ds`` at its slots; ``ihg_gat_symmetrize`` exact on integers; two launches bitwise equal."""
    g = R.ladder(kind, chunk, repeated, dev())
    for design in R.ladder_designs(head, act, backward=True):
        what = f'{kind} chunk {chunk} repeated {repeated} {head} {act} {design} backward'
        fwd = Forward(g, R.design_case(g, design, head), act, what=what)
        first, second = Backward(fwd), Backward(fwd)
        _same((first.ds.view, first.ds_edge.view, first.node_sums.view), (second.ds.view, second.ds_edge.view, second.node_sums.view), what)
        first.check(design)
    if kind == 'gat':
        ints = torch.from_numpy(_rng(1, chunk).integers(-1000, 1001, len(g.ids)).astype(np.float32))
        R.assert_equal(_symmetrize(g, ints).cpu(), R.symmetrize64(g, ints), 'symmetrize on the ladder')
    elif act == 'leaky_relu':
        _edges_bwd(g, 8, head, 'a', True, _rng(2, chunk), f'edges_bwd on the ladder, {head}')


# =============================================================================================
# light rows at the lane boundaries of the row gather-dot, every width and geometry
# =============================================================================================
WIDE = (8, 16, 32, 64, 128, 256, 320)    # 16-byte path in geometries a, b: G = 4 (idle lanes), 4, 8, 16, 32, 64, 64 with a second column chunk
NARROW = (3, 30, 100)                    # 4-byte path: G = 4, 32, 64 with a second column chunk


@pytest.mark.parametrize('geometry', AR.GEOMETRIES)
@pytest.mark.parametrize('dim', WIDE + NARROW)
def test_light_rows_every_width_and_geometry(dim, geometry):
    """Row lengths 0, 1, G - 1, G, G + 1, 7 ... 9, 15 ... 17, 2 G + 3, 200 for the row gather-dot's G at this width and geometry, ``h``, ``ef``, ``dout`` and the
    hyperedge-gradient output in geometry a - d.  Integer inputs: ``z`` EQUALS the float64 scores under both heads (product head: the gather-dot; concatenation:
    the projections); with a zero attention vector the scores are equal, and ``ds`` - hence ``d alpha``, the gather-dot of the backward - is exact on the rows of
    power-of-two length and 0 on the rows of length 1; ``ihg_phase2_edges_bwd`` is exact.  In geometry a one float case per head is held to the bounds."""
    lanes = AR.group_lanes(dim, AR.vec_of(dim, geometry))
    rng = _rng(3, dim, geometry)
    lengths = AR.light_lengths(lanes, rng)
    for kind in ('gat', 'phase2'):
        g = R.graph_from_lengths(kind, lengths, 0, device=dev(), seed=dim)
        assert g.csr.n_heavy == 0 and {1, lanes, 200} <= set(np.diff(g.ptr)[g.hub_rows].tolist())
        for head in R.HEADS:
            what = f'light rows {kind} dim {dim} geometry {geometry} {head}'
            for act in ('leaky_relu', 'relu'):
                Forward(g, R.integer_case(g, head, dim, rng), act, geometry, what + f' integers {act}').check('integer', hold_alpha=False)
            fwd = Forward(g, R.zero_weight_case(g, head, dim, rng), 'leaky_relu', geometry, what + ' zero attention vector')
            fwd.check('equal')
            bwd = Backward(fwd, geometry)
            bwd.check('equal')
            single = torch.from_numpy(np.diff(g.ptr) == 1)[torch.from_numpy(R.row_of(g))]
            assert bool((bwd.ds.view.cpu()[single] == 0).all()), f'{what}: ds of a row of length 1 is not 0'
            if geometry == 'a':
                fwd = Forward(g, R.float_case(g, head, dim, rng), 'tanh' if head == 'product' else 'leaky_relu', geometry, what + ' float')
                fwd.check('float')
                Backward(fwd, geometry).check('float')
            if kind == 'phase2':
                _edges_bwd(g, dim, head, geometry, True, rng, f'edges_bwd dim {dim} geometry {geometry} {head}')
                if geometry == 'a':
                    _edges_bwd(g, dim, head, geometry, False, rng, f'edges_bwd dim {dim} {head} float')


# =============================================================================================
# second grid-stride trips (references on the device)
# =============================================================================================
@pytest.mark.parametrize('kind', ['gat', 'phase2'])
def test_second_trip_of_the_scalar_passes(kind):
    """140,000 rows of 1 ... 3 entries: more units than the 131,072 one grid of the softmax, its backward and the source sums takes in one trip."""
    g = R.short_rows_graph(kind, 140000, lambda r: 1 + r % 3, 0, dev(), pool=100000)
    assert g.n_rows + g.csr.n_segments > R.MAX_SCALAR_UNITS
    what = f'second trip, scalar passes, {kind}'
    fwd = Forward(g, R.float_case(g, 'concatenation', 8, _rng(4)), 'leaky_relu', what=what)
    fwd.check('float', device=dev())
    Backward(fwd).check('float', device=dev())


@pytest.mark.parametrize('kind', ['gat', 'phase2'])
def test_second_trip_of_the_row_gather_dot(kind):
    """40,000 rows at d = 256 on aligned rows (G = 64: one unit per wave, 32,768 per trip): integer inputs, ``z`` exact under the product head; with a zero
    attention vector ``ds`` (rows of 1 and 2 entries: powers of two) is exact, hence so is the backward's gather-dot."""
    g = R.short_rows_graph(kind, 40000, lambda r: 1 + r % 2, 0, dev(), pool=500)
    assert g.n_rows + g.csr.n_segments > R.MAX_ROWDOT_UNITS_G64
    what = f'second trip, row gather-dot, {kind}'
    Forward(g, R.integer_case(g, 'product', 256, _rng(5)), 'relu', what=what).check('integer', hold_alpha=False, device=dev())
    fwd = Forward(g, R.zero_weight_case(g, 'product', 256, _rng(6)), 'leaky_relu', what=what)
    fwd.check('equal', device=dev())
    Backward(fwd).check('equal', device=dev())


@pytest.mark.parametrize('kind', ['gat', 'phase2'])
def test_second_trip_of_the_finish_kernels(kind):
    """9,000 split rows of 4 entries at threshold 2 (and the split rows on the other side of the graph): more than the 8,192 workgroups of a finish launch."""
    g = R.short_rows_graph(kind, 9000, lambda r: 4 + 0 * r, 2, dev())
    assert g.csr.n_heavy > R.MAX_FINISH_ROWS
    what = f'second trip, finish kernels, {kind}'
    fwd = Forward(g, R.float_case(g, 'concatenation', 8, _rng(7)), 'leaky_relu', what=what)
    fwd.check('float', device=dev())
    Backward(fwd).check('float', device=dev())


def test_second_trip_of_symmetrize():
    """nnz = 2,240,000 > 2,097,152 entries of one grid: ``ds + ds[mirror]`` on integers is exact."""
    g = R.short_rows_graph('gat', 280000, lambda r: 4 + 0 * r, 0, dev(), pool=100000)
    assert len(g.ids) > R.MAX_FLAT
    ints = torch.randint(-1000, 1001, (len(g.ids),), generator=torch.Generator().manual_seed(8)).float().to(dev())
    R.assert_equal(_symmetrize(g, ints), R.symmetrize64(g, ints), 'symmetrize, second trip')


def test_second_trip_of_the_edge_slot_copy():
    """3 E = 2,100,600 > 2,097,152 entries at d = 4: ``ds_edge[pos[p]] == ds[p]`` bitwise over every entry (``Backward`` asserts it), ds within its bound."""
    g = R.short_rows_graph('phase2', 233400, lambda r: 3 + 0 * r, 0, dev(), pool=50000)
    assert len(g.ids) > R.MAX_FLAT
    what = 'second trip, edge-slot copy'
    fwd = Forward(g, R.float_case(g, 'concatenation', 4, _rng(9)), 'leaky_relu', what=what)
    fwd.check('float', device=dev())
    Backward(fwd).check('float', device=dev())


# =============================================================================================
# degenerate plans
# =============================================================================================
@pytest.mark.parametrize('kind', ['gat', 'phase2'])
@pytest.mark.parametrize('which', ['no_edges', 'only_split', 'split_among_isolated'])
def test_degenerate_plans(kind, which):
    """No edges at all (every row sum is 0, nothing else is written; phase 2 without hyperedges launches nothing); only split rows; one split row among
    isolated rows."""
    g = R.small_graph(kind, which, dev())
    for head in R.HEADS:
        what = f'{which} {kind} {head}'
        fwd = Forward(g, R.float_case(g, head, 8, _rng(10)), 'leaky_relu', what=what)
        bwd = Backward(fwd)
        if which == 'no_edges' and kind == 'phase2':
            bwd.node_sums.assert_untouched(what)
            continue
        fwd.check('float')
        bwd.check('float')
        empty = torch.from_numpy(np.diff(g.ptr) == 0)
        assert bool((bwd.S.cpu()[empty] == 0).all()), f'{what}: the row sum of a row without entries is not 0'
