"""The matrix-core contractions, each entry point on its own through the C ABI: the interactive layer's hyperedge form (``ihg_interact_fwd``, ``ihg_interact_bwd``,
``ihg_interact_bwd_user_reduced``, ``_user_reduced_planes``, ``ihg_interact_bwd_gathered``), its node-level form (``ihg_node_interact_fwd``,
``ihg_node_interact_bwd_weight``) and the node-level linear maps (``ihg_node_linear_fwd``, ``_bwd_input``, ``_bwd_weight`` and the ``_typed`` pair).

Every output is held PER ELEMENT against a float64 reference of that launch (``tests/contraction_reference.py``): *exact cases* - integer operands, power-of-two
scales, ``sum |terms|`` of every output element checked below 2^24 - with ``torch.equal`` over ladders derived from the kernels' tile sizes and tile ranges, user
runs, node types and rising row magnitudes; *float cases* within ``((K + c) 2^-24 + L) sum |terms|``.  ``tests/test_contraction_host.py`` holds a numpy emulation to
the same verdicts and shows that nine ways of being wrong fail them.  Every written tensor is a view into a sentinel-filled buffer with guard rows in front and
behind and guard columns where ``ld > dim``, NaN where every element must be written; the workspace is exactly as long as the library asks, with a guard behind
it; every source is compared with its copy after the launch."""
import ctypes

import numpy as np
import pytest
import torch

import contraction_reference as R
from test_aggregate_kernels import SENTINEL, Padded
from test_attention_kernels import Guarded, Source
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

NAN = float('nan')
WORST = {}                               # kernel -> worst error / bound of the float cases (printed when the module is done, recorded in DESIGN.md section 5)


def _set_arith(monkeypatch, arith):
    monkeypatch.setenv('IHG_INTERACT_ARITH', 'f32') if arith == 'f32' else monkeypatch.delenv('IHG_INTERACT_ARITH', raising=False)


def _lib_ops():
    from ihgnn_amd import _lib, ops
    return _lib, _lib.load(), ops


def _out(rows, cols, geometry, fill=NAN):
    """An output view [rows, cols] pre-filled with ``fill`` (NaN: every element must be written; None: the sentinel stays)."""
    t = Padded((rows, cols), geometry)
    if fill is not None:
        t.view.fill_(fill)
    t.before = t.buf.clone()
    return t


def _workspace(n_bytes):
    assert n_bytes >= 0 and n_bytes % 4 == 0
    return Guarded(n_bytes // 4, fill=-7.0), n_bytes


def _ld(t):
    return int(t.view.stride(0))


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)


@pytest.fixture(scope='module', autouse=True)
def _report_worst_ratios():
    """After the module's tests: the worst ``error / bound`` per kernel of the float cases that ran (each was asserted where it was measured; shown with ``-s``)."""
    yield
    for name in sorted(WORST):
        print(f'worst error / bound: {name}: {WORST[name]:.3f}')


# =============================================================================================
# the hyperedge form
# =============================================================================================
class EdgeOperands:
    """The sources of one case on the device: ``h``, ``p``, ``w``, ``dout``, ``dy`` as padded views in ``geometry`` ('a' contiguous, 'b' a column slice with
    ``ld % 4 == 0``; both 16-byte aligned), ``i3`` and ``dy_scale`` with their copies."""

    def __init__(self, case, geometry='a'):
        self.case = case
        f = lambda t: t.float()
        self.h, self.p, self.w = Padded(f(case.h), geometry), Padded(f(case.p), geometry), Padded(f(case.w), geometry)
        self.dout, self.dy = Padded(f(case.dout), geometry), Padded(f(case.dy), geometry)
        self.i3, self.dy_scale = Source(case.i3.int()), Source(f(case.dy_scale))
        self.all = (self.h, self.p, self.w, self.dout, self.dy, self.i3, self.dy_scale)

    def assert_unchanged(self, what):
        for src in self.all:
            src.assert_unchanged(what)


def _fwd(x, geometry, what, expect=None):
    _lib, lib, ops = _lib_ops()
    c = x.case
    e, d = len(c.i3), c.dim
    out = _out(e, d, geometry)
    ws, ws_bytes = _workspace(int(lib.ihg_interact_fwd_workspace_bytes(e, d, c.order)))
    rc = lib.ihg_interact_fwd(ops._ptr(x.h.view), _ld(x.h), ops._ptr(x.p.view), _ld(x.p), ops._ptr(x.i3.t), ops._ptr(x.w.view), _ld(x.w), c.order, ops._ptr(out.view), _ld(out),
                              ops._ptr(ws.arg), ws_bytes, e, d, ops._stream())
    torch.cuda.synchronize()
    assert rc == (_lib.OK if expect is None else expect), f'{what}: ihg_interact_fwd returned {rc}: {_lib.last_error()}'
    out.assert_guards(what)
    ws.assert_guards(what)
    x.assert_unchanged(what)
    return out.view


class Backward:
    """One launch of a backward entry: ``g`` [E, 3, d] or ``g2`` [E, 2, d], ``dh`` [n_users, d] (sentinel where nothing must be written), ``dw`` [d, k d] whose
    first-order columns keep the sentinel, the stored ``dout`` of the gathering form."""

    def __init__(self, entry, x, geometry, what, with_dw=True, store_dout=True, planes=None, dout_rows=None, expect=None):
        _lib, lib, ops = _lib_ops()
        c = x.case
        e, d, k = len(c.i3), c.dim, R.weight_columns(c.order)
        self.slots = 3 if entry == 'bwd' else 2
        self.g = _out(e, self.slots * d, 'a')
        self.dh = _out(c.n_users, d, geometry, fill=None)
        self.dw = _out(d, k * d, geometry, fill=None) if with_dw else None
        if with_dw:
            self.dw.view[:, 3 * d:] = NAN
            self.dw.before = self.dw.buf.clone()
        self.dout = _out(e, d, geometry) if entry == 'gathered' and store_dout else None
        ws, ws_bytes = _workspace(int(lib.ihg_interact_bwd_workspace_bytes(e, d, c.order)))
        src = x.dout if dout_rows is None else dout_rows
        common = (ops._ptr(x.h.view), _ld(x.h), ops._ptr(x.i3.t), ops._ptr(x.w.view), _ld(x.w), c.order)
        dw_args = (ops._ptr(self.dw.view) if with_dw else None, _ld(self.dw) if with_dw else 0)
        tail = (ops._ptr(ws.arg), ws_bytes, e, d, ops._stream())
        if entry == 'bwd':
            rc = lib.ihg_interact_bwd(*common, ops._ptr(src.view), _ld(src), ops._ptr(self.g.view), *dw_args, *tail)
        elif entry == 'user_reduced':
            rc = lib.ihg_interact_bwd_user_reduced(*common, ops._ptr(src.view), _ld(src), ops._ptr(self.g.view), ops._ptr(self.dh.view), _ld(self.dh), *dw_args, *tail)
        elif entry == 'planes':
            rc = lib.ihg_interact_bwd_user_reduced_planes(*common, ops._ptr(planes[0].view), ops._ptr(planes[1]), ops._ptr(self.g.view), ops._ptr(self.dh.view), _ld(self.dh), *tail)
        else:
            rc = lib.ihg_interact_bwd_gathered(*common, ops._ptr(x.dy.view), _ld(x.dy), ops._ptr(x.dy_scale.t), ops._ptr(self.dout.view) if self.dout else None,
                                               _ld(self.dout) if self.dout else 0, ops._ptr(self.g.view), ops._ptr(self.dh.view), _ld(self.dh), *dw_args, *tail)
        torch.cuda.synchronize()
        assert rc == (_lib.OK if expect is None else expect), f'{what}: {entry} returned {rc}: {_lib.last_error()}'
        self.outputs = [t for t in (self.g, self.dh, self.dw, self.dout) if t is not None]
        for t in self.outputs:
            t.assert_guards(what)
        ws.assert_guards(what)
        x.assert_unchanged(what)
        if dout_rows is not None:
            dout_rows.assert_unchanged(what)
        if expect is not None:
            for t in self.outputs + [ws]:
                t.assert_untouched(what)
            return
        if entry == 'bwd':
            self.dh.assert_untouched(what)
        if with_dw:
            assert bool((self.dw.view[:, :3 * d] == SENTINEL).all()), f'{what}: the first-order columns of dw were written'

    def bits(self):
        return [t.view.clone() for t in self.outputs]


def _check_backward(entry, b, x, exact, arithmetic, what):
    """Every output of a backward launch against the float64 reference: ``torch.equal`` (exact) or the per-element bound (returns nothing; notes the worst ratio)."""
    c = x.case
    d, e = c.dim, len(c.i3)
    gathered = entry in ('gathered', 'planes')                           # the hyperedges' cotangents are sums of three scaled rows of dy
    shared = c.reference                                                 # one reference per case, shared by the call forms
    if gathered not in shared:
        dout, dout_mag = R.gathered_dout64(c) if gathered else (None, None)
        want = R.bwd64(c, dout, dout_mag)
        if exact:
            for name in ('g_mag', 'dh_mag', 'dw_mag') + (('dout_mag',) if gathered else ()):
                R.ensure_exact(dout_mag if name == 'dout_mag' else want[name], 0.5 if gathered else 1.0, f'{what} {name}')
        shared[gathered] = (dout, dout_mag, want)
    dout, dout_mag, want = shared[gathered]
    g_name = 'g' if entry == 'bwd' else 'g2'
    got_g = b.g.view.view(e, b.slots, d)
    users = c.i3[:, 0].long()
    has = want['has_edges']
    assert bool((b.dh.view[~has] == SENTINEL).all()) or entry == 'bwd', f'{what}: the dh row of a user without hyperedges was written'
    if exact:
        R.assert_equal(got_g, want[g_name], f'{what}: {g_name}')
        if gathered and b.dout is not None:
            R.assert_equal(b.dout.view, dout, f'{what}: stored dout')
        if entry != 'bwd':
            R.assert_equal(b.dh.view[has], want['dh'][has], f'{what}: dh')
        if b.dw is not None:
            R.assert_equal(b.dw.view[:, 3 * d:], want['dw'], f'{what}: dw')
        return
    nb_g = 3 if c.order == 3 else 2
    _note(f'members {entry} d={d} {arithmetic}', R.assert_within(got_g, want[g_name], R.float_bound('members', nb_g * d, want[g_name + '_mag'], arithmetic, gathered), f'{what}: {g_name}'))
    if gathered and b.dout is not None:
        _note(f'gathered dout d={d}', R.assert_within(b.dout.view, dout, R.float_bound('gathered_dout', 3, dout_mag, 'f32'), f'{what}: stored dout'))
    if entry != 'bwd':
        run = torch.bincount(users, minlength=c.n_users).double()[:, None]
        bound = R.float_bound('dh', run * nb_g * d, want['dh_mag'], arithmetic, gathered)
        _note(f'user sums {entry} d={d} {arithmetic}', R.assert_within(b.dh.view[has], want['dh'][has], bound[has], f'{what}: dh'))
    if b.dw is not None:
        _note(f'weights {entry} d={d} {arithmetic}', R.assert_within(b.dw.view[:, 3 * d:], want['dw'], R.float_bound('dw', e, want['dw_mag'], arithmetic, gathered), f'{what}: dw'))


def _edge_case(*args, **kw):
    return R.edge_case(*args, **kw).to(dev())


def _magnitude(entry):
    """Operands in [-m, m]: 4, or 2 where the hyperedges' cotangents are sums of three scaled rows (so that ``sum |terms|`` of dw stays under the cap at 65 k hyperedges)."""
    return 2 if entry in ('gathered', 'planes') else 4


def _planes_of(x, what):
    """The cotangent rows of a case from its ``dy`` twice: fp32 rows from ``ihg_edge_gather_sum`` and fp16 planes + inverse scales from ``ihg_edge_gather_sum_planes``."""
    _lib, lib, ops = _lib_ops()
    c = x.case
    e, d = len(c.i3), c.dim
    rows, planes = _out(e, d, 'a'), _out(e, d, 'a')
    inv = torch.full((8 + e + 8,), SENTINEL, dtype=torch.float32, device=dev())
    assert lib.ihg_edge_gather_sum(ops._ptr(x.dy.view), _ld(x.dy), ops._ptr(x.i3.t), ops._ptr(x.dy_scale.t), None, 1.0, None, ops._ptr(rows.view), d, e, d, ops._stream()) == _lib.OK, what
    assert lib.ihg_edge_gather_sum_planes(ops._ptr(x.dy.view), _ld(x.dy), ops._ptr(x.i3.t), ops._ptr(x.dy_scale.t), None, ops._ptr(planes.view), ops._ptr(inv[8:]), e, d,
                                          ops._stream()) == _lib.OK, what
    torch.cuda.synchronize()
    rows.before, planes.before = rows.buf.clone(), planes.buf.clone()
    assert bool((inv[:8] == SENTINEL).all()) and bool((inv[8 + e:] == SENTINEL).all())
    return rows, (planes, inv[8:8 + e])


def _run_entry(entry, x, geometry, exact, arithmetic, what):
    """One case through one entry in every call form the entry has."""
    c = x.case
    if entry == 'fwd':
        want, mag = R.fwd64(c)
        got = _fwd(x, geometry, what)
        if exact:
            R.ensure_exact(mag, 1.0, what)
            R.assert_equal(got, want, f'{what}: out')
        else:
            k = 3 + R.product_blocks(c.order) * c.dim
            _note(f'fwd d={c.dim} {arithmetic}', R.assert_within(got, want, R.float_bound('fwd', k, mag, arithmetic), f'{what}: out'))
    elif entry in ('bwd', 'user_reduced'):
        _check_backward(entry, Backward(entry, x, geometry, what), x, exact, arithmetic, what)
        _check_backward(entry, Backward(entry, x, geometry, what + ' dw == NULL', with_dw=False), x, exact, arithmetic, what + ' dw == NULL')
    elif entry == 'gathered':
        _check_backward(entry, Backward(entry, x, geometry, what), x, exact, arithmetic, what)
        _check_backward(entry, Backward(entry, x, geometry, what + ' dw == NULL', with_dw=False), x, exact, arithmetic, what + ' dw == NULL')
        _check_backward(entry, Backward(entry, x, geometry, what + ' dw == dout == NULL', with_dw=False, store_dout=False), x, exact, arithmetic, what + ' dw == dout == NULL')
    else:
        rows, planes = _planes_of(x, what)
        from_planes = Backward('planes', x, geometry, what, with_dw=False, planes=planes)
        from_rows = Backward('user_reduced', x, geometry, what + ' (fp32 rows)', with_dw=False, dout_rows=rows)
        for a, b in zip(from_planes.bits(), from_rows.bits()):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: the planes entry and the fp32-row call differ in a bit'
        _check_backward('planes', from_planes, x, exact, arithmetic, what)


EDGE_INSTANCES = [(entry, dim, arith) for entry in R.ENTRIES for dim in R.MFMA_DIMS + R.SCALAR_DIMS for arith in R.ARITHS
                  if R.edge_launch(entry, dim, 3, arith)['supported'] and not (dim in R.SCALAR_DIMS + (32,) and arith == 'f32')]     # (d = 8, 12, 32: one set of kernels in either mode)


def test_supported_answers_match_the_launch_table(monkeypatch):
    """``*_supported`` in both arithmetic modes at every width against ``contraction_reference.edge_launch`` / ``node_launch`` / ``node_linear_accumulates``."""
    _lib, lib, ops = _lib_ops()
    for arith in R.ARITHS:
        _set_arith(monkeypatch, arith)
        for dim in R.MFMA_DIMS + R.SCALAR_DIMS:
            for order in R.ORDERS:
                where = (arith, dim, order)
                assert bool(lib.ihg_interact_bwd_user_reduced_supported(dim, order, dim)) == R.edge_launch('user_reduced', dim, order, arith)['supported'], where
                assert bool(lib.ihg_interact_bwd_user_reduced_planes_supported(dim, order, dim)) == R.edge_launch('planes', dim, order, arith)['supported'], where
                assert bool(lib.ihg_interact_bwd_gathered_supported(dim, order, dim, dim)) == R.edge_launch('gathered', dim, order, arith)['supported'], where
                if dim in R.MFMA_DIMS:
                    assert bool(lib.ihg_node_interact_fwd_supported(dim, order, dim, 3 * dim, dim)) == R.node_launch('fwd', dim, arith)['supported'], where
                    assert bool(lib.ihg_node_interact_bwd_weight_supported(dim, order, dim, 3 * dim, dim)) == R.node_launch('weight', dim, arith)['supported'], where
            if dim in R.MFMA_DIMS:
                assert bool(lib.ihg_node_linear_bwd_accumulates(dim, dim, dim, dim)) == R.node_linear_accumulates(dim, arith), (arith, dim)


@pytest.mark.parametrize('order', R.ORDERS)
@pytest.mark.parametrize('entry,dim,arith', EDGE_INSTANCES)
def test_edge_ladder_exact(entry, dim, arith, order, monkeypatch):
    """Hyperedge counts 1, TE - 1, TE, TE + 1, RANGES TE - 1, RANGES TE, RANGES TE + 1, (2 RANGES + 1) TE + 5 of every kernel behind the entry: every output
    element EQUALS the float64 reference; outputs alternate between contiguous rows and column slices of a wider buffer."""
    _set_arith(monkeypatch, arith)
    for k, n_edges in enumerate(R.edge_ladder(entry, dim, order, arith)):
        geometry = 'ab'[k % 2]
        what = f'{entry} d={dim} order {order} {arith} E={n_edges} geometry {geometry}'
        x = EdgeOperands(_edge_case(n_edges, dim, order, ('ladder', entry, dim, order, n_edges), m=_magnitude(entry)), geometry)
        _run_entry(entry, x, geometry, True, R.edge_launch(entry, dim, order, arith)['arithmetic'], what)


UR_INSTANCES = [(entry, dim, arith) for entry, dim, arith in EDGE_INSTANCES if entry in ('user_reduced', 'planes', 'gathered')]


@pytest.mark.parametrize('order', R.ORDERS)
@pytest.mark.parametrize('entry,dim,arith', UR_INSTANCES)
def test_user_runs_exact(entry, dim, arith, order, monkeypatch):
    """The user-run ladder of ``contraction_reference.user_runs`` for the entry's member-gradient kernel (a range that is one run, a run through three ranges, runs that
    end and start on a range's edge, runs of TE - 1, TE, TE + 1, users with one hyperedge, users without any at the start, between runs and at the end, five hyperedges
    whose query and item are one and the same node row), then every user with one hyperedge and one user owning everything (operands in [-1, 1]): ``dh`` EQUALS the float64 sums, rows of
    users without hyperedges keep the sentinel."""
    _set_arith(monkeypatch, arith)
    launch = R.edge_launch(entry, dim, order, arith)
    members = launch['kernels'][0]
    runs = R.user_runs(members)
    n_edges = len(runs['users'])
    for name, layout, m in (('ladder', (runs['users'], runs['n_users']), 4), ('singles', R.run_layout('singles', n_edges), 4), ('one', R.run_layout('one', n_edges), 1)):
        what = f'{entry} d={dim} order {order} {arith} user runs: {name}'
        case = _edge_case(n_edges, dim, order, ('runs', entry, dim, order, name), m=min(m, _magnitude(entry)), layout=layout)
        if name == 'ladder':
            b, e = runs['same_rows']
            case.i3[b:e, 1:] = case.i3[b, 1]                                  # the same node row as query AND item of five neighbouring hyperedges
        x = EdgeOperands(case, 'a')
        _run_entry(entry, x, 'b' if name == 'ladder' else 'a', True, launch['arithmetic'], what)


@pytest.mark.parametrize('entry,dim,arith', EDGE_INSTANCES)
def test_edge_float(entry, dim, arith, monkeypatch):
    """Per kernel instance and order: one ``randn`` case (scales in [0.5, 1.5)), and for EACH operand split among the launch's kernels (the launch table records it
    per kernel: three bf16 terms in the forward and the weight gradient, two fp16 terms in the member gradients) one case whose every operand is that split's
    adversarial significand (``split_emulation.worst_*``), all positive, under a power of two; the fp32-MFMA and scalar launches get the significand with every low
    bit set.  Per element within ``((K + c) 2^-24 + L) sum |terms|``."""
    _set_arith(monkeypatch, arith)
    for order in R.ORDERS:
        launch = R.edge_launch(entry, dim, order, arith)
        for design in R.float_designs(launch):
            what = f'{entry} d={dim} order {order} {arith} float {design}'
            x = EdgeOperands(R.float_case(entry, dim, order, arith, design).to(dev()), 'a')
            _run_entry(entry, x, 'a', False, launch['arithmetic'], what)


@pytest.mark.parametrize('entry', ['user_reduced', 'planes', 'gathered'])
def test_refused_geometries_write_nothing(entry, monkeypatch):
    """Every (d, arithmetic mode) the launch table says the entry does not cover: ``IHG_ERR_INVALID``, every output and the workspace untouched."""
    _lib, lib, ops = _lib_ops()
    refused = 0
    for arith in R.ARITHS:
        _set_arith(monkeypatch, arith)
        for dim in R.MFMA_DIMS + R.SCALAR_DIMS:
            if R.edge_launch(entry, dim, 3, arith)['supported']:
                continue
            refused += 1
            what = f'{entry} d={dim} {arith} refused'
            x = EdgeOperands(_edge_case(70, dim, 3, ('refused', dim)), 'a')
            if entry == 'planes':
                planes = (_out(70, dim, 'a'), torch.ones(70, device=dev()))
                Backward(entry, x, 'a', what, with_dw=False, planes=planes, expect=_lib.ERR_INVALID)
            else:
                Backward(entry, x, 'a', what, expect=_lib.ERR_INVALID)
    assert refused >= 3


# =============================================================================================
# the node-level form
# =============================================================================================
def _tb(type_begin):
    return (ctypes.c_int64 * 4)(*type_begin)


class NodeOperands:
    def __init__(self, case, geometry='a'):
        self.case = case
        f = lambda t: t.float()
        self.h, self.sums, self.dy, self.w = Padded(f(case.h), geometry), Padded(f(case.sums), geometry), Padded(f(case.dy), geometry), Padded(f(case.w), geometry)
        self.degree, self.scale, self.bias = Source(f(case.degree)), Source(f(case.scale)), Source(f(case.bias))
        self.all = (self.h, self.sums, self.dy, self.w, self.degree, self.scale, self.bias)

    def assert_unchanged(self, what):
        for src in self.all:
            src.assert_unchanged(what)


def _node_fwd(x, geometry, what, use_scale=True, use_bias=True, expect=None):
    _lib, lib, ops = _lib_ops()
    c = x.case
    out = _out(c.n, c.dim, geometry)
    ws, ws_bytes = _workspace(int(lib.ihg_node_interact_fwd_workspace_bytes(c.dim)))
    rc = lib.ihg_node_interact_fwd(ops._ptr(x.h.view), _ld(x.h), ops._ptr(x.sums.view), _ld(x.sums), ops._ptr(x.degree.t), ops._ptr(x.scale.t) if use_scale else None,
                                   ops._ptr(x.bias.t) if use_bias else None, ops._ptr(x.w.view), _ld(x.w), c.order, _tb(c.type_begin), ops._ptr(out.view), _ld(out),
                                   ops._ptr(ws.arg), ws_bytes, c.dim, ops._stream())
    torch.cuda.synchronize()
    assert rc == (_lib.OK if expect is None else expect), f'{what}: ihg_node_interact_fwd returned {rc}: {_lib.last_error()}'
    out.assert_guards(what)
    ws.assert_guards(what)
    x.assert_unchanged(what)
    if expect is not None:
        out.assert_untouched(what)
        ws.assert_untouched(what)
    return out.view


def _node_weight(x, geometry, what, use_scale=True, expect=None):
    _lib, lib, ops = _lib_ops()
    c = x.case
    d, k = c.dim, R.weight_columns(c.order)
    dw = _out(d, k * d, geometry, fill=None)
    dw.view[:, 3 * d:] = NAN
    dw.before = dw.buf.clone()
    ws, ws_bytes = _workspace(int(lib.ihg_node_interact_bwd_weight_workspace_bytes(d, c.order)))
    rc = lib.ihg_node_interact_bwd_weight(ops._ptr(x.h.view), _ld(x.h), ops._ptr(x.sums.view), _ld(x.sums), ops._ptr(x.dy.view), _ld(x.dy), ops._ptr(x.scale.t) if use_scale else None,
                                          c.order, _tb(c.type_begin), ops._ptr(dw.view), _ld(dw), ops._ptr(ws.arg), ws_bytes, d, ops._stream())
    torch.cuda.synchronize()
    assert rc == (_lib.OK if expect is None else expect), f'{what}: ihg_node_interact_bwd_weight returned {rc}: {_lib.last_error()}'
    dw.assert_guards(what)
    ws.assert_guards(what)
    x.assert_unchanged(what)
    if expect is not None:
        dw.assert_untouched(what)
        ws.assert_untouched(what)
        return None
    assert bool((dw.view[:, :3 * d] == SENTINEL).all()), f'{what}: the first-order columns of dw were written'
    return dw.view[:, 3 * d:]


NODE_INSTANCES = [(dim, 'split') for dim in R.MFMA_DIMS]                # (under IHG_INTERACT_ARITH=f32: d = 32 runs the same kernels, the other widths are refused)


def _node_check(case, geometry, arithmetic, what, exact=True, options=((True, True),)):
    x = NodeOperands(case.to(dev()), geometry)
    d = case.dim
    for use_scale, use_bias in options:
        tag = f'{what} scale {use_scale} bias {use_bias}'
        want, mag = R.node_fwd64(case, use_scale, use_bias)
        got = _node_fwd(x, geometry, tag, use_scale, use_bias)
        dw_want, dw_mag = R.node_weight64(case, use_scale)
        dw = _node_weight(x, geometry, tag, use_scale)
        if exact:
            R.ensure_exact(mag, 0.5, tag + ' out')
            R.ensure_exact(dw_mag, 0.5, tag + ' dw')
            R.assert_equal(got, want, tag + ': out')
            R.assert_equal(dw, dw_want, tag + ': dw')
        else:
            k = len(R.X_BLOCKS[:7 if case.order == 3 else 6]) * d + 1
            _note(f'node fwd d={d}', R.assert_within(got, want, R.float_bound('node_fwd', k, mag, arithmetic), tag + ': out'))
            _note(f'node weight d={d}', R.assert_within(dw, dw_want, R.float_bound('node_weight', case.n, dw_mag, arithmetic), tag + ': dw'))


@pytest.mark.parametrize('order', R.ORDERS)
@pytest.mark.parametrize('dim,arith', NODE_INSTANCES)
def test_node_types_exact(dim, arith, order, monkeypatch):
    """``ihg_node_interact_fwd`` and ``ihg_node_interact_bwd_weight`` with arbitrary integer ``sums``, ``degree``, power-of-two scales, an integer bias and
    ``type_begin`` over the type ladder - 0, 1, TILE - 1, TILE, TILE + 1, GROUP TILE +- 1 rows in each of the three positions, empty first / last / two empty types;
    isolated nodes (degree 0, zero sums) come out exactly 0: every element EQUALS the float64 reference; with and without scale and bias on the first cases."""
    _set_arith(monkeypatch, arith)
    arithmetic = R.node_launch('fwd', dim, arith)['arithmetic']
    for k, tb in enumerate(R.type_cases(dim)):
        case = R.NodeCase(tb, dim, order, R._gen('types', dim, order, k), True, m=3)
        options = ((True, True), (False, True), (True, False), (False, False)) if k < 2 else ((True, True),)
        _node_check(case, 'ab'[k % 2], arithmetic, f'node d={dim} order {order} {arith} type_begin {tb}', options=options)


@pytest.mark.parametrize('dim,arith', NODE_INSTANCES)
def test_node_weight_ranges_exact(dim, arith, monkeypatch):
    """Enough rows of one type that its tile ranges of the weight-gradient kernel take 1, 2 and 3 tiles each (``contraction_reference.node_weight_plan``), the type
    in each position: ``dw`` EQUALS the float64 reference."""
    _set_arith(monkeypatch, arith)
    for k, per in enumerate((1, 2, 3)):
        rows = [7, 40, 33]
        rows[k] = R.rows_for_tiles_per_range(dim, per)
        tb = tuple(int(v) for v in np.concatenate([[0], np.cumsum(rows)]))
        assert R.node_weight_plan(tb, dim)[k][1] == per, (tb, R.node_weight_plan(tb, dim))
        case = R.NodeCase(tb, dim, 3, R._gen('ranges', dim, per), True, m=2)
        _node_check(case, 'a', R.node_launch('weight', dim, arith)['arithmetic'], f'node weight ranges d={dim} per {per}')


def _running_scale_cases(tile):
    """(rows of the one type, per-row exponents of the two operands, zero rows of the two operands)."""
    n = 5 * tile
    cases = []
    for place, n_rows in (('last', n), ('first_of_tile', n), ('alone', n + 1)):
        up = R.rising_exponents(n_rows, tile, 8, place)
        cases.append((n_rows, (up, up // 2), None))
        cases.append((n_rows, (np.zeros(n_rows, np.int64), up), None))
    z = np.zeros(n, bool)
    first = z.copy()
    first[:tile] = True
    some = z.copy()
    some[::3] = True
    up = R.rising_exponents(n, tile, 6, 'last')
    cases += [(n, (up, up), (some, z)), (n, (up, up), (some, np.roll(some, 1))), (n, (up, up), (first, first))]
    return cases


@pytest.mark.parametrize('dim,arith', NODE_INSTANCES)
def test_node_weight_running_scale_exact(dim, arith, monkeypatch):
    """Rows that are integers times 2^k with k rising along the sweep (on ``h``, on ``dy``, on both), the largest row the last row of the last tile, the first row of
    a tile, alone in a partial last tile; all-zero rows on one side, on both sides, as a whole first tile: still exact, so a weight-gradient kernel that does not
    rescale its accumulators when its running scale rises cannot pass."""
    _set_arith(monkeypatch, arith)
    tile = R.node_launch('weight', dim, arith)['tile']
    for k, (n, row_exp, zero_rows) in enumerate(_running_scale_cases(tile)):
        tb = (0, 3, 3 + n, 3 + n + 2)
        pad = lambda e: np.concatenate([np.zeros(3, e.dtype), e, np.zeros(2, e.dtype)])
        case = R.NodeCase(tb, dim, 3, R._gen('scale', dim, k), True, m=2, row_exp=tuple(pad(e) for e in row_exp),
                          zero_rows=None if zero_rows is None else tuple(pad(z) for z in zero_rows))
        _node_check(case, 'a', 'split', f'node running scale d={dim} {arith} case {k}')


@pytest.mark.parametrize('dim,arith', NODE_INSTANCES)
def test_node_float(dim, arith, monkeypatch):
    """``randn`` operands and sums, scales in [0.5, 1.5), 3 types of 70 / 9 / 131 rows, both orders; and the same shapes with every operand the adversarial
    significand of the kernels' split (two fp16 terms; d = 32: every low bit set), all positive, under a power of two: per element within the bound."""
    _set_arith(monkeypatch, arith)
    launch = R.node_launch('fwd', dim, arith)
    for order in R.ORDERS:
        for design in ('randn', 'worst'):
            case = R.NodeCase((0, 70, 79, 210), dim, order, R._gen('nodefloat', dim, order), False)
            if design == 'worst':
                R.make_worst(case, ('h', 'sums', 'dy', 'w', 'bias'), launch['split'], dim + order)
            _node_check(case, 'a', launch['arithmetic'], f'node float {design} d={dim} order {order} {arith}', exact=False)


def test_node_form_refused_writes_nothing(monkeypatch):
    """d = 64 / 128 / 256 under ``IHG_INTERACT_ARITH=f32``: both node-level entries return ``IHG_ERR_INVALID`` and write nothing."""
    _lib, lib, ops = _lib_ops()
    _set_arith(monkeypatch, 'f32')
    for dim in (64, 128, 256):
        assert not R.node_launch('fwd', dim, 'f32')['supported']
        x = NodeOperands(R.NodeCase((0, 7, 19, 40), dim, 3, R._gen('noderefused', dim), True).to(dev()))
        _node_fwd(x, 'a', f'node fwd refused d={dim}', expect=_lib.ERR_INVALID)
        _node_weight(x, 'a', f'node weight refused d={dim}', expect=_lib.ERR_INVALID)


# =============================================================================================
# the node-level linear maps: exact cases over the type ladder
# =============================================================================================
def _linear_run(c, arith, what, typed_entry=False):
    _lib, lib, ops = _lib_ops()
    d, n, tb = c.dim, c.n, c.type_begin
    want = R.linear64(c)
    for name in ('out', 'dx', 'dw', 'db'):
        R.ensure_exact(want[name + '_mag'], 1.0, f'{what} {name}')
    R.ensure_exact(want['dx_mag'] + c.prefill.abs(), 1.0, f'{what} dx accumulated')
    f = lambda t: t.float()
    w, b = Padded(f(c.w), 'a'), Source(f(c.bias))
    ws, ws_bytes = _workspace(int(lib.ihg_node_linear_workspace_bytes(d)))
    pad = (1, 0, 1) if typed_entry else (0, 0, 0)                          # typed rows: the users' and items' blocks with a padding row in front, as embedding tables have

    def rows_of(t, geometry, fill=None):
        """``t`` [N, d] as one padded view, or (typed entry) as three separately allocated blocks; returns (holders, pointer argument, ld)."""
        if not typed_entry:
            p = Padded(f(t), geometry) if fill is None else _out(n, d, geometry, fill)
            if fill is not None and t is not None:
                p.view.copy_(f(t))
                p.before = p.buf.clone()
            return [p], ops._ptr(p.view), _ld(p)
        blocks = []
        for k in range(3):
            rows = tb[k + 1] - tb[k] + pad[k]
            p = _out(rows, d, 'a', fill if fill is not None else 7.0)
            if t is not None:
                p.view[pad[k]:].copy_(f(t[tb[k]:tb[k + 1]]))
            p.before = p.buf.clone()
            blocks.append(p)
        ptrs = (ctypes.c_void_p * 3)(*(blk.view.data_ptr() + pad[k] * d * 4 for k, blk in enumerate(blocks)))
        return blocks, ptrs, d

    def gathered(blocks):
        return blocks[0].view if not typed_entry else torch.cat([blk.view[pad[k]:] for k, blk in enumerate(blocks)])

    geometry = 'b' if not typed_entry else 'a'
    xs, x_arg, ld_x = rows_of(c.x, 'a')
    g = Padded(f(c.g), 'a')
    sources = xs + [g, w, b]
    tbc = _tb(tb)
    # forward
    out = _out(n, d, geometry)
    fwd = lib.ihg_node_linear_fwd_typed if typed_entry else lib.ihg_node_linear_fwd
    rc = fwd(x_arg, ld_x, ops._ptr(w.view), _ld(w), c.stride, ops._ptr(b.t), c.mask, 0, tbc, ops._ptr(out.view), _ld(out), ops._ptr(ws.arg), ws_bytes, d, ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.OK, f'{what}: forward returned {rc}: {_lib.last_error()}'
    out.assert_guards(what)
    R.assert_equal(out.view, want['out'], f'{what}: out')
    # input gradient on its own
    if not typed_entry:
        dx = _out(n, d, geometry)
        rc = lib.ihg_node_linear_bwd_input(ops._ptr(g.view), _ld(g), ops._ptr(w.view), _ld(w), c.stride, tbc, ops._ptr(dx.view), _ld(dx), ops._ptr(ws.arg), ws_bytes, d, ops._stream())
        torch.cuda.synchronize()
        assert rc == _lib.OK, f'{what}: bwd_input returned {rc}: {_lib.last_error()}'
        dx.assert_guards(what)
        R.assert_equal(dx.view, want['dx'], f'{what}: dx of bwd_input')
    # weight gradient: without dx, with dx, adding onto a prefilled dx where the library says it can
    can_add = not typed_entry and bool(lib.ihg_node_linear_bwd_accumulates(d, d, d, d))
    assert typed_entry or can_add == R.node_linear_accumulates(d, arith)
    for with_dx, add in ((False, 0), (True, 0)) + (((True, 1),) if can_add else ()):
        tag = f'{what} dx {with_dx} accumulate {add}'
        dw, dbias = _out(d, c.w.shape[1], 'b' if not typed_entry else 'a'), Guarded(d)
        geometry_dx = 'a' if add else geometry                            # (ihg_node_linear_bwd_accumulates was asked about contiguous rows)
        dxs, dx_arg, ld_dx = rows_of(c.prefill if add else None, geometry_dx, fill=NAN) if with_dx else ([], None, 0)
        if typed_entry:
            rc = lib.ihg_node_linear_bwd_weight_typed(ops._ptr(g.view), _ld(g), x_arg, ld_x, tbc, ops._ptr(dw.view), _ld(dw), c.stride, ops._ptr(dbias.arg), c.mask, 0,
                                                      ops._ptr(w.view), _ld(w), dx_arg, ld_dx, 0b101, ops._ptr(ws.arg), ws_bytes, d, ops._stream())
        else:
            rc = lib.ihg_node_linear_bwd_weight(ops._ptr(g.view), _ld(g), x_arg, ld_x, tbc, ops._ptr(dw.view), _ld(dw), c.stride, ops._ptr(dbias.arg), c.mask, 0,
                                                ops._ptr(w.view), _ld(w), dx_arg, ld_dx, add, ops._ptr(ws.arg), ws_bytes, d, ops._stream())
        torch.cuda.synchronize()
        assert rc == _lib.OK, f'{tag}: bwd_weight returned {rc}: {_lib.last_error()}'
        for t in [dw, dbias] + dxs:
            t.assert_guards(tag)
        R.assert_equal(dw.view, want['dw'], f'{tag}: dw')
        R.assert_equal(dbias.view, want['db'], f'{tag}: dbias')
        if with_dx:
            R.assert_equal(gathered(dxs), want['dx'] + (c.prefill if add else 0), f'{tag}: dx')
            if typed_entry:
                assert all(bool((blk.view[:pad[k]] == 0).all()) for k, blk in enumerate(dxs)), f'{tag}: the padding rows of dx are not zero'
    ws.assert_guards(what)
    for src in sources:
        src.assert_unchanged(what)


@pytest.mark.parametrize('typed', [False, True])
@pytest.mark.parametrize('dim,arith', [(dim, arith) for dim in R.MFMA_DIMS + (12,) for arith in R.ARITHS if arith == 'split' or dim in (128, 256)])     # (d = 12, 32, 64: one set of kernels)
def test_node_linear_types_exact(dim, typed, arith, monkeypatch):
    """``ihg_node_linear_fwd``, ``_bwd_input`` and ``_bwd_weight`` (without ``dx``, with it, adding onto an integer prefill where ``ihg_node_linear_bwd_accumulates`` says
    so) on integer operands over the type ladder: ``out``, ``dx``, ``dw``, ``dbias`` EQUAL the float64 reference; ``out``, ``dx`` and ``dw`` are column slices of wider
    buffers whose guard columns are checked."""
    _set_arith(monkeypatch, arith)
    for k, tb in enumerate(R.type_cases(dim if dim in R.MFMA_DIMS else 32)):
        if tb[3] == 0:
            continue
        c = R.LinearCase(tb, dim, typed, R._gen('linear', dim, typed, k))
        _linear_run(c, arith, f'node linear d={dim} typed {typed} {arith} type_begin {tb}')


@pytest.mark.parametrize('dim', [128, 256])
def test_node_linear_typed_entries_exact(dim, monkeypatch):
    """``ihg_node_linear_fwd_typed`` / ``ihg_node_linear_bwd_weight_typed`` over three separately allocated row blocks (padding rows in front of the users' and the
    items') on a part of the type ladder: exact, the padding rows of ``dx`` zeroed."""
    _lib, lib, ops = _lib_ops()
    _set_arith(monkeypatch, 'split')
    assert bool(lib.ihg_node_linear_typed_supported(dim, dim, dim))
    for k, tb in enumerate(R.type_cases(dim)[::4]):
        for typed in (False, True):
            c = R.LinearCase(tb, dim, typed, R._gen('typed entries', dim, typed, k))
            _linear_run(c, 'split', f'typed entries d={dim} typed {typed} type_begin {tb}', typed_entry=True)


@pytest.mark.parametrize('arith', R.ARITHS)
@pytest.mark.parametrize('dim', [128, 256])
def test_node_linear_running_scale_exact(dim, arith, monkeypatch):
    """The dense weight gradient with rows that are integers times 2^k, k rising along the sweep; the largest row last, first of a tile, alone in a partial tile; zero
    rows on one side, both sides, a whole first tile: exact."""
    _set_arith(monkeypatch, arith)
    for k, (n, row_exp, zero_rows) in enumerate(_running_scale_cases(32)):
        c = R.LinearCase((0, n, n, n), dim, False, R._gen('dense scale', dim, k), m=2, row_exp=row_exp, zero_rows=zero_rows)
        _linear_run(c, arith, f'dense running scale d={dim} {arith} case {k}')


