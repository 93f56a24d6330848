"""The kernels at the batch end of a training step, each launch on its own through the C ABI: ``ihg_batch_scatter_add``, ``ihg_batch_combine``,
``ihg_batch_rows_add``, ``ihg_batch_rows_put``, ``ihg_batch_node_rows``, ``ihg_zero_rows``, ``ihg_mark_rows``, ``ihg_zero_floats`` (``csrc/tail.hip``,
``csrc/common.hpp``) and ``ihg_compose_first_order_fwd`` / ``_bwd`` (``csrc/dense.hip``).

The cases, the float64 references and the verdicts are in ``tests/batch_rows_reference.py``: exact integer cases held with ``torch.equal``, float cases per element
to ``(m + 4) 2^-24 sum |terms|`` AND bit for bit to the batch-order float32 sum the header promises; ladders taken from the kernels' loop bounds (64-id windows, trips
of 16 members, chunks of 256 columns, the 64 KiB and 128 KiB instances, a second grid-stride trip).  ``tests/test_batch_rows_host.py`` holds a numpy emulation of
the kernels' scheme to the same verdicts on the same cases and shows that the named wrong variants fail them, so a failing case here is a wrong kernel.  Every
written tensor is a view into a sentinel-filled buffer with guards around it, every source is compared with its copy after the launch, every launch runs twice and
the two results are compared bit for bit.  The largest case is 32,768 rows of 8 columns: none of these shapes is the workload's."""
import ctypes

import numpy as np
import pytest
import torch

import batch_rows_reference as R
from test_aggregate_kernels import GUARD as ROW_GUARD, SENTINEL, Padded
from test_attention_kernels import Guarded, Source

pytestmark = pytest.mark.gpu

assert np.float32(SENTINEL) == R.SENTINEL
WORST = {}                               # kernel -> worst error / bound of the float cases (printed when the module is done, recorded in DESIGN.md section 5)
CASES = {}                               # kernel -> launches checked


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    CASES[kernel] = CASES.get(kernel, 0) + 1


@pytest.fixture(scope='module', autouse=True)
def _report_worst_ratios():
    """After the module's tests: the cases that ran and the worst ``error / bound`` per kernel of the float cases (each was asserted where it was measured; shown with ``-s``)."""
    yield
    print(f'batch-row cases checked: {sum(CASES.values())} ({", ".join(f"{k} {v}" for k, v in sorted(CASES.items()))})')
    for name in sorted(WORST):
        print(f'worst error / bound: {name}: {WORST[name]:.3f}')


def _api():
    from ihgnn_amd import _lib, ops
    return _lib.load(), _lib, ops


def _sync_ok(rc, what):
    from ihgnn_amd import _lib
    torch.cuda.synchronize()
    assert rc == _lib.OK, f'{what}: returned {rc}: {_lib.last_error()}'


def _arena(values):
    """A flat float32 arena on the device behind guards, holding ``values`` (numpy)."""
    g = Guarded(len(values), fill=0.0)
    if len(values):
        g.view.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)))
    g.before = g.buf.clone()
    return g


def _as(g, dtype, n):
    """The first ``n`` elements of a ``Guarded`` payload seen as ``dtype`` (the payload is 256 bytes into a torch allocation: aligned for every type)."""
    return g.view.view(dtype)[:n]


def _matrix(values):
    """``values`` [rows, ld] (numpy, NaN and sentinel columns included) behind guard rows; ``.ptr``: the address of its first row even where it has no rows."""
    p = Padded(torch.from_numpy(np.ascontiguousarray(values, np.float32)), 'a') if values.shape[0] else Padded((0, values.shape[1]), 'a')
    p.ptr = ctypes.c_void_p(p.buf.data_ptr() + ROW_GUARD * p.buf.stride(0) * 4)
    return p


def _guard_rows_kept(p, what):
    n = p.rows
    for part, was in ((p.buf[:ROW_GUARD], p.before[:ROW_GUARD]), (p.buf[ROW_GUARD + n:], p.before[ROW_GUARD + n:])):
        assert torch.equal(part.view(torch.int32), was.view(torch.int32)), f'{what}: a guard row was written'


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def _twice(run, what):
    """``run()`` -> tuple of numpy outputs, called twice on fresh buffers: the same bits (no atomics, fixed order)."""
    first, second = run(), run()
    for a, b in zip(first, second):
        assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b)), f'{what}: two launches differ'
    return first


# =============================================================================================
# ihg_batch_scatter_add
# =============================================================================================
def _scatter(case, dest):
    lib, _, ops = _api()
    assert case.n <= R.SCATTER_MAX_WIDE and int(case.rows.max()) < dest.n_nodes and dest.width == case.width
    src, rows = _matrix(case.rowgrad), Source(torch.from_numpy(case.rows))

    def run():
        dense = _arena(dest.arena)
        tail = _arena(dest.tail_arena) if dest.tail is not None else None
        off, n_tail = dest.tail if dest.tail is not None else (0, 0)
        rc = lib.ihg_batch_scatter_add(src.ptr, case.rowgrad.shape[1], case.width, ops._ptr(rows.t), case.n, ops._ptr(dense.arg), dest.ld_dense, dest.block_width,
                                       dest.block_stride, None if tail is None else ops._ptr(tail.arg), off, n_tail, ops._stream())
        _sync_ok(rc, case.what)
        dense.assert_guards(case.what)
        if tail is not None:
            tail.assert_guards(case.what)
        return dense.view.cpu().numpy(), None if tail is None else tail.view.cpu().numpy()
    got_dense, got_tail = _twice(run, case.what)
    src.assert_unchanged(case.what)
    rows.assert_unchanged(case.what)
    _note('ihg_batch_scatter_add', R.check_scatter(case, dest, got_dense, got_tail))


@pytest.mark.parametrize('group', ['members', 'n', 'widths', 'forms', 'float'])
def test_batch_scatter_add(group):
    """'members': 1 ... 64 members of one destination inside a 64-window, 65 / 129 / hundreds across windows, the window positions, negative ids; 'n': 1 ... 32,768
    rows; 'widths': 1 ... 513 columns; 'forms': plain matrix, blocks with a sentinel gap, the tail column at its range edges, all on non-zero contents; 'float': both
    verdicts on float payloads, the batch-order one on a case that makes the order visible."""
    for case, dest in R.scatter_cases(group):
        _scatter(case, dest)


# =============================================================================================
# ihg_batch_combine
# =============================================================================================
def _combine(case, block_rows):
    lib, _, ops = _api()
    assert case.n <= R.SCATTER_MAX_WIDE
    rows = Source(torch.from_numpy(case.rows))
    what = f'{case.what}, blocks of {block_rows}'

    def run():
        rowgrad = _matrix(case.rowgrad)
        leader = Guarded(case.n, fill=0.0)
        _as(leader, torch.int32, case.n).fill_(-1)
        rc = lib.ihg_batch_combine(rowgrad.ptr, case.rowgrad.shape[1], case.width, ops._ptr(rows.t), case.n, block_rows, ops._ptr(leader.arg), ops._stream())
        _sync_ok(rc, what)
        leader.assert_guards(what)
        _guard_rows_kept(rowgrad, what)
        return rowgrad.buf[ROW_GUARD:ROW_GUARD + case.n].cpu().numpy(), _as(leader, torch.int32, case.n).cpu().numpy()
    got, got_leader = _twice(run, what)
    rows.assert_unchanged(what)
    _note('ihg_batch_combine', R.check_combine(case, block_rows, got, got_leader))


@pytest.mark.parametrize('group', ['members', 'n', 'widths', 'blocks', 'float'])
def test_batch_combine(group):
    """The scatter's id lists, row counts and widths in one block; 'blocks': disjoint blocks of 0 (= n), 1, 63, 64, 65, 1,100, n, n + 1, 16,384 and 16,385 rows (the
    same id in several blocks: a leader in each, no row summed across).  ``leader`` exactly 0 / 1 behind guards, followers' rows, negative rows and the columns beyond
    ``width`` (NaN) unchanged bit for bit."""
    for case, block_rows in R.combine_cases(group):
        _combine(case, block_rows)


# =============================================================================================
# ihg_batch_rows_add, ihg_batch_rows_put
# =============================================================================================
def _rows_add(case, dest):
    lib, _, ops = _api()
    assert int(case.rows.max()) < dest.n_nodes
    src, rows, leader = _matrix(case.src), Source(torch.from_numpy(case.rows)), Source(torch.from_numpy(case.leader))

    def run():
        if dest.tail is not None:
            out = _arena(dest.tail_arena)
            rc = lib.ihg_batch_rows_add(src.ptr, case.src.shape[1], 1, ops._ptr(rows.t), ops._ptr(leader.t), case.n, None, 0, ops._ptr(out.arg), dest.tail[0], dest.tail[1],
                                        ops._stream())
        else:
            out = _arena(dest.arena)
            rc = lib.ihg_batch_rows_add(src.ptr, case.src.shape[1], case.width, ops._ptr(rows.t), ops._ptr(leader.t), case.n, ops._ptr(out.arg), dest.ld_dense, None, 0, 0,
                                        ops._stream())
        _sync_ok(rc, case.what)
        out.assert_guards(case.what)
        return (out.view.cpu().numpy(),)
    got, = _twice(run, case.what)
    for s in (src, rows, leader):
        s.assert_unchanged(case.what)
    _note('ihg_batch_rows_add', R.check_rows_add(case, dest, got))


@pytest.mark.parametrize('group', ['widths', 'n', 'tail', 'float'])
def test_batch_rows_add(group):
    """Leader rows added onto non-zero contents; the rows of followers (leader = 0) are NaN and must not be read; negative rows with leader = 1 are skipped; the tail
    value is added once and only inside [tail_row_offset, tail_row_offset + tail_rows)."""
    for case, dest in R.rows_add_cases(group):
        _rows_add(case, dest)


def _rows_put(case, typed, assign):
    lib, _, ops = _api()
    tb = typed.type_begin
    assert tb[0] <= int(case.rows[case.live()].min()) and int(case.rows.max()) < tb[3]
    src, rows, leader = _matrix(case.src), Source(torch.from_numpy(case.rows)), Source(torch.from_numpy(case.leader))

    def run():
        outs = [_matrix(a) for a in typed.arenas]                             # three allocations, each behind guards of its own
        rc = lib.ihg_batch_rows_put(src.ptr, case.src.shape[1], case.width, ops._ptr(rows.t), ops._ptr(leader.t), case.n,
                                    (ctypes.c_void_p * 3)(*(o.ptr.value for o in outs)), typed.ld, (ctypes.c_int64 * 4)(*tb), assign, ops._stream())
        _sync_ok(rc, case.what)
        for o in outs:
            _guard_rows_kept(o, case.what)
        return tuple(o.buf[ROW_GUARD:ROW_GUARD + o.rows].cpu().numpy() for o in outs)
    got = _twice(run, case.what)
    for s in (src, rows, leader):
        s.assert_unchanged(case.what)
    _note('ihg_batch_rows_put', R.check_rows_put(case, typed, assign, got))


def test_batch_rows_put():
    """Typed destinations: rows at begin1 - 1, begin1, begin2 - 1, begin2 and at the first and last row of every type, an empty type, a numbering that does not start
    at 0; ``assign`` = 1 writes the listed rows and leaves every other byte its sentinel, ``assign`` = 0 adds onto non-zero contents."""
    for case, typed, assign in R.rows_put_cases():
        _rows_put(case, typed, assign)


# =============================================================================================
# refusals, empty launches, ihg_batch_scatter_workspace_bytes
# =============================================================================================
def test_refused_and_empty_launches_write_nothing():
    lib, L, ops = _api()
    case, dest = R.scatter_cases('forms')[0]
    src, rows = _matrix(case.rowgrad), Source(torch.from_numpy(case.rows))
    leader = Source(torch.from_numpy(np.ones(case.n, np.int32)))
    dense, flags = _arena(dest.arena), Guarded(case.n, fill=-3.0)
    ld, w, n, s = case.rowgrad.shape[1], case.width, case.n, ops._stream()
    p = ops._ptr
    typed = (ctypes.c_void_p * 3)(*(dense.arg.data_ptr(),) * 3)
    tb = (ctypes.c_int64 * 4)(0, 10, 20, dest.n_nodes)
    refused = {
        'scatter: 32,769 rows': lambda: lib.ihg_batch_scatter_add(src.ptr, ld, w, p(rows.t), R.SCATTER_MAX_WIDE + 1, p(dense.arg), dest.ld_dense, w, 0, None, 0, 0, s),
        'scatter: negative rows': lambda: lib.ihg_batch_scatter_add(src.ptr, ld, w, p(rows.t), -1, p(dense.arg), dest.ld_dense, w, 0, None, 0, 0, s),
        'scatter: width 0': lambda: lib.ihg_batch_scatter_add(src.ptr, ld, 0, p(rows.t), n, p(dense.arg), dest.ld_dense, w, 0, None, 0, 0, s),
        'scatter: ld < width': lambda: lib.ihg_batch_scatter_add(src.ptr, w - 1, w, p(rows.t), n, p(dense.arg), dest.ld_dense, w, 0, None, 0, 0, s),
        'scatter: block_width 0': lambda: lib.ihg_batch_scatter_add(src.ptr, ld, w, p(rows.t), n, p(dense.arg), dest.ld_dense, 0, 0, None, 0, 0, s),
        'scatter: ld_dense < block_width': lambda: lib.ihg_batch_scatter_add(src.ptr, ld, w, p(rows.t), n, p(dense.arg), w - 1, w, 0, None, 0, 0, s),
        'scatter: null rowgrad': lambda: lib.ihg_batch_scatter_add(None, ld, w, p(rows.t), n, p(dense.arg), dest.ld_dense, w, 0, None, 0, 0, s),
        'scatter: null rows': lambda: lib.ihg_batch_scatter_add(src.ptr, ld, w, None, n, p(dense.arg), dest.ld_dense, w, 0, None, 0, 0, s),
        'scatter: null dense': lambda: lib.ihg_batch_scatter_add(src.ptr, ld, w, p(rows.t), n, None, dest.ld_dense, w, 0, None, 0, 0, s),
        'combine: 32,769 rows': lambda: lib.ihg_batch_combine(src.ptr, ld, w, p(rows.t), R.SCATTER_MAX_WIDE + 1, 0, p(flags.arg), s),
        'combine: width 0': lambda: lib.ihg_batch_combine(src.ptr, ld, 0, p(rows.t), n, 0, p(flags.arg), s),
        'combine: ld < width': lambda: lib.ihg_batch_combine(src.ptr, w - 1, w, p(rows.t), n, 0, p(flags.arg), s),
        'combine: null rowgrad': lambda: lib.ihg_batch_combine(None, ld, w, p(rows.t), n, 0, p(flags.arg), s),
        'combine: null rows': lambda: lib.ihg_batch_combine(src.ptr, ld, w, None, n, 0, p(flags.arg), s),
        'combine: null leader': lambda: lib.ihg_batch_combine(src.ptr, ld, w, p(rows.t), n, 0, None, s),
        'rows_add: width 0': lambda: lib.ihg_batch_rows_add(src.ptr, ld, 0, p(rows.t), p(leader.t), n, p(dense.arg), dest.ld_dense, None, 0, 0, s),
        'rows_add: ld < width': lambda: lib.ihg_batch_rows_add(src.ptr, w - 1, w, p(rows.t), p(leader.t), n, p(dense.arg), dest.ld_dense, None, 0, 0, s),
        'rows_add: ld_dense < width': lambda: lib.ihg_batch_rows_add(src.ptr, ld, w, p(rows.t), p(leader.t), n, p(dense.arg), w - 1, None, 0, 0, s),
        'rows_add: no destination': lambda: lib.ihg_batch_rows_add(src.ptr, ld, w, p(rows.t), p(leader.t), n, None, dest.ld_dense, None, 0, 0, s),
        'rows_add: null leader': lambda: lib.ihg_batch_rows_add(src.ptr, ld, w, p(rows.t), None, n, p(dense.arg), dest.ld_dense, None, 0, 0, s),
        'rows_add: negative rows': lambda: lib.ihg_batch_rows_add(src.ptr, ld, w, p(rows.t), p(leader.t), -1, p(dense.arg), dest.ld_dense, None, 0, 0, s),
        'rows_put: width 0': lambda: lib.ihg_batch_rows_put(src.ptr, ld, 0, p(rows.t), p(leader.t), n, typed, dest.ld_dense, tb, 1, s),
        'rows_put: ld_dense < width': lambda: lib.ihg_batch_rows_put(src.ptr, ld, w, p(rows.t), p(leader.t), n, typed, w - 1, tb, 1, s),
        'rows_put: null destinations': lambda: lib.ihg_batch_rows_put(src.ptr, ld, w, p(rows.t), p(leader.t), n, None, dest.ld_dense, tb, 1, s),
        'rows_put: null type ranges': lambda: lib.ihg_batch_rows_put(src.ptr, ld, w, p(rows.t), p(leader.t), n, typed, dest.ld_dense, None, 1, s),
        'zero_rows: dim 0': lambda: lib.ihg_zero_rows(p(dense.arg), dest.ld_dense, 0, p(rows.t), n, s),
        'zero_rows: ld < dim': lambda: lib.ihg_zero_rows(p(dense.arg), 3, 4, p(rows.t), n, s),
        'zero_rows: null rows': lambda: lib.ihg_zero_rows(p(dense.arg), dest.ld_dense, 4, None, n, s),
        'zero_floats: negative n': lambda: lib.ihg_zero_floats(p(dense.arg), -1, s),
        'zero_floats: null pointer': lambda: lib.ihg_zero_floats(None, 5, s),
        'node_rows: negative batch': lambda: lib.ihg_batch_node_rows(p(rows.t), p(rows.t), p(rows.t), -1, 0, 0, p(dense.arg), None, s),
        'node_rows: null output': lambda: lib.ihg_batch_node_rows(p(rows.t), p(rows.t), p(rows.t), 2, 0, 0, None, None, s),
    }
    for what, call in refused.items():
        rc = call()
        torch.cuda.synchronize()
        assert rc == L.ERR_INVALID, f'{what}: returned {rc}'
        for out in (dense, flags):
            out.assert_untouched(what)
        src.assert_unchanged(what)
    empty = {
        'scatter': lambda: lib.ihg_batch_scatter_add(None, ld, w, None, 0, None, dest.ld_dense, w, 0, None, 0, 0, s),
        'combine': lambda: lib.ihg_batch_combine(None, ld, w, None, 0, 0, None, s),
        'rows_add': lambda: lib.ihg_batch_rows_add(None, ld, w, None, None, 0, None, dest.ld_dense, None, 0, 0, s),
        'rows_put': lambda: lib.ihg_batch_rows_put(None, ld, w, None, None, 0, None, dest.ld_dense, None, 1, s),
        'zero_rows': lambda: lib.ihg_zero_rows(None, dest.ld_dense, 4, None, 0, s),
        'zero_floats': lambda: lib.ihg_zero_floats(None, 0, s),
        'mark_rows': lambda: lib.ihg_mark_rows(None, None, 0, None, 1, s),
        'node_rows': lambda: lib.ihg_batch_node_rows(None, None, None, 0, 3, 4, None, None, s),
    }
    for what, call in empty.items():
        rc = call()
        torch.cuda.synchronize()
        assert rc == L.OK, f'{what} of nothing: returned {rc}'
    for out in (dense, flags):
        out.assert_untouched('empty launches')
    assert [int(lib.ihg_batch_scatter_workspace_bytes(n)) for n in (0, R.SCATTER_MAX, R.SCATTER_MAX + 1, R.SCATTER_MAX_WIDE, R.SCATTER_MAX_WIDE + 1, -1)] == [0, 0, 0, 0, -1, -1]
    assert int(lib.ihg_batch_scatter_max_rows()) == R.SCATTER_MAX_WIDE


# =============================================================================================
# the small kernels
# =============================================================================================
@pytest.mark.parametrize('b', R.NODE_ROWS_B)
def test_batch_node_rows(b):
    """3 b around one workgroup (256 threads) and around one grid (524,288 threads): the int64 list, and the optional int32 one, equal users | queries + query_row0 |
    items + item_row0 behind guards."""
    lib, L, ops = _api()
    rng = np.random.default_rng(b)
    ids = [rng.integers(0, 1 << 20, max(b, 1)).astype(np.int64) for _ in range(3)]
    srcs = [Source(torch.from_numpy(x)) for x in ids]
    want = R.node_rows_reference(ids[0][:b], ids[1][:b], ids[2][:b], 1 << 21, 3 << 21)
    for with32 in (True, False):
        def run():
            out64, out32 = Guarded(2 * 3 * b, fill=-1.0), Guarded(3 * b, fill=-1.0)
            rc = lib.ihg_batch_node_rows(*(ops._ptr(x.t) for x in srcs), b, 1 << 21, 3 << 21, ops._ptr(out64.arg), ops._ptr(out32.arg) if with32 else None, ops._stream())
            _sync_ok(rc, f'node rows b = {b}')
            out64.assert_guards(f'node rows b = {b}')
            if with32:
                out32.assert_guards(f'node rows b = {b}')
            else:
                out32.assert_untouched(f'node rows b = {b}: no int32 list asked for')
            return _as(out64, torch.int64, 3 * b).cpu().numpy(), _as(out32, torch.int32, 3 * b).cpu().numpy()
        got64, got32 = _twice(run, f'node rows b = {b}')
        assert np.array_equal(got64, want), f'b = {b}: first difference at {np.nonzero(got64 != want)[0][:4]}'
        assert not with32 or np.array_equal(got32, want.astype(np.int32))
    for x in srcs:
        x.assert_unchanged(f'node rows b = {b}')
    _note('ihg_batch_node_rows', 0.0)


@pytest.mark.parametrize('n', [1, R.GRID_WAVES, R.GRID_WAVES + 1])
@pytest.mark.parametrize('dim', R.ZERO_ROWS_DIMS)
def test_zero_rows(dim, n):
    """Listed rows (repeated ones among them) zero in their first ``dim`` columns; every unlisted row, every column beyond ``dim`` and the guards unchanged."""
    lib, L, ops = _api()
    rng = np.random.default_rng([dim, n])
    table = rng.integers(1, 9, (700, dim)).astype(np.float32)
    rows = 2 * rng.integers(0, 350, n).astype(np.int64)                       # even rows only: the odd ones are never listed
    idx = Source(torch.from_numpy(rows))

    def run():
        base = Padded(torch.from_numpy(table), 'b')
        assert base.buf.stride(0) > dim
        _sync_ok(lib.ihg_zero_rows(ops._ptr(base.view), base.buf.stride(0), dim, ops._ptr(idx.t), n, ops._stream()), f'zero rows {dim} x {n}')
        base.assert_guards(f'zero rows {dim} x {n}')
        return (base.view.cpu().numpy(),)
    got, = _twice(run, f'zero rows {dim} x {n}')
    assert np.array_equal(got, R.zero_rows_reference(table, dim, rows)) and bool((got[1::2] != 0).all())
    idx.assert_unchanged(f'zero rows {dim} x {n}')
    _note('ihg_zero_rows', 0.0)


@pytest.mark.parametrize('form', ['rows64', 'rows32'])
@pytest.mark.parametrize('n', R.MARK_ROWS_N)
def test_mark_rows(n, form):
    """``mask[rows[k]] = value`` with byte stores: value 1, then 0, over repeated rows; every other byte of the mask (its neighbours in the same word) unchanged."""
    lib, L, ops = _api()
    rng = np.random.default_rng(n)
    n_mask = 300001
    rows = 1 + 3 * rng.integers(0, n_mask // 3, n).astype(np.int64)           # bytes 1, 4, 7, ...: three of every four words keep a neighbour
    idx = Source(torch.from_numpy(rows if form == 'rows64' else rows.astype(np.int32)))
    holder = Guarded((n_mask + 3) // 4, fill=0.0)
    mask = _as(holder, torch.uint8, n_mask)
    before = rng.integers(2, 250, n_mask).astype(np.uint8)
    mask.copy_(torch.from_numpy(before))
    for value in (1, 0):
        r64, r32 = (ops._ptr(idx.t), None) if form == 'rows64' else (None, ops._ptr(idx.t))
        _sync_ok(lib.ihg_mark_rows(r64, r32, n, ops._ptr(mask), value, ops._stream()), f'mark rows {form} n = {n}')
        holder.assert_guards(f'mark rows {form} n = {n}')
        assert np.array_equal(mask.cpu().numpy(), R.mark_rows_reference(before, rows, value)), f'mark rows {form} n = {n} value {value}'
    idx.assert_unchanged(f'mark rows {form}')
    snapshot = holder.buf.clone()
    for what, (r64, r32) in {'both lists': (ops._ptr(idx.t), ops._ptr(idx.t)), 'neither list': (None, None)}.items():
        rc = lib.ihg_mark_rows(r64, r32, n, ops._ptr(mask), 1, ops._stream())
        torch.cuda.synchronize()
        assert rc == L.ERR_INVALID and torch.equal(holder.buf.view(torch.int32), snapshot.view(torch.int32)), f'mark rows with {what}: returned {rc}'
    _note('ihg_mark_rows', 0.0)


@pytest.mark.parametrize('n', R.ZERO_FLOATS_N)
def test_zero_floats(n):
    """``p[0 .. n) = 0`` from an address 4 bytes past a 16-byte boundary: the float in front, the floats behind and the guards unchanged."""
    lib, L, ops = _api()
    holder = Guarded(n + 6, fill=7.0)
    p = holder.view[1:]
    assert p.data_ptr() % 16 == 4
    _sync_ok(lib.ihg_zero_floats(ops._ptr(p), n, ops._stream()), f'zero floats {n}')
    holder.assert_guards(f'zero floats {n}')
    got = holder.view.cpu().numpy()
    assert got[0] == 7.0 and bool((got[1:1 + n] == 0).all()) and bool((got[1 + n:] == 7.0).all())
    _note('ihg_zero_floats', 0.0)


# =============================================================================================
# ihg_compose_first_order_fwd / _bwd
# =============================================================================================
def _wide(values):
    """A 2-D operand in geometry (b): a column slice of a wider matrix (its row stride above the minimum, sentinel columns on both sides), guard rows around it."""
    return Padded(torch.from_numpy(np.ascontiguousarray(values, np.float32)), 'b')


def _ld(p):
    return int(p.buf.stride(0))


def _compose(case):
    lib, L, ops = _api()
    d, what = case.dim, case.what
    a, w, dw_eff = _wide(case.a), _wide(case.w), _wide(case.dw_eff)
    b, c, db_eff = Source(torch.from_numpy(case.b)), Source(torch.from_numpy(case.c)), Source(torch.from_numpy(case.db_eff.reshape(-1)))
    assert _ld(a) > 3 * d and _ld(w) > d

    def run():
        w_eff, b_eff = Padded((d, 3 * d), 'b'), Guarded(3 * d)
        w_eff.view.fill_(float('nan'))
        rc = lib.ihg_compose_first_order_fwd(ops._ptr(a.view), _ld(a), ops._ptr(c.t) if case.with_c else None, ops._ptr(w.view), _ld(w), ops._ptr(b.t), ops._ptr(w_eff.view),
                                             _ld(w_eff), ops._ptr(b_eff.arg), d, ops._stream())
        _sync_ok(rc, what + ' forward')
        da, dw, dc, db = Padded((d, 3 * d), 'b'), Padded((d, d), 'b'), Guarded(d), Guarded(d)
        da.view.fill_(float('nan')), dw.view.fill_(float('nan'))
        rc = lib.ihg_compose_first_order_bwd(ops._ptr(a.view), _ld(a), ops._ptr(w.view), _ld(w), ops._ptr(b.t), ops._ptr(dw_eff.view), _ld(dw_eff), ops._ptr(db_eff.t),
                                             ops._ptr(da.view), _ld(da), ops._ptr(dc.arg) if case.with_c else None, ops._ptr(dw.view), _ld(dw), ops._ptr(db.arg), d, ops._stream())
        _sync_ok(rc, what + ' backward')
        for out in (w_eff, b_eff, da, dw, dc, db):
            out.assert_guards(what)
        if not case.with_c:
            dc.assert_untouched(what + ': dc is NULL')
        return tuple(t.view.cpu().numpy() for t in (w_eff, b_eff, da, dw, db, dc))
    got = dict(zip(('w_eff', 'b_eff', 'da', 'dw', 'db', 'dc'), _twice(run, what)))
    for src in (a, w, dw_eff, b, c, db_eff):
        src.assert_unchanged(what)
    got['b_eff'] = got['b_eff'].reshape(3, d)
    fwd, bwd = R.compose_fwd_reference(case), R.compose_bwd_reference(case)
    for name, ref in list(fwd.items()) + list(bwd.items()):
        if name == 'dc' and not case.with_c:
            continue
        _note(f'ihg_compose_first_order {name}', R.hold_compose(got[name], ref, case.exact, f'{what}: {name}'))


@pytest.mark.parametrize('part', [0, 1, 2])
def test_compose_first_order(part):
    """d = 1 ... 256 on exact operands (``torch.equal``) with ``c`` / ``dc`` given and NULL, float operands at 9, 65, 96, 129 held per element; every row stride above
    its minimum with sentinel columns, every output pre-filled with NaN behind guards."""
    for case in R.compose_cases()[part::3]:
        _compose(case)


def test_compose_first_order_refuses_bad_widths():
    lib, L, ops = _api()
    out, src = Guarded(64, fill=-2.0), Source(torch.ones(64))
    o, i, s = ops._ptr(out.arg), ops._ptr(src.t), ops._stream()
    for d in (0, 1025, -3):
        assert lib.ihg_compose_first_order_fwd(i, 4000, i, i, 4000, i, o, 4000, o, d, s) == L.ERR_INVALID
        assert lib.ihg_compose_first_order_bwd(i, 4000, i, 4000, i, i, 4000, i, o, 4000, o, o, 4000, o, d, s) == L.ERR_INVALID
    for bad in range(3):                                                       # a row stride below its minimum (d = 4: 12, 4, 12)
        lds = [12, 4, 12]
        lds[bad] -= 1
        assert lib.ihg_compose_first_order_fwd(i, lds[0], i, i, lds[1], i, o, lds[2], o, 4, s) == L.ERR_INVALID
    for bad in range(5):
        lds = [12, 4, 12, 12, 4]
        lds[bad] -= 1
        assert lib.ihg_compose_first_order_bwd(i, lds[0], i, lds[1], i, i, lds[2], i, o, lds[3], o, o, lds[4], o, 4, s) == L.ERR_INVALID
    assert lib.ihg_compose_first_order_fwd(None, 12, i, i, 4, i, o, 12, o, 4, s) == L.ERR_INVALID
    assert lib.ihg_compose_first_order_bwd(i, 12, i, 4, i, i, 12, i, o, 12, o, None, 4, o, 4, s) == L.ERR_INVALID
    torch.cuda.synchronize()
    out.assert_untouched('refused compose launches')
    src.assert_unchanged('refused compose launches')
