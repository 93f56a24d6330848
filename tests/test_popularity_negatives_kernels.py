"""``ihg_sample_pool_weighted`` (``csrc/tail.hip``) through the C ABI, into guarded, sentinel-prefilled int64 buffers: bit for bit against the sequential definition of
``tests/popularity_negatives_reference.py`` (the one ``tests/test_popularity_negatives_host.py`` holds the chunked scheme to, and whose attempts per row it bounds), the
form without lists, the bits of ``ihg_sample_pool_excluding`` / ``ihg_sample_pool`` / ``ihg_sample_negatives`` under unit and equal weights, the prefix property, the
smallest catalogues, guards intact, nothing written on a refusal.  Every table passed to a launch is strictly ascending and every list short enough: the promises."""
import functools

import numpy as np
import pytest
import torch

import popularity_negatives_reference as P

pytestmark = pytest.mark.gpu

GUARD = 8                                                   # words either side of every output


def dev():
    return torch.device('cuda:0')


def guarded(n, fill=-1):
    t = torch.full((n + 2 * GUARD,), fill, dtype=torch.int64, device=dev())
    t[:GUARD], t[-GUARD:] = -7, -7
    return t


def intact(*buffers):
    return all(bool((b[:GUARD] == -7).all() and (b[-GUARD:] == -7).all()) for b in buffers)


@functools.lru_cache(maxsize=None)
def lists_on(n_items):
    ptr, items = P.lists_of(n_items)
    return torch.from_numpy(ptr.copy()).to(dev()), torch.from_numpy(items.copy()).to(dev())


@functools.lru_cache(maxsize=None)
def table_on(name, n_items):
    """``(cum on the device, total)`` through ``ops.item_sampling_table``, which checks the strict ascent."""
    from ihgnn_amd import ops
    cum, total = ops.item_sampling_table(P.WEIGHTS[name](n_items), device=dev())
    assert total == int(P.table(name, n_items)[-1]) and torch.equal(cum.cpu(), torch.from_numpy(P.table(name, n_items).copy()))
    return cum, total


def launch(n_rows, n_items, m, table, rows=None, lists=None, longest=0, seed=P.SEED, counter=P.COUNTER, out=None, total=None):
    """The C entry point; ``rows`` / ``lists`` ``None``: the form with ``n_lists == 0`` and three null pointers."""
    from ihgnn_amd import _lib, ops
    out = guarded(n_rows * m) if out is None else out
    cum, own_total = table
    rows_d = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, np.int64)).to(dev())
    ptr_d, items_d = lists if lists is not None else (None, None)
    status = _lib.load().ihg_sample_pool_weighted(seed, counter, n_rows, n_items, m, ops._ptr(cum), own_total if total is None else total, ops._ptr(rows_d),
                                                  0 if lists is None else int(ptr_d.shape[0]) - 1, ops._ptr(ptr_d), ops._ptr(items_d), longest, ops._ptr(out[GUARD:]),
                                                  ops._stream())
    torch.cuda.synchronize()
    return status, out


@pytest.mark.parametrize('rows', P.POOL_ROWS)
def test_draw_equals_the_sequential_definition(rows):
    """Lists of lengths 0, 1, 63, 64, 65 and 100 mixed over the rows, one row id below the lists and (from three rows on) one above them; the ``squares`` table at every
    storable catalogue size of the pool cases, the whole-complement corner among them, and ``powerlaw`` at 1000 items."""
    ran = 0
    for r, m, n_items, name in P.GPU_CASES:
        if r != rows:
            continue
        want, attempts = P.expected(r, m, n_items, name)
        assert attempts.max() <= P.MAX_ATTEMPTS                              # (asserted on the host as well: no row of a launch needs more)
        of_row = P.rows_to_lists(rows, P.N_LISTS)
        status, out = launch(rows, n_items, m, table_on(name, n_items), of_row, lists_on(n_items), P.LONGEST)
        assert status == 0 and intact(out), (rows, m, n_items, name)
        got = out[GUARD:-GUARD].view(rows, m).cpu()
        assert torch.equal(got, torch.from_numpy(want.copy())), (rows, m, n_items, name)
        ran += 1
    assert ran >= 17


def test_form_without_lists():
    """``n_lists == 0`` with three null pointers: no row has a list.  Against the definition, and against the launch with lists that no row names."""
    rows, n_items = 300, 1000
    for name in ('squares', 'powerlaw'):
        table = table_on(name, n_items)
        for m in (1, 16, 17, 100, 256):
            status, out = launch(rows, n_items, m, table)
            assert status == 0 and intact(out), (name, m)
            got = out[GUARD:-GUARD].view(rows, m)
            assert torch.equal(got.cpu(), torch.from_numpy(P.pool_draw_weighted(P.SEED, P.COUNTER, rows, n_items, m, P.table(name, n_items)).copy())), (name, m)
            for of_row in (np.full(rows, -1), np.full(rows, P.N_LISTS)):
                status, named = launch(rows, n_items, m, table, of_row, lists_on(n_items), P.LONGEST)
                assert status == 0 and intact(named) and torch.equal(named[GUARD:-GUARD].view(rows, m), got), (name, m)


def test_unit_and_equal_weights_give_the_uniform_launches():
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    rows, n_items = 300, 1000
    ptr_d, items_d = lists_on(n_items)
    of_row = P.rows_to_lists(rows, P.N_LISTS)
    rows_d = torch.from_numpy(of_row).to(dev())
    for m in P.EQUIVALENCE_M:
        excluding = torch.empty(rows, m, dtype=torch.int64, device=dev())
        assert lib.ihg_sample_pool_excluding(P.SEED, P.COUNTER, rows, n_items, m, ops._ptr(rows_d), P.N_LISTS, ops._ptr(ptr_d), ops._ptr(items_d), P.LONGEST,
                                             ops._ptr(excluding), ops._stream()) == 0
        plain = torch.empty(rows, m, dtype=torch.int64, device=dev())
        assert lib.ihg_sample_pool(P.SEED, P.COUNTER, rows, n_items, m, ops._ptr(plain), ops._stream()) == 0
        for name in ('unit', 'equal'):
            status, out = launch(rows, n_items, m, table_on(name, n_items), of_row, (ptr_d, items_d), P.LONGEST)
            assert status == 0 and intact(out) and torch.equal(out[GUARD:-GUARD].view(rows, m), excluding), (name, m)
            status, out = launch(rows, n_items, m, table_on(name, n_items))
            assert status == 0 and intact(out) and torch.equal(out[GUARD:-GUARD].view(rows, m), plain), (name, m)
        if m <= 16:
            few = torch.empty(rows, m, dtype=torch.int64, device=dev())
            assert lib.ihg_sample_negatives(P.SEED, P.COUNTER, rows, n_items, m, ops._ptr(few), ops._stream()) == 0
            assert torch.equal(few, plain)


def test_op_prefix_and_smallest_catalogues():
    """``ops.sample_pool_weighted``: the launch (strided row ids included); the first c columns of a call with m are a call with c; one and two items."""
    from ihgnn_amd import _lib, ops
    rows, n_items, m = 65, 1000, 100
    ptr, items = P.lists_of(n_items)
    lists = lists_on(n_items)
    of_row = P.rows_to_lists(rows, P.N_LISTS)
    table = table_on('powerlaw', n_items)
    triples = torch.zeros(rows, 3, dtype=torch.int64, device=dev())
    triples[:, 0] = torch.from_numpy(of_row).to(dev())
    got = ops.sample_pool_weighted(99, 7, rows, n_items, m, table, triples[:, 0], lists, P.LONGEST, device=dev())
    assert got.shape == (rows, m) and got.dtype == torch.int64
    assert torch.equal(got.cpu(), torch.from_numpy(P.pool_draw_weighted(99, 7, rows, n_items, m, P.table('powerlaw', n_items), of_row, ptr, items).copy()))
    bare = ops.sample_pool_weighted(99, 7, rows, n_items, m, table, device=dev())
    assert torch.equal(bare.cpu(), torch.from_numpy(P.pool_draw_weighted(99, 7, rows, n_items, m, P.table('powerlaw', n_items)).copy()))
    for c in (1, 16, 17, 64, 65):
        status, out = launch(rows, n_items, c, table, of_row, lists, P.LONGEST, seed=99, counter=7)
        assert status == 0 and intact(out) and torch.equal(out[GUARD:-GUARD].view(rows, c), got[:, :c]), c
    assert ops.sample_pool_weighted(99, 7, 0, n_items, m, table, triples[:0, 0], lists, P.LONGEST, device=dev()).shape == (0, m)
    assert ops.sample_pool_weighted(99, 7, 0, n_items, m, table, device=dev()).shape == (0, m)
    # one item: the one value.  Two items of weights 1 and 3 (a modest ratio: the light item is one attempt in four): both of them, and the light one alone once the
    # heavy one is listed - m + max_list_len = n_items
    one = ops.item_sampling_table(np.array([5], np.int64), device=dev())
    status, out = launch(70, 1, 1, one)
    assert status == 0 and intact(out) and bool((out[GUARD:-GUARD] == 0).all())
    two, two_host = ops.item_sampling_table(np.array([1, 3], np.int64), device=dev()), P.cum_of([1, 3])
    counted = []
    want = P.pool_draw_weighted(P.SEED, P.COUNTER, 70, 2, 2, two_host, attempts=counted)
    assert counted[0].max() <= 64
    status, out = launch(70, 2, 2, two)
    pair = out[GUARD:-GUARD].view(70, 2).cpu()
    assert status == 0 and intact(out) and torch.equal(pair, torch.from_numpy(want.copy())) and bool((pair.sum(1) == 1).all()) and 35 < int(pair[:, 0].sum()) < 70
    heavy_listed = (torch.tensor([0, 1], dtype=torch.int64, device=dev()), torch.tensor([1], dtype=torch.int32, device=dev()))
    counted = []
    P.pool_draw_weighted(P.SEED, P.COUNTER, 70, 2, 1, two_host, np.zeros(70, np.int64), np.array([0, 1]), np.array([1]), attempts=counted)
    assert counted[0].max() <= 64
    status, out = launch(70, 2, 1, two, np.zeros(70, np.int64), heavy_listed, 1)
    assert status == 0 and intact(out) and bool((out[GUARD:-GUARD] == 0).all())


def test_refusals_leave_the_buffer_untouched_and_no_rows_do_nothing():
    from ihgnn_amd import _lib, ops
    rows, n_items, m = 65, 1000, 100
    lists = lists_on(n_items)
    of_row = P.rows_to_lists(rows, P.N_LISTS)
    table = table_on('squares', n_items)
    triples_u = torch.from_numpy(of_row).to(dev())
    out = guarded(rows * m)
    for bad_m, bad_items, longest, total in ((0, 1000, 100, None), (257, 1000, 100, None), (100, 99, 0, None), (100, 1000, 901, None), (100, 1000, -1, None),
                                             (100, 1000, 100, 999), (100, 1000, 100, -1)):
        status, out = launch(rows, bad_items, bad_m, table, of_row, lists, longest, out=out, total=total)
        assert status == _lib.ERR_INVALID, (bad_m, bad_items, longest, total)
        if bad_items == n_items:                                            # (ops refuses a table of another catalogue's size itself)
            with pytest.raises(_lib.IhgnnHipError, match='ihg_sample_pool_weighted'):
                ops.sample_pool_weighted(99, 7, rows, bad_items, bad_m, (table[0], table[1] if total is None else total), triples_u, lists, longest, device=dev())
    with pytest.raises(ValueError, match='does not belong to 99 items'):
        ops.sample_pool_weighted(99, 7, rows, 99, 10, table, device=dev())
    assert intact(out) and bool((out[GUARD:-GUARD] == -1).all())
    status, out = launch(0, n_items, m, table, of_row[:0], lists, P.LONGEST, out=out)
    assert status == _lib.OK and intact(out) and bool((out[GUARD:-GUARD] == -1).all())
    status, out = launch(0, n_items, m, table, out=out)
    assert status == _lib.OK and intact(out) and bool((out[GUARD:-GUARD] == -1).all())
