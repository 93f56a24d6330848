"""``ihg_sample_pool_excluding`` (``csrc/tail.hip``) through the C ABI, into guarded, sentinel-prefilled int64 buffers: bit for bit against the sequential definition of
``tests/filter_negatives_reference.py`` (the one ``tests/test_filter_negatives_host.py`` holds the chunked scheme to), the bits of ``ihg_sample_pool`` /
``ihg_sample_negatives`` with empty lists, the prefix property, guards intact, nothing written on a refusal, uniformity over the complement."""
import functools

import numpy as np
import pytest
import torch

import filter_negatives_reference as F
import hard_negatives_reference as H

pytestmark = pytest.mark.gpu

GUARD = 8                                                   # words either side of every output
N_LISTS = 13
SEED, COUNTER = 7919 * 5 + 2, (3 << 32) + 41


def dev():
    return torch.device('cuda:0')


def guarded(n, fill=-1):
    t = torch.full((n + 2 * GUARD,), fill, dtype=torch.int64, device=dev())
    t[:GUARD], t[-GUARD:] = -7, -7
    return t


def intact(*buffers):
    return all(bool((b[:GUARD] == -7).all() and (b[-GUARD:] == -7).all()) for b in buffers)


@functools.lru_cache(maxsize=None)
def lists_of(n_items):
    """The case's lists (lengths 0, 1, 63, 64, 65, 100 in turn) on the host and on the device; made once per catalogue size."""
    ptr, items = F.make_lists(N_LISTS, n_items)
    ptr.setflags(write=False), items.setflags(write=False)
    return ptr, items, torch.from_numpy(ptr.copy()).to(dev()), torch.from_numpy(items.copy()).to(dev())


def launch(n_rows, n_items, m, rows, ptr_d, items_d, longest, seed=SEED, counter=COUNTER, out=None):
    from ihgnn_amd import _lib, ops
    out = guarded(n_rows * m) if out is None else out
    rows_d = torch.from_numpy(np.ascontiguousarray(rows, np.int64)).to(dev())
    status = _lib.load().ihg_sample_pool_excluding(seed, counter, n_rows, n_items, m, ops._ptr(rows_d), int(ptr_d.shape[0]) - 1, ops._ptr(ptr_d), ops._ptr(items_d), longest,
                                                   ops._ptr(out[GUARD:]), ops._stream())
    torch.cuda.synchronize()
    return status, out


@pytest.mark.parametrize('rows', F.POOL_ROWS)
def test_draw_equals_the_sequential_definition(rows):
    """Lists of lengths 0, 1, 63, 64, 65 and 100 mixed over the rows, one row id below the lists and (from three rows on) one above them."""
    for r, m, n_items in F.POOL_CASES + ((65, 156, 256),):
        if r != rows:
            continue
        ptr, items, ptr_d, items_d = lists_of(n_items)
        of_row = F.rows_to_lists(rows, N_LISTS)
        status, out = launch(rows, n_items, m, of_row, ptr_d, items_d, F.LONGEST)
        assert status == 0 and intact(out), (rows, m, n_items)
        got = out[GUARD:-GUARD].view(rows, m).cpu()
        want = F.pool_draw_excluding(SEED, COUNTER, rows, n_items, m, of_row, ptr, items)
        assert torch.equal(got, torch.from_numpy(want.copy())), (rows, m, n_items)
        if m + F.LONGEST == n_items:                                        # the corner: a row with a list of 100 draws the whole complement
            for row in np.flatnonzero(np.isin(of_row, np.flatnonzero(np.diff(ptr) == F.LONGEST))):
                assert (np.sort(got[row].numpy()) == np.setdiff1d(np.arange(n_items), F._run(of_row, ptr, items, row))).all(), (rows, m, n_items, row)


def test_empty_lists_give_the_unfiltered_launches():
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    rows, n_items = 300, 1000
    ptr, items, ptr_d, items_d = lists_of(n_items)
    empty_ptr = torch.zeros(4, dtype=torch.int64, device=dev())
    unread = torch.zeros(1, dtype=torch.int32, device=dev())                # (an empty tensor has no address)
    for m in (1, 10, 16, 17, 100, 256):
        plain = torch.empty(rows, m, dtype=torch.int64, device=dev())
        assert lib.ihg_sample_pool(SEED, COUNTER, rows, n_items, m, ops._ptr(plain), ops._stream()) == 0
        for of_row, p, i in ((np.arange(rows) % 3, empty_ptr, unread), (np.full(rows, -1), ptr_d, items_d), (np.full(rows, N_LISTS), ptr_d, items_d)):
            status, out = launch(rows, n_items, m, of_row, p, i, F.LONGEST)
            assert status == 0 and intact(out) and torch.equal(out[GUARD:-GUARD].view(rows, m), plain), m
        if m <= 16:
            few = torch.empty(rows, m, dtype=torch.int64, device=dev())
            assert lib.ihg_sample_negatives(SEED, COUNTER, rows, n_items, m, ops._ptr(few), ops._stream()) == 0
            assert torch.equal(few, plain)
        assert torch.equal(plain.cpu(), torch.from_numpy(H.pool_draw(SEED, COUNTER, rows, n_items, m).copy()))


def test_op_prefix_and_refusals():
    """``ops.sample_pool_excluding``: the launch (strided row ids included); the first c columns of a call with m are a call with c; a refusal writes nothing."""
    from ihgnn_amd import _lib, ops
    rows, n_items, m = 65, 1000, 100
    ptr, items, ptr_d, items_d = lists_of(n_items)
    of_row = F.rows_to_lists(rows, N_LISTS)
    triples = torch.zeros(rows, 3, dtype=torch.int64, device=dev())
    triples[:, 0] = torch.from_numpy(of_row).to(dev())
    got = ops.sample_pool_excluding(99, 7, rows, n_items, m, triples[:, 0], (ptr_d, items_d), F.LONGEST, device=dev())
    assert got.shape == (rows, m) and got.dtype == torch.int64
    assert torch.equal(got.cpu(), torch.from_numpy(F.pool_draw_excluding(99, 7, rows, n_items, m, of_row, ptr, items).copy()))
    for c in (1, 16, 17, 64, 65):
        status, out = launch(rows, n_items, c, of_row, ptr_d, items_d, F.LONGEST, seed=99, counter=7)
        assert status == 0 and intact(out) and torch.equal(out[GUARD:-GUARD].view(rows, c), got[:, :c]), c
    assert ops.sample_pool_excluding(99, 7, 0, n_items, m, triples[:0, 0], (ptr_d, items_d), F.LONGEST, device=dev()).shape == (0, m)
    out = guarded(rows * m)
    for bad_m, bad_items, longest in ((0, 1000, 100), (257, 1000, 100), (100, 99, 0), (100, 1000, 901), (100, 1000, -1)):
        status, out = launch(rows, bad_items, bad_m, of_row, ptr_d, items_d, longest, out=out)
        assert status == _lib.ERR_INVALID, (bad_m, bad_items, longest)
        with pytest.raises(_lib.IhgnnHipError, match='ihg_sample_pool_excluding'):
            ops.sample_pool_excluding(99, 7, rows, bad_items, bad_m, triples[:, 0], (ptr_d, items_d), longest, device=dev())
    assert intact(out) and bool((out[GUARD:-GUARD] == -1).all())


def test_draws_are_uniform_over_the_complement():
    """Pearson's chi-square of the 30 allowed items' counts over 20,000 rows x 5 draws, 29 degrees of freedom: below 58.30, the 99.9 % point.  The kernel is bit-equal to
    the CPU reference (21.03 on these inputs), so this guards the definition rather than the launch."""
    u = F.UNIFORM
    ptr = torch.tensor([0, len(u['listed'])], dtype=torch.int64, device=dev())
    items = torch.tensor(u['listed'], dtype=torch.int32, device=dev())
    status, out = launch(u['rows'], u['n_items'], u['m'], np.zeros(u['rows'], np.int64), ptr, items, len(u['listed']), seed=u['seed'], counter=u['counter'])
    assert status == 0 and intact(out)
    draws = out[GUARD:-GUARD].view(u['rows'], u['m']).cpu().numpy()
    want = F.pool_draw_excluding(u['seed'], u['counter'], u['rows'], u['n_items'], u['m'], np.zeros(u['rows'], np.int64), np.array([0, 10]), np.array(u['listed']))
    assert (draws == want).all()
    chi2 = F.chi_square(draws, u['n_items'], u['listed'])
    print(f'chi-square of the 30 allowed items over {draws.size} draws: {chi2:.2f}')
    assert chi2 < F.CHI2_CRITICAL
