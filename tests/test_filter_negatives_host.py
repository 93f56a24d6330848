"""Filtered negatives (``--filter_negatives``) without a GPU: the kernel's chunked scheme is the sequential definition and its mutation is caught, the filtered rows are
the plain pool stream with the listed values deleted, and the host side - the entry point's refusals (which come before any launch), the symbol, the flag and what refuses
it, the host sampler, the startup share."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import filter_negatives_reference as F
import hard_negatives_reference as H
import logged_negatives_reference as L
from conftest import REPO

CPU = torch.device('cpu')


# ---------------------------------------------------------------------------------------------
# the stream
# ---------------------------------------------------------------------------------------------
def _case(n_rows, n_items, n_lists=13):
    ptr, items = F.make_lists(n_lists, n_items)
    return F.rows_to_lists(n_rows, n_lists), ptr, items


def test_chunked_draw_is_the_sequential_draw_and_the_list_check_matters():
    seed, counter = 11, 4
    for n_items, m in ((256, 156), (101, 1), (165, 65), (1000, 256), (1000, 17), (2 ** 40, 65)):
        rows, ptr, items = _case(20, n_items)
        want = F.pool_draw_excluding(seed, counter, 20, n_items, m, rows, ptr, items)
        assert (F.pool_draw_excluding_chunked(seed, counter, 20, n_items, m, rows, ptr, items) == want).all(), (n_items, m)
    # the list looked at for the first lane of a chunk only: listed values are drawn, and the rows leave the sequential stream
    rows, ptr, items = _case(20, 256)
    want = F.pool_draw_excluding(seed, counter, 20, 256, 156, rows, ptr, items)
    broken = F.pool_draw_excluding_chunked(seed, counter, 20, 256, 156, rows, ptr, items, mutation=F.MUTATIONS[0])
    assert (broken != want).any()
    assert any(np.isin(broken[r], F._run(rows, ptr, items, r)).any() for r in range(20))
    assert not any(np.isin(want[r], F._run(rows, ptr, items, r)).any() for r in range(20))


def test_the_corner_needs_few_chunks_and_gives_the_complement():
    """m + L = n_items = 256 with 65 rows: every row of a list of 100 is a permutation of the 156 items off its list, within 32 chunks of 64 attempts."""
    rows, ptr, items = _case(65, 256)
    chunks = []
    got = F.pool_draw_excluding_chunked(5, 9, 65, 256, 156, rows, ptr, items, chunks=chunks)
    assert max(chunks) <= 32
    full = 0
    for r in range(65):
        run = F._run(rows, ptr, items, r)
        assert len(set(got[r].tolist())) == 156 and not np.isin(got[r], run).any()
        if len(run) == 100:
            full += 1
            assert (np.sort(got[r]) == np.setdiff1d(np.arange(256), run)).all()
    assert full >= 10


def test_filtered_rows_are_the_pool_stream_with_the_listed_values_deleted():
    seed, counter = 7919 * 3 + 1, (5 << 32) + 17
    for n_items, m in ((356, 100), (1000, 64), (2 ** 40, 17)):
        rows, ptr, items = _case(65, n_items)
        unfiltered = H.pool_draw(seed, counter, 65, n_items, 256)
        got = F.pool_draw_excluding(seed, counter, 65, n_items, m, rows, ptr, items)
        assert (got == F.delete_listed(unfiltered, rows, ptr, items, m)).all(), (n_items, m)
        for c in (1, 16, m - 1):                                             # the first c columns are what a call with c gives
            assert (F.pool_draw_excluding(seed, counter, 65, n_items, c, rows, ptr, items) == got[:, :c]).all(), (n_items, m, c)
    # all lists empty, or every row id outside the lists: the plain pool, and for m <= 16 ihg_sample_negatives' reference
    empty_ptr, no_items = np.zeros(4, np.int64), np.zeros(0, np.int32)
    rows, ptr, items = _case(65, 1000)
    for m in (10, 16, 40):
        plain = H.pool_draw(seed, counter, 65, 1000, m)
        assert (F.pool_draw_excluding(seed, counter, 65, 1000, m, np.arange(65) % 3, empty_ptr, no_items) == plain).all()
        assert (F.pool_draw_excluding(seed, counter, 65, 1000, m, np.full(65, -1), ptr, items) == plain).all()
        assert (F.pool_draw_excluding(seed, counter, 65, 1000, m, np.full(65, 13), ptr, items) == plain).all()
        if m <= 16:
            assert (L.sample_negatives(seed, counter, 65, 1000, m) == plain).all()


def test_the_reference_is_uniform_over_the_complement():
    u = F.UNIFORM
    ptr, items = np.array([0, len(u['listed'])], np.int64), np.array(u['listed'], np.int32)
    draws = F.pool_draw_excluding(u['seed'], u['counter'], u['rows'], u['n_items'], u['m'], np.zeros(u['rows'], np.int64), ptr, items)
    chi2 = F.chi_square(draws, u['n_items'], u['listed'])
    print(f'chi-square of the 30 allowed items over {draws.size} draws: {chi2:.2f}')
    assert chi2 < F.CHI2_CRITICAL
    assert abs(chi2 - 21.03) < 0.005                                         # the recorded value for exactly these inputs: the stream has not moved


def test_cases_cover_the_ladder():
    assert {rows for rows, _, _ in F.POOL_CASES} == {1, 65, 300} and {m for _, m, _ in F.POOL_CASES} == {1, 16, 17, 64, 65, 256}
    for m in F.POOL_M:
        sizes = {n for _, mm, n in F.POOL_CASES if mm == m}
        assert sizes >= {1000, 2 ** 40} and ((m + F.LONGEST in sizes) == (m + F.LONGEST <= 256))
    ptr, items = F.make_lists(13, 1000)
    assert sorted(set(np.diff(ptr).tolist())) == [0, 1, 63, 64, 65, 100]
    for l in range(13):
        run = items[ptr[l]:ptr[l + 1]]
        assert (np.diff(run) > 0).all() and items.dtype == np.int32
    rows = F.rows_to_lists(65, 13)
    assert ((rows < 0) | (rows >= 13)).sum() == 2 and F.rows_to_lists(1, 13).tolist() == [-1]


# ---------------------------------------------------------------------------------------------
# the entry point's refusals, the symbol
# ---------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_before_any_launch():
    """This runs where there is no GPU: an answer at all means that nothing was launched."""
    from ihgnn_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)                                               # a non-null address that is never dereferenced

    def call(n_rows=5, n_items=1000, m=20, rows=p, n_lists=3, ptr=p, items=p, longest=100, out=p):
        return lib.ihg_sample_pool_excluding(1, 2, n_rows, n_items, m, rows, n_lists, ptr, items, longest, out, None)

    for m, n_items in ((0, 1000), (-1, 1000), (257, 1000), (11, 10), (1, 0)):
        assert call(m=m, n_items=n_items, longest=0) == _lib.ERR_INVALID, (m, n_items)
        assert 'ihg_sample_pool_excluding' in _lib.last_error() and '1 <= m <= min(256, n_items)' in _lib.last_error()
    for bad in (dict(n_lists=0), dict(n_lists=-2), dict(longest=-1)):
        assert call(**bad) == _lib.ERR_INVALID and 'n_lists >= 1 and max_list_len >= 0' in _lib.last_error(), bad
    for m, longest, n_items in ((20, 981, 1000), (256, 745, 1000), (1, 1000, 1000), (10, 2 ** 40, 2 ** 40)):
        assert call(m=m, longest=longest, n_items=n_items) == _lib.ERR_INVALID and 'm + max_list_len <= n_items' in _lib.last_error(), (m, longest, n_items)
    for operand in ('rows', 'ptr', 'items', 'out'):
        assert call(**{operand: None}) == _lib.ERR_INVALID and 'ihg_sample_pool_excluding: null pointer' in _lib.last_error(), operand
    assert call(n_rows=-1) == _lib.ERR_INVALID
    # no rows: nothing to write, nothing launched - once the sizes have passed
    assert call(n_rows=0, rows=None, ptr=None, items=None, out=None) == _lib.OK
    assert call(n_rows=0, m=20, longest=981) == _lib.ERR_INVALID
    assert call(n_rows=0, m=20, longest=980, rows=None, out=None) == _lib.OK                # the border m + max_list_len = n_items is legal


def test_symbol_is_declared_exported_and_the_abi_stays():
    from ihgnn_amd import _lib
    lib = _lib.load()
    assert lib.ihg_abi_version() == 37 and _lib.ABI_VERSION == 37           # an entry point was added, none changed
    header = open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read()
    name = 'ihg_sample_pool_excluding'
    assert re.search(r'^int ' + name + r'\(', header, re.M) and name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and hasattr(lib, name), f'{name} declared but not exported'
    # ihg_sample_pool's arguments with (list_of_row, n_lists, list_ptr, list_items, max_list_len) in front of `out`
    pool = _lib.SIGNATURES['ihg_sample_pool'][1]
    v, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib.SIGNATURES[name] == (ctypes.c_int, pool[:5] + [v, i64, v, v, i64] + pool[5:])
    declared = re.search(r'^int ' + name + r'\((.*?)\);', header, re.M | re.S).group(1)
    assert [a.split()[-1].lstrip('*') for a in declared.split(',')] == ['seed', 'counter', 'n_rows', 'n_items', 'm', 'list_of_row', 'n_lists', 'list_ptr', 'list_items',
                                                                       'max_list_len', 'out', 'stream']


def test_op_checks_its_tensors_on_the_host():
    from ihgnn_amd import _lib, ops
    rows, ptr, items = torch.zeros(5, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    for bad in ((rows.int(), (ptr, items)), (rows, (ptr.int(), items)), (rows, (ptr, items.long())), (rows.reshape(5, 1), (ptr, items))):
        with pytest.raises(TypeError, match='sample_pool_excluding'):
            ops.sample_pool_excluding(1, 2, 5, 100, 10, bad[0], bad[1], 0, device='cuda:0')
    with pytest.raises(_lib.IhgnnHipError, match='GPU tensor'):
        ops.sample_pool_excluding(1, 2, 5, 100, 10, rows, (ptr, items), 0, device='cuda:0')       # CPU tensors: refused for what they are - there is no fall-back


# ---------------------------------------------------------------------------------------------
# the flag, the settings, the driver's refusals
# ---------------------------------------------------------------------------------------------
def _dataset(k=2, **kwargs):
    """The seven-item dataset of ``test_exclude_host``: user 0 has items 1, 4; user 1 none; user 2 item 0; user 3 items 0, 5, 6."""
    from ihgnn_amd.Dataset import GraphDataset
    from test_exclude_host import _dataset as base
    triples = base().pos_triples
    return GraphDataset.from_arrays(4, 4, 7, 6, np.arange(4), np.arange(4), triples, random_negative_sample_size=k, device=CPU, **kwargs)


def test_flag_and_settings():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    assert Gs.Training.filter_negatives is False and parse_args([]).filter_negatives is False
    assert parse_args(['--filter_negatives']).filter_negatives is True
    kept = Gs.non_random_negative_sample_size
    try:
        driver.apply_training_settings(parse_args(['--filter_negatives', '--hard_negatives', '50', '--loss', 'bpr', '--clip_grad_norm', '1']))
        assert Gs.Training.filter_negatives is True and Gs.Training.negative_pool == 50 and Gs.Training.loss == 'bpr'
        driver.apply_training_settings(parse_args([]))                       # assigned both ways: a run without the flag draws uniformly, whatever ran before it
        assert Gs.Training.filter_negatives is False
        driver.apply_training_settings(parse_args(['--filter_negatives']))
        assert Gs.Training.filter_negatives is True
        with pytest.raises(ValueError, match='--filter_negatives.*--logged_negatives'):
            driver.apply_training_settings(parse_args(['--filter_negatives', '--logged_negatives', '2']))
        with pytest.raises(ValueError, match='--filter_negatives.*--logged_negatives'):
            driver.apply_training_settings(parse_args(['--filter_negatives', '--logged_negatives', '2', '--device_sampling']))      # on both loaders
        Gs.non_random_negative_sample_size = 3                               # the setting edited in place, as the reference is driven
        with pytest.raises(ValueError, match='--filter_negatives.*--logged_negatives'):
            driver.apply_training_settings(parse_args(['--filter_negatives']))
    finally:
        Gs.non_random_negative_sample_size = kept
        Gs.Training.loss, Gs.Training.negative_pool, Gs.Training.clip_grad_norm, Gs.Training.filter_negatives = 'bce', 0, 0.0, False
    driver.check_srrl_settings(parse_args(['--model', 'Srrl']), 1)
    with pytest.raises(NotImplementedError, match='--filter_negatives'):
        driver.check_srrl_settings(parse_args(['--model', 'Srrl', '--filter_negatives']), 1)


def test_half_catalogue_policy_and_the_datasets_own_checks():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Dataset import GraphDataset
    ds = _dataset()
    assert ds.max_user_items == 3 and ds.max_user_items == 3 and ds.filter_negatives is False
    with pytest.raises(ValueError, match='--filter_negatives.*half the catalogue'):
        driver.check_filtered_negatives(ds, 1)                               # 1 + 3 > 7 // 2
    with pytest.raises(ValueError, match='--filter_negatives.*half the catalogue'):
        driver.check_filtered_negatives(ds, 2)
    # twenty items, the longest history three: up to seven negatives per positive pass, eight do not
    triples = np.array([[0, 0, 4], [0, 0, 5], [0, 0, 19], [1, 0, 2]], np.int64)
    wide = GraphDataset.from_arrays(2, 1, 20, 1, np.zeros(1, np.int64), np.zeros(1, np.int64), triples, device=CPU)
    driver.check_filtered_negatives(wide, 7)
    with pytest.raises(ValueError, match='8 negatives per positive \\+ 3 items'):
        driver.check_filtered_negatives(wide, 8)
    with pytest.raises(ValueError, match='filter_negatives.*logged'):
        GraphDataset.from_arrays(2, 1, 20, 1, np.zeros(1, np.int64), np.zeros(1, np.int64), triples, non_random_negative_sample_size=1, device=CPU, filter_negatives=True)
    too_many = _dataset(k=5, filter_negatives=True)                          # user 3: 5 + 3 > 7 - no five unseen items exist
    with pytest.raises(ValueError, match='filter_negatives'):
        too_many[1]
    assert len(too_many[3][1]) == 5                                          # user 2 has one item: five of the other six


def test_getitem_draws_outside_the_users_items():
    ds = _dataset(filter_negatives=True)
    ptr, items = ds.user_item_lists
    random.seed(3)
    for draw in range(200):
        index = draw % len(ds)
        (u, q, i, flag), negatives = ds[index]
        assert (u, q, i) == tuple(ds.pos_triples[index]) and flag == 1
        seen = set(items[ptr[u]:ptr[u + 1]].tolist())
        assert len(negatives) == 2 and len(set(negatives)) == 2 and not seen & set(negatives) and all(0 <= n < 7 for n in negatives)
        assert i in seen                                                      # (so the positive itself is never a negative)
    assert ds.user_item_set(3) == {0, 5, 6} and ds.user_item_set(1) == frozenset() and ds.user_item_set(3) is ds.user_item_set(3)


def test_getitem_without_the_flag_is_random_sample():
    ds = _dataset()
    for s in (0, 1, 77):
        for index in range(len(ds)):
            random.seed(s)
            want = random.sample(range(7), 2)
            random.seed(s)
            assert ds[index] == (tuple(ds.pos_triples[index]) + (1,), want)
    assert '_user_item_sets' not in ds.__dict__                              # nothing of the filter is built


def test_startup_share_is_a_brute_force_count():
    from ihgnn_amd import Main as driver
    ds = _dataset()
    hits = sum(1 for u, _, _ in ds.pos_triples.tolist() for item in range(7) if any(uu == u and ii == item for uu, _, ii in ds.pos_triples.tolist()))
    assert hits == 3 * 2 + 1 * 1 + 3 * 3
    assert driver.own_item_share(ds) == pytest.approx(hits / (7 * 7), abs=1e-15)
