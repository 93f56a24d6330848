"""Popularity-weighted negatives (``--popularity_negatives``) without a GPU: the kernel's chunked scheme is the sequential definition and its mutations are caught on the
GPU tests' own cases, unit and equal weights give the uniform streams' bits, the first accepted value follows the weights over the complement, and the host side - the entry
point's refusals (which come before any launch), the symbol, the weights and the table, the flag and what refuses it, the mass policy, the host sampler, the startup shares."""
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
import popularity_negatives_reference as P
from conftest import REPO

CPU = torch.device('cpu')


# ---------------------------------------------------------------------------------------------
# the stream
# ---------------------------------------------------------------------------------------------
def test_chunked_draw_is_the_sequential_draw_on_the_gpu_cases():
    """Every ``squares`` case of the GPU test with its lists, the whole-complement corner included.  Row r's draw does not depend on the number of rows but its list does
    (``rows_to_lists``), so the 300-row cases are held to the definition on their first, middle and last 20 rows."""
    checked = 0
    for rows, m, n_items, name in P.GPU_CASES:
        if name != 'squares':
            continue
        want, attempts = P.expected(rows, m, n_items, name)
        assert attempts.max() <= P.MAX_ATTEMPTS and attempts.min() >= m, (rows, m, n_items)
        ptr, items = P.lists_of(n_items)
        of_row = P.rows_to_lists(rows, P.N_LISTS)
        keep = np.arange(rows) if rows <= 65 else np.r_[0:20, rows // 2 - 10:rows // 2 + 10, rows - 20:rows]
        got = P.pool_draw_weighted_chunked(P.SEED, P.COUNTER, rows, n_items, m, P.table(name, n_items), of_row, ptr, items, only=keep)
        assert (got[keep] == want[keep]).all(), (rows, m, n_items)
        checked += 1
    assert checked == 34


def test_each_mutation_leaves_the_definition_on_a_gpu_case():
    # the low half of the threshold only: the squares table's sum is 25.5 * 2^29 per item, so every case has thresholds beyond 2^32 (the mutated draw reaches the first
    # three items only and is cut off)
    rows, m, n_items, name = case = (65, 17, 1000, 'squares')
    assert case in P.GPU_CASES
    want, _ = P.expected(*case)
    ptr, items = P.lists_of(n_items)
    of_row = P.rows_to_lists(rows, P.N_LISTS)
    cum = P.table(name, n_items)
    assert int(cum[-1]) > 2 ** 32
    assert (P.pool_draw_weighted_chunked(P.SEED, P.COUNTER, rows, n_items, m, cum, of_row, ptr, items) == want).all()
    assert (P.pool_draw_weighted_chunked(P.SEED, P.COUNTER, rows, n_items, m, cum, of_row, ptr, items, mutation=P.MUTATIONS[0]) != want).any()
    # the lower bound: a threshold that equals cum[i] belongs to item i, not i - 1.  With weights of 2^29 and more that is one threshold in 2^29; with the unit table of
    # the equivalence cases it is every threshold
    assert 16 in P.EQUIVALENCE_M
    unit = P.table('unit', 1000)
    plain = P.pool_draw_weighted(P.SEED, P.COUNTER, 20, 1000, 16, unit)
    assert (P.pool_draw_weighted_chunked(P.SEED, P.COUNTER, 20, 1000, 16, unit) == plain).all()
    assert (P.pool_draw_weighted_chunked(P.SEED, P.COUNTER, 20, 1000, 16, unit, mutation=P.MUTATIONS[1]) != plain).any()


def test_unit_and_equal_weights_give_the_uniform_streams():
    """The three consequences of the header: ``cum[i] = i`` (and every weight 2^32, because ``umulhi(r, I 2^32) >> 32 == umulhi(r, I)``) is the filtered pool draw, without
    lists the pool draw, for m <= 16 the 16-draw sampler; and the first c columns of a call with m are a call with c."""
    seed, counter = 7919 * 3 + 1, (5 << 32) + 17
    for n_items in (356, 1000):
        ptr, items = P.lists_of(n_items)
        of_row = P.rows_to_lists(65, P.N_LISTS)
        for name in ('unit', 'equal'):
            cum = P.table(name, n_items)
            for m in (1, 10, 16, 17, 100, 256):
                got = P.pool_draw_weighted(seed, counter, 65, n_items, m, cum, of_row, ptr, items)
                assert (got == F.pool_draw_excluding(seed, counter, 65, n_items, m, of_row, ptr, items)).all(), (n_items, name, m)
                bare = P.pool_draw_weighted(seed, counter, 65, n_items, m, cum)
                assert (bare == H.pool_draw(seed, counter, 65, n_items, m)).all(), (n_items, name, m)
                if m <= 16:
                    assert (bare == L.sample_negatives(seed, counter, 65, n_items, m)).all(), (n_items, name, m)
    # the prefix property on a weighted table with lists
    ptr, items = P.lists_of(1000)
    of_row = P.rows_to_lists(65, P.N_LISTS)
    for name in ('squares', 'powerlaw'):
        cum = P.table(name, 1000)
        whole = P.pool_draw_weighted(seed, counter, 65, 1000, 100, cum, of_row, ptr, items)
        for c in (1, 16, 17, 64, 65, 99):
            assert (P.pool_draw_weighted(seed, counter, 65, 1000, c, cum, of_row, ptr, items) == whole[:, :c]).all(), (name, c)
        for row in range(65):
            assert len(set(whole[row].tolist())) == 100 and not np.isin(whole[row], F._run(of_row, ptr, items, row)).any()


def test_cases_reach_both_ends_of_the_catalogue_and_the_corner_gives_the_complement():
    drawn = {}
    for case in P.GPU_CASES:
        rows, m, n_items, name = case
        want, attempts = P.expected(*case)
        assert attempts.max() <= P.MAX_ATTEMPTS, case                        # what lets the GPU test run these rows at all
        assert want.min() >= 0 and want.max() < n_items
        drawn.setdefault((n_items, name), set()).update(np.unique(want).tolist())
    for key in ((1000, 'squares'), (1000, 'powerlaw'), (256, 'squares')):      # the lightest item of `squares` is item 0, the lightest of `powerlaw` the last
        assert 0 in drawn[key] and key[0] - 1 in drawn[key], key
    assert {rows for rows, _, _, _ in P.GPU_CASES} == {1, 65, 300} and {m for _, m, _, _ in P.GPU_CASES} == set(P.POOL_M) | {156}
    assert all(name == 'squares' and n <= 256 for _, m, n, name in P.GPU_CASES if m + P.LONGEST == n)
    rows, m, n_items = P.CORNER
    want, _ = P.expected(rows, m, n_items, 'squares')
    ptr, items = P.lists_of(n_items)
    of_row = P.rows_to_lists(rows, P.N_LISTS)
    full = 0
    for row in range(rows):
        run = F._run(of_row, ptr, items, row)
        if len(run) == P.LONGEST:
            full += 1
            assert (np.sort(want[row]) == np.setdiff1d(np.arange(n_items), run)).all()
    assert full >= 8
    weights = np.diff(P.table('squares', n_items))
    assert weights.max() // weights.min() == 64


@pytest.mark.parametrize('law, recorded, most_attempts', [(P.SQUARES_LAW, (29.1, 29.3), 9), (P.POWERLAW_LAW, (69.9, 73.1), 1)], ids=['squares', 'powerlaw'])
def test_first_accepted_value_follows_the_weights_over_the_complement(law, recorded, most_attempts):
    """Column 0 only: its law is exactly the weights renormalised over the items off the list (later columns also depend on what was accepted before).  Pearson's
    chi-square against the 99.9 % point, on both streams; the recorded values say that the stream has not moved."""
    cum = P.table(law['table'], law['n_items'])
    listed = np.array(law['listed'], np.int64)
    for (seed, counter), value in zip(P.STREAMS, recorded):
        first, attempts = P.first_draw_weighted(seed, counter, law['rows'], cum, listed)
        lead = 300
        by_definition = P.pool_draw_weighted(seed, counter, lead, law['n_items'], 1, cum, np.zeros(lead, np.int64), np.array([0, len(listed)]), listed)
        assert (first[:lead] == by_definition[:, 0]).all()
        chi2, smallest = P.chi_square_weighted(first, cum, listed)
        print(f'{law["table"]} over {law["n_items"]} items, {law["rows"]} rows, stream {(seed, counter)}: chi-square {chi2:.2f} (critical {law["critical"]}), '
              f'smallest expected count {smallest:.1f}, most attempts {attempts.max()}')
        assert chi2 <= law['critical']
        assert abs(chi2 - value) < 0.06 and attempts.max() <= most_attempts and smallest >= 5
    if law is P.POWERLAW_LAW:
        assert abs(smallest - 1131) < 1


# ---------------------------------------------------------------------------------------------
# the entry point's refusals, the symbol
# ---------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_before_any_launch():
    """This runs where there is no GPU: an answer at all means that nothing was launched."""
    from ihgnn_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)                                               # a non-null address that is never dereferenced

    def call(n_rows=5, n_items=1000, m=20, cum=p, total=1000 << 32, rows=p, n_lists=3, ptr=p, items=p, longest=100, out=p):
        return lib.ihg_sample_pool_weighted(1, 2, n_rows, n_items, m, cum, total, rows, n_lists, ptr, items, longest, out, None)

    for m, n_items in ((0, 1000), (-1, 1000), (257, 1000), (11, 10), (1, 0)):
        assert call(m=m, n_items=n_items, longest=0, total=2 ** 40) == _lib.ERR_INVALID, (m, n_items)
        assert 'ihg_sample_pool_weighted' in _lib.last_error() and '1 <= m <= min(256, n_items)' in _lib.last_error()
    for total in (999, 0, -1, -2 ** 63):                                    # below one per item; 2^63 and beyond do not fit the int64 and arrive negative
        assert call(total=total) == _lib.ERR_INVALID and 'n_items <= total < 2^63' in _lib.last_error(), total
    assert call(n_rows=0, total=1000) == _lib.OK and call(n_rows=0, total=2 ** 63 - 1) == _lib.OK
    for bad in (dict(n_lists=-1), dict(n_lists=-2 ** 40), dict(longest=-1)):
        assert call(**bad) == _lib.ERR_INVALID and 'n_lists >= 0 and max_list_len >= 0' in _lib.last_error(), bad
    for m, longest, n_items in ((20, 981, 1000), (256, 745, 1000), (1, 1000, 1000), (10, 2 ** 20, 2 ** 20)):
        assert call(m=m, longest=longest, n_items=n_items, total=2 ** 60) == _lib.ERR_INVALID and 'm + max_list_len <= n_items' in _lib.last_error(), (m, longest, n_items)
    for operand in ('cum', 'rows', 'ptr', 'items', 'out'):
        assert call(**{operand: None}) == _lib.ERR_INVALID and 'ihg_sample_pool_weighted: null pointer' in _lib.last_error(), operand
    for operand in ('cum', 'out'):                                          # without lists the list pointers may be null, these two may not
        assert call(n_lists=0, rows=None, ptr=None, items=None, longest=0, **{operand: None}) == _lib.ERR_INVALID and 'null pointer' in _lib.last_error(), operand
    assert call(n_rows=-1) == _lib.ERR_INVALID
    # no rows: nothing to write, nothing launched - once the sizes have passed
    assert call(n_rows=0, cum=None, rows=None, ptr=None, items=None, out=None) == _lib.OK
    assert call(n_rows=0, n_lists=0, cum=None, rows=None, ptr=None, items=None, out=None, longest=0) == _lib.OK
    assert call(n_rows=0, m=20, longest=981) == _lib.ERR_INVALID
    assert call(n_rows=0, m=20, longest=980, rows=None, out=None) == _lib.OK                # the border m + max_list_len = n_items is legal


def test_symbol_is_declared_exported_and_the_abi_stays():
    from ihgnn_amd import _lib
    lib = _lib.load()
    assert lib.ihg_abi_version() == 37 and _lib.ABI_VERSION == 37           # an entry point was added, none changed
    header = open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read()
    name = 'ihg_sample_pool_weighted'
    assert re.search(r'^int ' + name + r'\(', header, re.M) and name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and hasattr(lib, name), f'{name} declared but not exported'
    # ihg_sample_pool_excluding's arguments with (cum, total) after m
    excluding = _lib.SIGNATURES['ihg_sample_pool_excluding'][1]
    assert _lib.SIGNATURES[name] == (ctypes.c_int, excluding[:5] + [ctypes.c_void_p, ctypes.c_int64] + excluding[5:])
    declared = re.search(r'^int ' + name + r'\((.*?)\);', header, re.M | re.S).group(1)
    assert [a.split()[-1].lstrip('*') for a in declared.split(',')] == ['seed', 'counter', 'n_rows', 'n_items', 'm', 'cum', 'total', 'list_of_row', 'n_lists', 'list_ptr',
                                                                       'list_items', 'max_list_len', 'out', 'stream']


def test_ops_check_their_operands_on_the_host():
    from ihgnn_amd import _lib, ops
    # the table: the one place where the launch's promise of a strictly ascending cum is checked - before anything goes to a device
    for bad, told in ((np.array([5, 0, 3]), 'every weight must be >= 1'), (np.array([5, -2, 3]), 'every weight must be >= 1'),
                      (torch.tensor([4, 0], dtype=torch.int64), 'every weight must be >= 1'), (np.array([2 ** 62, 2 ** 62]), r'2\^63 or more'),
                      (np.array([2 ** 62, 2 ** 62 - 1, 1]), r'2\^63 or more')):
        with pytest.raises(ValueError, match=told):
            ops.item_sampling_table(bad, device='cuda:0')
    for bad in (np.array([1.0, 2.0]), np.array([1, 2], np.int32), np.ones((2, 2), np.int64), np.zeros(0, np.int64)):
        with pytest.raises(TypeError, match='item_sampling_table'):
            ops.item_sampling_table(bad, device='cuda:0')
    cum = torch.arange(101, dtype=torch.int64)
    rows, ptr, items = torch.zeros(5, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    for table, r, lists in (((cum.int(), 100), None, None), ((cum.reshape(1, -1), 100), None, None), ((cum, 100), rows.int(), (ptr, items)), ((cum, 100), rows, (ptr.int(), items)),
                            ((cum, 100), rows, (ptr, items.long()))):
        with pytest.raises(TypeError, match='sample_pool_weighted'):
            ops.sample_pool_weighted(1, 2, 5, 100, 10, table, r, lists, 0, device='cuda:0')
    with pytest.raises(ValueError, match='rows and lists come together'):
        ops.sample_pool_weighted(1, 2, 5, 100, 10, (cum, 100), rows, None, 0, device='cuda:0')
    with pytest.raises(ValueError, match='rows and lists come together'):
        ops.sample_pool_weighted(1, 2, 5, 100, 10, (cum, 100), None, (ptr, items), 0, device='cuda:0')
    with pytest.raises(_lib.IhgnnHipError, match='GPU tensor'):
        ops.sample_pool_weighted(1, 2, 5, 100, 10, (cum, 100), device='cuda:0')                    # CPU tensors: refused for what they are - there is no fall-back


# ---------------------------------------------------------------------------------------------
# the dataset: weights, table, the host sampler
# ---------------------------------------------------------------------------------------------
def _dataset(k=2, **kwargs):
    """The seven-item dataset of ``test_exclude_host``: user 0 has items 1, 4; user 1 none; user 2 item 0; user 3 items 0, 5, 6."""
    from ihgnn_amd.Dataset import GraphDataset
    from test_exclude_host import _dataset as base
    triples = base().pos_triples
    return GraphDataset.from_arrays(4, 4, 7, 6, np.arange(4), np.arange(4), triples, random_negative_sample_size=k, device=CPU, **kwargs)


def _skewed(items=40, k=2, **kwargs):
    """``items`` items of which item i is bought ``1000 // (i + 1) // 40`` times (25, 12, 8, 6, 5, 4, 3, 3, 2, 2, 2, 2, 1 ..., 0 from item 25 on), each time by another of
    ten users in turn."""
    from ihgnn_amd.Dataset import GraphDataset
    item = np.repeat(np.arange(items), 1000 // (np.arange(items) + 1) // 40)
    triples = np.stack([np.arange(len(item)) % 10, np.zeros(len(item), np.int64), item], 1).astype(np.int64)
    return GraphDataset.from_arrays(10, 1, items, 1, np.zeros(1, np.int64), np.zeros(1, np.int64), triples, random_negative_sample_size=k, device=CPU, **kwargs)


def test_item_sampling_weights():
    ds = _skewed(popularity_power=0.75)
    counts = np.bincount(ds.pos_triples[:, 2], minlength=40)
    w = ds.item_sampling_weights
    assert w.dtype == np.int64 and w.shape == (40,) and w.min() >= 1 and w.max() == 2 ** 32 and w[0] == 2 ** 32 and counts[-1] == 0
    assert (w == P.dataset_weights(counts, 0.75)).all() and ds.item_sampling_weights is w
    order = np.argsort(counts, kind='stable')
    assert (np.diff(w[order]) >= 0).all() and all(w[a] == w[b] for a in range(40) for b in range(40) if counts[a] == counts[b])
    assert w[counts == 0].min() == round(2 ** 32 * (1 / 26) ** 0.75)        # a never-bought item can still be drawn
    assert (_skewed(popularity_power=1.0).item_sampling_weights == np.rint(2.0 ** 32 * (counts + 1) / 26)).all()
    # an exponent next to 0 gives the `equal` table: the uniform draw
    flat = _skewed(popularity_power=1e-12)
    assert (flat.item_sampling_weights == P.equal_weights(40)).all()
    cum, total = flat.item_sampling_cum
    assert cum == P.table('equal', 40).tolist() and total == 40 << 32
    off = _skewed()
    assert off.popularity_power == 0.0
    with pytest.raises(ValueError, match='popularity_power = 0'):
        off.item_sampling_weights


def test_dataset_refusals():
    from ihgnn_amd.Dataset import GraphDataset
    for bad in (-0.1, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='popularity_power must be in'):
            _dataset(popularity_power=bad)
    triples = np.array([[0, 0, 4], [0, 0, 5], [0, 0, 19], [1, 0, 2]], np.int64)
    with pytest.raises(ValueError, match='popularity_power.*logged'):
        GraphDataset.from_arrays(2, 1, 20, 1, np.zeros(1, np.int64), np.zeros(1, np.int64), triples, non_random_negative_sample_size=1, device=CPU, popularity_power=0.75)
    with pytest.raises(ValueError, match='popularity_power'):
        _dataset(k=8, popularity_power=0.75)[0]                              # eight distinct items of seven
    too_many = _dataset(k=5, filter_negatives=True, popularity_power=0.75)   # user 3: 5 + 3 > 7 - no five unseen items exist
    with pytest.raises(ValueError, match='popularity_power'):
        too_many[1]
    assert len(too_many[3][1]) == 5                                          # user 2 has one item: five of the other six


def test_getitem_draws_weighted_distinct_and_unseen_under_the_filter():
    for filtered in (False, True):
        ds = _dataset(filter_negatives=filtered, popularity_power=0.75)
        ptr, items = ds.user_item_lists
        random.seed(3)
        own = 0
        for draw in range(300):
            index = draw % len(ds)
            (u, q, i, flag), negatives = ds[index]
            assert (u, q, i) == tuple(ds.pos_triples[index]) and flag == 1
            seen = set(items[ptr[u]:ptr[u + 1]].tolist())
            assert len(negatives) == 2 and len(set(negatives)) == 2 and all(0 <= n < 7 for n in negatives)
            own += len(seen & set(negatives))
        assert (own == 0) == filtered
    # the draw is bisect_right over the running sum at random.randrange(total): the stream can be replayed
    ds = _skewed(popularity_power=0.75)
    cum, total = ds.item_sampling_cum
    assert cum[0] == 0 and total == cum[-1] == int(ds.item_sampling_weights.sum()) and len(cum) == 41
    random.seed(11)
    _, got = ds[0]
    random.seed(11)
    want = []
    while len(want) < 2:
        t = random.randrange(total)
        item = max(i for i in range(40) if cum[i] <= t)
        if item not in want:
            want.append(item)
    assert got == want
    # and it is weighted: the most bought item of forty comes far more often than one in forty
    random.seed(5)
    firsts = [ds[0][1][0] for _ in range(2000)]
    share = ds.item_sampling_weights[0] / ds.item_sampling_weights.sum()
    assert share > 0.1 and abs(firsts.count(0) / 2000 - share) < 4 * np.sqrt(share * (1 - share) / 2000)


def test_getitem_without_the_flag_is_random_sample():
    ds = _dataset()
    for s in (0, 1, 77):
        for index in range(len(ds)):
            random.seed(s)
            want = random.sample(range(7), 2)
            random.seed(s)
            assert ds[index] == (tuple(ds.pos_triples[index]) + (1,), want)
    assert not {'_item_weights', '_item_cum', '_item_table_device'} & set(ds.__dict__)          # nothing of the weighted draw is built


# ---------------------------------------------------------------------------------------------
# the flag, the settings, the driver's refusals
# ---------------------------------------------------------------------------------------------
def _reset():
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    Gs.Training.loss, Gs.Training.negative_pool, Gs.Training.clip_grad_norm, Gs.Training.filter_negatives, Gs.Training.popularity_power = 'bce', 0, 0.0, False, 0.0


def test_flag_and_settings():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Helpers.ArgsParser import checked_popularity_power, parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    assert Gs.Training.popularity_power == 0.0 and parse_args([]).popularity_negatives == 0.0
    assert parse_args(['--popularity_negatives']).popularity_negatives == 0.75                  # a bare flag
    assert parse_args(['--popularity_negatives', '--filter_negatives']).popularity_negatives == 0.75
    assert parse_args(['--popularity_negatives', '0.5']).popularity_negatives == 0.5 and parse_args(['--popularity_negatives', '1']).popularity_negatives == 1.0
    for bad in ('-0.25', '1.01', 'nan', 'inf', 'often'):
        with pytest.raises(SystemExit):
            parse_args(['--popularity_negatives', bad])
        with pytest.raises(ValueError, match='--popularity_negatives'):
            checked_popularity_power(bad)
    kept = Gs.non_random_negative_sample_size

    class Args:                                                              # a caller that builds its own args gets the parser's check
        popularity_negatives = 1.5
    try:
        driver.apply_training_settings(parse_args(['--popularity_negatives', '--filter_negatives', '--hard_negatives', '50', '--loss', 'bpr', '--clip_grad_norm', '1']))
        assert Gs.Training.popularity_power == 0.75 and Gs.Training.filter_negatives is True and Gs.Training.negative_pool == 50 and Gs.Training.loss == 'bpr'
        driver.apply_training_settings(parse_args([]))                       # assigned both ways: a run without the flag draws uniformly, whatever ran before it
        assert Gs.Training.popularity_power == 0.0
        for loss in ('bce', 'bpr', 'softmax'):
            driver.apply_training_settings(parse_args(['--popularity_negatives', '0.5', '--loss', loss]))
            assert Gs.Training.popularity_power == 0.5 and Gs.Training.loss == loss
        with pytest.raises(ValueError, match='--popularity_negatives takes an exponent'):
            driver.apply_training_settings(Args())
        assert Gs.Training.popularity_power == 0.5                           # a refusal assigns nothing
        with pytest.raises(ValueError, match='--popularity_negatives.*--logged_negatives'):
            driver.apply_training_settings(parse_args(['--popularity_negatives', '--logged_negatives', '2']))
        with pytest.raises(ValueError, match='--popularity_negatives.*--logged_negatives'):
            driver.apply_training_settings(parse_args(['--popularity_negatives', '--logged_negatives', '2', '--device_sampling']))      # on both loaders
        Gs.non_random_negative_sample_size = 3                               # the setting edited in place, as the reference is driven
        with pytest.raises(ValueError, match='--popularity_negatives.*--logged_negatives'):
            driver.apply_training_settings(parse_args(['--popularity_negatives']))
    finally:
        Gs.non_random_negative_sample_size = kept
        _reset()
    driver.check_srrl_settings(parse_args(['--model', 'Srrl']), 1)
    with pytest.raises(NotImplementedError, match='--popularity_negatives'):
        driver.check_srrl_settings(parse_args(['--model', 'Srrl', '--popularity_negatives']), 1)


def test_mass_policy_on_a_dataset_built_to_cross_it():
    """Forty items; the weights are ``dataset_weights`` of the counts.  The policy: the ``per_positive`` heaviest weights, plus under the filter the heaviest user history,
    stay within half of the sum."""
    from ihgnn_amd import Main as driver
    ds = _skewed(popularity_power=1.0)
    w = np.sort(ds.item_sampling_weights)[::-1]
    total = int(w.sum())
    most = int(np.flatnonzero(2 * np.cumsum(w) <= total).max()) + 1          # the largest count of negatives whose heaviest choice is within half
    assert 1 <= most < 10
    driver.check_popularity_negatives(ds, most)
    with pytest.raises(ValueError) as refused:
        driver.check_popularity_negatives(ds, most + 1)
    assert f'weigh {int(w[:most + 1].sum())}' in str(refused.value) and f'({total}, 40 items)' in str(refused.value) and 'the heaviest user history' not in str(refused.value)
    # a flatter exponent passes the same count
    driver.check_popularity_negatives(_skewed(popularity_power=0.25), most + 1)
    # under the filter the heaviest history counts as well: what passed alone is refused with it
    filtered = _skewed(popularity_power=1.0, filter_negatives=True)
    ptr, items = filtered.user_item_lists
    history = max(int(filtered.item_sampling_weights[items[ptr[u]:ptr[u + 1]]].sum()) for u in range(10))
    assert history > 0 and 2 * (int(w[:most].sum()) + history) > total
    with pytest.raises(ValueError) as refused:
        driver.check_popularity_negatives(filtered, most)
    assert f'weigh {int(w[:most].sum()) + history}' in str(refused.value) and 'the heaviest user history' in str(refused.value)
    # one negative and a light history pass
    wide = _skewed(items=400, popularity_power=0.75, filter_negatives=True)
    driver.check_popularity_negatives(wide, 10)


def test_startup_shares_are_brute_force_counts():
    from ihgnn_amd import Main as driver
    ds = _skewed(items=400, popularity_power=0.75)
    w = ds.item_sampling_weights.astype(np.float64)
    shares = driver.popularity_shares(ds)
    assert shares['head_items'] == 4 and shares['uniform_head_share'] == 0.01
    assert shares['head_share'] == pytest.approx(w[:4].sum() / w.sum(), rel=1e-12) and shares['head_share'] > 4 * 0.01
    triples = ds.pos_triples.tolist()
    bought = {}
    for u, _, i in triples:
        bought.setdefault(u, set()).add(i)
    own = sum(w[sorted(bought[u])].sum() for u, _, _ in triples) / (len(triples) * w.sum())
    assert shares['own_item_share'] == pytest.approx(own, rel=1e-12)
    assert shares['own_item_share'] > driver.own_item_share(ds)              # popular items are the ones a user is most likely to have: the hint to add the filter
    small = _dataset(popularity_power=0.5)
    assert driver.popularity_shares(small)['head_items'] == 1                # (user 1 has no items: an empty run of the CSR)
