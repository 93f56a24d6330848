"""Logged (non-random) negatives on the host: the list layout the device sampler reads (``GraphDataset.logged_negative_lists``), the reference's sampling rule in
``GraphDataset.__getitem__`` (``Dataset.py:107-119``), the numpy emulation of ``ihg_device_batch`` (``tests/logged_negatives_reference.py``) - its structure, its
generator contract and the uniformity of its position stream - and the ``--logged_negatives`` flag.  The GPU is held bit for bit to the emulation in
``tests/test_logged_negatives_kernel.py``, so the statistics checked here need no GPU run."""
import os
import random
import re

import numpy as np
import pytest
import torch

import logged_negatives_reference as R
from conftest import GOLDEN, REPO

CPU = torch.device('cpu')


def file_dataset(name, rand=10, nonrand=0):
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    d = os.path.join(GOLDEN, name)
    return GraphDataset(os.path.join(d, 'graph_info.txt'), os.path.join(d, 'queries_multihot.txt'), os.path.join(d, 'train_data.csv'), PpsHyperGraph, rand, nonrand, CPU)


def array_dataset(rand=3, nonrand=2, items=12):
    """``items`` items (12; every id used is below 12); pair (0, 0) has five logged negatives with a repeat, (1, 1) one, (2, 0) none, (3, 3) is logged without a positive; (0, 0) has two positives."""
    from ihgnn_amd.Dataset import GraphDataset
    triples = np.array([[0, 0, 1], [1, 1, 2], [2, 0, 3], [0, 0, 4]], np.int64)
    neg = np.array([[0, 0, 7], [1, 1, 5], [0, 0, 9], [3, 3, 2], [0, 0, 7], [0, 0, 11], [3, 3, 4], [0, 0, 8]], np.int64)
    ds = GraphDataset.from_arrays(4, 4, items, 6, np.array([0, 1, 2, 3], np.int64), np.array([0, 1, 2, 3], np.int64), triples,
                                  random_negative_sample_size=rand, non_random_negative_sample_size=nonrand, device=CPU, neg_triples=neg)
    return ds


def assert_lists_match_the_dict(ds):
    pair_of_edge, neg_ptr, neg_items = ds.logged_negative_lists
    table = ds.neg_items_for_user_query_pair
    assert pair_of_edge.dtype == np.int32 and neg_ptr.dtype == np.int64 and neg_items.dtype == np.int32
    assert pair_of_edge.shape == (len(ds),) and neg_ptr[0] == 0 and neg_ptr[-1] == len(neg_items) and bool((np.diff(neg_ptr) >= 0).all())
    pairs = {}
    for e, (u, q, _) in enumerate(ds.pos_triples.tolist()):
        p = int(pair_of_edge[e])
        assert pairs.setdefault(p, (u, q)) == (u, q)                          # one index per pair ...
        assert neg_items[neg_ptr[p]:neg_ptr[p + 1]].tolist() == table.get((u, q), [])
    assert sorted(pairs) == list(range(len(neg_ptr) - 1)) and len(set(pairs.values())) == len(pairs)      # ... every index used, no pair twice
    with_positive = set(pairs.values())
    assert len(neg_items) == sum(len(v) for key, v in table.items() if key in with_positive)            # lists of pairs without a positive are dropped
    assert ds.logged_negative_lists[2] is neg_items                                                       # built once


@pytest.mark.parametrize('name', ['f1_data', 'f9_data'])
def test_lists_hold_the_dict_of_the_fixture_files(name):
    """For every positive of F1 / F9 the pair's range of ``neg_items`` is the list ``neg_items_for_user_query_pair`` holds: file order, repeats kept, a pair in two
    logs has both logs' items, a pair without logged negatives an empty range."""
    ds = file_dataset(name)
    assert_lists_match_the_dict(ds)
    pair_of_edge, neg_ptr, _ = ds.logged_negative_lists
    lengths = np.diff(neg_ptr)
    assert lengths.max() > 0
    if name == 'f1_data':
        assert lengths.min() == 0                                                                         # F1 has pairs with no negatives
        rows = ds.search_logs
        assert sum(1 for log in rows if (log.user, log.query) == (0, 0)) >= 2                             # and pair (0, 0) in two logs


def test_lists_of_a_corpus_given_as_arrays():
    ds = array_dataset()
    assert ds.neg_items_for_user_query_pair == {(0, 0): [7, 9, 7, 11, 8], (1, 1): [5], (3, 3): [2, 4]}
    assert_lists_match_the_dict(ds)
    pair_of_edge, neg_ptr, neg_items = ds.logged_negative_lists
    assert pair_of_edge[0] == pair_of_edge[3] and len(neg_ptr) == 4 and len(neg_items) == 6
    from ihgnn_amd.Dataset import GraphDataset
    plain = GraphDataset.from_arrays(4, 4, 12, 6, np.arange(4), np.arange(4), ds.pos_triples, device=CPU)                  # without neg_triples: as before
    assert plain._neg_triples.shape == (0, 3) and plain.neg_items_for_user_query_pair == {} and len(plain.logged_negative_lists[2]) == 0
    assert plain.logged_negative_lists[1].tolist() == [0, 0, 0, 0]


def test_host_sampler_follows_the_reference_rule():
    """``__getitem__`` with nonrand = 2, rand = 3 (``Dataset.py:110-119``): a pair with >= 2 logged negatives gives two entries of its list (at distinct positions)
    first, then 3 distinct catalogue items; a pair with fewer gives 5 - len random items, then the whole list in order."""
    ds = array_dataset(rand=3, nonrand=2)
    random.seed(11)
    for _ in range(200):
        head, negs = ds[0]
        assert head == (0, 0, 1, 1) and len(negs) == 5
        remaining = [7, 9, 7, 11, 8]
        for item in negs[:2]:
            remaining.remove(item)                                           # two entries of the list, 7 twice only as often as the list has it
        assert len(set(negs[2:])) == 3 and all(0 <= x < 12 for x in negs[2:])
        head, negs = ds[1]
        assert head == (1, 1, 2, 1) and negs[4:] == [5] and len(set(negs[:4])) == 4 and all(0 <= x < 12 for x in negs[:4])
        head, negs = ds[2]
        assert head == (2, 0, 3, 1) and len(set(negs)) == 5 and all(0 <= x < 12 for x in negs)
    both = {tuple(ds[0][1][:2]) for _ in range(300)}
    assert (7, 7) in both and len(both) > 5                                  # the list's repeat can be drawn twice; the draw is random
    f1 = file_dataset('f1_data', rand=3, nonrand=2)
    table = f1.neg_items_for_user_query_pair
    for e, (u, q, i) in enumerate(f1.pos_triples.tolist()):
        logged = table.get((u, q), [])
        head, negs = f1[e]
        assert head == (u, q, i, 1) and len(negs) == 5
        if len(logged) >= 2:
            left = list(logged)
            for item in negs[:2]:
                left.remove(item)
            assert len(set(negs[2:])) == 3
        else:
            assert negs[5 - len(logged):] == logged and len(set(negs[:5 - len(logged)])) == 5 - len(logged)


# ---------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------
def test_mix64_and_multiply_high_agree_with_python_integers():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    b = np.concatenate([rng.integers(0, 2 ** 64, 500, dtype=np.uint64), rng.integers(1, 2 ** 31, 500, dtype=np.uint64)])
    a[:4] = [0, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32]
    b[:4] = [2 ** 64 - 1, 2 ** 64 - 1, 1, 2 ** 32]
    assert R.mulhi(a, b).tolist() == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]

    def mix(x):
        m = 2 ** 64 - 1
        x = (x + 0x9E3779B97F4A7C15) & m
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
        return x ^ (x >> 31)
    assert R.mix64(a).tolist() == [mix(int(x)) for x in a]
    assert mix(0) == 0xE220A8397B1DCDAF                                      # splitmix64's first output from state 0


corpus = R.corpus


def check_structure(pack, pos, edge_ids, tables, n_items, k_rand, k_logged, seed, counter):
    """Every row of ``pack`` against the rule of ``include/ihgnn_hip.h``, row by row: the layout, which entries are random and which from the list, the random
    entries against the plain sampler's prefix, the drawn positions distinct, in range and (``len == k_logged``) a permutation.  WHICH positions a row draws is taken
    from the emulation's own ``draw_distinct`` - that part restates the generator contract (stream key, attempts from 0) and is not an independent reference; the
    distribution of the positions is ``test_position_stream_is_uniform``'s to check."""
    k, n = k_rand + k_logged, len(edge_ids)
    assert pack.shape == (4, n * (1 + k))
    plain = R.sample_negatives(seed, counter, n, n_items, k)
    pair_of_edge, neg_ptr, neg_items = tables
    for row, e in enumerate(edge_ids.tolist()):
        u, q, i = pos[e].tolist()
        assert pack[:, row].tolist() == [u, q, i, 1]
        cols = slice(n + row * k, n + (row + 1) * k)
        assert pack[0, cols].tolist() == [u] * k and pack[1, cols].tolist() == [q] * k and pack[3, cols].tolist() == [0] * k
        negs = pack[2, cols].tolist()
        p = int(pair_of_edge[e])
        logged = neg_items[neg_ptr[p]:neg_ptr[p + 1]].tolist()
        if len(logged) >= k_logged:
            drawn, rest = negs[:k_logged], negs[k_logged:]
            assert rest == plain[row, :k_rand].tolist()                       # the random items: the plain sampler's first k_rand of this row
            positions = R.draw_distinct(R.row_keys(seed, counter, n)[row:row + 1] ^ R.POSITION_STREAM, max(len(logged), 1), k_logged)[0].tolist()
            assert len(set(positions)) == k_logged and all(0 <= x < len(logged) for x in positions)
            assert drawn == [logged[x] for x in positions]
            if len(logged) == k_logged:
                assert sorted(positions) == list(range(k_logged))            # a permutation of the list
        else:
            c = k - len(logged)
            assert negs[c:] == logged and negs[:c] == plain[row, :c].tolist()
        random_part = negs[k_logged:] if len(logged) >= k_logged else negs[:k - len(logged)]
        assert len(set(random_part)) == len(random_part) and all(0 <= x < n_items for x in random_part)


@pytest.mark.parametrize('k_rand,k_logged', [(3, 2), (0, 1), (0, 16), (1, 3), (10, 6), (5, 5), (4, 0)])
def test_emulated_rows_have_the_structure_of_the_rule(k_rand, k_logged):
    """len in {0, 1, k_logged - 1, k_logged, k_logged + 1, 1000}: logged entries at distinct drawn positions then random items, or random items then the whole list."""
    lengths = np.array([x for x in (0, 1, k_logged - 1, k_logged, k_logged + 1, 1000) if x >= 0] * 4, np.int64)
    pos, tables = corpus(lengths, k_logged)
    edge_ids = np.random.default_rng(5).permutation(len(lengths))
    pack = R.device_batch(21, 4, pos, edge_ids, tables, 50, k_rand, k_logged)
    check_structure(pack, pos, edge_ids, tables, 50, k_rand, k_logged, 21, 4)


def test_emulation_without_logged_negatives_is_the_plain_sampler():
    pos, tables = corpus(np.full(300, 4), 0)
    edge_ids = np.arange(300)[::-1].copy()
    for tab in (tables, None):
        pack = R.device_batch(8, 2, pos, edge_ids, tab, 50, 10, 0)
        assert np.array_equal(pack[2, 300:].reshape(300, 10), R.sample_negatives(8, 2, 300, 50, 10))
    full = R.sample_negatives(1, 0, 300, 10, 10)
    assert all(sorted(r) == list(range(10)) for r in full.tolist())          # k == I: permutations of the catalogue


def test_emulation_is_a_pure_function_of_seed_counter_and_row():
    lengths = np.full(2000, 40)
    pos, tables = corpus(lengths, 3, n_items=1000, repeats=False)
    edge_ids = np.arange(2000)

    def negatives(seed, counter, ids=edge_ids):
        return R.device_batch(seed, counter, pos, ids, tables, 1000, 4, 3)[2, len(ids):].reshape(len(ids), 7)
    a = negatives(5, 1)
    assert np.array_equal(a, negatives(5, 1))
    assert (a != negatives(5, 2)).mean() > 0.5 and (a != negatives(6, 1)).mean() > 0.5
    assert (a[:, :3] != negatives(5, 2)[:, :3]).mean() > 0.5                 # the position stream moves with the counter too
    # the draws of row r depend on r, not on how many rows the launch has
    assert np.array_equal(a[:100, 3:], negatives(5, 1, edge_ids[:100])[:, 3:])


def test_position_stream_is_uniform():
    """20,000 rows share one 12-entry list, k_logged = 3: chi-square of the first logged slot alone and of the inclusion counts over the 12 positions, both below
    11 + 6 sqrt(22) (the statistic and margin of ``test_device_negative_sampling_has_random_sample_semantics``).  The seeds are fixed: the verdict is deterministic."""
    n = 20000
    pos = np.stack([np.zeros(n), np.zeros(n), np.arange(n) % 50], 1).astype(np.int64)
    tables = (np.zeros(n, np.int32), np.array([0, 12], np.int64), np.arange(100, 112, dtype=np.int32))        # item 100 + position
    pack = R.device_batch(5, 1, pos, np.arange(n), tables, 50, 2, 3)
    drawn = pack[2, n:].reshape(n, 5)[:, :3] - 100
    assert drawn.min() >= 0 and drawn.max() < 12 and bool((np.sort(drawn, 1)[:, 1:] != np.sort(drawn, 1)[:, :-1]).all())
    bound = 11 + 6 * np.sqrt(2 * 11)
    first = np.bincount(drawn[:, 0], minlength=12)
    chi_first = ((first - n / 12) ** 2 / (n / 12)).sum()
    included = np.bincount(drawn.reshape(-1), minlength=12)
    chi_included = ((included - 3 * n / 12) ** 2 / (3 * n / 12)).sum()
    print(f'chi-square, 11 dof: first slot {chi_first:.2f}, inclusion {chi_included:.2f} (bound {bound:.2f})')
    assert chi_first < bound and chi_included < bound


# ---------------------------------------------------------------------------------------------
# command line, settings, ABI
# ---------------------------------------------------------------------------------------------
def test_logged_negatives_flag_sets_both_settings():
    from ihgnn_amd import Main
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    old = (Gs.random_negative_sample_size, Gs.non_random_negative_sample_size, Gs.negative_sample_size)
    try:
        assert parse_args([]).logged_negatives == 0
        args = parse_args(['--logged_negatives', '3', '--device_sampling'])
        assert args.logged_negatives == 3 and args.device_sampling
        Main.apply_sampling_settings(args)
        assert Gs.non_random_negative_sample_size == 3 and Gs.negative_sample_size == Gs.random_negative_sample_size + 3
        Main.apply_sampling_settings(parse_args([]))                         # 0: the setting stays
        assert Gs.non_random_negative_sample_size == 3 and Gs.negative_sample_size == Gs.random_negative_sample_size + 3
        with pytest.raises(ValueError):
            Main.apply_sampling_settings(parse_args(['--logged_negatives', '-1']))
    finally:
        Gs.random_negative_sample_size, Gs.non_random_negative_sample_size, Gs.negative_sample_size = old
    assert old == (10, 0, 10)


def test_device_batch_is_declared_and_the_abi_version_stays():
    from ihgnn_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+ihg_device_batch\s*\(', text)
    assert 'ihg_device_batch' in _lib.SIGNATURES and len(_lib.SIGNATURES['ihg_device_batch'][1]) == 13
    assert _lib.ABI_VERSION == 37 == _lib.load().ihg_abi_version()             # an entry point was added, none changed
    assert hasattr(_lib.load(), 'ihg_device_batch')


def test_device_batches_names_its_limit():
    """More than 16 negatives (on a catalogue of 50 items: only that limit can refuse 17), or more than the catalogue holds (13 of 12 items: within the 16), is refused
    before anything is launched, each with a message that names its own limit."""
    ds = array_dataset(rand=10, nonrand=7, items=50)
    with pytest.raises(ValueError, match='at most 16 negatives'):
        next(ds.device_batches(2))
    ds = array_dataset(rand=10, nonrand=3)                                   # 13 > 12 items
    with pytest.raises(ValueError, match='item_count = 12'):
        next(ds.device_batches(2))
