"""The host side of per-search exclusion lists, where there is no GPU: ``ops.exclusion_lists`` normalises what it is given, ``GraphDataset.user_item_lists`` holds
every user's training items, ``seen_lists_for_logs`` keeps a log's own positives rankable, ``--filter_seen`` parses and ``--model Srrl`` refuses it, every bad argument
of ``ihg_search_topk_excluding`` is refused before a launch, ``RawGnn._check_search_inputs`` checks the lists, and ``tests/exclude_reference.py`` agrees with
``search_reference`` where the two say the same thing."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import exclude_reference as E
import ranking_reference as R
import search_reference as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


def _flat(runs):
    offsets = np.cumsum([0] + [len(r) for r in runs]).astype(np.int64)
    flat = np.asarray([i for r in runs for i in r], np.int64)
    return torch.from_numpy(offsets), torch.from_numpy(flat)


def _runs(ptr, items):
    return [items[int(ptr[r]):int(ptr[r + 1])].tolist() for r in range(len(ptr) - 1)]


@pytest.mark.parametrize('n_items', [1, 7, 100])
def test_exclusion_lists_sort_and_deduplicate_every_run(n_items):
    from ihgnn_amd import ops
    rng = np.random.default_rng(n_items)
    for n_rows in (1, 2, 9):
        runs = [rng.integers(0, n_items, size=int(rng.integers(0, 3 * n_items + 1))).tolist() for _ in range(n_rows)]        # shuffled, with repeats
        runs[n_rows // 2] = []                                                                                            # an empty run in the middle (or the only one)
        if n_rows > 2:
            runs[0], runs[-1] = [], list(range(n_items))[::-1]                                                            # empty first, every item (descending) last
        ptr, items = ops.exclusion_lists(*_flat(runs), n_items)
        assert ptr.dtype == torch.int64 and items.dtype == torch.int32 and ptr.shape == (n_rows + 1,) and int(ptr[0]) == 0 and int(ptr[-1]) == items.numel()
        assert _runs(ptr, items) == [sorted(set(r)) for r in runs]
        again = ops.exclusion_lists(ptr, items, n_items)                                                                  # a normal form: unchanged by a second pass
        assert torch.equal(again[0], ptr) and torch.equal(again[1], items)
    ptr, items = ops.exclusion_lists(torch.tensor([0]), torch.zeros(0, dtype=torch.int64), n_items)                       # no run at all
    assert ptr.tolist() == [0] and items.numel() == 0


def test_exclusion_lists_check_host_tensors():
    from ihgnn_amd import ops
    good = (torch.tensor([0, 2, 3]), torch.tensor([4, 0, 6]))
    assert _runs(*ops.exclusion_lists(*good, 7)) == [[0, 4], [6]]
    for offsets, items in ((good[0], torch.tensor([4, 0, 7])), (good[0], torch.tensor([-1, 0, 6])),                       # ids outside [0, I)
                           (torch.tensor([1, 2, 3]), good[1]), (torch.tensor([0, 3, 2]), good[1]), (torch.tensor([0, 2, 4]), good[1]),   # offsets: start, order, end
                           (torch.zeros(0, dtype=torch.int64), good[1])):
        with pytest.raises(ValueError):
            ops.exclusion_lists(offsets, items, 7)
    with pytest.raises(ValueError, match='exclude_rows without exclude'):
        ops.search_topk(torch.zeros(4, 4), torch.zeros(1, dtype=torch.int64), 0, 0, torch.zeros(4), 0.5, 1, queries=torch.zeros(1, dtype=torch.int64),
                        exclude_rows=torch.zeros(1, dtype=torch.int64))


def _dataset():
    from ihgnn_amd.Dataset import GraphDataset
    # user 0: items 4, 1 (4 twice, under two queries); user 1: none; user 2: item 0; user 3: items 6, 5, 0
    triples = np.array([[0, 0, 4], [3, 1, 6], [0, 1, 1], [2, 2, 0], [3, 0, 5], [0, 2, 4], [3, 3, 0]], np.int64)
    return GraphDataset.from_arrays(4, 4, 7, 6, np.arange(4), np.arange(4), triples, device=CPU)


def test_user_item_lists_of_a_dataset_from_arrays():
    ds = _dataset()
    ptr, items = ds.user_item_lists
    assert ptr.dtype == np.int64 and items.dtype == np.int32
    assert _runs(ptr, items) == [[1, 4], [], [0], [0, 5, 6]]
    assert ds.user_item_lists[0] is ptr                                    # built once
    on = ds.user_item_lists_on(CPU)
    assert on[0].dtype == torch.int64 and on[1].dtype == torch.int32 and on[0].tolist() == ptr.tolist() and on[1].tolist() == items.tolist()
    assert ds.user_item_lists_on(CPU)[1] is on[1]                          # copied once


def test_seen_lists_keep_the_logs_own_positives_rankable():
    from ihgnn_amd.Helpers.TrainTestHelper import seen_lists_for_logs
    ptr, items = _dataset().user_item_lists
    logs = [(0, 1, [4], None, True),                                       # the test positive was also bought in training: it stays rankable, item 1 goes
            (3, 0, [2, 5], None, True),                                    # one of two positives seen
            (1, 2, [3], None, True),                                       # a user without training items
            (2, 3, [0], None, True),                                       # everything the user has seen is the positive
            (3, 1, [1], None, True)]                                       # nothing in common
    offsets, flat = seen_lists_for_logs(logs, [0, 1, 2, 3, 4], ptr, items)
    assert _runs(offsets, np.asarray(flat)) == [[1], [0, 6], [], [], [0, 5, 6]]
    offsets, flat = seen_lists_for_logs(logs, [4, 0], ptr, items)          # a chunk is any subset, in its own order
    assert _runs(offsets, np.asarray(flat)) == [[0, 5, 6], [1]]
    assert seen_lists_for_logs(logs, [], ptr, items) == ([0], [])


def test_the_flag_parses_and_srrl_refuses_it():
    from ihgnn_amd import Main
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    assert parse_args([]).filter_seen is False and parse_args(['--filter_seen']).filter_seen is True
    assert Gs.Evaluation.filter_seen is False                              # off unless asked for
    try:
        Main.apply_evaluation_settings(parse_args(['--filter_seen', '--cutoffs', '20']))
        assert Gs.Evaluation.filter_seen is True and Gs.Evaluation.extra_cutoffs == (20,)
        Main.apply_evaluation_settings(parse_args([]))                     # assigned both ways
        assert Gs.Evaluation.filter_seen is False and Gs.Evaluation.extra_cutoffs == ()
    finally:
        Gs.Evaluation.filter_seen, Gs.Evaluation.extra_cutoffs = False, ()
    Main.check_srrl_settings(parse_args(['--model', 'Srrl']), 1)
    with pytest.raises(NotImplementedError, match='filter_seen'):
        Main.check_srrl_settings(parse_args(['--model', 'Srrl', '--filter_seen']), 1)
    from ihgnn_amd import Search
    assert 'exclude_seen' in open(Search.__file__).read()


def test_entry_points_are_declared_in_header_binding_and_library():
    from ihgnn_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('ihg_search_topk_excluding_workspace_bytes', 'ihg_search_topk_excluding'):
        assert re.search(r'\b' + name + r'\s*\(', text) and name in _lib.SIGNATURES and hasattr(lib, name), name
    # ihg_search_topk's arguments with (excl_ptr, excl_items, excl_row, n_excl_rows) behind `item_mask`
    search = _lib.SIGNATURES['ihg_search_topk'][1]
    assert _lib.SIGNATURES['ihg_search_topk_excluding'] == (ctypes.c_int, search[:13] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64] + search[13:])
    assert _lib.SIGNATURES['ihg_search_topk_excluding_workspace_bytes'] == _lib.SIGNATURES['ihg_search_topk_workspace_bytes']
    assert _lib.ABI_VERSION == 37 == _lib.load().ihg_abi_version()        # entry points were added, none changed


def test_bad_arguments_are_refused_before_any_launch():
    """This runs where there is no GPU: an answer at all means that nothing was launched."""
    from ihgnn_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)                                             # a non-null, 16-byte aligned address that is never dereferenced

    def call(dim=64, n_items=1000, k=10, n_pairs=1, queries=p, query_rows=None, ld_q=0, q_dim=0, mask=None, ptr=p, items=p, row=None, n_rows=1, space=p, nbytes=1 << 40,
             cosine=0):
        return lib.ihg_search_topk_excluding(p, 2000, dim, 0, 0, n_items, p, p, queries, query_rows, ld_q, q_dim, mask, ptr, items, row, n_rows, 0.5, n_pairs, k, p, p, space,
                                             nbytes, cosine, None, None)

    def refused(text='ihg_search_topk_excluding', **kw):
        rc = call(**kw)
        return rc == _lib.ERR_INVALID and 'ihg_search_topk_excluding' in _lib.last_error() and text in _lib.last_error()

    # ihg_search_topk's own checks, with its codes
    assert refused(queries=p, query_rows=p, ld_q=32, q_dim=32) and refused(queries=None, query_rows=None)
    for q_dim in (0, -1, 65):
        assert refused(queries=None, query_rows=p, ld_q=64, q_dim=q_dim)
    assert refused(queries=None, query_rows=p, ld_q=31, q_dim=32)
    for cosine in (0, 1):
        for k in (0, -1, 129):
            assert refused('128', k=k, cosine=cosine)
    assert refused(dim=1265) and refused(n_items=0) and refused(dim=2001)
    # the lists
    assert refused('go together', ptr=p, items=None) and refused('go together', ptr=None, items=p)
    assert refused('excl_row without lists', ptr=None, items=None, row=p)
    assert refused('n_excl_rows', n_rows=0) and refused('n_excl_rows', n_rows=-1, row=p)
    assert refused('n_excl_rows', n_pairs=3, n_rows=2) and refused('n_excl_rows', n_pairs=3, n_rows=4)        # without excl_row: one run per pair
    # a bad size or query source is reported before a bad list (the order of ihg_search_topk, then the lists)
    assert refused('128', k=129, ptr=p, items=None) and refused('exactly one', queries=None, query_rows=None, ptr=None, items=p)
    # the workspace: that of ihg_search_topk + 4 bytes per pair, rounded up to 16
    for n_pairs in (1, 4, 5, 33):
        need = lib.ihg_search_topk_excluding_workspace_bytes(n_pairs, 1000, 64, 128)
        assert need == lib.ihg_search_topk_workspace_bytes(n_pairs, 1000, 64, 128) + (4 * n_pairs + 15) // 16 * 16
        for short in (dict(nbytes=16), dict(nbytes=need - 1), dict(space=None), dict(space=ctypes.c_void_p(4100))):
            assert refused('workspace', k=128, n_pairs=n_pairs, n_rows=n_pairs, **short)
        assert refused('workspace', k=128, n_pairs=n_pairs, ptr=None, items=None, nbytes=need - 1)           # the size is this entry's with or without lists
    for k in (0, 129):
        assert lib.ihg_search_topk_excluding_workspace_bytes(1, 1000, 64, k) == 0
    # the same bad arguments with nothing to do are still bad; a good empty call launches nothing
    assert refused(n_pairs=0, k=129) and refused('go together', n_pairs=0, items=None) and refused('n_excl_rows', n_pairs=0, n_rows=0)
    assert call(n_pairs=0) == _lib.OK and call(n_pairs=0, ptr=None, items=None) == _lib.OK and call(n_pairs=0, row=p, n_rows=7, mask=p) == _lib.OK


def _stub(user_count=5, query_count=4, item_count=7, vocab_size=9):
    ds = types.SimpleNamespace(user_count=user_count, query_count=query_count, item_count=item_count, vocab_size=vocab_size)
    return types.SimpleNamespace(dataset=ds, gnns=[types.SimpleNamespace(graph=types.SimpleNamespace(self_loops=False))])


def test_model_search_checks_the_lists_on_the_host():
    from ihgnn_amd.Models import RawGnn
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    check = lambda **kw: RawGnn._check_search_inputs(_stub(), t(0, -1, 4), t(3, 0, 1), None, None, None, **kw)
    assert check() == (None, None) and check(exclude_seen=True) == (None, None)
    assert check(exclude=(t(0, 2, 2, 3), t(6, 0, 6))) == (None, None) and check(exclude=(t(0, 0, 0, 0), t())) == (None, None)
    for bad in (dict(exclude=(t(0, 2, 2, 3), t(6, 0, 6)), exclude_seen=True),                   # both
                dict(exclude=(t(0, 2, 3), t(6, 0, 6))), dict(exclude=(t(0, 2, 2, 3, 3), t(6, 0, 6))),    # one run per search
                dict(exclude=(t(1, 2, 2, 3), t(6, 0, 6))), dict(exclude=(t(0, 2, 1, 3), t(6, 0, 6))), dict(exclude=(t(0, 2, 2, 4), t(6, 0, 6))),
                dict(exclude=(t(0, 2, 2, 3), t(6, 0, 7))), dict(exclude=(t(0, 2, 2, 3), t(-1, 0, 6))),   # ids outside [0, I)
                dict(exclude=t(0, 2, 2, 3))):                                                            # not a pair
        with pytest.raises(ValueError):
            check(**bad)


@pytest.mark.parametrize('cosine', [False, True])
def test_reference_excluding_a_run_is_masking_it_out(cosine):
    """On one pair the two references say the same thing: leaving out run c is the mask ``~run``, and with a mask besides it is ``mask & ~run``."""
    base = R.float_case('randn', 1, 70, 48, 0.3)
    run = [3, 69, 0, 31, 32, 3]
    for mask in (None, S.mask_pattern('every_other', 70)):
        case = E.ExcludeCase(base, [run], mask=mask)
        assert case.lists[0].tolist() == [0, 3, 31, 32, 69] and case.csr()[0].tolist() == [0, 5]
        allowed = np.ones(70, bool) if mask is None else mask.copy()
        allowed[run] = False
        assert np.array_equal(case.allowed()[0], allowed)
        same = S.SearchCase(base, mask=allowed)
        for k in (1, 10, 40, 128):
            assert case.targets(k).tolist() == [same.target(k)]            # (an excluded id outside the mask is not subtracted twice: 32 and 0 are both)
            got, want = E.expected(case, k, cosine), S.expected(same, k, cosine)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert E.float_verdict(got[0], got[1], case, k, cosine, 'self') == S.masked_float_verdict(want[0], want[1], same, k, cosine, 'self')
        one = case.single(0)
        assert np.array_equal(one.mask, allowed) and torch.equal(one.scores64(cosine), case.scores64(cosine))


def test_reference_states_rows_targets_and_the_verdicts():
    base = R.float_case('randn', 5, 40, 48, 0.3)
    lists = [[1, 2, 3], list(range(40)), []]
    case = E.ExcludeCase(base, lists, rows=[0, 1, -1, 0, 2], anon=[False, False, True, False, False])
    assert [case.run_of(c).tolist() for c in range(5)] == [[1, 2, 3], list(range(40)), [], [1, 2, 3], []]
    assert case.targets(38).tolist() == [37, 0, 38, 37, 38] and case.csr()[0].tolist() == [0, 3, 43, 43]
    scores, items = E.expected(case, 38, False)
    assert bool((items[1] == -1).all()) and bool((scores[1] == -E.FLT_MAX).all()) and int(items[0, 36]) >= 0 and int(items[0, 37]) == -1
    assert not bool(torch.isin(items[[0, 3]], torch.tensor([1, 2, 3], dtype=torch.int32)).any())
    free = S.SearchCase(base, anon=case.anon)
    full = R.expected(free, 40, False)
    fs, fi = E.filtered_prefix(full[0], full[1], case, 38)
    assert torch.equal(fi, items) and torch.equal(fs, scores)
    assert torch.equal(items[2], full[1][2, :38]) and torch.equal(items[4], full[1][4, :38])     # an empty run and row -1: the ranking without lists
    assert 0 < E.float_verdict(scores, items, case, 38, False, 'self') < 1
    wrong = items.clone()
    wrong[3, 0] = 2                                                        # an excluded item of pair 3 - allowed for pair 2, whose verdict would pass it
    with pytest.raises(AssertionError, match='pair 3'):
        E.float_verdict(scores, wrong, case, 38, False, 'self')
    short = items.clone()
    short[0, 36] = -1                                                      # the tail begins one rank early
    with pytest.raises(AssertionError):
        E.float_verdict(scores, short, case, 38, False, 'self')
    assert E.ExcludeCase(base, [[]] * 5).targets(10).tolist() == [10] * 5 and E.ExcludeCase(base, [[]] * 5).csr()[1].shape == (1,)
