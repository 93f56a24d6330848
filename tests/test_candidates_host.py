"""Per-search candidate lists on the host (no GPU): ``ops.candidate_lists`` against a per-row ``np.unique``; the float32 emulation of the list kernels' summation scheme
(``candidates_reference.emulate``) passes every verdict on every case of ``test_candidates_kernels.py``, and each named way of being wrong fails a named case; the
sampled-evaluation sets (exactly N distinct ids besides the log's own, the same whatever the chunking or the rank split); ``parse_shortlist_line``;
``--eval_candidates`` parses, is assigned both ways and refused where it cannot apply; the argument checks of ``ihg_search_candidates`` come before any launch."""
import ctypes
import io
import types

import numpy as np
import pytest
import torch

import candidates_reference as CR
import ranking_reference as R
import search_reference as S


def _t(*v):
    return torch.tensor(v, dtype=torch.int64)


def _per_row_unique(offsets, items):
    runs = [np.unique(np.asarray(items[offsets[r]:offsets[r + 1]], np.int64)) for r in range(len(offsets) - 1)]
    ptr = np.zeros(len(runs) + 1, np.int64)
    np.cumsum([len(r) for r in runs], out=ptr[1:])
    return ptr, (np.concatenate(runs) if runs else np.zeros(0, np.int64))


def test_candidate_lists_against_a_per_row_unique():
    from ihgnn_amd import ops
    rng = np.random.default_rng(0)
    for n_rows, n_items in ((1, 1), (5, 7), (40, 300), (3, 2 ** 31 - 100)):
        lengths = rng.integers(0, 9, n_rows)
        lengths[rng.integers(0, n_rows)] = 0                               # an empty row
        offsets = np.concatenate([[0], np.cumsum(lengths)])
        items = rng.integers(0, n_items, offsets[-1])
        if len(items) > 2:
            items[1] = items[0]                                            # a repeat
        ptr, ids = ops.candidate_lists(torch.from_numpy(offsets), torch.from_numpy(items), n_items)
        want_ptr, want_ids = _per_row_unique(offsets, items)
        assert ptr.dtype == torch.int64 and ids.dtype == torch.int32
        assert ptr.tolist() == want_ptr.tolist() and ids.tolist() == want_ids.tolist()
    ptr, ids = ops.candidate_lists(_t(0, 0, 0, 0), _t(), 9)                # all rows empty
    assert ptr.tolist() == [0, 0, 0, 0] and ids.numel() == 0 and ids.dtype == torch.int32
    ptr, ids = ops.candidate_lists(_t(0, 4, 4, 6), _t(8, 0, 8, 3, 2, 2), 9)
    assert ptr.tolist() == [0, 3, 3, 4] and ids.tolist() == [0, 3, 8, 2]
    for bad in ((_t(0, 2), _t(0, 9)), (_t(0, 2), _t(-1, 3)), (_t(1, 2), _t(0, 1)), (_t(0, 3), _t(0, 1)), (_t(0, 2, 1, 2), _t(0, 1)), (_t(), _t())):
        with pytest.raises(ValueError, match='candidate'):
            ops.candidate_lists(bad[0], bad[1], 9)


def test_exclusion_lists_keeps_its_results_and_messages():
    from ihgnn_amd import ops
    ptr, ids = ops.exclusion_lists(_t(0, 4, 4, 6), _t(8, 0, 8, 3, 2, 2), 9)
    assert ptr.tolist() == [0, 3, 3, 4] and ids.tolist() == [0, 3, 8, 2]
    with pytest.raises(ValueError, match=r'excluded item id outside \[0, 9\)'):
        ops.exclusion_lists(_t(0, 1), _t(9), 9)
    with pytest.raises(ValueError, match='exclusion_lists: offsets run from 0 to the 2 ids without decreasing'):
        ops.exclusion_lists(_t(0, 3), _t(1, 2), 9)
    with pytest.raises(ValueError, match='exclusion_lists: offsets holds at least the leading 0'):
        ops.exclusion_lists(_t(), _t(), 9)


def _verdict(case, k, cosine, out):
    """Every verdict of ``test_candidates_kernels.py`` that needs no GPU, on one call's output."""
    scores, items, passes, flat = out
    what = f'{case.name} k={k} cosine={cosine}'
    for c, n in enumerate(case.targets(k).tolist()):
        limit = (max(n, 1) + CR.TOP - 1) // CR.TOP
        assert 0 <= int(passes[c]) <= limit and (n > 0 or int(passes[c]) == 0), f'{what}: search {c}: passes'
        assert bool((items[c, n:] == -1).all()) and bool((scores[c, n:] == -R.FLT_MAX).all()) and bool((items[c, :n] >= 0).all()), f'{what}: search {c}: the tail'
    if case.exact:
        R.ensure_exact(case, cosine)
        CR.assert_exact(scores, items, case, k, cosine, what)
    else:
        CR.float_verdict(scores, items, case, k, cosine, what)
    CR.all_scores_verdict(flat, case, cosine, what)
    if case.cand_row_of is None:
        want = CR.ranking_of_floats(flat, case, k)
        assert torch.equal(scores.view(torch.int32), want[0].view(torch.int32)) and torch.equal(items, want[1]), f'{what}: not the ranking of the returned floats'


@pytest.mark.parametrize('cosine', [False, True])
def test_the_emulation_passes_every_verdict_on_every_kernel_case(cosine):
    """The kernels' own scheme, in float32 on the CPU, is inside the derived bound on every float case and EXACT on every exact design - the three cosine designs
    included: none of them moves to the float verdict."""
    cases = CR.all_cases(cosine)
    assert {c.dim for c, _, _ in cases} >= set(CR.DIMS) and {k for _, k, _ in cases} == set(CR.KS)
    assert sum(c.exact for c, _, _ in cases) == len(CR.EXACT_COSINE if cosine else CR.EXACT_DOT)
    for case, k, _ in cases:
        _verdict(case, k, cosine, CR.emulate(case, k, cosine))


def test_the_ladder_of_run_lengths_and_the_bound_constants():
    assert CR.run_lengths(11, 2100) == [0, 1, 2, 10, 11, 12, 63, 64, 65, 255, 256, 257, 513, 2100]
    assert [CR.group_width(d) for d in (1, 3, 4, 5, 30, 64, 65, 100, 384, 1280, 2048)] == [1, 1, 1, 2, 8, 16, 16, 16, 16, 16, 16]
    assert [CR.gamma(d) for d in (1, 4, 64, 128, 2048)] == [3 + 4 + 0 + 1, 8, 3 + 4 + 4 + 1, 3 + 8 + 4 + 1, 3 + 128 + 4 + 1]
    runs = CR.runs_by_length(CR.N_PAIRS, 300, 11)
    assert [len(r) for r in runs[:14]] == [0, 1, 2, 10, 11, 12, 63, 64, 65, 255, 256, 257, 300, 300]
    assert any(len(r) and r[0] == 0 for r in runs) and any(len(r) and r[-1] == 299 for r in runs)
    case, k, _ = CR.shared_runs_case(False)
    owner = case.owner_of_run()
    assert (case.cand_row_of == -1).any() and (case.cand_row_of >= len(case.cand)).any() and (owner == -1).any()
    users = case.base.users.numpy()
    shared = [np.flatnonzero(case.cand_row_of == r) for r in range(len(case.cand))]
    assert any(len(s) > 1 and len(set(users[s].tolist())) > 1 for s in shared)     # searches of different users on one run


# (mutation, the case it must fail, how the failure shows)
def _named(name, cosine=False):
    cases = {f'float{j}': c for j, c in enumerate(CR.float_cases(cosine))}
    cases.update({f'exact{j}': c for j, c in enumerate(CR.exact_cases(cosine))})
    cases.update(shared=CR.shared_runs_case(cosine), long=CR.one_long_run_case(cosine))
    return cases[name]


MUTANTS = (('stale_mixed_row', 'float3'),                # 70 searches of 13 users x 11 queries: the previous search's row is another row
           ('drop_last_partial_chunk', 'long'),          # 2,100 = 8 chunks + 52 ids
           ('ties_by_higher_id', 'exact1'),              # all_equal: every score ties
           ('boundary_not_advanced', 'float3'),          # k = 128: thirteen trips
           ('excluded_still_ranked', 'float0'),          # a run's first, last and every other id excluded
           ('mask_bit_of_next_item', 'float1'),          # the mask of the even ids
           ('cand_row_ignored', 'shared'),
           ('tail_at_min_k_len', 'float4'))              # mask and exclusion both remove entries of the runs


@pytest.mark.parametrize('mutation,name', MUTANTS)
def test_each_named_mutation_of_the_emulation_fails_its_case(mutation, name):
    case, k, _ = _named(name)
    _verdict(case, k, False, CR.emulate(case, k, False))
    with pytest.raises(AssertionError):
        _verdict(case, k, False, CR.emulate(case, k, False, mutation))


def test_every_mutation_is_tried():
    assert {m for m, _ in MUTANTS} == set(CR.MUTATIONS)


# ---------------------------------------------------------------------------------------------
# sampled evaluation
# ---------------------------------------------------------------------------------------------
def _logs(n_logs, item_count, seed=0):
    rng = np.random.default_rng(seed)
    logs = []
    for i in range(n_logs):
        items = rng.choice(item_count, size=int(rng.integers(1, 5)), replace=False).tolist()
        logs.append((int(rng.integers(0, 5)), int(rng.integers(0, 4)), items, [1] * len(items), True))
    return logs


def test_sampled_sets_hold_exactly_n_other_items():
    from ihgnn_amd.Helpers.TrainTestHelper import sampled_candidate_set
    item_count = 50
    logs = _logs(40, item_count)
    for n in (1, 9, 30):
        for i, log in enumerate(logs):
            got = sampled_candidate_set(i, log[2], item_count, n, seed=3)
            own = set(log[2])
            assert got.dtype == np.int32 and np.all(np.diff(got) > 0) and got.min() >= 0 and got.max() < item_count
            assert own <= set(got.tolist()) and len(got) == len(own) + n     # exactly n distinct ids, none of them the log's own
            assert np.array_equal(got, sampled_candidate_set(i, log[2], item_count, n, seed=3))
        assert any(not np.array_equal(sampled_candidate_set(i, logs[i][2], item_count, n, seed=3), sampled_candidate_set(i, logs[i][2], item_count, n, seed=4)) for i in range(40))
    # the rule itself, restated
    rng = np.random.default_rng([3, 7])
    draw = rng.choice(item_count, size=9 + len(set(logs[7][2])), replace=False, shuffle=False)
    rest = [int(x) for x in draw if int(x) not in set(logs[7][2])][:9]
    assert sorted(set(logs[7][2]) | set(rest)) == sampled_candidate_set(7, logs[7][2], item_count, 9, seed=3).tolist()
    # N + |items| >= I: the whole catalogue
    assert sampled_candidate_set(0, [1, 2, 3], 10, 7, 0).tolist() == list(range(10)) and sampled_candidate_set(0, [1, 2, 3], 10, 9, 0).tolist() == list(range(10))
    assert len(sampled_candidate_set(0, [1, 2, 3], 10, 6, 0)) == 9


def test_sampled_sets_do_not_depend_on_chunking_or_rank_split():
    from ihgnn_amd.Helpers.TrainTestHelper import SampledCandidates
    item_count = 60
    logs = _logs(37, item_count, seed=1)
    whole = SampledCandidates(logs, range(37), item_count, 12, seed=5)
    assert whole.ptr[0] == 0 and whole.ptr[-1] == len(whole.items) and whole.items.dtype == np.int32

    def sets(built, part):
        offsets, flat = built.lists_for(part)
        assert offsets.dtype == torch.int64 and flat.dtype == torch.int32
        return [flat[offsets[j]:offsets[j + 1]].tolist() for j in range(len(part))]

    want = sets(whole, list(range(37)))
    for world in (2, 3):                                                   # each rank builds only its share
        bounds = [37 * r // world for r in range(world + 1)]
        for r in range(world):
            share = list(range(bounds[r], bounds[r + 1]))
            mine = SampledCandidates(logs, share, item_count, 12, seed=5)
            assert sets(mine, share) == want[bounds[r]:bounds[r + 1]]
    for chunk in (1, 5, 36):
        got = [s for lo in range(0, 37, chunk) for s in sets(whole, list(range(lo, min(lo + chunk, 37))))]
        assert got == want
    assert sets(whole, [30, 2, 2]) == [want[30], want[2], want[2]]         # (any order: not only contiguous shares)
    loader = types.SimpleNamespace(logs=logs)
    first = SampledCandidates.for_loader(loader, list(range(37)), item_count, 12, 5)
    assert SampledCandidates.for_loader(loader, list(range(37)), item_count, 12, 5) is first          # built once per run
    assert SampledCandidates.for_loader(loader, list(range(37)), item_count, 13, 5) is not first


def test_eval_candidates_flag_parses_and_is_refused_where_it_cannot_apply():
    from ihgnn_amd import Main
    from ihgnn_amd.Helpers.ArgsParser import checked_candidate_count, parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    assert parse_args([]).eval_candidates == 0 and parse_args(['--eval_candidates', '99']).eval_candidates == 99
    assert Gs.Evaluation.sampled_candidates == 0 and Gs.Evaluation.candidate_seed == 0      # off unless asked for
    try:
        Main.apply_evaluation_settings(parse_args(['--eval_candidates', '99', '--filter_seen']))
        assert Gs.Evaluation.sampled_candidates == 99 and Gs.Evaluation.filter_seen is True
        Main.apply_evaluation_settings(parse_args([]))                     # assigned both ways
        assert Gs.Evaluation.sampled_candidates == 0 and Gs.Evaluation.filter_seen is False
        with pytest.raises(ValueError, match='eval_candidates'):
            Main.apply_evaluation_settings(types.SimpleNamespace(eval_candidates=-1))
    finally:
        Gs.Evaluation.sampled_candidates, Gs.Evaluation.filter_seen, Gs.Evaluation.extra_cutoffs = 0, False, ()
    for bad in ('-1', 'many', '1.5'):
        with pytest.raises(SystemExit):
            parse_args(['--eval_candidates', bad])
    assert checked_candidate_count(99, 100) == 99 and checked_candidate_count(0, 1) == 0
    for n, count in ((100, 100), (101, 100), (-1, 100)):
        with pytest.raises(ValueError, match='eval_candidates'):
            checked_candidate_count(n, count)
    Main.check_srrl_settings(parse_args(['--model', 'Srrl']), 1)
    with pytest.raises(NotImplementedError, match='eval_candidates'):
        Main.check_srrl_settings(parse_args(['--model', 'Srrl', '--eval_candidates', '99']), 1)


def test_parse_shortlist_line():
    from ihgnn_amd.Search import parse_search_line, parse_shortlist_line
    assert parse_shortlist_line('3\t4 5 6\t10 2 2 7\n') == (3, [4, 5, 6], [10, 2, 2, 7])
    assert parse_shortlist_line('-1\t\t5\n') == (-1, [], [5])
    assert parse_shortlist_line('2\t1 2\t\n') == (2, [1, 2], []) and parse_shortlist_line('2\t1 2') == (2, [1, 2], []) and parse_shortlist_line('2') == (2, [], [])
    with pytest.raises(ValueError):
        parse_shortlist_line('2\t1\t3\t4')
    with pytest.raises(ValueError):
        parse_shortlist_line('2\t1\tx')
    assert parse_search_line('3\t4 5 6\n') == (3, [4, 5, 6])                # (the two-field parser stays)


def _stub(user_count=5, query_count=4, item_count=7, vocab_size=9):
    ds = types.SimpleNamespace(user_count=user_count, query_count=query_count, item_count=item_count, vocab_size=vocab_size)
    return types.SimpleNamespace(dataset=ds, gnns=[types.SimpleNamespace(graph=types.SimpleNamespace(self_loops=False))])


def test_model_search_checks_the_shortlists_on_the_host():
    from ihgnn_amd.Models import RawGnn
    check = lambda **kw: RawGnn._check_search_inputs(_stub(), _t(0, -1, 4), _t(3, 0, 1), None, None, None, **kw)
    assert check(candidate_lists=(_t(0, 2, 2, 3), _t(6, 0, 6))) == (None, None) and check(candidate_lists=(_t(0, 0, 0, 0), _t())) == (None, None)
    assert check(candidate_lists=(np.array([0, 2, 2, 3]), np.array([6, 0, 6])), exclude_seen=True) == (None, None)
    for bad in (dict(candidate_lists=(_t(0, 2, 3), _t(6, 0, 6))), dict(candidate_lists=(_t(0, 2, 2, 3, 3), _t(6, 0, 6))),      # one run per search
                dict(candidate_lists=(_t(1, 2, 2, 3), _t(6, 0, 6))), dict(candidate_lists=(_t(0, 2, 1, 3), _t(6, 0, 6))), dict(candidate_lists=(_t(0, 2, 2, 4), _t(6, 0, 6))),
                dict(candidate_lists=(_t(0, 2, 2, 3), _t(6, 0, 7))), dict(candidate_lists=(_t(0, 2, 2, 3), _t(-1, 0, 6))),      # ids outside [0, I)
                dict(candidate_lists=_t(0, 2, 2, 3))):                                                                          # not a pair
        with pytest.raises(ValueError, match='candidate'):
            check(**bad)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from ihgnn_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    assert lib.ihg_search_candidates_max_dim() == CR.MAX_DIM >= 2048
    assert lib.ihg_search_candidates_workspace_bytes(70, 1000, 64, 10) == CR.workspace_bytes(70, 1000) == 4000 + 576 + 1120
    assert lib.ihg_search_candidates_workspace_bytes(70, 0, 64, 10) == CR.workspace_bytes(70, 0)
    for bad in ((0, 10, 64, 10), (70, -1, 64, 10), (70, 10, 0, 10), (70, 10, CR.MAX_DIM + 1, 10), (70, 10, 64, 0), (70, 10, 64, 129)):
        assert lib.ihg_search_candidates_workspace_bytes(*bad) == 0

    def call(dim=64, ld=64, k=10, n_pairs=3, queries=p, query_rows=None, q_dim=0, ld_q=0, excl=(None, None, None, 0), cand_ptr=p, cand_items=p, cand_row=None, n_runs=3,
             total=5, space=p, nbytes=1 << 20, features=p):
        return lib.ihg_search_candidates(features, ld, dim, 5, 9, 100, p, p, queries, query_rows, ld_q, q_dim, None, *excl, cand_ptr, cand_items, cand_row, n_runs, total,
                                         0.5, n_pairs, k, p, p, None, space, nbytes, 0, None, None)

    def refused(match=None, **kw):
        rc = call(**kw)
        return rc == _lib.ERR_INVALID and (match is None or match in _lib.last_error())

    assert refused('bad size', k=0) and refused('bad size', k=129) and refused('bad size', ld=63) and refused('bad size', dim=0)
    assert refused('exactly one', queries=None) and refused('exactly one', query_rows=p, q_dim=4, ld_q=4)
    assert refused('q_dim', queries=None, query_rows=p, q_dim=65, ld_q=65) and refused('q_dim', queries=None, query_rows=p, q_dim=4, ld_q=3)
    assert refused('go together', excl=(p, None, None, 3)) and refused('excl_row without', excl=(None, None, p, 3)) and refused('n_excl_rows', excl=(p, p, None, 2))
    assert refused('n_cand_rows', n_runs=2) and refused('n_cand_rows', n_runs=0, cand_row=p) and refused('total', total=-1)
    assert refused('null pointer', cand_ptr=None) and refused('null pointer', cand_items=None) and refused('null pointer', features=None)
    assert refused('widest', dim=CR.MAX_DIM + 1, ld=CR.MAX_DIM + 1)
    need = CR.workspace_bytes(3, 5)
    assert refused('workspace', nbytes=need - 1) and refused('workspace', space=None) and refused('workspace', space=ctypes.c_void_p(4100))
    assert call(n_pairs=0) == _lib.OK and call(n_pairs=0, n_runs=0, cand_ptr=None, cand_items=None) == _lib.OK and refused(n_pairs=0, k=129)


def test_ops_search_candidates_refuses_on_the_host():
    from ihgnn_amd import _lib, ops
    f = torch.zeros(20, 8)
    with pytest.raises(_lib.IhgnnHipError, match='float32 GPU feature matrix'):
        ops.search_candidates(f, _t(0), 3, 10, torch.zeros(10), 0.5, 5, lists=(_t(0, 1), _t(2)), queries=_t(0))
    with pytest.raises(ValueError, match='exclude_rows without exclude'):
        ops.search_candidates(f, _t(0), 3, 10, torch.zeros(10), 0.5, 5, lists=(_t(0, 1), _t(2)), queries=_t(0), exclude_rows=_t(0))
    with pytest.raises(ValueError, match=r'lists is \(offsets, items\)'):
        ops.search_candidates(f, _t(0), 3, 10, torch.zeros(10), 0.5, 5, lists=_t(0, 1), queries=_t(0))
