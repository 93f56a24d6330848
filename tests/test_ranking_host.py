"""No GPU: ``tests/ranking_reference.py`` held to its own conditions.  The restated launch geometry is pinned to ``ihg_score_topk_workspace_bytes`` (which launches
nothing); every exact design passes ``ensure_exact`` and its emulation EQUALS the float64 scores in the stable ranking; every float design's emulation meets the
per-score bound and the ranking verdict; every mutation of the emulation fails a named design; the deep passes stay within ``ceil(min(k, I) / 10)`` and
``one_list`` attains that."""
import numpy as np
import pytest
import torch

import ranking_reference as R

# (pairs, items, width): one wave's tile, a partial last tile, nine tiles over eight waves, empty runs, two k-steps and a column tail
SMALL = [(5, 7, 9), (3, 33, 17), (5, 257, 48), (33, 100, 16), (2, 300, 100)]


def _lib():
    from ihgnn_amd import _lib
    return _lib.load()


def test_geometry_restated_equals_the_library():
    lib = _lib()
    assert lib.ihg_score_topk_max_dim() == 1264 and R.eval_pair_tiles(624) == 2 and R.eval_pair_tiles(625) == 1 and lib.ihg_score_topk_max_k() == R.DEEP_MAX
    for dim in (1, 7, 16, 17, 64, 100, 624, 625, 1264):
        for n_pairs in (1, 5, 31, 32, 33, 64, 65, 129, 600, 4096, 40000):
            for n_items in (1, 10, 32, 33, 255, 256, 257, 1023, 1024, 2016, 2017, 4100, 65504, 65505, 300001):
                assert lib.ihg_score_topk_workspace_bytes(n_pairs, n_items, dim) == R.workspace_bytes(n_pairs, n_items, dim), (n_pairs, n_items, dim)
                assert lib.ihg_score_topk_deep_workspace_bytes(n_pairs, n_items, dim, 128) == R.deep_workspace_bytes(n_pairs, n_items, dim), (n_pairs, n_items, dim)
    # the shapes tests/test_ranking_kernels.py relies on
    assert (R.eval_slices(5, 2016, 64), R.eval_slices(5, 2017, 64), R.eval_slices(5, 4100, 64)) == (1, 2, 4)
    assert (R.eval_slices(8, 65504, 16), R.eval_slices(8, 65505, 16)) == (63, 64) and R.n_lists(8, 65505, 16) == 1024


def test_list_of_partitions_the_items_by_run_and_lane_half():
    for n_pairs, n_items, dim in SMALL + [(5, 2017, 64), (5, 4100, 64)]:
        lists = R.list_of(n_pairs, n_items, dim)
        ranges = R.tile_ranges(n_pairs, n_items, dim)
        assert ranges[0][0] == 0 and ranges[-1][1] == (n_items + 31) // 32 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        assert lists.max() < R.n_lists(n_pairs, n_items, dim)
        for item in (0, 3, 4, 7, 8, n_items - 1):
            if item < n_items:
                run = [r for r, (b, e) in enumerate(ranges) if b <= item // 32 < e][0]
                assert lists[item] == 2 * run + (item % 8 >= 4)


def _designs(cosine):
    return R.COSINE_EXACT_DESIGNS if cosine else R.EXACT_DESIGNS


@pytest.mark.parametrize('cosine', [False, True])
def test_exact_designs_are_exact_and_the_emulation_equals_the_ranking(cosine):
    for j, design in enumerate(_designs(cosine)):
        n_pairs, n_items, dim = SMALL[j % len(SMALL)]
        if design == 'identity':
            n_items = dim = (17, 100)[j % 2]
        case = R.exact_case(design, n_pairs, n_items, dim, cosine, R.LAMS_EXACT[j % 2])
        R.ensure_exact(case, cosine)
        for k, deep in ((10, False), (3, False), (21, True), (128, True)):
            scores, items, passes = R.emulate(case, k, cosine, deep)
            R.assert_exact(torch.from_numpy(scores), torch.from_numpy(items), case, k, cosine, f'{case.name} k={k} deep={deep}')
            if deep:
                assert np.all((1 <= passes) & (passes <= R.max_passes(k, n_items))), case.name
                # the emulation fed the float32 of the float64 scores (what the GPU module does at sizes where the column loop would be slow) is the same call
                again = R.emulate(case, k, cosine, deep, scores=case.scores64(cosine).float().numpy())
                assert np.array_equal(again[1], items) and np.array_equal(again[2], passes)


def test_a_case_beyond_the_cap_is_refused():
    case = R.exact_case('random', 3, 33, 17)
    case.features[case.item_row0:] *= 4096
    case._scores.clear()
    with pytest.raises(ValueError):
        R.ensure_exact(case)
    case = R.exact_case('random', 3, 33, 17)
    case.features[case.item_row0] += 2.0 ** -9                              # more than 11 significant bits in an item row
    with pytest.raises(ValueError):
        R.ensure_exact(case)


@pytest.mark.parametrize('cosine', [False, True])
def test_float_designs_meet_the_bound_and_the_ranking_verdict(cosine):
    worst = 0.0
    for j, design in enumerate(R.FLOAT_DESIGNS):
        for i, lam in enumerate(R.LAMS_FLOAT):
            n_pairs, n_items, dim = SMALL[(i + j) % len(SMALL)]
            case = R.float_case(design, n_pairs, n_items, dim, lam)
            for k, deep in ((10, False), (50, True)):
                scores, items, _ = R.emulate(case, k, cosine, deep)
                worst = max(worst, R.float_verdict(torch.from_numpy(scores), torch.from_numpy(items), case, k, cosine, f'{case.name} k={k}'))
    case = R.float_case('randn', 2, 40, 1264, 0.3)                          # the widest row: 79 k-steps
    scores, items, _ = R.emulate(case, 10, cosine)
    worst = max(worst, R.float_verdict(torch.from_numpy(scores), torch.from_numpy(items), case, 10, cosine, case.name))
    print(f'worst error / bound of the emulation, {"cosine" if cosine else "dot product"} head: {worst:.3f}')
    assert 0 < worst <= 1


def _fails(case, k, cosine, deep, mutation):
    scores, items, passes = R.emulate(case, k, cosine, deep, mutation)
    try:
        R.assert_exact(torch.from_numpy(scores), torch.from_numpy(items), case, k, cosine, mutation)
    except AssertionError:
        return True
    return False


def test_every_mutation_fails_a_named_design():
    failing = {                                                             # mutation -> (design, (pairs, items, width), k, deep)
        'drop_hi_lo': ('mixed_bits', (5, 70, 48), 10, False),
        'read_column_tail': ('identity', (5, 17, 17), 10, False),
        'padded_item_competes': ('random', (5, 7, 9), 10, False),
        'ties_by_higher_id': ('tied_across', (5, 257, 48), 10, False),
        'worst_last_entry_for_t': ('one_list_dec', (5, 257, 48), 50, True),
        'boundary_not_advanced': ('descending', (33, 100, 16), 21, True),
        'drop_tenth_entry': ('one_list_dec', (5, 257, 48), 10, False),
    }
    for mutation, (design, shape, k, deep) in failing.items():
        case = R.exact_case(design, *shape)
        R.ensure_exact(case)
        assert not _fails(case, k, False, deep, None), (mutation, design)
        assert _fails(case, k, False, deep, mutation), f'{mutation} passes {design}'
    # the tie that the deep boundary rests in after pass 1 (ranks 10 | 11 in ONE list): the order of the two ids decides what pass 2 begins with
    case = R.exact_case('tie_at_boundary', 5, 257, 48)
    assert not _fails(case, 21, False, True, None) and _fails(case, 21, False, True, 'ties_by_higher_id')
    # the lists' geometry shows in nothing but the passes.  Swapping the lane halves relabels the same two sets of a tile, so NO output can tell it (held here: the
    # three outputs are equal); the halves taken as the tile's two runs of sixteen split the winners of one_list over two lists, and the call needs fewer passes
    case = R.exact_case('one_list_dec', 5, 2016, 64)
    s32 = case.scores64(False).float().numpy()
    right = R.emulate(case, 128, deep=True, scores=s32)
    assert np.all(right[2] == 13)
    assert all(np.array_equal(a, b) for a, b in zip(right, R.emulate(case, 128, deep=True, scores=s32, mutation='swap_lane_halves')))
    assert np.all(R.emulate(case, 128, deep=True, scores=s32, mutation='halves_by_sixteen')[2] < 13)
    # a pair past n_pairs has no user and no query: reading one is an error of its own
    case = R.exact_case('random', 5, 7, 9)
    with pytest.raises(IndexError):
        R.emu_scores(case, mutation='score_pair_past_end')
    assert set(failing) | {'swap_lane_halves', 'halves_by_sixteen', 'score_pair_past_end'} == set(R.MUTATIONS)


@pytest.mark.parametrize('cosine', [False, True])
def test_deep_passes_one_list_attains_the_maximum(cosine):
    """``one_list`` puts the best items into ONE list - all 128 that a list of 2016 items in one slice holds: every pass ranks exactly ten, so every k needs its
    full ``ceil(min(k, I) / 10)`` passes; designs that spread the winners need fewer.  ``tie_at_boundary`` does the same with ranks 10 | 11, 20 | 21, ... bit-equal:
    every pass but the last leaves the boundary inside a tie."""
    for design in ('one_list_dec', 'one_list_inc', 'tie_at_boundary'):
        case = R.exact_case(design, 5, 2016, 64, cosine)
        R.ensure_exact(case, cosine)
        s32 = case.scores64(cosine).float().numpy()
        lists = R.list_of(5, 2016, 64)
        assert np.bincount(lists).max() == 128
        for c, top in enumerate(R.expected(case, 128, cosine)[1].numpy()):
            assert len(set(lists[top].tolist())) == 1, f'{case.name}: the best 128 of pair {c} are not in one list'
            if design == 'tie_at_boundary':
                ranked = np.sort(s32[c])[::-1]
                assert all(ranked[r - 1] == ranked[r] and ranked[r] > ranked[r + 1] for r in range(10, 128, 10)), f'{case.name}: ranks 10 | 11, 20 | 21, ... do not tie'
                assert np.any(np.diff(top[:128]) < 0) and np.any(np.diff(top[:128]) > 0), f'{case.name}: the winners lie in id order'
        for k in (11, 20, 21, 50, 128):
            scores, items, passes = R.emulate(case, k, cosine, True, scores=s32)
            R.assert_exact(torch.from_numpy(scores), torch.from_numpy(items), case, k, cosine, f'{case.name} k={k}')
            assert np.all(passes == R.max_passes(k, 2016)), (design, k, passes)
    spread = R.exact_case('one_per_list', 5, 2016, 64, cosine)
    assert np.all(R.emulate(spread, 128, cosine, True, scores=spread.scores64(cosine).float().numpy())[2] < 13)
    few = R.exact_case('ascending', 5, 7, 9, cosine)
    assert np.all(R.emulate(few, 128, cosine, True)[2] == 1) and R.max_passes(128, 7) == 1
