"""CPU side of the batch-row tests (``tests/test_batch_rows_kernels.py`` holds the GPU side): the cases of ``tests/batch_rows_reference.py`` keep the exact condition,
its vectorised references equal plain loops, every ladder holds a case on each side of the boundary it claims, a numpy emulation of each kernel's scheme passes
both verdicts on the cases the GPU file runs, and each of the named wrong variants (``batch_rows_reference.MUTATIONS``) fails a verdict on a named case."""
import numpy as np
import pytest
import torch

import batch_rows_reference as R

SCATTER_GROUPS = ('members', 'n', 'widths', 'forms', 'float')
COMBINE_GROUPS = ('members', 'n', 'widths', 'blocks', 'float')
ROWS_ADD_GROUPS = ('widths', 'n', 'tail', 'float')


def _fails(check):
    """True if the check refuses the result - a verdict (AssertionError) or a write outside the payload (IndexError: on the GPU a guard would change)."""
    try:
        check()
    except (AssertionError, IndexError):
        return True
    return False


def _scatter_failures(mutation, group, order=True):
    return {c.name for c, d in R.scatter_cases(group) if _fails(lambda: R.check_scatter(c, d, *R.emu_scatter(c, d, mutation), order=order))}


def _combine_failures(mutation, group, order=True):
    return {c.name for c, b in R.combine_cases(group) if _fails(lambda: R.check_combine(c, b, *R.emu_combine(c, b, mutation), order=order))}


# ---------------------------------------------------------------------------------------------
# the cases themselves
# ---------------------------------------------------------------------------------------------
def test_generators_keep_the_exact_condition():
    """Every exact case's references pass ``ensure_exact`` where they are built (it raises otherwise); a case past the cap IS refused; the float cases are not integers."""
    n_exact = 0
    for group in SCATTER_GROUPS:
        for c, d in R.scatter_cases(group):
            ref = R.scatter_reference(c, d)
            if c.exact:
                n_exact += 1
                assert float(ref.dense.mag.max()) < R.CAP and bool((c.values == np.round(c.values)).all()) and np.abs(c.values).max() <= 8
            assert np.isnan(c.rowgrad[:, c.width:]).all() and c.rowgrad.shape[1] > c.width
    for c, b in R.combine_cases('blocks'):
        assert float(R.group_sums(c, b).mag.max()) < R.CAP
    assert n_exact >= 55
    big = R.RowCase('past the cap', np.zeros(3, np.int64), 2, values=np.full((3, 2), 2.0 ** 23, np.float32))
    with pytest.raises(ValueError):
        R.group_sums(big)
    for case in R.compose_cases():
        fwd, bwd = R.compose_fwd_reference(case), R.compose_bwd_reference(case)          # (ensure_exact inside)
        if case.exact:
            assert max(float(r.mag.max()) for r in list(fwd.values()) + list(bwd.values())) < R.CAP and np.abs(case.a).max() <= 2
    assert float(R.compose_bwd_reference(R.ComposeCase(256, True))['dw'].mag.max()) <= 3 * 256 * 4


def test_vectorised_references_equal_plain_loops():
    for group in ('members', 'forms', 'widths'):
        for c, d in R.scatter_cases(group):
            ref = R.scatter_reference(c, d)
            want, tail = R.scatter_reference_loops(c, d)
            assert np.array_equal(ref.dense.want.numpy(), want), c.what
            assert d.tail is None or np.array_equal(ref.tail.want.numpy(), tail), c.what
    for c, b in R.combine_cases('blocks')[:8] + R.combine_cases('members'):
        sums = R.group_sums(c, b)
        first, want = R.group_sums_loops(c, b)
        assert np.array_equal(sums.first, first) and np.array_equal(sums.want, want), c.what
        lead = sums.leader == 1                                              # the batch-order sum, as a plain loop per leader
        for k in np.nonzero(lead)[0][:50]:
            acc = np.zeros(c.width, np.float32)
            for j in np.nonzero(first == k)[0]:
                acc = acc + c.values[j]
            assert np.array_equal(acc.view(np.int32), sums.seq[k].view(np.int32))
    for case in R.compose_cases():
        if case.dim <= 12:
            fwd, bwd = R.compose_fwd_reference(case), R.compose_bwd_reference(case)
            w_eff, b_eff, da, dw, db = R.compose_reference_loops(case)
            for got, want in ((fwd['w_eff'], w_eff), (fwd['b_eff'], b_eff), (bwd['da'], da), (bwd['dw'], dw), (bwd['db'], db)):
                assert np.allclose(got.want.numpy(), want, rtol=1e-13, atol=1e-13) and (not case.exact or np.array_equal(got.want.numpy(), want))


def test_every_ladder_holds_both_sides_of_its_boundary():
    counts = {name: int((rows == R.HOT).sum()) for name, rows in R.member_count_lists()}
    in_window = sorted(v for k, v in counts.items() if 'one window' in k)
    for edge in (R.MEMBERS, 2 * R.MEMBERS, R.WAVE):                         # a trip, two trips, the window
        assert edge in in_window and edge - 1 in in_window and (edge + 1 in in_window or edge + 1 in counts.values())
    for name, rows in R.member_count_lists():
        pos = np.nonzero(rows == R.HOT)[0]
        assert ('one window' in name) == (pos[0] // R.WAVE == pos[-1] // R.WAVE)
    assert counts['hundreds of members'] >= 300
    rows = R.position_lists()[0][1]
    firsts = {int(np.nonzero(rows == i)[0][0]) % R.WAVE for i in (R.HOT, 8, 9)}
    assert firsts == {0, 1, R.WAVE - 1} and rows[-1] == R.HOT and len(rows) % R.WAVE != 0
    assert list(np.nonzero(rows == 8)[0][1:]) == [2 * R.WAVE - 1, 2 * R.WAVE]
    assert list(np.nonzero(rows == 9)[0]) == [R.WAVE - 1, 130] and 130 >= len(rows) // R.WAVE * R.WAVE       # its only later member: in the last, partial window
    for edge in (R.WAVE, R.GRID_WAVES, R.SCATTER_MAX):
        assert edge in R.N_LADDER and edge + 1 in R.N_LADDER
    assert max(R.N_LADDER) == R.SCATTER_MAX_WIDE and R.GRID_WAVES in R.ROWS_N_LADDER and R.GRID_WAVES + 1 in R.ROWS_N_LADDER and max(R.ROWS_N_LADDER) > 2 * R.GRID_WAVES
    for edge in (R.WAVE, R.CHUNK_COLS):
        assert {edge - 1, edge, edge + 1} <= set(R.WIDTH_LADDER)
    assert max(R.WIDTH_LADDER) > 2 * R.CHUNK_COLS
    blocks = [(len(rows), b) for _, rows, b in R.combine_block_cases()]
    assert {b for _, b in blocks} == {0, 1, 63, 64, 65, 1100, R.COMBINE_N, R.COMBINE_N + 1, R.SCATTER_MAX, R.SCATTER_MAX + 1}
    assert R.COMBINE_N % 1100 not in (0,) and 1100 % R.WAVE != 0 and R.COMBINE_N_WIDE > R.SCATTER_MAX + 1
    _, rows, _ = R.combine_block_cases()[5]                                  # the same id in two blocks: leaders of their own
    merged, split = R.first_occurrence(rows, 0), R.first_occurrence(rows, 1100)
    assert int((split == np.arange(len(rows))).sum()) > int((merged == np.arange(len(rows))).sum())
    tails = R.dest_form_cases()[0][1]                                        # tr = -1, 0, tail_rows - 1, tail_rows
    assert {4, 5, 13, 14} <= set(tails.tolist())
    for b in R.NODE_ROWS_B[2:]:
        assert any(3 * b <= edge < 3 * (b + 1) or 3 * (b - 1) <= edge < 3 * b for edge in (256, R.GRID_THREADS))
    assert 3 * 85 <= 256 < 3 * 86 and 3 * 174762 <= R.GRID_THREADS < 3 * 174763
    assert {255, 256, 257} <= set(R.ZERO_FLOATS_N) and max(R.ZERO_FLOATS_N) > R.GRID_THREADS and max(R.MARK_ROWS_N) > R.GRID_THREADS
    dims = set(R.COMPOSE_DIMS)
    assert {7, 8, 9} <= dims and {63, 64, 65} <= dims and {128, 129} <= dims
    assert any(3 * d * d <= R.COMPOSE_WAVES for d in dims if d > 64) and any(3 * d * d > R.COMPOSE_WAVES for d in dims)
    for tb in R.TYPED_BEGINS:
        rows = R.typed_rows_for(tb, np.random.default_rng(0))
        for r in (tb[1] - 1, tb[1], tb[2] - 1, tb[2]):
            assert r in rows or not tb[0] <= r < tb[3]
    assert any(tb[t] == tb[t + 1] for tb in R.TYPED_BEGINS for t in range(3)) and any(tb[0] > 0 for tb in R.TYPED_BEGINS)


# ---------------------------------------------------------------------------------------------
# the emulation passes both verdicts on the cases the GPU file runs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group', SCATTER_GROUPS)
def test_emulated_scatter_passes_both_verdicts(group):
    assert _scatter_failures(None, group) == set()


@pytest.mark.parametrize('group', COMBINE_GROUPS)
def test_emulated_combine_passes_both_verdicts(group):
    assert _combine_failures(None, group) == set()


def test_emulated_rows_add_and_put_pass_both_verdicts():
    for group in ROWS_ADD_GROUPS:
        for c, d in R.rows_add_cases(group):
            R.check_rows_add(c, d, R.emu_rows_add(c, d))
    for c, typed, assign in R.rows_put_cases():
        R.check_rows_put(c, typed, assign, R.emu_rows_put(c, typed, assign))


def _compose_failures(mutation):
    failed = set()
    for case in R.compose_cases():
        fwd, bwd = R.compose_fwd_reference(case), R.compose_bwd_reference(case)
        w_eff, b_eff = R.emu_compose_fwd(case, mutation)
        got = dict(R.emu_compose_bwd(case, mutation), w_eff=w_eff, b_eff=b_eff)
        for name, ref in list(fwd.items()) + list(bwd.items()):
            if _fails(lambda: R.hold_compose(got[name], ref, case.exact, f'{case.what} {name}')):
                failed.add((case.dim, case.exact, case.with_c, name))
    return failed


def test_emulated_compose_passes_its_verdicts():
    assert _compose_failures(None) == set()


# ---------------------------------------------------------------------------------------------
# every wrong variant fails, by name
# ---------------------------------------------------------------------------------------------
def test_mutation_drop_17th_member():
    failed = _scatter_failures('drop_17th_member', 'members')
    assert {'17 members in one window', '33 members in one window', '64 members in one window', 'hundreds of members'} <= failed
    assert not failed & {'15 members in one window', '16 members in one window', '2 members in one window'}
    assert '17 members in one window' in _combine_failures('drop_17th_member', 'members')


def test_mutation_drop_next_window():
    failed = _scatter_failures('drop_next_window', 'members')
    assert {'65 members across windows', '129 members across windows', 'window positions'} <= failed and '64 members in one window' not in failed
    assert 'window positions' in _combine_failures('drop_next_window', 'members')


def test_mutation_walk_from_k_plus_1_and_from_lo():
    """The leader's own row dropped; and every occurrence walking the block from its start (no follower retired): earlier rows counted again."""
    assert '1 members in one window' in _scatter_failures('walk_from_k_plus_1', 'members') and 'n = 1' in _scatter_failures('walk_from_k_plus_1', 'n')
    failed = _scatter_failures('followers_walk_from_lo', 'members')
    assert '2 members in one window' in failed and '1 members in one window' not in failed


def test_mutation_merge_across_blocks():
    failed = _combine_failures('merge_across_blocks', 'blocks')
    assert {'blocks of 1', 'blocks of 63', 'blocks of 64', 'blocks of 65', 'blocks of 1100', f'blocks of {R.SCATTER_MAX} (n = {R.COMBINE_N_WIDE})'} <= failed
    assert 'blocks of 0' not in failed and f'blocks of {R.COMBINE_N + 1}' not in failed


def test_mutation_negative_leader():
    assert {'a negative id alone', 'negative ids first, between members and last', 'negative ids across windows'} <= _combine_failures('negative_leader', 'members')
    assert 'a negative id alone' in _scatter_failures('negative_leader', 'members')


def test_mutation_drop_second_chunk():
    failed = _scatter_failures('drop_second_chunk', 'widths')
    assert failed == {f'width ladder {w}' for w in (R.CHUNK_COLS + 1, 2 * R.CHUNK_COLS + 1)}
    assert f'width ladder {R.CHUNK_COLS + 1}' in _combine_failures('drop_second_chunk', 'widths')


def test_mutation_tail_per_lane():
    for c, d in R.rows_add_cases('tail'):
        assert _fails(lambda: R.check_rows_add(c, d, R.emu_rows_add(c, d, 'tail_per_lane'))), c.what
    assert 'a tail alone' in _scatter_failures('tail_per_lane', 'forms')


@pytest.mark.parametrize('mutation', ['tail_low_edge', 'tail_high_edge'])
def test_mutation_tail_range_off_by_one(mutation):
    assert {'a tail alone', '2 blocks of 32 columns and a tail'} <= _scatter_failures(mutation, 'forms')
    c, d = R.rows_add_cases('tail')[0]
    assert _fails(lambda: R.check_rows_add(c, d, R.emu_rows_add(c, d, mutation)))


def test_mutation_block_mod_width():
    failed = _scatter_failures('block_mod_width', 'forms')
    assert {'2 blocks of 32 columns', '4 blocks of 65 columns', '2 blocks of 1 columns', '4 blocks of 32 columns and a tail'} <= failed
    assert not failed & {'1 blocks of 32 columns', 'plain matrix'}


def test_mutation_typed_gt_and_assign_zero_fill():
    gt, fill = set(), set()
    for c, typed, assign in R.rows_put_cases():
        if _fails(lambda: R.check_rows_put(c, typed, assign, R.emu_rows_put(c, typed, assign, 'typed_gt'))):
            gt.add(c.name)
        if _fails(lambda: R.check_rows_put(c, typed, assign, R.emu_rows_put(c, typed, assign, 'assign_zero_fill'))):
            fill.add(c.name)
    assert {f'rows_put types {tb} assign {a}' for tb in R.TYPED_BEGINS for a in (0, 1)} <= gt
    assert {f'rows_put types {tb} assign 1' for tb in R.TYPED_BEGINS} <= fill and not any(name.endswith('assign 0') for name in fill)


def test_mutation_follower_overwritten():
    failed = _combine_failures('follower_overwritten', 'members')
    assert {'2 members in one window', 'window positions', 'negative ids first, between members and last'} <= failed


def test_mutation_reverse_order_fails_the_batch_order_verdict_alone():
    for failures, group in ((_scatter_failures, 'float'), (_combine_failures, 'float')):
        assert 'order made visible' in failures('reverse_order', group)
        assert failures('reverse_order', group, order=False) == set()                   # ... while every float bound holds
    assert _scatter_failures('reverse_order', 'members', order=False) == set() == _scatter_failures('reverse_order', 'members')      # (exact cases: any order)


def test_mutations_of_the_compose_pair():
    failed = _compose_failures('compose_c_every_type')
    assert {(d, e, c, n) for d, e, c, n in failed} and all(n == 'b_eff' and c for _, _, c, n in failed) and {d for d, _, c, _ in failed} >= {7, 9, 32, 64, 96, 129}
    failed = _compose_failures('compose_da_without_bias_term')
    assert all(n == 'da' for *_, n in failed) and {d for d, *_ in failed} >= set(R.COMPOSE_DIMS) - {1}
    failed = _compose_failures('compose_tail_skipped')
    assert {d for d, *_ in failed} == {d for d in R.COMPOSE_DIMS if d % 8} and {n for *_, n in failed} == {'w_eff', 'b_eff', 'dw', 'db'}
    failed = _compose_failures('compose_second_wave_trip_skipped')
    assert {d for d, *_ in failed} == {d for d in R.COMPOSE_DIMS if d > 64} and all(n == 'da' for *_, n in failed)


def test_every_mutation_is_shown():
    import sys
    source = open(sys.modules[__name__].__file__).read()
    assert all(f"'{m}'" in source for m in R.MUTATIONS)


def test_small_kernel_references():
    users, queries, items = np.array([3, 0]), np.array([1, 1]), np.array([0, 5])
    assert R.node_rows_reference(users, queries, items, 10, 20).tolist() == [3, 0, 11, 11, 20, 25]
    base = np.arange(12, dtype=np.float32).reshape(4, 3) + 1
    assert R.zero_rows_reference(base, 2, [1, 1, 3]).tolist() == [[1, 2, 3], [0, 0, 6], [7, 8, 9], [0, 0, 12]]
    assert R.mark_rows_reference(np.full(5, 9, np.uint8), [4, 0, 4], 1).tolist() == [1, 9, 9, 9, 1]
    assert torch.equal(torch.from_numpy(R.first_occurrence(np.array([5, -1, 5, 6, 5]), 2)), torch.tensor([0, -1, 2, 3, 4]))
