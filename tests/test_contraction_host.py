"""CPU twin of ``tests/test_contraction_kernels.py``: the generators and their caps, the ladders recomputed from the launch table's numbers, the numpy emulation of
``tests/contraction_reference.py`` held to the same verdicts - on miniature kernels (tiles of 8, 16 ranges) for the ladders, and on the GPU test's own float cases at
d = 32 / 64 / 128 - and nine ways of being wrong, each shown to fail a named case."""
import numpy as np
import pytest
import torch

import contraction_reference as R
import split_emulation as SE

ARITHMETICS = ('two_fp16', 'three_bf16', 'f32')
LABEL = {'two_fp16': 'split', 'three_bf16': 'split', 'f32': 'f32'}


_case = R.edge_case


SMALL = R.Kernel('small', 8, 16, 'contiguous')         # a user-reduced kernel in miniature: tiles of 8, 16 ranges


# =============================================================================================
# the ladders are what their names say
# =============================================================================================
def _deal(n_rows, te, ranges, deal):
    """``(largest number of tiles in a range, ranges with a tile, rows of the last tile)`` by handing the tiles out one by one - no use of ``Kernel``'s own methods:
    contiguous: ``per = ceil(tiles / ranges)`` tiles to each range in turn, as the kernels compute it; strided: tile t to range t % ranges."""
    fills = [min(te, n_rows - r0) for r0 in range(0, n_rows, te)]
    per = (len(fills) + ranges - 1) // ranges
    owner = [t // per if deal == 'contiguous' else t % ranges for t in range(len(fills))]
    counts = np.bincount(np.asarray(owner, np.int64), minlength=ranges)
    assert len(counts) == ranges                                           # no tile beyond the last range
    return int(counts.max()), int((counts > 0).sum()), fills[-1]


def test_edge_ladders_walk_the_seams():
    """For every kernel of every supported launch, from the numbers (tiles handed out one by one, ``_deal``): ``per`` goes 1 -> 2 at RANGES TE + 1 and is 3 at the
    last rung, which leaves whole ranges empty under the contiguous deal and a partial last tile of 5; TE + 1 leaves a last tile of one hyperedge.  ``Kernel``'s
    own ``per`` / ``used_ranges`` / ``last_fill`` agree with that on every rung."""
    seen = 0
    for entry in R.ENTRIES:
        for dim in R.MFMA_DIMS:
            for arith in R.ARITHS:
                for order in R.ORDERS:
                    launch = R.edge_launch(entry, dim, order, arith)
                    ladder = R.edge_ladder(entry, dim, order, arith)
                    for k in launch['kernels']:
                        seen += 1
                        te, r = k.te, k.ranges
                        assert set(k.ladder()) <= set(ladder)
                        dealt = {n: _deal(n, te, r, k.deal) for n in k.ladder()}
                        for n, (per, used, fill) in dealt.items():
                            assert (k.per(n), k.used_ranges(n), k.last_fill(n)) == (per, used, fill), (k.name, n)
                        assert [dealt[n][0] for n in k.ladder()] == [1, 1, 1, 1, 1, 1, 2, 3]
                        assert [dealt[n][1] for n in k.ladder()[:6]] == [1, 1, 1, 2, r, r] and [dealt[n][2] for n in k.ladder()] == [1, te - 1, te, 1, te - 1, te, 1, 5]
                        assert dealt[k.ladder()[-1]][1] < r if k.deal == 'contiguous' else dealt[k.ladder()[-1]][1] == r
                        assert [k.per(n) for n in (1, te, te + 1, r * te - 1, r * te)] == [1] * 5
                        assert k.used_ranges(te) == 1 and k.used_ranges(te + 1) == 2 and k.used_ranges(r * te) == r
                        assert k.per(r * te + 1) == 2 and k.last_fill(r * te + 1) == 1 and k.last_fill(te - 1) == te - 1 and k.last_fill(te + 1) == 1
                        last = k.ladder()[-1]
                        assert k.per(last) == 3 and k.last_fill(last) == 5
                        if k.deal == 'contiguous':
                            assert k.used_ranges(last) == -(-(2 * r + 2) // 3) < r                    # whole empty ranges at the end
                            assert k.used_ranges(r * te + 1) == r // 2 + 1
    assert seen > 60


def test_launch_table_covers_what_the_issue_names():
    tes = {k.te for e in R.ENTRIES for d in R.MFMA_DIMS for a in R.ARITHS for k in R.edge_launch(e, d, 3, a)['kernels']}
    ranges = {k.ranges for e in R.ENTRIES for d in R.MFMA_DIMS for a in R.ARITHS for k in R.edge_launch(e, d, 3, a)['kernels']}
    assert {16, 32} <= tes and {32, 64, 128, 256, 2048} <= ranges
    assert R.edge_launch('fwd', 256, 3, 'f32')['kernels'][0].deal == 'strided'
    assert R.edge_launch('fwd', 12, 3, 'split')['arithmetic'] == 'scalar' and not R.edge_launch('gathered', 12, 3, 'split')['supported']
    for dim in (64, 128, 256):
        assert R.edge_launch('bwd', dim, 2, 'split')['arithmetic'] == 'split' and R.edge_launch('bwd', dim, 2, 'f32')['arithmetic'] == 'f32'
    assert R.edge_launch('bwd', 32, 3, 'split')['arithmetic'] == 'f32'


@pytest.mark.parametrize('kernel', [R._members(32, 'split', True), R._members(64, 'split', True), R._members(128, 'split', True), R._members(256, 'split', True),
                                    R._members(128, 'f32', True), SMALL], ids=lambda k: f'{k.name}-{k.te}-{k.ranges}')
def test_user_runs_are_what_they_say(kernel):
    runs = R.user_runs(kernel)
    users, te, named, rs = runs['users'], kernel.te, runs['named'], runs['runs']
    n_edges = len(users)
    per, used, fill = _deal(n_edges, te, kernel.ranges, kernel.deal)
    p = per * te
    assert per == 2 == runs['per'] and fill == 5 and used < kernel.ranges
    assert bool((np.diff(users) >= 0).all())
    for user, b, e in rs:                                                   # a run is all of a user's hyperedges
        assert bool((users[b:e] == user).all()) and (b == 0 or users[b - 1] != user) and (e == n_edges or users[e] != user)
    assert rs[named['one_range']][1:] == (0, p)                             # range 0 is one run
    assert rs[named['ends_on_range_end']][2] == 2 * p == rs[named['starts_on_range_begin']][1]
    _, b, e = rs[named['through_ranges']]
    assert b % te != 0 and e - b == 3 * p + 1
    first_range, last_range = b // p, (e - 1) // p
    assert last_range - first_range >= 3 and b > first_range * p and e < (last_range + 1) * p      # the middle ranges lie wholly inside it
    assert [rs[named[f'run_{k:+d}']][2] - rs[named[f'run_{k:+d}']][1] for k in (-1, 0, 1)] == [te - 1, te, te + 1]
    assert all(rs[named['singles'] + k][2] - rs[named['singles'] + k][1] == 1 for k in range(2 * te + 3))
    assert rs[named['last']][2] == n_edges
    present = np.zeros(runs['n_users'], bool)
    present[users] = True
    assert not present[:2].any() and not present[-3:].any() and (~present[2:-3]).sum() >= len(rs) // 3 - 1


def test_type_cases_hold_the_ladder_in_every_position():
    for dim in R.MFMA_DIMS:
        group = 4 if dim == 256 else 8
        cases = [np.diff(tb) for tb in R.type_cases(dim)]
        for tile in (16, 32):
            for pos in range(3):
                assert set(R.type_ladder(tile, group)) <= {int(c[pos]) for c in cases}, (dim, tile, pos)
        assert any(c[0] == 0 and c[1] > 0 and c[2] > 0 for c in cases) and any(c[2] == 0 and c[0] > 0 and c[1] > 0 for c in cases)
        assert sum(1 for c in cases if (c == 0).sum() == 2) == 3
        assert R.type_ladder(32, group) == [0, 1, 31, 32, 33, 32 * group - 1, 32 * group + 1]


def test_node_weight_plan_reaches_one_two_and_three_tiles_per_range():
    for dim, ranges in ((32, 512), (64, 256), (128, 128), (256, 32)):
        for k, per in enumerate((1, 2, 3)):
            rows = [7, 40, 33]
            rows[k] = R.rows_for_tiles_per_range(dim, per)
            tb = tuple(int(v) for v in np.concatenate([[0], np.cumsum(rows)]))
            plan = R.node_weight_plan(tb, dim)
            assert plan[k][1] == per and sum(n for n, _ in plan) <= ranges and all(n >= 1 for n, _ in plan), (dim, per, plan)
    assert R.node_weight_plan((0, 0, 40, 40), 64) == [(0, 0), (2, 1), (0, 0)]


def test_rising_exponents_place_the_largest_row():
    for tile in (16, 32):
        n = 5 * tile
        assert int(np.argmax(R.rising_exponents(n, tile, 5, 'last'))) == n - 1
        assert int(np.argmax(R.rising_exponents(n, tile, 5, 'first_of_tile'))) == 4 * tile
        e = R.rising_exponents(n + 1, tile, 5, 'alone')
        assert int(np.argmax(e)) == n and (n + 1) % tile == 1
        assert bool((np.diff(e[:n]) >= 0).all()) and e[0] == 0 and (e == 5).sum() == 1


# =============================================================================================
# the generators and their caps
# =============================================================================================
@pytest.mark.parametrize('order', R.ORDERS)
@pytest.mark.parametrize('dim', [8, 32, 64])
def test_exact_cases_stay_under_the_cap(dim, order):
    c = _case(150, dim, order, ('cap', dim, order))
    out, mag = R.fwd64(c)
    assert 0 < R.ensure_exact(mag) < R.CAP and bool((out == out.round()).all())
    dout, dmag = R.gathered_dout64(c)
    R.ensure_exact(dmag, 0.5)
    for want in (R.bwd64(c), R.bwd64(c, dout, dmag)):
        for name in ('g', 'dw', 'dh'):
            R.ensure_exact(want[name + '_mag'], 0.5)
            assert bool((want[name].abs() <= want[name + '_mag']).all())
    n = R.NodeCase((0, 17, 40, 75), dim, order, R._gen('cap', dim), True, m=3)
    R.ensure_exact(R.node_fwd64(n)[1], 0.5)
    R.ensure_exact(R.node_weight64(n)[1], 0.5)
    assert bool(n.isolated.any()) and bool((R.node_fwd64(n)[0][n.isolated] == 0).all())      # isolated nodes: exactly zero rows


def test_reference_shortcuts_equal_the_plain_sums():
    """The chunked tall product and the run sums by running-sum differences against ``a.T @ b`` and ``index_add_`` on an integer case."""
    c = _case(3000, 16, 3, ('shortcuts',))
    assert torch.equal(R._tn(c.dout, c.dout.abs()), c.dout.T @ c.dout.abs())
    want = R.bwd64(c)
    users = c.i3[:, 0].long()
    assert torch.equal(want['dh'], torch.zeros(c.n_users, 16, dtype=torch.float64).index_add_(0, users, want['g'][:, 0]))
    assert torch.equal(want['has_edges'], torch.bincount(users, minlength=c.n_users) > 0)


def test_a_case_beyond_the_cap_is_refused_not_skipped():
    c = _case(6000, 64, 3, ('beyond',), layout=R.run_layout('one', 6000))
    with pytest.raises(ValueError, match='2\\^24'):
        R.ensure_exact(R.bwd64(c)['dh_mag'])
    small = _case(6000, 64, 3, ('beyond',), m=1, layout=R.run_layout('one', 6000))
    R.ensure_exact(R.bwd64(small)['dh_mag'])
    with pytest.raises(ValueError, match='multiple'):
        R.ensure_exact(torch.tensor([0.25]), 0.5)


def test_split_arithmetic_is_exact_on_small_integers():
    """Third-order products of integers in [-4, 4] against integer weights, K = 7 d: both splits give the float64 product exactly (``split_emulation``)."""
    rng = R._gen('ints')
    for d in (64, 128):
        x = rng.integers(-4, 5, (40, 7 * d)) * rng.integers(-4, 5, (40, 7 * d)) * rng.integers(-4, 5, (40, 7 * d))
        w = rng.integers(-4, 5, (d, 7 * d))
        want = x.astype(np.float64) @ w.T.astype(np.float64)
        assert np.array_equal(SE.dot_two_fp16(x, w), want) and np.array_equal(SE.dot_three_bf16(x, w), want)
        assert np.array_equal(R.emu_dot(x, w, 'two_fp16'), want) and np.array_equal(R.emu_dot(x, w, 'three_bf16'), want)


# =============================================================================================
# the emulation passes the verdicts
# =============================================================================================
def _emu_backward(c, arithmetic, kernel, mutation=None, dout=None):
    g = R.emu_members(c, arithmetic, mutation, dout)
    users = c.i3[:, 0].numpy().astype(np.int64)
    dh = R.emu_user_reduce(g[:, 0], users, c.n_users, kernel, mutation, prefill=-1.5)
    i3, h = c.i3.numpy().astype(np.int64), c.h.numpy().astype(np.float32)
    hu, hq, hi = (h[i3[:, s]] for s in range(3))
    z = [hu * hq, hq * hi, hi * hu] + ([(hu * hq) * hi] if c.order == 3 else [])
    d32 = c.dout.numpy().astype(np.float32) if dout is None else dout
    wk = R.Kernel('weight', kernel.te, kernel.ranges, kernel.deal)
    dw = np.concatenate([R.emu_weight(d32, zb, wk, arithmetic, mutation) for zb in z], 1)
    return torch.from_numpy(g), torch.from_numpy(dh), torch.from_numpy(dw)


def _verdict_exact(c, arithmetic, kernel, mutation=None):
    """The exact verdicts of the GPU test on the emulation: raises AssertionError where an output differs."""
    out, mag = R.fwd64(c)
    R.ensure_exact(mag)
    got = torch.from_numpy(R.emu_fwd(c, arithmetic, mutation, te=kernel.te))
    R.assert_equal(got, out, 'out')
    want = R.bwd64(c)
    g, dh, dw = _emu_backward(c, arithmetic, kernel, mutation)
    for name in ('g', 'dh', 'dw'):
        R.ensure_exact(want[name + '_mag'])
    R.assert_equal(g, want['g'], 'g')
    has = want['has_edges']
    assert bool((dh[~has] == -1.5).all()), 'the dh row of a user without hyperedges was written'
    R.assert_equal(dh[has], want['dh'][has], 'dh')
    R.assert_equal(dw, want['dw'], 'dw')


def _verdict_float(c, arithmetic, kernel, mutation=None):
    label = LABEL[arithmetic]
    out, mag = R.fwd64(c)
    d, e = c.dim, len(c.i3)
    nb_g = 3 if c.order == 3 else 2
    worst = [R.assert_within(torch.from_numpy(R.emu_fwd(c, arithmetic, mutation, te=kernel.te)), out, R.float_bound('fwd', 3 + R.product_blocks(c.order) * d, mag, label), 'out')]
    want = R.bwd64(c)
    g, dh, dw = _emu_backward(c, arithmetic, kernel, mutation)
    worst.append(R.assert_within(g, want['g'], R.float_bound('members', nb_g * d, want['g_mag'], label), 'g'))
    run = torch.bincount(c.i3[:, 0].long(), minlength=c.n_users).double()[:, None]
    has = want['has_edges']
    worst.append(R.assert_within(dh[has], want['dh'][has], R.float_bound('dh', run * nb_g * d, want['dh_mag'], label)[has], 'dh'))
    worst.append(R.assert_within(dw, want['dw'], R.float_bound('dw', e, want['dw_mag'], label), 'dw'))
    return max(worst)


def _small_runs_case(dim, order, exact, key, m=4):
    runs = R.user_runs(SMALL)
    return _case(len(runs['users']), dim, order, key, exact, m, layout=(runs['users'], runs['n_users'])), runs


@pytest.mark.parametrize('arithmetic', ARITHMETICS)
@pytest.mark.parametrize('order', R.ORDERS)
def test_emulation_is_exact_on_the_exact_cases(arithmetic, order):
    """Hyperedge ladder rungs and the user-run ladder of the miniature kernel (tiles of 8, 16 ranges) at d = 16: the emulation EQUALS the float64 reference."""
    for n_edges in SMALL.ladder():
        _verdict_exact(_case(n_edges, 16, order, ('emu', order, n_edges)), arithmetic, SMALL)
    c, _ = _small_runs_case(16, order, True, ('emu runs', order))
    _verdict_exact(c, arithmetic, SMALL)
    for kind in ('singles', 'one'):
        n = SMALL.ladder()[-1]
        _verdict_exact(_case(n, 16, order, ('emu', kind), m=1 if kind == 'one' else 4, layout=R.run_layout(kind, n)), arithmetic, SMALL)


@pytest.mark.parametrize('arithmetic', ARITHMETICS)
def test_emulation_passes_the_float_bound(arithmetic):
    """``randn`` operands and the adversarial significands of the arithmetic's split, orders 2 and 3, d = 64: every output within the bound the kernels are held to."""
    for order in R.ORDERS:
        c, _ = _small_runs_case(64, order, False, ('emu float', order))
        assert _verdict_float(c, arithmetic, SMALL) <= 1.0
        R.make_worst(c, ('h', 'w', 'dout', 'p'), arithmetic, order)
        assert _verdict_float(c, arithmetic, SMALL) <= 1.0


@pytest.mark.parametrize('arithmetic', ARITHMETICS)
def test_node_level_emulation_passes_both_verdicts(arithmetic):
    for k, tb in enumerate(R.type_cases(64)[::5]):
        c = R.NodeCase(tb, 16, 3, R._gen('emu node', k), True, m=3)
        want, mag = R.node_fwd64(c)
        R.ensure_exact(mag, 0.5)
        R.assert_equal(torch.from_numpy(R.emu_node_fwd(c, arithmetic)), want, f'type_begin {tb}')
    c = R.NodeCase((0, 70, 79, 210), 64, 3, R._gen('emu node float'), False)
    want, mag = R.node_fwd64(c)
    assert R.assert_within(torch.from_numpy(R.emu_node_fwd(c, arithmetic)), want, R.float_bound('node_fwd', 7 * 64 + 1, mag, LABEL[arithmetic]), 'node float') <= 1.0


def _verdict_launch(entry, dim, order, arith, design):
    """The float verdicts of the GPU test on ITS OWN case (``contraction_reference.float_case``), every kernel of the launch emulated with the tile size, the ranges,
    the deal and the operand split the launch table records for it.  Returns the worst error / bound."""
    launch = R.edge_launch(entry, dim, order, arith)
    c = R.float_case(entry, dim, order, arith, design)
    label, d, e = launch['arithmetic'], c.dim, len(c.i3)
    if entry == 'fwd':
        k = launch['kernels'][0]
        out, mag = R.fwd64(c)
        return R.assert_within(torch.from_numpy(R.emu_fwd(c, k.arithmetic, te=k.te)), out, R.float_bound('fwd', 3 + R.product_blocks(order) * d, mag, label), 'out')
    members, weights = launch['kernels']
    want = R.bwd64(c)
    nb_g = 3 if order == 3 else 2
    g = R.emu_members(c, members.arithmetic)
    worst = [R.assert_within(torch.from_numpy(g), want['g'], R.float_bound('members', nb_g * d, want['g_mag'], label), 'g')]
    if entry == 'user_reduced':
        users = c.i3[:, 0].numpy().astype(np.int64)
        dh = torch.from_numpy(R.emu_user_reduce(g[:, 0], users, c.n_users, members, prefill=-1.5))
        run, has = torch.bincount(c.i3[:, 0].long(), minlength=c.n_users).double()[:, None], want['has_edges']
        assert bool((dh[~has] == -1.5).all())
        worst.append(R.assert_within(dh[has], want['dh'][has], R.float_bound('dh', run * nb_g * d, want['dh_mag'], label)[has], 'dh'))
    i3, h = c.i3.numpy().astype(np.int64), c.h.numpy().astype(np.float32)
    hu, hq, hi = (h[i3[:, s]] for s in range(3))
    z = [hu * hq, hq * hi, hi * hu] + ([(hu * hq) * hi] if order == 3 else [])
    dw = np.concatenate([R.emu_weight(c.dout.numpy().astype(np.float32), zb, weights, weights.arithmetic) for zb in z], 1)
    worst.append(R.assert_within(torch.from_numpy(dw), want['dw'], R.float_bound('dw', e, want['dw_mag'], label), 'dw'))
    return max(worst)


@pytest.mark.parametrize('entry,dim,arith', [('fwd', 64, 'split'), ('bwd', 64, 'split'), ('user_reduced', 64, 'split'), ('fwd', 64, 'f32'), ('bwd', 64, 'f32'),
                                             ('user_reduced', 32, 'split'), ('fwd', 128, 'split')])
def test_emulation_passes_the_gpu_float_cases_themselves(entry, dim, arith):
    """The very float cases ``test_edge_float`` sends to the GPU at these instances - ``randn`` and one adversarial design per operand split of the launch (the
    backward at d = 64: two fp16 terms for the member gradients AND three bf16 terms for the weight gradient) - through the emulation of the launch's kernels."""
    launch = R.edge_launch(entry, dim, 3, arith)
    designs = R.float_designs(launch)
    assert designs[1:] == {('fwd', 'split'): ['worst three_bf16'], ('bwd', 'split'): ['worst two_fp16', 'worst three_bf16'],
                           ('user_reduced', 'split'): ['worst two_fp16', 'worst three_bf16']}.get((entry, launch['arithmetic']), ['worst f32'])
    for order in R.ORDERS:
        for design in designs:
            assert _verdict_launch(entry, dim, order, arith, design) <= 1.0


def test_each_split_meets_its_own_adversarial_significand():
    """What the two significands do under the OTHER split: the two-fp16 one loses about 2^-29 per product under three bf16 terms, the three-bf16 one stays below its
    own 2^-21 - so a launch is given the significand of the split its kernels use, per kernel (``Kernel.arithmetic``)."""
    two, three = R.worst_significand('two_fp16'), R.worst_significand('three_bf16')
    loss = lambda dot, s: float(abs(dot(np.full((1, 32), s, np.float32), np.full((1, 32), s, np.float32))[0, 0] - 32 * float(s) ** 2) / (32 * float(s) ** 2))
    assert 2.0 ** -23 < loss(SE.dot_two_fp16, two) <= 2.0 ** -21 and 2.0 ** -23 < loss(SE.dot_three_bf16, three) <= 2.0 ** -21
    assert loss(SE.dot_three_bf16, two) < 2.0 ** -27
    assert R.worst_significand('f32') == three
    assert [k.arithmetic for k in R.edge_launch('bwd', 128, 3, 'split')['kernels']] == ['two_fp16', 'three_bf16']
    assert R.edge_launch('fwd', 256, 2, 'split')['kernels'][0].arithmetic == 'three_bf16' and R.node_launch('weight', 64, 'split')['split'] == 'two_fp16'
    assert all(k.arithmetic == 'f32' for d in R.MFMA_DIMS for k in R.edge_launch('bwd', d, 3, 'f32')['kernels'])


def _running_scale_operands(tile=16):
    rng = R._gen('running')
    n = 5 * tile + 1
    up = R.rising_exponents(n, tile, 6, 'alone')
    a = rng.integers(-2, 3, (n, 24)) * np.ldexp(1.0, up)[:, None]
    b = rng.integers(-2, 3, (n, 40)) * np.ldexp(1.0, up // 2)[:, None]
    a[:tile] = 0                                                             # a whole first tile of zero rows
    b[tile + 3] = 0
    return a.astype(np.float32), b.astype(np.float32), tile


def test_running_scale_emulation_is_exact():
    a, b, tile = _running_scale_operands()
    want = a.astype(np.float64).T @ b.astype(np.float64)
    R.ensure_exact(torch.from_numpy(np.abs(a).astype(np.float64).T @ np.abs(b).astype(np.float64)))
    assert np.array_equal(R.emu_running_scale_weight(a, b, tile), want)


# =============================================================================================
# nine ways of being wrong, each failing a named case
# =============================================================================================
def _fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError as exc:
        return str(exc)
    return None


def test_mutation_1_a_dropped_hyperedge_of_the_last_partial_tile_fails_the_ladder_rung_te_plus_1():
    c = _case(SMALL.te + 1, 16, 3, ('emu', 3, SMALL.te + 1))
    assert _fails(_verdict_exact, c, 'two_fp16', SMALL) is None
    assert 'out' in _fails(_verdict_exact, c, 'two_fp16', SMALL, 'drop_edge_of_last_partial_tile')


def test_mutation_2_a_padded_row_counted_in_dw_fails_the_last_ladder_rung():
    c = _case(SMALL.ladder()[-1], 16, 3, ('emu', 3, SMALL.ladder()[-1]))
    assert 'dw' in _fails(_verdict_exact, c, 'three_bf16', SMALL, 'count_padded_row')


def test_mutation_3_a_wrong_weight_block_for_one_type_fails_the_type_ladder():
    tb = R.type_cases(64)[0]
    c = R.NodeCase(tb, 16, 3, R._gen('emu node', 0), True, m=3)
    want, _ = R.node_fwd64(c)
    R.assert_equal(torch.from_numpy(R.emu_node_fwd(c, 'two_fp16')), want, 'types')
    message = _fails(R.assert_equal, torch.from_numpy(R.emu_node_fwd(c, 'two_fp16', 'wrong_weight_block')), want, 'types')
    assert message is not None
    lo = tb[2]                                                               # only the items' rows are wrong
    assert torch.equal(torch.from_numpy(R.emu_node_fwd(c, 'two_fp16', 'wrong_weight_block'))[:lo], want[:lo].float())
    # and a reference with the users' table for every type is NOT the reference: the kernel's own table is held, not assumed
    other, _ = R.node_fwd64(c, w_block_of={t: R.W_BLOCK_OF[0] for t in range(3)})
    assert not torch.equal(other, want)


def test_mutation_4_a_dropped_boundary_entry_fails_the_run_ladder():
    c, runs = _small_runs_case(16, 3, True, ('emu runs', 3))
    message = _fails(_verdict_exact, c, 'two_fp16', SMALL, 'drop_boundary_entry')
    assert message is not None and 'dh' in message


def test_mutation_5_a_run_through_three_ranges_closed_early_fails_the_run_ladder():
    c, runs = _small_runs_case(16, 3, True, ('emu runs', 3))
    message = _fails(_verdict_exact, c, 'f32', SMALL, 'close_run_early')
    assert message is not None and 'dh' in message
    user = runs['runs'][runs['named']['through_ranges']][0]
    want = R.bwd64(c)
    g = R.emu_members(c, 'f32')
    dh = torch.from_numpy(R.emu_user_reduce(g[:, 0], runs['users'], c.n_users, SMALL, 'close_run_early', prefill=-1.5))
    wrong = (dh != want['dh'].float()).any(1) & want['has_edges']
    assert wrong.nonzero().flatten().tolist() == [user]                      # exactly the run that lies in more than two ranges


def test_mutation_6_hi_lo_omitted_fails_the_float_case():
    c, _ = _small_runs_case(64, 3, False, ('emu float', 3))
    assert _fails(_verdict_float, c, 'two_fp16', SMALL) is None
    assert _fails(_verdict_float, c, 'two_fp16', SMALL, 'omit_hi_lo') is not None


def test_mutation_7_accumulators_not_rescaled_fail_the_running_scale_case():
    a, b, tile = _running_scale_operands()
    want = a.astype(np.float64).T @ b.astype(np.float64)
    assert not np.array_equal(R.emu_running_scale_weight(a, b, tile, 'no_rescale'), want)


def test_mutation_8_bias_scaled_twice_fails_the_type_ladder():
    c = R.NodeCase(R.type_cases(64)[5], 16, 3, R._gen('emu node', 5), True, m=3)
    want, _ = R.node_fwd64(c)
    assert _fails(R.assert_equal, torch.from_numpy(R.emu_node_fwd(c, 'f32', 'bias_scaled_twice')), want, 'types') is not None
    twice, _ = R.node_fwd64(c, bias_scale_twice=True)                        # (the same mistake in the reference's copy is not the reference either)
    assert not torch.equal(twice, want)


def test_mutation_9_a_partial_kept_in_fp16_fails_the_float_case():
    c, _ = _small_runs_case(64, 3, False, ('emu float', 3))
    with np.errstate(invalid='ignore'):                                      # (fp16 partials overflow at the adversarial magnitudes: inf - inf further on)
        for arithmetic in ARITHMETICS:
            assert _fails(_verdict_float, c, arithmetic, SMALL, 'fp16_partial') is not None
