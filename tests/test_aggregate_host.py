"""CPU guard of ``tests/aggregate_reference.py``: the generators keep the exact condition, the vectorised references equal plain loops, the split-row ladder holds a
row in every interval of the finish kernel's loops that it claims, and the float bound leaves room for a sequential float32 sum (so a kernel that misses it on the GPU
is wrong, the bar is not tight)."""
import numpy as np
import pytest
import torch

import aggregate_reference as R


def _k5_inputs(dim, n_edges, on, exact, seed, n_nodes=41, i3=None):
    rng = np.random.default_rng(seed)
    if i3 is None:
        i3 = torch.from_numpy(rng.integers(0, n_nodes, (n_edges, 3)).astype(np.int32))
    src, kw = R.k5_case(dim, i3, on, exact, rng, n_nodes)
    return src, i3, kw


def _k7_inputs(lengths, dim, options, exact, seed):
    rng = np.random.default_rng(seed)
    n_src = len(lengths) + 5
    ptr, ids = R.csr_from_lengths(lengths, n_src, rng)
    src, kw = R.k7_case(ptr, ids, n_src, dim, options, exact, rng)
    return src, torch.from_numpy(ptr), torch.from_numpy(ids), kw


ALL_ON = R.K7_ALL_ON


def test_launch_geometry_table():
    """dim -> G as the issue lists it, the hyperedge counts around a wave's share of K5, the geometries' alignment."""
    assert [R.group_lanes(d, 4) for d in R.WIDE_DIMS] == [4, 8, 16, 32, 64, 64, 4]
    assert [R.group_lanes(d, 1) for d in R.NARROW_DIMS] == [4, 8, 16, 32, 64, 64]
    assert [R.k5_epw(g) for g in (4, 8, 16, 32, 64)] == [16, 16, 12, 6, 3]
    assert R.k5_edge_counts(64) == [0, 1, 2, 3, 4, 11] and R.MAX_WAVES == 65536
    for dim in R.ALL_DIMS:
        for geometry in R.GEOMETRIES:
            ld, col0 = R.geometry_of(dim, geometry)
            assert ld >= col0 + dim
            wide = dim % 4 == 0 and ld % 4 == 0 and col0 % 4 == 0
            assert (R.vec_of(dim, geometry) == 4) == wide, (dim, geometry)
    assert R.vec_of(100, 'c') == 1 and R.group_lanes(100, 1) == 64 and R.vec_of(256, 'd') == 1


@pytest.mark.parametrize('dim', R.ALL_DIMS)
def test_k5_cases_are_exact_and_match_loops(dim):
    g = R.group_lanes(dim, R.vec_of(dim, 'a'))
    for on in (False, True):
        for n_edges in R.k5_edge_counts(g):
            src, i3, kw = _k5_inputs(dim, n_edges, on, True, seed=dim)
            ref = R.edge_gather_reference(src, i3, **kw)
            R.assert_exact_condition(ref, f'K5 dim {dim} E {n_edges}')
            assert torch.equal(ref.want, R.edge_gather_loops(src, i3, **kw))
        src, i3, kw = _k5_inputs(dim, 0, on, True, seed=dim + 1, i3=R.reuse_i3(41))
        ref = R.edge_gather_reference(src, i3, **kw)
        R.assert_exact_condition(ref, f'K5 dim {dim} reuse')
        if dim <= 32:
            assert torch.equal(ref.want, R.edge_gather_loops(src, i3, **kw))


def test_reuse_list_has_the_blocks_it_claims():
    i3 = R.reuse_i3(41).numpy()
    col0 = i3[:-1, 0]
    cuts = np.flatnonzero(np.diff(col0) != 0) + 1
    runs = np.diff(np.concatenate([[0], cuts, [len(col0)]]))
    assert list(runs[:10]) == [1, 2, 3, 4, 7, 1, 2, 3, 4, 7] and set(runs) == {1, 2, 3, 4, 7}
    for b, e in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(col0)]])):
        assert len(set(i3[b:e, 1])) == e - b and len(set(i3[b:e, 2])) == e - b
    assert len(set(i3[-1])) == 1
    for g, u in R.K5_U.items():                                                          # a block crosses a lane group's boundary at every U > 1
        if u > 1:
            assert any(b // u != (e - 1) // u for b, e in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(col0)]])))


@pytest.mark.parametrize('dim', R.ALL_DIMS)
def test_k7_light_cases_are_exact_and_match_loops(dim):
    for geometry in ('a', 'c'):
        g = R.group_lanes(dim, R.vec_of(dim, geometry))
        lengths = R.light_lengths(g, np.random.default_rng(dim))
        assert {0, 1, g - 1, g, g + 1, 7, 8, 9, 15, 16, 17, 2 * g + 3, 200} <= set(lengths) and lengths[:4] == [0, 200, 0, 0]
        for options in ((), ALL_ON, ('mode1', 'src_scale')):
            src, ptr, ids, kw = _k7_inputs(lengths, dim, options, True, seed=dim)
            ref = R.segment_sum_reference(src, ptr, ids, **kw)
            R.assert_exact_condition(ref, f'K7 dim {dim} {options}')
            if dim <= 16:
                assert torch.equal(ref.want, R.segment_sum_loops(src, ptr, ids, **kw))


def test_masked_rows_do_not_reach_the_reference():
    src, ptr, ids, kw = _k7_inputs([0, 3, 9, 1, 17], 7, ALL_ON, True, seed=3)
    poisoned = src.clone()
    poisoned[kw['src_mask'] == 0] = float('nan')
    a, b = R.segment_sum_reference(src, ptr, ids, **kw), R.segment_sum_reference(poisoned, ptr, ids, **kw)
    assert torch.equal(a.want, b.want) and bool(torch.isfinite(b.want).all()) and torch.equal(a.n, b.n)
    assert torch.equal(b.want, R.segment_sum_loops(src, ptr, ids, **kw))


@pytest.mark.parametrize('dim', R.ALL_DIMS)
def test_ladder_rows_sit_in_the_intervals_they_claim(dim):
    """The segment counts recomputed from ``Csr``'s plan (built on the CPU): the ladder's, and between them they take every path through the finish kernel's loops."""
    from ihgnn_amd.layout import Csr
    for geometry in ('a', 'c'):
        g = R.group_lanes(dim, R.vec_of(dim, geometry))
        groups = R.finish_groups(g)
        lengths = R.ladder_lengths(g, np.random.default_rng(dim))
        ptr, ids = R.csr_from_lengths(lengths, len(lengths) + 5, np.random.default_rng(dim))
        csr = Csr(ptr, ids, torch.device('cpu'), heavy_threshold=2, heavy_chunk=2)
        counts = np.diff(csr.heavy_segptr.numpy())
        rows = csr.heavy_rows.numpy()
        assert sorted(counts) == sorted(R.ladder_segment_counts(g) + [6]) and csr.n_heavy == len(counts)
        assert all(counts[k] == (lengths[r] + 1) // 2 for k, r in enumerate(rows))
        seg_len = (csr.seg_end - csr.seg_begin).numpy()
        assert set(seg_len) == {1, 2} and (seg_len == 1).sum() == 1                      # one odd row: its last segment holds one entry
        assert sum(1 for n in lengths if n <= 2) >= 5
        trips = {int(s): R.finish_trips(int(s), groups) for s in counts}
        seen = set().union(*[set(t) for t in trips.values()])
        assert min(counts) < groups                                                      # a row with idle lane groups
        assert any(t16 == 0 and t4 == 0 and tail == 1 for t16, t4, tail in seen)
        assert any(t16 == 0 and t4 == 1 for t16, t4, tail in seen) and any(t16 == 0 and t4 == 3 and tail == 3 for t16, t4, tail in seen)
        assert any(t16 == 1 and t4 == 0 and tail == 0 for t16, t4, tail in seen) and any(t16 == 1 and t4 == 0 and tail == 1 for t16, t4, tail in seen)
        assert any(t16 == 1 and t4 == 1 for t16, t4, tail in seen) and any(t16 == 2 for t16, t4, tail in seen)
        assert len(set(trips[16 * groups - 1])) == 2                                     # some lane groups in the 16-deep loop, the last one not
        assert all(sum(d * t for d, t in zip((16, 4, 1), trip)) * groups >= s - groups for s, ts in trips.items() for trip in ts)
        assert all(sum(sum(d * t for d, t in zip((16, 4, 1), trip)) for trip in ts) == s for s, ts in trips.items())


def test_capped_segments_are_longer_and_even(monkeypatch):
    from ihgnn_amd import layout
    monkeypatch.setattr(layout, 'HEAVY_MAX_SEGMENTS', 8)
    ptr, ids = R.csr_from_lengths([1, 101, 2], 8, np.random.default_rng(0))
    csr = layout.Csr(ptr, ids, torch.device('cpu'), heavy_threshold=2, heavy_chunk=2)
    seg_len = (csr.seg_end - csr.seg_begin).tolist()
    assert seg_len == [14] * 7 + [3] and csr.n_heavy == 1


@pytest.mark.parametrize('dim', [8, 16, 32])
def test_pair_cases_are_exact_and_match_loops(dim):
    g = R.group_lanes(dim, 4)
    rng = np.random.default_rng(dim)
    lengths = [2 * k for k in (0, 1, g // 2, g // 2 + 1, 0, 3)] + [2 * k for k in R.ladder_segment_counts(g)[:4]]
    ptr, ids = R.csr_from_lengths(lengths, 23, rng)
    h = R.features(rng, 23, dim, True)
    for pw in (None, R.weights(rng, len(ids) // 2, True)):
        ref = R.pair_sums_reference(h, torch.from_numpy(ptr), torch.from_numpy(ids), pw)
        R.assert_exact_condition(ref, f'pairs dim {dim}', bits=0)
        if dim <= 16:
            assert torch.equal(ref.want, R.pair_sums_loops(h, torch.from_numpy(ptr), torch.from_numpy(ids), pw))


def test_largest_ladders_keep_the_exact_condition():
    """The longest rows of the suite (4,230 entries at G = 4; 2,115 weighted pairs) with every option on stay below 2^24 units."""
    rng = np.random.default_rng(1)
    lengths = R.ladder_lengths(4, rng)
    src, ptr, ids, kw = _k7_inputs(lengths, 16, ALL_ON, True, seed=2)
    assert R.assert_exact_condition(R.segment_sum_reference(src, ptr, ids, **kw), 'ladder, all options') > 1 << 16
    for mode in ('mode1', 'mode2'):
        src, ptr, ids, kw = _k7_inputs(lengths, 3, ('src_scale', 'entry_scale', mode), True, seed=3)
        R.assert_exact_condition(R.segment_sum_reference(src, ptr, ids, **kw), f'ladder, {mode}')
    ptr, ids = R.csr_from_lengths(R.pair_ladder_lengths(4, rng), 29, rng)
    ref = R.pair_sums_reference(R.features(rng, 29, 8, True), torch.from_numpy(ptr), torch.from_numpy(ids), R.weights(rng, len(ids) // 2, True))
    R.assert_exact_condition(ref, 'pair ladder', bits=0)


def test_exact_condition_refuses_a_case_that_is_not_exact():
    src = torch.ones(4, 2)
    ptr, ids = torch.tensor([0, 3]), torch.tensor([0, 1, 2])
    with pytest.raises(AssertionError, match='not a multiple'):
        R.assert_exact_condition(R.segment_sum_reference(src, ptr, ids, src_scale=torch.full((4,), 1 / 32)), 'sixteenths')
    big = torch.full((3, 1), 8.0)
    ids = torch.zeros(300000, dtype=torch.int64)
    with pytest.raises(AssertionError, match='not below 2\\^24'):
        R.assert_exact_condition(R.segment_sum_reference(big, torch.tensor([0, 300000]), ids, src_scale=torch.full((3,), 4.0)), 'too long')


def test_exact_verdict_notices_one_dropped_entry():
    src, ptr, ids, kw = _k7_inputs([4, 0, 9], 5, (), True, seed=9)
    ref = R.segment_sum_reference(src, ptr, ids, **kw)
    R.assert_exact(ref.want.float(), ref, 'complete')
    short = torch.cat([ids[:6], ids[7:]])
    dropped = R.segment_sum_reference(src, torch.tensor([0, 4, 4, 12]), short, **kw)
    assert bool((src[ids[6]] != 0).any())
    with pytest.raises(AssertionError, match='differ from the exact sum'):
        R.assert_exact(dropped.want.float(), ref, 'one entry short')


def test_float_bound_has_room_for_a_sequential_float32_sum():
    """Rows of 1 ... 4,230 addends, every option on, evaluated operation by operation in float32 in list order: within the bound, and (printed) by how much."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for n in (1, 3, 17, 200, 4230):
        dim, n_src = 8, 50
        src = R.features(rng, n_src, dim, False)
        ids = torch.from_numpy(rng.integers(0, n_src, n))
        ptr = torch.tensor([0, n])
        ss, es, osc, sw = R.scales(rng, n_src, False), R.weights(rng, n, False), R.scales(rng, 1, False), R.weights(rng, 1, False)
        acc_in = R.integers(rng, (1, dim))
        for mode in (1, 2):
            ref = R.segment_sum_reference(src, ptr, ids, src_scale=ss, entry_scale=es, out_scale=osc, mode=mode, self_weight=sw, acc_in=acc_in)
            w = (ss[ids] * es).numpy().astype(np.float32)                                # one rounding: the product of the two weights
            terms = (w[:, None] * src[ids].numpy()).astype(np.float32)
            own = (np.float32(sw[0] * ss[0]) * src[0].numpy()).astype(np.float32)
            s = R.sequential_float32_sum(np.concatenate([terms, own[None]]))
            s = (s * osc.numpy()[0] if mode == 1 else s / osc.numpy()[0]).astype(np.float32)
            got = torch.from_numpy((s + acc_in.numpy()[0]).astype(np.float32))[None]
            assert float(ref.n) == n + 2
            worst = max(worst, R.assert_within_float_bound(got, ref, f'sequential float32, n = {n}, mode {mode}'))
    assert 0 < worst <= 0.5


def test_float_bound_catches_sixteen_bit_partials():
    """What the bound is for: the same sum with its terms kept in fp16 misses it."""
    rng = np.random.default_rng(6)
    src = R.features(rng, 40, 8, False)
    ids, ptr = torch.from_numpy(rng.integers(0, 40, 64)), torch.tensor([0, 64])
    ref = R.segment_sum_reference(src, ptr, ids)
    half = src[ids].half().float().double().sum(0)[None].float()
    with pytest.raises(AssertionError, match='is off by'):
        R.assert_within_float_bound(half, ref, 'fp16 terms')


def test_mean_verdict():
    total, lens = torch.tensor([[7.0, -3.0], [0.0, 0.0], [10.0, 1.0]], dtype=torch.float64), torch.tensor([3.0, 0.0, 64.0])
    good = torch.tensor([[7 / 3, -1.0], [0.0, 0.0], [10 / 64, 1 / 64]], dtype=torch.float32)
    R.assert_mean_of_exact_sum(good, total, lens, 'means')
    bad = good.clone()
    bad[0, 0] = torch.nextafter(torch.nextafter(good[0, 0], torch.tensor(9.0)), torch.tensor(9.0))
    with pytest.raises(AssertionError, match='more than one float away'):
        R.assert_mean_of_exact_sum(bad, total, lens, 'two floats off')


def test_bag_backward_reference_matches_autograd():
    rng = np.random.default_rng(7)
    lens = np.array([0, 1, 2, 3, 64, 4, 0])
    ptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    words = torch.from_numpy(rng.integers(1, 20, int(ptr[-1])))
    table = R.features(rng, 20, 5, False).double().requires_grad_(True)
    dout = R.features(rng, len(lens), 5, False)
    out = torch.nn.functional.embedding_bag(words, table, torch.from_numpy(ptr[:-1]), mode='mean')
    out.backward(dout.double())
    ref = R.bag_mean_backward_reference(dout, torch.from_numpy(ptr), words, 20)
    assert bool(((ref.want - table.grad).abs() <= 2.0 ** -23 * ref.mag).all())           # per element; the reference uses the layout's float32 1 / len: 2^-24 per term
    assert bool((ref.want[0] == 0).all()) and float(ref.n[0]) == 0
