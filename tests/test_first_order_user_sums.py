"""The users' rows of the layer-0 first-order gradient from the member-gradient kernel (``ops.FIRST_ORDER_USER_SUMS`` /
``ihg_interact_bwd_gathered_first_order``, d = 128): hyperedges are numbered by user, so ``dp[u] = sum over u's hyperedges of dout[e]`` is a run sum of the
cotangents ``dout[e] = sum_m out_scale[m] dy[m]`` that kernel forms anyway.  ``ops._interact_to_nodes_backward`` is called with the switch on and off on
hand-built layouts that walk every part of the run-sum code (at d = 128 the kernel cuts the tiles of 32 hyperedges into 128 contiguous ranges, one per pair of
workgroups):

  * ``e1``: one hyperedge.
  * ``two_ranges`` (E = 64: two ranges of one tile): runs 0-19 / 20-40 / 41-63 - the middle one crosses from the first range into the second.
  * ``ladder`` (E = 1,451, one tile per range, E no multiple of 32): run lengths 1, 7, 8, 9 (the 8-row window), 31, 32, 33 (the tile), 100 (four ranges), a run of 32
    that ends exactly at a tile's end, a run of 200 (seven ranges), users without hyperedges between users that have some.
  * ``ranges_of_tiles`` (E = 20,011: five tiles per range): the same lengths many times over, runs of 100 inside a range (the carry from tile to tile), a run of 700
    over five ranges, runs that end at a range's end.

Verdicts: (1) with small-integer ``dy``, ``out_scale`` and ``h`` every fp32 sum is exact: ``dp`` is EQUAL with the switch on and off on every row, and so are
``dh`` and ``dw``; (2) with normal inputs the users' rows stay within ``(3 deg(u) + 2) 2^-24 sum |terms|`` per element of the float64 sum over the triples (a
sequential fp32 sum of ``3 deg(u)`` products: ``tests/test_aggregate_kernels.py``'s bound), query and item rows are EQUAL in both modes, ``dh`` and ``dw`` too;
(3) the row of a user without hyperedges is exactly zero.  (Measured on an MI355X: the largest error of a user row is 0.02 - 0.42 of its bound in either
mode.  d = 64 has no such kernel instance and keeps the full two-hop launch.)
"""
import numpy as np
import pytest
import torch

from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

DIM = 128
U24 = 2.0 ** -24


def _runs(name):
    """``(run lengths, users to leave without hyperedges in front of each run)``"""
    rng = np.random.default_rng(len(name))
    if name == 'e1':
        return [1], [2]
    if name == 'two_ranges':
        return [20, 21, 23], [0, 1, 2]
    ladder = [31, 1, 32, 7, 8, 9, 8, 33, 100, 3, 32, 32, 5, 27, 200, 64, 1, 1, 30]      # 31 + 1 = a tile; the 32 behind it ends at a tile's end, as do 32, 32 further on
    if name == 'ladder':
        lengths = ladder + [int(x) for x in rng.integers(1, 40, 30)]
        lengths.append(1451 - sum(lengths))
        assert lengths[-1] > 0
        return lengths, [int(x) for x in rng.integers(0, 3, len(lengths))]
    assert name == 'ranges_of_tiles'
    lengths = [160, 100, 60, 700, 100, 20, 100] + ladder                                  # 160 = a range; 100 + 60 ends at a range's end; 700: five ranges
    while sum(lengths) < 20011 - 400:
        lengths += [int(x) for x in rng.permutation(ladder + [int(y) for y in rng.integers(1, 70, 12)])]
    lengths.append(20011 - sum(lengths))
    assert lengths[-1] > 0
    return lengths, [int(x) for x in rng.integers(0, 2, len(lengths))]


_cases = {}


def _case(name):
    """The layout, the triples in the layout's hyperedge order, degrees of the users - built once per name and left unchanged."""
    if name not in _cases:
        from ihgnn_amd.layout import IncidenceLayout
        lengths, gaps = _runs(name)
        rng = np.random.default_rng([3, len(lengths)])
        users, u = [], 0
        for n, gap in zip(lengths, gaps):
            u += gap
            users += [u] * n
            u += 1
        n_users = u + 2                                                  # (two more users without hyperedges at the end)
        e = len(users)
        # few queries and items: the first-order launch walks the merged (weighted) two-hop list; many: the plain one
        n_q, n_i = (257, 4001) if name == 'ranges_of_tiles' else (17, 211)
        triples = np.stack([np.asarray(users), rng.integers(0, n_q, e), rng.integers(0, n_i, e)], axis=1).astype(np.int64)
        lay = IncidenceLayout(triples, n_users, n_q, n_i, dev(), edge_order='user', edge_multiplicity='0', compact_nodes='0')
        assert lay.user_sorted and lay.edge_weight is None and lay.edge_count == e
        assert lay.two_hop_merged_default == (name == 'ladder')
        deg = np.bincount(users, minlength=n_users)
        assert np.array_equal(lay.self_weight.cpu().numpy()[:n_users], deg.astype(np.float32))      # the identity the run sums rest on: self_weight[u] = deg(u)
        assert np.array_equal(np.sort(lay.users_without_hyperedges().cpu().numpy()), np.nonzero(deg == 0)[0])
        _cases[name] = (lay, lay.i3_host.astype(np.int64), deg)
    return _cases[name]


def _inputs(lay, order, integers, seed):
    gen = torch.Generator().manual_seed(seed)
    n, k = lay.node_count, 6 if order == 2 else 7
    if integers:
        h = torch.randint(-2, 3, (n, DIM), generator=gen).float()
        dy = torch.randint(-4, 5, (n, DIM), generator=gen).float()
        scale = torch.randint(1, 4, (n,), generator=gen).float()
    else:
        h = torch.randn(n, DIM, generator=gen)
        dy = torch.randn(n, DIM, generator=gen)
        scale = torch.rand(n, generator=gen) + 0.25
    w = torch.randn(DIM, k * DIM, generator=gen) / np.sqrt(k * DIM)
    return h, w, dy, scale


def _backward(lay, order, tensors, user_sums, monkeypatch):
    """``(dh, dp, dw, roles launched)`` of ``ops._interact_to_nodes_backward`` in the node-level-weight branch (pair sums given)."""
    from ihgnn_amd import ops, profiler
    monkeypatch.setattr(ops, 'FIRST_ORDER_USER_SUMS', user_sums)
    h, w, dy, scale = (t.to(dev()) for t in tensors)
    sums = ops.node_pair_sums_raw(h, lay)
    dw = torch.zeros_like(w)
    profiler.start()
    dh, dp = ops._interact_to_nodes_backward(h, w, dy, lay, order, scale, dw, sums)
    launched = profiler.summary()
    profiler.stop()
    torch.cuda.synchronize()
    return dh, dp, dw, launched


def _modes(name, order, integers, monkeypatch):
    from ihgnn_amd import _lib
    lay, i3, deg = _case(name)
    assert _lib.load().ihg_interact_bwd_gathered_first_order_supported(DIM, order, DIM, DIM)
    tensors = _inputs(lay, order, integers, 11 * order + len(name))
    on = _backward(lay, order, tensors, True, monkeypatch)
    off = _backward(lay, order, tensors, False, monkeypatch)
    # both modes run the member kernel and the first-order launch; with the switch on that launch walks the query and item rows only
    for launched in (on[3], off[3]):
        assert 'interact_bwd' in launched and 'k7.two_hop_first_order_gradient' in launched and 'edge_gather_sum' not in launched, sorted(launched)
    assert on[3]['k7.two_hop_first_order_gradient']['launches'] == off[3]['k7.two_hop_first_order_gradient']['launches'] == 1
    return lay, i3, deg, tensors, on, off


NAMES = ('e1', 'two_ranges', 'ladder', 'ranges_of_tiles')


@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('name', NAMES)
def test_exact_sums_are_equal_with_and_without_the_user_sums(name, order, monkeypatch):
    lay, i3, deg, tensors, on, off = _modes(name, order, True, monkeypatch)
    h, w, dy, scale = tensors
    ref = torch.zeros(lay.node_count, DIM, dtype=torch.float64)
    dout = (scale[:, None].double() * dy.double())[torch.from_numpy(i3)].sum(1)          # [E, d]: exact in fp32 too
    for m in range(3):
        ref.index_add_(0, torch.from_numpy(i3[:, m]), dout)
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(off[1].cpu().double(), ref)                                       # (the inputs do make every sum exact)
    assert torch.equal(on[1], off[1])
    assert torch.equal(on[0], off[0]) and torch.equal(on[2], off[2])
    assert bool((on[1][:lay.user_count][torch.from_numpy(deg == 0).to(dev())] == 0).all())


@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('name', NAMES)
def test_user_rows_stay_within_the_sequential_sum_bound(name, order, monkeypatch):
    lay, i3, deg, tensors, on, off = _modes(name, order, False, monkeypatch)
    h, w, dy, scale = tensors
    users = lay.user_count
    terms = (scale[:, None].double() * dy.double())[torch.from_numpy(i3)]                # [E, 3, d]
    ref = torch.zeros(users, DIM, dtype=torch.float64).index_add_(0, torch.from_numpy(i3[:, 0]), terms.sum(1))
    mag = torch.zeros(users, DIM, dtype=torch.float64).index_add_(0, torch.from_numpy(i3[:, 0]), terms.abs().sum(1))
    bound = (3.0 * torch.from_numpy(deg).double()[:, None] + 2.0) * U24 * mag
    for label, got in (('on', on[1]), ('off', off[1])):
        err = (got[:users].cpu().double() - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f'{name} order {order} switch {label}: largest error / bound = {worst:.3f}, largest error = {float(err.max()):.3e}')
        assert bool((err <= bound).all()), (label, worst)
    assert torch.equal(on[1][users:], off[1][users:])                                    # query and item rows: the same launch code over a row list
    assert torch.equal(on[0], off[0]) and torch.equal(on[2], off[2])
    zero = torch.from_numpy(deg == 0).to(dev())
    assert bool(zero.any()) and bool((on[1][:users][zero] == 0).all())
