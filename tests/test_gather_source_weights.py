"""The K7 launches that read their per-source factor beside the id (``IHG_SRC_SCALE_IN_ENTRIES``: ``entry_scale[p] = src_scale[ids[p]] (* weight[p])``, the
layout's ``two_hop_source_weights``) against the launches that gather ``src_scale`` by id: the same products added in the same order, so the results are EQUAL bit
for bit (``torch.equal``), and both stay within the per-element bound of ``tests/test_aggregate_kernels.py`` of the float64 sums (``aggregate_reference``).

Kernel level: a hand-made list with rows of 0, 1, G - 1, G, G + 1, 2 G and 2 G + 1 ids (G = d / 4 lanes own a row and take G ids per chunk) and two split rows of
four segments whose last holds three ids, at d = 64, 128 and 256.  Operator level: a graph of 300 nodes and 3,000 hyperedges with a hub query, through
``ops.node_two_hop`` and its backward with the weights on and off, over the plain and the merged list.

This covers the per-entry source weights only.  A unit table in place of the ``row_order`` / ``rowptr`` legs (and with it a second pair-sums entry point to
compare) does not exist: the pair sums take no source scale and are not touched.
"""
import numpy as np
import pytest
import torch

import aggregate_reference as R
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

DIMS = (64, 128, 256)


def _to(t):
    return None if t is None else t.to(dev())


def _kernel_case(dim, options, seed):
    """``(csr, src, kw, ref)``: the list, float inputs for ``options`` (``aggregate_reference.k7_case``) and the float64 reference.  The second hub is the row whose
    ids are all unlisted under a source mask."""
    from ihgnn_amd.layout import Csr
    g = dim // 4
    rng = np.random.default_rng([7, dim, seed])
    hub = 6 * g + 3                                                      # threshold 4 G, segments of 2 G: 2 G + 2 G + 2 G + 3
    lengths = [0, 1, g - 1, g, g + 1, 2 * g, 2 * g + 1]
    lengths = [hub, 0] + [int(x) for x in rng.permutation(lengths + lengths)] + [hub, 1]
    dead = len(lengths) - 2
    n_src = len(lengths) + 16 * hub                                      # (the ids of one hub are a sixteenth of the source rows: unlisting them leaves the rest alone)
    ptr, ids = R.csr_from_lengths(lengths, n_src, rng)
    csr = Csr(ptr, ids, dev(), heavy_threshold=4 * g, heavy_chunk=2 * g)
    assert csr.n_heavy == 2 and csr.n_segments == 8
    assert (csr.seg_end - csr.seg_begin).tolist() == [2 * g, 2 * g, 2 * g, 3] * 2
    src, kw = R.k7_case(ptr, ids, n_src, dim, options, False, rng, listed=0.4, dead_row=dead)
    if 'src_mask' in options:
        mask = kw['src_mask']                                            # the first hub has listed ids, the second none
        assert int(mask[torch.from_numpy(ids[ptr[dead]:ptr[dead + 1]]).long()].sum()) == 0 and int(mask[torch.from_numpy(ids[:hub]).long()].sum()) > 0
    ref = R.segment_sum_reference(src, torch.from_numpy(ptr), torch.from_numpy(ids), **kw)
    return csr, src, kw, ref


def _launch(csr, src, kw, folded):
    """One launch: ``src_scale`` gathered by id, or (``folded``) read from the entries."""
    from ihgnn_amd import ops
    src_scale, entry = _to(kw['src_scale']), _to(kw.get('entry_scale'))
    if folded:
        w = src_scale[csr.ids.long()]
        entry = w if entry is None else w * entry                        # float32, src_scale[id] first: the kernel's own product
    out = _to(kw['acc_in'].clone()) if 'acc_in' in kw else None
    got = ops.node_segment_sum_raw(_to(src), csr, src_scale, _to(kw.get('out_scale')), kw.get('mode', 0), out=out, entry_scale=entry,
                                   self_weight=_to(kw.get('self_weight')), src_mask=_to(kw.get('src_mask')), accumulate=out is not None, src_scale_in_entries=folded)
    torch.cuda.synchronize()
    return got.cpu()


CASES = {
    'two_hop_with_source_scale': ('src_scale', 'self_weight'),
    'merged_list_with_source_scale': ('src_scale', 'entry_scale', 'self_weight', 'mode1'),
    'masked_pull': ('src_scale', 'self_weight', 'src_mask'),
    'masked_pull_merged': ('src_scale', 'entry_scale', 'self_weight', 'src_mask'),
    'accumulate': ('src_scale', 'entry_scale', 'self_weight', 'mode1', 'accumulate'),
    'no_self_term': ('src_scale', 'mode2'),
}


@pytest.mark.parametrize('case', sorted(CASES))
@pytest.mark.parametrize('dim', DIMS)
def test_scale_in_entries_equals_scale_by_id(dim, case):
    csr, src, kw, ref = _kernel_case(dim, CASES[case], sorted(CASES).index(case))
    what = f'K7 scale in entries, d {dim}, {case}'
    by_id = _launch(csr, src, kw, False)
    in_entries = _launch(csr, src, kw, True)
    assert torch.equal(in_entries.view(torch.int32), by_id.view(torch.int32)), \
        f'{what}: {int((in_entries != by_id).sum())} elements differ from the launch that gathers the scale by id'
    R.assert_within_float_bound(in_entries, ref, what)
    R.assert_within_float_bound(by_id, ref, what + ' (by id)')


@pytest.mark.parametrize('dim', DIMS)
def test_scale_in_entries_exact(dim):
    """The same list on exact inputs (small integers, power-of-two scales): equal to the float64 sum, no tolerance - a dropped or mis-weighted entry cannot hide."""
    from ihgnn_amd.layout import Csr
    g = dim // 4
    rng = np.random.default_rng([8, dim])
    lengths = [6 * g + 3, 0, 1, g - 1, g, g + 1, 2 * g, 2 * g + 1]
    n_src = len(lengths) + 9
    ptr, ids = R.csr_from_lengths(lengths, n_src, rng)
    csr = Csr(ptr, ids, dev(), heavy_threshold=4 * g, heavy_chunk=2 * g)
    for options in (('src_scale', 'self_weight'), ('src_scale', 'entry_scale', 'self_weight', 'mode1', 'accumulate'), ('src_scale', 'entry_scale', 'src_mask')):
        src, kw = R.k7_case(ptr, ids, n_src, dim, options, True, rng)
        ref = R.segment_sum_reference(src, torch.from_numpy(ptr), torch.from_numpy(ids), **kw)
        R.assert_exact_condition(ref, f'd {dim} {options}')
        R.assert_exact(_launch(csr, src, kw, True), ref, f'K7 scale in entries, exact, d {dim}, {options}')


# ---------------------------------------------------------------------------------------------
# operator level: the layout's weights through ops.node_two_hop and its backward
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hub_graph():
    from ihgnn_amd.layout import IncidenceLayout
    rng = np.random.default_rng(11)
    users, queries, items, edges = 120, 30, 150, 3000
    triples = np.stack([rng.integers(0, users - 1, edges), rng.integers(0, queries, edges), rng.integers(0, items, edges)], axis=1)      # (the last user is isolated)
    triples[:1100, 1] = 0                                                # the hub: 2,200 ids in the plain list, 18 segments
    lay = IncidenceLayout(triples, users, queries, items, dev(), edge_multiplicity='0', compact_nodes='0')
    assert lay.hop2_csr.n_heavy >= 1 and lay.hop2_csr.n_segments >= 3
    return lay


def _two_hop_round_trip(lay, x, cot, in_scale, out_scale, cotangent_rows):
    from ihgnn_amd import ops
    xr = x.clone().requires_grad_(True)
    y = ops.node_two_hop(xr, lay, in_scale, out_scale, cotangent_rows=cotangent_rows)
    y.backward(cot)
    first = ops._two_hop_first_order_gradient(cot, lay, out_scale)
    torch.cuda.synchronize()
    return y.detach().cpu(), xr.grad.cpu(), first.cpu()


@pytest.mark.parametrize('merged', [False, True])
@pytest.mark.parametrize('dim', DIMS)
def test_two_hop_with_layout_weights_equals_without(hub_graph, monkeypatch, dim, merged):
    """HGCN's scalings (a source scale in the forward AND the backward), dense and with a masked pull whose listed rows hold the hub in one run and not in the other
    (the masked pull itself keeps the per-id gather either way; its forward and the first-order gradient beside it do not)."""
    from ihgnn_amd import ops
    lay = hub_graph
    monkeypatch.setattr(ops, 'TWO_HOP_MERGED', merged)
    gen = torch.Generator(device=dev()).manual_seed(dim + merged)
    n = lay.node_count
    x = torch.randn(n, dim, generator=gen, device=dev())
    hub = lay.user_count                                                 # query 0
    in_scale, out_scale = lay.inv_sqrt_deg, lay.inv_deg
    for listed in (None, [hub, 3, 17, n - 1], [5, 3, 17, n - 1]):
        cot = torch.randn(n, dim, generator=gen, device=dev())
        rows = None
        if listed is not None:
            rows = torch.tensor(listed, dtype=torch.int64, device=dev())
            keep = torch.zeros(n, 1, device=dev())
            keep[rows] = 1
            cot = cot * keep
        monkeypatch.setattr(ops, 'SOURCE_WEIGHTS', False)
        want = _two_hop_round_trip(lay, x, cot, in_scale, out_scale, rows)
        monkeypatch.setattr(ops, 'SOURCE_WEIGHTS', True)
        got = _two_hop_round_trip(lay, x, cot, in_scale, out_scale, rows)
        assert lay.has_two_hop_source_weights(in_scale, merged) and lay.has_two_hop_source_weights(out_scale, merged)
        for name, a, b in zip(('output', 'input gradient', 'first-order gradient'), got, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'd {dim} merged {merged} listed {listed}: {name} differs from the launch that gathers the scale by id'
    # the first-order gradient of the last round against the float64 sum over the plain list (the merged list is the same sum with equal terms taken together)
    csr = lay.hop2_csr
    ref = R.segment_sum_reference(cot.cpu(), csr.ptr.cpu(), csr.ids.cpu(), src_scale=out_scale.cpu(), self_weight=lay.self_weight.cpu())
    R.assert_within_float_bound(got[2], ref, f'first-order gradient through the layout weights, d {dim} merged {merged}')
