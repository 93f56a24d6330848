"""``tests/attention_reference.py`` on the host: the ladder builders, the float64 references against the two layers' own restatements, the float32 emulation of the
softmax kernels' scheme inside every bound on every case ``tests/test_attention_kernels.py`` runs - a failing GPU case is then a wrong kernel, not a tight bar -
and the mutations of the emulation that the verdicts must catch.  No GPU needed."""
import numpy as np
import pytest
import torch

import attention_reference as R

F = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def emulated_forward(g, case, act, design, what, mutation=None):
    """z: the float64 scores rounded once (the kernel's own z stands in on the GPU); alpha: the emulation's."""
    z = R.z64(g, case, act).want.float()
    alpha = _t(R.emulate_forward(g, z.numpy(), mutation))
    return z, alpha, R.check_forward(g, case, act, design, z, alpha, what)


def emulated_backward(g, case, act, design, z, alpha, what, mutation=None):
    ga = R.dalpha64(g, case)[0].float()
    ds, S = R.emulate_backward(g, z.numpy(), alpha.numpy(), ga.numpy(), act, mutation)
    src = None
    if g.kind == 'gat' and case.head == 'concatenation':
        src = torch.zeros(g.n_rows).index_add_(0, _t(R.row_of(g)), _t(ds)[_t(g.table)])
    return R.check_backward(g, case, act, design, z, alpha, _t(ds), _t(S), src, what)


# ---------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,chunk,repeated', R.LADDER_GRAPHS)
def test_ladders_reach_the_wanted_segment_counts(kind, chunk, repeated):
    g = R.ladder(kind, chunk, repeated)
    counts = R.assert_ladder(g)
    print(f'{kind} chunk {chunk} repeated {repeated}: hub segment counts {sorted(counts)}; {len(g.ids)} entries, {g.csr.n_heavy} split rows')
    if chunk == 2:
        assert {256, 257, 511, 512, 513, 1025} <= set(counts) and max(g.hub_lens) == 2050
        assert 6 in counts and 11 in g.hub_lens                            # the odd row: its last segment holds one entry
        seg_len = (g.csr.seg_end - g.csr.seg_begin).numpy()
        assert (seg_len == 1).any() and seg_len.max() == 2
    else:
        assert set(counts) >= {255, 256, 257} and (g.csr.seg_end - g.csr.seg_begin).numpy().max() == 34
    assert {0, 1, 2} <= set(g.hub_lens.tolist())
    n = len(g.ids)
    if kind == 'gat':
        m = g.table
        np.testing.assert_array_equal(m[m], np.arange(n))                 # mirror: an involution that swaps row and column
        np.testing.assert_array_equal(R.row_of(g)[m], g.ids)
        heavy = np.zeros(g.n_rows, bool)
        heavy[g.csr.heavy_rows.numpy()] = True
        rows = R.row_of(g)
        assert (heavy[rows] & heavy[rows[m]]).any() or chunk != 2          # mirror crosses split rows
    else:
        np.testing.assert_array_equal(np.sort(g.table), np.arange(n))      # pos: a permutation of [0, 3 E)
        np.testing.assert_array_equal(g.table // 3, g.ids)
        assert (g.mult is not None) == repeated
    for where in ('first', 'last', 'deep'):
        R.winners(g, where)


# ---------------------------------------------------------------------------------------------
# the float64 references against the layers' restatements
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('head', R.HEADS)
@pytest.mark.parametrize('act', R.ACTS)
def test_references_agree_with_the_gat_restatement(head, act, monkeypatch):
    from test_gat_layer import attention64
    monkeypatch.setattr(R, 'SLOPE', 0.01)                                  # (the restatement's float64 slope; the kernels and the references here use float32(0.01))
    g = R.graph_from_lengths('gat', [5, 1, 0, 9, 3, 17], 4, seed=1)
    case = R.float_case(g, head, 8, np.random.default_rng(3))
    h, w, c = (t.double().requires_grad_(True) for t in (case.x, case.w, case.c))
    y, alpha = attention64(h, w, c, g.ptr, g.ids, head, act)
    y.backward(case.dout.double())
    z = R.z64(g, case, act).want
    assert float((z - R.act64(attention64.pre.detach(), act)).abs().max()) <= 1e-12
    ar = R.alpha64(g, z)
    assert float((ar.want - alpha.detach()).abs().max()) <= 1e-12
    ref = R.ds64(g, z, ar.want, R.dalpha64(g, case)[0], act)
    assert float((ref.ds - attention64.pre.grad).abs().max()) <= 1e-12
    sym = R.symmetrize64(g, ref.ds)
    np.testing.assert_allclose(sym.numpy(), (ref.ds + ref.ds[_t(g.table)]).numpy(), rtol=0, atol=0)


@pytest.mark.parametrize('head', R.HEADS)
@pytest.mark.parametrize('act', R.ACTS)
@pytest.mark.parametrize('repeated', [False, True])
def test_references_agree_with_the_phase2_restatement(head, act, repeated, monkeypatch):
    from ihgnn_amd.layout import IncidenceLayout
    monkeypatch.setattr(R, 'SLOPE', 0.01)
    from test_phase2_layer import attention64
    rng = np.random.default_rng(4)
    triples = np.stack([rng.integers(0, 6, 40), rng.integers(0, 3, 40), rng.integers(0, 5, 40)], 1)
    if repeated:
        triples = np.concatenate([triples, triples[::2], triples[::5]])
    lay = IncidenceLayout(triples, 6, 3, 5, R.CPU, heavy_threshold=4, edge_multiplicity='1' if repeated else '0', compact_nodes='0')
    g = R.graph_of('phase2', lay)
    assert (g.mult is not None) == repeated
    case = R.float_case(g, head, 8, rng)
    h, ef, w, c = (t.double().requires_grad_(True) for t in (case.h, case.x, case.w, case.c))
    y, alpha = attention64(h, ef, w, c, lay, head, act)
    y.backward(case.dout.double())
    pre = attention64.kept[0]
    z = R.z64(g, case, act).want
    assert float((z - R.act64(pre.detach(), act)).abs().max()) <= 1e-12
    ar = R.alpha64(g, z)
    assert float((ar.want - alpha.detach()).abs().max()) <= 1e-12
    ref = R.ds64(g, z, ar.want, R.dalpha64(g, case)[0], act)
    assert float((ref.ds - pre.grad).abs().max()) <= 1e-12
    # the hyperedge gradient: d ef = sum_k alpha_edge dout[member k] + the score term, against autograd's
    pos = _t(g.table)
    alpha_edge, ds_edge = torch.zeros(len(g.ids), dtype=torch.float64), torch.zeros(len(g.ids), dtype=torch.float64)
    alpha_edge[pos], ds_edge[pos] = ar.want, ref.ds
    want, _ = R.edges_bwd64(case.dout, case.h, _t(lay.i3_host), alpha_edge, ds_edge, case.w, head)
    assert float((want - ef.grad).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------
# the emulation inside every bound, on the cases of the GPU file
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,chunk,repeated', R.LADDER_GRAPHS)
@pytest.mark.parametrize('head', R.HEADS)
@pytest.mark.parametrize('act', R.ACTS)
def test_emulation_is_inside_every_bound_on_the_ladders(kind, chunk, repeated, head, act):
    g = R.ladder(kind, chunk, repeated)
    for design in R.ladder_designs(head, act):
        what = f'emulation {kind} chunk {chunk} repeated {repeated} {head} {act} {design}'
        case = R.design_case(g, design, head)
        z, alpha, _ = emulated_forward(g, case, act, design, what)
        if design in R.ladder_designs(head, act, backward=True):
            emulated_backward(g, case, act, design, z, alpha, what)


@pytest.mark.parametrize('kind', ['gat', 'phase2'])
@pytest.mark.parametrize('which', ['light', 'no_edges', 'only_split', 'split_among_isolated'])
def test_emulation_is_inside_every_bound_on_the_small_graphs(kind, which):
    g = R.small_graph(kind, which)
    for head in R.HEADS:
        case = R.float_case(g, head, 8, np.random.default_rng(5))
        z, alpha, _ = emulated_forward(g, case, 'leaky_relu', 'float', f'emulation {kind} {which} {head}')
        emulated_backward(g, case, 'leaky_relu', 'float', z, alpha, f'emulation {kind} {which} {head}')


# ---------------------------------------------------------------------------------------------
# mutations of the emulation: each must FAIL the verdict of the named case
# ---------------------------------------------------------------------------------------------
MUTATION_CASES = {
    # mutation: (graph, design, act) - the forward case whose verdict catches it
    'drop_segment': (('gat', 2, False), 'equal', 'leaky_relu'),           # one of 1,025 equal partials: the row moves by 1e-3, its bound is 1.3e-4
    'first_trip_only': (('phase2', 2, False), 'equal', 'leaky_relu'),     # the rows of more than 256 segments lose their tail
    'max_without_rescale': (('phase2', 2, False), 'ascending', 'relu'),   # every merge ought to rescale
    'mult_not_in_denominator': (('phase2', 2, True), 'equal', 'leaky_relu'),
    'fp16_partial': (('gat', 2, False), 'staircase', 'leaky_relu'),       # 1 + e^-k is not an fp16 value: 2^-11 of a partial
}


@pytest.mark.parametrize('mutation', sorted(MUTATION_CASES))
def test_a_mutated_forward_fails_its_case(mutation):
    graph, design, act = MUTATION_CASES[mutation]
    g = R.ladder(*graph)
    case = R.design_case(g, design)
    emulated_forward(g, case, act, design, f'unmutated {design}')
    with pytest.raises(AssertionError):
        emulated_forward(g, case, act, design, f'mutation {mutation}', mutation)


def test_a_backward_without_the_shift_fails_on_nearly_equal_dalpha():
    """``c`` formed from the raw ``d alpha = 4096 + (-3 ... 3)`` carries eps n |c| of rounding against a spread of 3: the per-entry bound, which scales with the
    spread about the row's first entry, SEPARATES this mutation (measured here: shifted 0.15 of the bound, unshifted 1,700 times the bound), so it is an
    assertion and not only a record."""
    g = R.ladder('gat', 2, False)
    case = R.near_equal_dalpha_case(g)
    z, alpha, _ = emulated_forward(g, case, 'leaky_relu', 'equal', 'nearly equal d alpha')
    emulated_backward(g, case, 'leaky_relu', 'equal', z, alpha, 'nearly equal d alpha, shifted')
    with pytest.raises(AssertionError):
        emulated_backward(g, case, 'leaky_relu', 'equal', z, alpha, 'nearly equal d alpha, no shift', 'no_g0_shift')


def test_exactness_condition_refuses_what_is_not_exact():
    with pytest.raises(AssertionError):
        R.assert_exact_condition(torch.tensor([float(1 << 24)], dtype=torch.float64))
    with pytest.raises(AssertionError):
        R.assert_exact_condition(torch.tensor([0.5], dtype=torch.float64))
    assert R.assert_exact_condition(torch.tensor([3.0, 7.0], dtype=torch.float64)) == 7


@pytest.mark.parametrize('dim,lanes', [(8, 4), (32, 8), (30, 32), (320, 64)])
def test_emulation_is_inside_every_bound_on_the_light_row_cases(dim, lanes):
    """The cases of ``test_light_rows_every_width_and_geometry`` (the geometry does not reach the emulation): integer scores, the zero attention vector, floats."""
    import aggregate_reference as AR
    rng = np.random.default_rng([3, dim])
    lengths = AR.light_lengths(lanes, rng)
    for kind in ('gat', 'phase2'):
        g = R.graph_from_lengths(kind, lengths, 0, seed=dim)
        for head in R.HEADS:
            what = f'emulation light rows {kind} dim {dim} {head}'
            for act in ('leaky_relu', 'relu'):
                case = R.integer_case(g, head, dim, rng)
                z = R.z64(g, case, act).want.float()
                R.check_forward(g, case, act, 'integer', z, _t(R.emulate_forward(g, z.numpy())), what, hold_alpha=False)
            case = R.zero_weight_case(g, head, dim, rng)
            z, alpha, _ = emulated_forward(g, case, 'leaky_relu', 'equal', what)
            emulated_backward(g, case, 'leaky_relu', 'equal', z, alpha, what)
            act = 'tanh' if head == 'product' else 'leaky_relu'
            case = R.float_case(g, head, dim, rng)
            z, alpha, _ = emulated_forward(g, case, act, 'float', what)
            emulated_backward(g, case, act, 'float', z, alpha, what)


@pytest.mark.parametrize('kind', ['gat', 'phase2'])
@pytest.mark.parametrize('n_hubs,per_row,threshold', [(140000, 3, 0), (9000, 4, 2)])
def test_emulation_is_inside_every_bound_on_the_second_trip_graphs(kind, n_hubs, per_row, threshold):
    g = R.short_rows_graph(kind, n_hubs, (lambda r: 1 + r % 3) if per_row == 3 else (lambda r: 4 + 0 * r), threshold, pool=100000 if per_row == 3 else 1000)
    assert g.n_rows + g.csr.n_segments > R.MAX_SCALAR_UNITS or g.csr.n_heavy > R.MAX_FINISH_ROWS
    case = R.float_case(g, 'concatenation', 8, np.random.default_rng(4))
    z, alpha, _ = emulated_forward(g, case, 'leaky_relu', 'float', f'emulation {kind} {n_hubs} rows')
    emulated_backward(g, case, 'leaky_relu', 'float', z, alpha, f'emulation {kind} {n_hubs} rows')


@pytest.mark.parametrize('head', R.HEADS)
@pytest.mark.parametrize('act', R.ACTS)
def test_plain_float32_evaluations_are_inside_the_z_and_hyperedge_gradient_bounds(head, act):
    """The two bounds that do not belong to the softmax scheme, each on a sequential float32 evaluation in numpy: ``z`` from ``randn`` features at d = 100 (the
    activation through numpy's float32 functions) and the hyperedge gradient of ``ihg_phase2_edges_bwd`` at ``8 eps sum |terms|``."""
    g = R.small_graph('phase2', 'light')
    rng = np.random.default_rng(6)
    d = 100
    case = R.float_case(g, head, d, rng)
    x, h, w, c = (t.numpy() for t in (case.x, case.h, case.w, case.c))
    rows = R.row_of(g)
    pre = np.zeros(len(g.ids), F)
    if head == 'concatenation':
        a, b = np.zeros(g.n_src, F), np.zeros(g.n_rows, F)
        for k in range(d):
            a, b = (a + x[:, k] * w[k]).astype(F), (b + h[:, k] * w[d + k]).astype(F)
        pre = (a[g.ids] + (b[rows] + c[0]).astype(F)).astype(F)
    else:
        for k in range(d):
            pre = (pre + ((h[rows, k] * w[k]).astype(F) * x[g.ids, k]).astype(F)).astype(F)
        pre = (pre + c[0]).astype(F)
    z = {'leaky_relu': lambda v: np.where(v > 0, v, F(0.01) * v), 'relu': lambda v: np.maximum(v, F(0)), 'tanh': np.tanh}[act](pre).astype(F)
    zr = R.z64(g, case, act)
    R.assert_within(_t(z), zr.want, zr.bound, f'sequential float32 {head} {act}', 'z')
    if act != 'leaky_relu':
        return
    e = g.n_src
    dout, al, s = rng.standard_normal((g.n_rows, d)).astype(F), rng.random(3 * e).astype(F), rng.standard_normal(3 * e).astype(F)
    i3 = g.layout.i3_host.astype(np.int64).reshape(-1, 3)
    acc = np.zeros((e, d), F)
    for k in range(3):
        acc = (acc + (al.reshape(e, 3)[:, k, None] * dout[i3[:, k]]).astype(F)).astype(F)
    if head == 'concatenation':
        s_sum = ((s.reshape(e, 3)[:, 0] + s.reshape(e, 3)[:, 1]).astype(F) + s.reshape(e, 3)[:, 2]).astype(F)
        acc = (acc + (s_sum[:, None] * w[None, :d]).astype(F)).astype(F)
    else:
        t = np.zeros((e, d), F)
        for k in range(3):
            t = (t + (s.reshape(e, 3)[:, k, None] * h[i3[:, k]]).astype(F)).astype(F)
        acc = (acc + (w[None, :] * t).astype(F)).astype(F)
    want, mag = R.edges_bwd64(_t(dout), case.h, _t(i3), _t(al), _t(s), case.w, head)
    R.assert_within(_t(acc), want, R.EDGES_BWD_ROUNDINGS * R.EPS * mag, f'sequential float32 {head}', 'hyperedge gradient')
