"""GPU: the GRU query encoder ``Gs.Query.transform == 'gru'`` (``ihg_gru_fwd/bwd`` in csrc/recurrent.hip, the four query-row producers of ``ihgnn_amd.ops``,
``EmbeddingLayer.query_transform = nn.GRU``, ``--query_transform gru``, ``RawGnn.search(words=)``) against a float64 restatement
(``tests/query_gru_reference.py``, held to ``torch.nn.GRU`` by ``tests/test_query_gru_host.py``).  The reference project has no such branch, so there is no fixture.

Bars: RTOL = 1e-5 of the tensor's largest magnitude (DESIGN section 5's contract); per row as well for the query rows and the word table's gradient (``row_rel``: over
the rows that can be non-zero - bags with words, words that occur - with the usual 5 % cap on rows under the floor; every other row must be exactly zero); a loss 1e-4.
Basis: torch in fp32 against float64 on the CPU at d = 32 / 128 / 256, Q = 130, bags of 0 .. 6 words and one of 40, is off by 1.6 - 4.8e-7 (rows), <= 3.1e-7 (table
and weight gradients), <= 1.6e-7 (bias gradients) of the largest magnitude: the bar leaves about 20 x over a plain fp32 evaluation.  The GRU has no kink: no cotangent
is masked."""
import functools
import os

import numpy as np
import pytest
import torch

import query_gru_reference as gref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RTOL = 1e-5
ROW_RTOL = 1e-5
LOSS_RTOL = 1e-4
MODEL_CASES = (('ihgnn', 2, 3, 32), ('ihgnn', 2, 2, 64), ('hgcn', 2, 1, 64))
EMB = 'embeddings.'
GRAD_NAMES = ('d_table', 'dw_ih', 'dw_hh', 'db_ih', 'db_hh')


def dev():
    return torch.device('cuda:0')


def as64(a):
    return a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)


def rel(a, b):
    a, b = as64(a), as64(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def row_rel(a, b, rows, floor=1e-3):
    """Largest per-row relative error over ``rows`` (a bool mask: the rows that can be non-zero) of ``b`` (the reference) above ``floor`` of its largest row - the floor
    may leave out at most 5 % of them; every row outside ``rows`` must be exactly zero on both sides."""
    a, b = as64(a), as64(b)
    assert float(np.abs(a[~rows]).max(initial=0.0)) == 0.0 and float(np.abs(b[~rows]).max(initial=0.0)) == 0.0
    a, b = a[rows], b[rows]
    if not len(b):
        return 0.0
    mag = np.abs(b).max(1)
    keep = mag > floor * max(mag.max(), 1e-30)
    assert int((~keep).sum()) <= 0.05 * max(len(keep), 1), int((~keep).sum())
    return float((np.abs(a - b).max(1)[keep] / mag[keep]).max())


class query_settings:
    """``Gs.Query.transform`` set for the block (``'gru'``, or ``None``: the bag mean), put back after it."""

    def __init__(self, transform='gru'):
        self.new = transform

    def __enter__(self):
        from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
        self.old, Gs.Query.transform = Gs.Query.transform, Gsv.mean if self.new is None else self.new

    def __exit__(self, *exc):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        Gs.Query.transform = self.old


def small():
    return np.load(os.path.join(GOLDEN, 'f2_small_workload.npz'))


def dataset_from_npz(w):
    from ihgnn_amd.Dataset import GraphDataset
    U, Q, I, V = (int(x) for x in w['counts'])
    return GraphDataset.from_arrays(U, Q, I, V, w['bag_words'], w['bag_offsets'], w['triples'], device=dev())


def synth_dataset(seed=21, counts=(300, 40, 200, 50, 4000), **kw):
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    w = synth.draw(*counts, seed=seed, distribution='powerlaw', **kw)
    return w, GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev())


def build_model(ds, kind, L, order, d, transform='gru'):
    from ihgnn_amd.Models import HGCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn
    with query_settings(transform):
        return RawGnn(dev(), ds, d, IHGNNLayer if kind == 'ihgnn' else HGCNLayer, L, order, False, HemPredictionLayer, 0.5).to(dev())


# ---------------------------------------------------------------------------------------------
# the kernels against float64
# ---------------------------------------------------------------------------------------------
def case_lengths(shape, q):
    if shape == 'ragged':
        if q == 1:
            return np.array([4], np.int64)                                # (the one bag has words)
        return gref.ragged_lengths(q, 40 if q == 130 else None)          # 0 .. 6 words, every 7th bag empty; one bag of 40 words among the 130
    if shape == 'equal':
        return np.full(q, 3, np.int64)
    return np.zeros(q, np.int64)                                          # 'none': no words at all


@functools.lru_cache(maxsize=None)
def gru_case(d, q, shape='ragged', vocab=50):
    """Operands (fp32 values), the float64 rows and gradients under a random cotangent, and the layout of one kernel case; computed once, shared, never changed."""
    lens = case_lengths(shape, q)
    words, offsets = gref.bags(lens, vocab, seed=1000 * d + q)
    ops32 = [t.float() for t in gref.operands(d, vocab, seed=d + q)]
    ops64 = [t.double().requires_grad_(True) for t in ops32]
    y64 = gref.gru_rows(ops64[0], words, offsets, *ops64[1:])
    cot = (torch.rand(y64.shape, generator=torch.Generator().manual_seed(q), dtype=torch.float64) - 0.5).float()
    (y64 * cot.double()).sum().backward()
    grads = [t.grad if t.grad is not None else torch.zeros_like(t) for t in ops64]
    used = np.zeros(vocab + 1, bool)
    used[words] = True
    return dict(words=words, offsets=offsets, lens=lens, vocab=vocab, ops=ops32, y=y64.detach(), grads=grads, cot=cot, used=used)


def run_case(c, out=None):
    """Forward + backward of ``ops.bag_mean`` with the GRU description on the case's operands: ``(y, [five gradients])``."""
    from ihgnn_amd import ops
    leaves = [t.to(dev()).requires_grad_(True) for t in c['ops']]
    bag = ops.BagLayout(c['words'], c['offsets'], c['vocab'] + 1, dev())
    y = ops.bag_mean(leaves[0], bag, transform=ops.QueryTransform('gru', leaves[1:]))
    y.backward(c['cot'].to(dev()))
    return y.detach(), [t.grad for t in leaves], bag


def check_case(c, y, grads, rows=True):
    errors = {'y': rel(y, c['y'])}
    for name, got, want in zip(GRAD_NAMES, grads, c['grads']):
        assert got is not None and got.shape == want.shape, name
        errors[name] = rel(got, want) if float(want.abs().max()) > 0 else float(got.abs().max())
    if rows:
        errors['y rows'] = row_rel(y, c['y'], c['lens'] > 0)
        errors['d_table rows'] = row_rel(grads[0], c['grads'][0], c['used'])
    print(' '.join(f'{k} {v / RTOL:.3f}' for k, v in errors.items()), '(error / bar)')
    for k, v in errors.items():
        assert v <= (ROW_RTOL if k.endswith('rows') else RTOL), (k, v)


@pytest.mark.parametrize('q', [1, 17, 130])
@pytest.mark.parametrize('d', [32, 64, 128, 256, 96, 30])
def test_gru_kernels_match_float64(d, q):
    """Rows and all five gradients under a random cotangent.  17 and 130 bags leave a part-filled tile of bags, 130 spans several; 96 and 30 run zero-padded at 128 / 32.
    With few bags most words never occur: their rows of the table's gradient must be exactly zero (``row_rel``)."""
    c = gru_case(d, q)
    y, grads, bag = run_case(c)
    assert (bag.length_order is None) == (q == 1)
    check_case(c, y, grads)


def test_gru_kernels_with_bags_of_equal_length():
    c = gru_case(64, 50, 'equal')
    y, grads, bag = run_case(c)
    assert bag.length_order is None                                       # already in decreasing order: the kernels take the bags as they are numbered
    check_case(c, y, grads)


def test_gru_kernels_with_a_one_word_vocabulary():
    """Every occurrence is the same table row: its gradient is one fixed-order sum over all of them (1 of the 2 rows is the padding row: ``rel`` only)."""
    c = gru_case(64, 130, 'ragged', vocab=1)
    y, grads, _ = run_case(c)
    check_case(c, y, grads, rows=False)
    assert float(grads[0][0].abs().max()) == 0.0


def test_gru_kernels_without_any_word():
    """No query has a word: zero rows and five zero gradients, all written."""
    c = gru_case(32, 9, 'none')
    y, grads, bag = run_case(c)
    assert bag.n_words == 0 and float(y.abs().max()) == 0.0 and tuple(y.shape) == (9, 32)
    for g, want in zip(grads, c['grads']):
        assert g.shape == want.shape and float(g.abs().max()) == 0.0


@pytest.mark.parametrize('d', [64, 30])
def test_gru_writes_a_column_slice(d):
    """``out`` as a column slice of a wider, NaN-filled matrix (the feature matrix of ``RawGnn.propagate``): the same bits as the dense call, nothing outside the slice."""
    from ihgnn_amd import ops
    c = gru_case(d, 130)
    leaves = [t.to(dev()) for t in c['ops']]
    bag = ops.BagLayout(c['words'], c['offsets'], c['vocab'] + 1, dev())
    qt = ops.QueryTransform('gru', leaves[1:])
    y = ops.bag_mean(leaves[0], bag, transform=qt)
    wide = torch.full((130, 3 * d + 5), float('nan'), device=dev())
    out = wide[:, d + 5:2 * d + 5]
    assert ops._query_rows_forward(leaves[0], bag, qt, out=out, keep=False) == ()
    assert torch.equal(out, y)
    assert bool(torch.isnan(wide[:, :d + 5]).all()) and bool(torch.isnan(wide[:, 2 * d + 5:]).all())


def test_gru_is_bitwise_reproducible():
    c = gru_case(128, 130)
    runs = [run_case(c)[:2] for _ in range(3)]
    for y, grads in runs[1:]:
        assert torch.equal(y, runs[0][0]) and all(torch.equal(a, b) for a, b in zip(grads, runs[0][1]))


# ---------------------------------------------------------------------------------------------
# the four producers, the models
# ---------------------------------------------------------------------------------------------
def step_gradients(m, batch):
    m.zero_grad(set_to_none=True)
    loss = m.bce_loss(*batch)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def float64_gradients(m, w, triples, kind, L, order, batch):
    u, q, i, y = (v.cpu().numpy() for v in batch)
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    return gref.model_step(sd, triples, (w.user_count, w.query_count, w.item_count), w.bag_words + 1, w.bag_offsets, kind, L, order, u, q, i, y.astype(np.float64))


def test_bag_mean_and_embed_all_nodes_agree_bit_for_bit():
    from ihgnn_amd.Models.EmbeddingLayers import EmbeddingLayer
    ds = dataset_from_npz(small())
    torch.manual_seed(4)
    with query_settings():
        emb = EmbeddingLayer(ds, 32).to(dev())
    U, Q = ds.user_count, ds.query_count
    u, q, it = emb(None, None, None)
    cot = torch.rand(U + Q + ds.item_count, 32, generator=torch.Generator().manual_seed(1)).to(dev())
    (torch.cat([u, q, it]) * cot).sum().backward()
    split = {n: p.grad.clone() for n, p in emb.named_parameters()}
    emb.zero_grad(set_to_none=True)
    x = emb.all_nodes()
    assert torch.equal(x, torch.cat([u, q, it]).detach())
    x.backward(cot)
    for n, p in emb.named_parameters():
        assert torch.equal(p.grad, split[n]), n
    assert all(float(split['query_transform.' + n].abs().max()) > 0 for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0'))


@pytest.mark.parametrize('kind,L,order,d', [('ihgnn', 2, 3, 128), ('hgcn', 2, 1, 64), ('ihgnn', 1, 3, 32)])
def test_step_reads_the_tables_in_place_with_the_gru(kind, L, order, d):
    """``IHG_NODE_TABLES`` on (the first layer and the batch tail read the tables and the GRU's query rows in place; its backward runs on the complete ``d_query``) and off
    (X0 assembled): loss and every gradient agree bit for bit and hold the float64 model; all four GRU parameters receive a gradient."""
    from ihgnn_amd import ops, profiler
    w, ds = synth_dataset(seed=33, counts=(150, 30, 110, 40, 2500))
    batch = next(iter(ds.sample_batches(60, 1, seed=9)))
    torch.manual_seed(11)
    m = build_model(ds, kind, L, order, d)
    results = []
    for tables in (True, False):
        ops.NODE_TABLES = tables
        try:
            profiler.start()
            results.append(step_gradients(m, batch) + (None,))
            profiler.stop()
            results[-1] = results[-1][:2] + (profiler.summary(),)
        finally:
            ops.NODE_TABLES = True
            profiler.stop()
    (l1, g1, s1), (l0, g0, s0) = results
    for s in (s1, s0):
        assert {'query_gru_fwd', 'query_gru_bwd'} <= set(s) and not {'bag_mean_fwd', 'bag_mean_bwd', 'query_transform_fwd'} & set(s)
    assert torch.equal(l1, l0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    want = float64_gradients(m, w, w.triples, kind, L, order, batch)
    assert abs(l1.item() - want['loss']) <= LOSS_RTOL * abs(want['loss'])
    for k in g1:
        print(f'{kind} d {d} {k}: {rel(g1[k], want["grads"][k]) / RTOL:.3f} of the bar')
        assert rel(g1[k], want['grads'][k]) <= RTOL, k
    assert all(float(g1[k].abs().max()) > 0 for k in gref.KEYS)


def test_step_on_a_compact_layout_with_multiplicities_with_the_gru(monkeypatch):
    """A layout that leaves the isolated nodes out and keeps a repeated triple once with its multiplicity against the every-node-a-row model on the same weights, and
    both against float64."""
    from ihgnn_amd import layout as layout_mod, synth
    from ihgnn_amd.Dataset import GraphDataset
    w = synth.draw(300, 40, 200, 50, 4000, seed=21)
    g = np.random.default_rng(4)
    live = [g.choice(n, n // 3, replace=False) for n in (300, 40, 200)]
    base = np.stack([g.choice(live[k], 3000) for k in range(3)], 1)
    triples = np.concatenate([base, base[:1500]])
    models, batch = {}, None
    for collapsed in (False, True):
        monkeypatch.setattr(layout_mod, 'COMPACT_NODES', '1' if collapsed else '0')
        monkeypatch.setattr(layout_mod, 'EDGE_MULTIPLICITY', '1' if collapsed else '0')
        ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, triples, device=dev())
        assert bool(getattr(ds.hypergraph.layout, 'compact', False)) == collapsed
        if batch is None:
            batch = next(iter(ds.sample_batches(80, 1, seed=5)))
        torch.manual_seed(7)
        models[collapsed] = build_model(ds, 'ihgnn', 2, 3, 64)
    models[True].load_state_dict(models[False].state_dict())
    l0, g0 = step_gradients(models[False], batch)
    l1, g1 = step_gradients(models[True], batch)
    want = float64_gradients(models[False], w, triples, 'ihgnn', 2, 3, batch)
    assert abs(l1.item() - l0.item()) <= 2e-6 * abs(l0.item()) and abs(l1.item() - want['loss']) <= LOSS_RTOL * abs(want['loss'])
    for k in g0:
        assert rel(g1[k], g0[k]) <= RTOL and rel(g1[k], want['grads'][k]) <= RTOL and rel(g0[k], want['grads'][k]) <= RTOL, k


def test_step_at_a_padded_width_with_the_gru():
    """d = 96 runs at 128: the GRU's operands zero-padded inside the op, the padding columns of every layer output exactly zero, the gradients the 96-wide model's."""
    w, ds = synth_dataset(seed=33, counts=(150, 30, 110, 40, 2500))
    batch = next(iter(ds.sample_batches(60, 1, seed=9)))
    torch.manual_seed(3)
    m = build_model(ds, 'ihgnn', 2, 3, 96)
    assert m.compute_width == 128
    with torch.no_grad():
        for x in m.propagate_layers():
            assert x.shape[1] == 128 and float(x[:, 96:].abs().max()) == 0.0
    l, g = step_gradients(m, batch)
    want = float64_gradients(m, w, w.triples, 'ihgnn', 2, 3, batch)
    assert abs(l.item() - want['loss']) <= LOSS_RTOL * abs(want['loss'])
    for k in g:
        assert g[k].shape == want['grads'][k].shape and rel(g[k], want['grads'][k]) <= RTOL, k


@pytest.mark.parametrize('path', ['forward', 'bce_loss'])
@pytest.mark.parametrize('kind,L,order,d', MODEL_CASES)
def test_models_match_the_float64_step(kind, L, order, d, path):
    """Scores, loss, every gradient and the parameters after one Adam step on both call paths - ``forward`` + ``BCEWithLogitsLoss`` (torch's Adam) and ``bce_loss`` (the
    fused batch tail; the library's Adam) - against the float64 step; the stepped parameters within what the gradient's bar allows (``adam_allowance``)."""
    w = small()
    ds = dataset_from_npz(w)
    torch.manual_seed(13)
    m = build_model(ds, kind, L, order, d)
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    U, Q, I = (int(c) for c in w['counts'][:3])
    rng = np.random.default_rng(6)
    u, q, i = rng.integers(0, U, 96), rng.integers(0, Q, 96), rng.integers(0, I, 96)
    flags = (rng.random(96) < 0.3).astype(np.float32)
    tu, tq, ti = (torch.from_numpy(v).to(dev()) for v in (u, q, i))
    tf = torch.from_numpy(flags).to(dev())
    step64 = gref.model_step(sd, w['triples'], w['counts'], w['bag_words'] + 1, w['bag_offsets'], kind, L, order, u, q, i, flags.astype(np.float64))
    if path == 'forward':
        opt = torch.optim.Adam(m.parameters(), 1e-3, weight_decay=0)
        scores = m(tu, tq, ti)
        loss = torch.nn.BCEWithLogitsLoss()(scores, tf)
        assert rel(scores, step64['scores']) <= RTOL
    else:
        from ihgnn_amd.optim import Adam
        opt = Adam(m.parameters(), 1e-3, weight_decay=0)
        loss = m.bce_loss(tu, tq, ti, tf)
    loss.backward()
    assert abs(loss.item() - step64['loss']) <= LOSS_RTOL * abs(step64['loss'])
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        print(f'   grad {n}: {rel(p.grad, step64["grads"][n]) / RTOL:.3f} of the bar')
        assert rel(p.grad, step64['grads'][n]) <= RTOL, n
    opt.step()
    for n, p in m.named_parameters():
        assert gref.adam_excess(p, step64['grads'][n], step64['adam'][n], RTOL) <= 1.0, n


@pytest.mark.parametrize('kind', ['gcn', 'gat', 'phase2'])
def test_other_layer_kinds_with_the_gru(kind):
    """GCN and GAT (the pairwise graph) and IHGNN with phase-2 attention over the GRU's query rows: X0's query rows are the float64 encoder's; a step gives every
    parameter a finite gradient; the encoder's own gradients are the float64 backward of the cotangent that reached the query rows of X0.  Repeatable bit for bit."""
    from ihgnn_amd.Helpers.Graph import Pps2DGraph
    from ihgnn_amd.Models import GATLayer, GCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn
    w, ds = synth_dataset(seed=33, counts=(150, 30, 110, 40, 2500))
    if kind != 'phase2':
        ds.graph_type = Pps2DGraph
    torch.manual_seed(2)
    with query_settings():
        if kind == 'phase2':
            m = RawGnn(dev(), ds, 32, IHGNNLayer, 2, 3, True, HemPredictionLayer, 0.5).to(dev())
        else:
            m = RawGnn(dev(), ds, 32, GCNLayer if kind == 'gcn' else GATLayer, 2, 1, False, HemPredictionLayer, 0.5).to(dev())
    u, q, i, y = next(iter(ds.sample_batches(60, 1, seed=9)))
    emb, seen = m.embeddings, []
    plain_all_nodes = emb.all_nodes

    def capturing(out=None):
        x = plain_all_nodes(out)
        if x.requires_grad:
            x.retain_grad()
            seen.append(x)
        return x
    emb.all_nodes = capturing
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        del seen[:]
        loss = torch.nn.BCEWithLogitsLoss()(m(u, q, i), y.float())
        loss.backward()
        assert len(seen) == 1 and np.isfinite(loss.item())
        runs.append((loss.item(), {k: p.grad.clone() for k, p in m.named_parameters()}, seen[0].detach().clone(), seen[0].grad.clone()))
    assert runs[0][0] == runs[1][0] and all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
    _, grads, x0, dx0 = runs[0]
    assert all(torch.isfinite(g).all() for g in grads.values()) and set(grads) == {k for k, _ in m.named_parameters()}
    U, Q = ds.user_count, ds.query_count
    table_key = EMB + 'embedding_bag_vocabulary.weight'
    sd = {k: gref.t64(v).requires_grad_(True) for k, v in m.state_dict().items() if k.startswith(EMB)}
    y64 = gref.gru_rows(sd[table_key], w.bag_words + 1, w.bag_offsets, *(sd[k] for k in gref.KEYS))
    assert rel(x0[U:U + Q], y64) <= RTOL
    y64.backward(dx0[U:U + Q].cpu().double())
    for k in gref.KEYS + (table_key,):
        assert rel(grads[k], sd[k].grad) <= RTOL, k


# ---------------------------------------------------------------------------------------------
# evaluation, search, recorded step, two ranks, kernel trace, driver
# ---------------------------------------------------------------------------------------------
def test_evaluation_features_and_top_items_with_the_gru():
    """``save_features_for_test`` (the GRU writes the query rows of the first column slice, storing nothing for a backward) equals the autograd path's features and the
    float64 model's; ``top_items`` over them equals the ranking of the float64 features."""
    from oracle import ihgnn_ref as ref
    w, ds = synth_dataset(seed=33, counts=(150, 30, 110, 40, 2500))
    torch.manual_seed(5)
    m = build_model(ds, 'ihgnn', 2, 3, 64)
    taped = m.propagate().detach()
    with torch.no_grad():
        m.save_features_for_test()
        feats = m._saved_output_feature
        assert torch.equal(feats, taped)
        sd = {k: gref.t64(v) for k, v in m.state_dict().items()}
        g64 = ref.HyperGraph(w.triples, w.user_count, w.query_count, w.item_count, dtype=torch.float64)
        f64 = torch.cat(gref.model_features(sd, g64, w.bag_words + 1, w.bag_offsets, 'ihgnn', 2, 3), 1)
        assert rel(feats, f64) <= RTOL
        users = torch.arange(0, 40, device=dev()); queries = torch.arange(0, 40, device=dev()) % ds.query_count
        items, scores = m.top_items(users, queries, 10)
        lam = m.prediction_layer.lambda_muq
        mixed = lam * f64[queries.cpu() + ds.query_start_index_in_graph] + (1 - lam) * f64[users.cpu()]
        all64 = mixed @ f64[ds.item_start_index_in_graph:].t() + sd['prediction_layer.items_bias']
        top64 = all64.topk(10, dim=1)
        assert rel(scores, top64.values) <= RTOL
        same = items.cpu().long() == top64.indices
        swapped = torch.gather(all64, 1, items.cpu().long())
        assert bool((same | ((swapped - top64.values).abs() <= RTOL * all64.abs().max())).all())
        m.clear_saved_feature()


def test_search_by_words_reads_their_order():
    """``RawGnn.search(users, words=, offsets=)`` on a GRU model: a bag that equals a training query's words gives that query's layer-0 row bit for bit; the same words
    reversed give another row (the bag mean cannot tell the two apart - that is the feature); ``users = -1`` works."""
    w, ds = synth_dataset(seed=33, counts=(150, 30, 110, 40, 2500))
    torch.manual_seed(5)
    m = build_model(ds, 'ihgnn', 2, 3, 64)
    ends = gref.bag_bounds(w.bag_words, w.bag_offsets)
    lens = np.diff(ends)
    picks = [int(k) for k in np.argsort(-lens, kind='stable')[:3]]
    assert lens[picks[0]] >= 2 and len(set(w.bag_words[ends[picks[0]]:ends[picks[0] + 1]].tolist())) >= 2
    with torch.no_grad():
        x0 = m.embeddings.embed_query()
        fwd = [w.bag_words[ends[k]:ends[k + 1]] for k in picks]
        flat, offsets = np.concatenate(fwd), np.cumsum([0] + [len(b) for b in fwd[:-1]])
        rows = m.embeddings.embed_bags(flat, offsets)
        assert torch.equal(rows, x0[torch.tensor(picks, device=dev())])
        back = m.embeddings.embed_bags(np.concatenate([b[::-1] for b in fwd]), offsets)
        assert not torch.equal(back[0], rows[0]) and float((back[0] - rows[0]).abs().max()) > 1e-4
        m.save_features_for_test()
        users = torch.tensor([0, 5, -1], device=dev())
        items, scores = m.search(users, words=flat, offsets=offsets, k=5)
        items_b, scores_b = m.search(users, words=np.concatenate([b[::-1] for b in fwd]), offsets=offsets, k=5)
        m.clear_saved_feature()
    assert tuple(items.shape) == (3, 5) and bool(torch.isfinite(scores).all()) and bool((items >= 0).all())
    assert not torch.equal(scores, scores_b)


def test_recorded_step_equals_the_eager_step_with_the_gru():
    """``CapturedTrainingStep`` over 8 batches is bitwise the eager step (losses, parameters); all four GRU parameters moved."""
    from ihgnn_amd.captured_step import CapturedTrainingStep
    from ihgnn_amd.optim import Adam
    w, ds = synth_dataset(seed=21)
    batches = list(ds.sample_batches(100, 8, seed=5))

    def run(recorded):
        torch.manual_seed(7)
        m = build_model(ds, 'ihgnn', 2, 3, 64)
        opt = Adam(m.parameters(), 1e-3, weight_decay=0)
        step = CapturedTrainingStep(m, opt, batches[0][0].shape[0], warmup_batch=batches[0]) if recorded else None
        losses = []
        for u, q, i, y in batches:
            if step is not None:
                losses.append(step.step(u, q, i, y).item())
            else:
                loss = m.bce_loss(u, q, i, y)
                loss.backward()
                assert all(p.grad is not None for p in m.parameters())
                opt.step(); opt.zero_grad()
                losses.append(loss.item())
        return losses, {k: v.clone() for k, v in m.state_dict().items()}

    l0, p0 = run(False)
    l1, p1 = run(True)
    assert l0 == l1
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    torch.manual_seed(7)
    fresh = build_model(ds, 'ihgnn', 2, 3, 64).state_dict()
    for k in gref.KEYS:
        assert not torch.equal(p0[k], fresh[k]), k


def test_two_ranks_on_one_gpu_with_the_gru(tmp_path):
    """``python -m ihgnn_amd.Main --query_transform gru`` as two ranks on GPU 0 over gloo: the checkpoints of a ``cotangent`` run and a ``flat`` run agree, hold the GRU's
    parameters, and no replica drift was logged."""
    import socket
    import subprocess
    import sys
    from ihgnn_amd import synth
    w = synth.draw(60, 20, 80, 25, 501, seed=4, eval_logs=30)
    synth.write_files(w, str(tmp_path / 'Data' / 'Synth' / 'Tiny'))
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    states = {}
    for sync in ('cotangent', 'flat'):
        with socket.socket() as sock:
            sock.bind(('127.0.0.1', 0))
            port = sock.getsockname()[1]
        procs = []
        for rank in range(2):
            env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), IHG_DIST_BACKEND='gloo',
                       HSA_ENABLE_IPC_MODE_LEGACY='0', PYTHONPATH=repo + os.pathsep + os.environ.get('PYTHONPATH', ''))
            procs.append(subprocess.Popen([sys.executable, '-m', 'ihgnn_amd.Main', '--ds', 'Synth/Tiny/', '--gnn', 'IHGNN', '--gnns', '2', '--fo', '3', '--emb', '32', '--ec', '2',
                                           '--est', '2', '--etf', '1', '-c', '--device', '0', '--grad_sync', sync, '--seed', '3', '--query_transform', 'gru'],
                                          cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = [p.communicate(timeout=600)[0] for p in procs]
        assert all(p.returncode == 0 for p in procs), outs[0][-3000:] + outs[1][-3000:]
        assert 'query transform gru' in outs[0]
        assert 'replicas drifted apart' not in outs[0] + outs[1]
        result_dir = tmp_path / 'Results' / 'Synth-Tiny-RawGnn-2IHGNNLayer-O3-emb32'
        saved = sorted(n for n in os.listdir(result_dir) if n.startswith('checkpoint_'))
        states[sync] = torch.load(os.path.join(result_dir, saved[-1]), map_location='cpu')['model']
        for n in saved:
            os.remove(os.path.join(result_dir, n))
    assert all(k in states['flat'] for k in gref.KEYS)
    for name, value in states['cotangent'].items():
        assert torch.isfinite(value).all()
        assert float((value - states['flat'][name]).abs().max()) <= 1e-3, name


def test_step_with_the_gru_launches_only_library_kernels(tmp_path):
    """Training steps (d = 128, 2 layers, order 3; tables read in place) under a kernel trace: between two Adam launches every kernel is one of the library's, and the GRU
    is one forward launch and three backward launches (plus the segment sum) whatever the bag lengths."""
    import csv
    import glob
    import shutil
    import subprocess
    import sys
    profiler_exe = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    if not os.path.exists(profiler_exe):
        pytest.skip('rocprofv3 not available')
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'gru_trace.py'
    script.write_text(f'''
import sys
sys.path.insert(0, {repo!r})
import torch
from ihgnn_amd import ops, synth
from ihgnn_amd.Dataset import GraphDataset
from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
from ihgnn_amd.optim import Adam
dev = torch.device('cuda:0')
w = synth.draw(300, 40, 200, 50, 4000, seed=21, distribution='powerlaw')
ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev)
batches = list(ds.sample_batches(100, 6, seed=5))
Gs.Query.transform = Gsv.gru
torch.manual_seed(1)
m = RawGnn(dev, ds, 128, IHGNNLayer, 2, 3, False, HemPredictionLayer, 0.5).to(dev)
m.batch_rows_only_last_layer = False
opt = Adam(m.parameters(), 1e-3, weight_decay=0)
for u, q, i, y in batches:
    loss = m.bce_loss(u, q, i, y)
    ops.backward(loss)
    opt.step(); opt.zero_grad()
torch.cuda.synchronize()
print('steps done')
''')
    out = str(tmp_path / 'trace')
    r = subprocess.run([profiler_exe, '--kernel-trace', '--output-format', 'csv', '-d', out, '--', sys.executable, str(script)], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0 and 'steps done' in r.stdout, r.stderr[-2000:]
    files = glob.glob(os.path.join(out, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no kernel trace written'
    rows = sorted(csv.DictReader(open(files[0])), key=lambda x: int(x['Start_Timestamp']))
    adam = [k for k, x in enumerate(rows) if 'adam_kernel' in x['Kernel_Name']]
    assert len(adam) >= 6
    for a, b in ((adam[2], adam[3]), (adam[-3], adam[-2])):
        step = [x['Kernel_Name'] for x in rows[a + 1:b + 1]]
        foreign = [n for n in step if 'at::native' in n or '__amd_rocclr' in n or 'elementwise_kernel' in n]
        assert not foreign, foreign
        short = sorted({n.split('(')[0] for n in step})
        for name in ('gru_fwd_kernel<128>', 'gru_bwd_steps_kernel<128>', 'gru_wgrad_kernel<128>', 'gru_finish_kernel'):
            assert sum(name in n for n in step) == 1, (name, short)


def test_driver_epoch_with_the_gru_writes_a_checkpoint_that_reloads(tmp_path, monkeypatch):
    """Two driver epochs with ``--query_transform gru``: finite metrics, a checkpoint with the GRU's keys that loads into a fresh GRU model and not into a mean model; the
    settings are put back afterwards."""
    import random
    from ihgnn_amd import Main as driver, synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    w = synth.draw(200, 30, 150, 40, 3000, seed=8, eval_logs=40)
    synth.write_files(w, str(tmp_path / 'Data' / 'Synth' / 'Tiny'))
    monkeypatch.chdir(tmp_path)
    old = Gs.Query.transform
    try:
        random.seed(11); torch.manual_seed(11)
        result = driver.main(['--ds', 'Synth/Tiny/', '--gnns', '2', '--fo', '3', '--emb', '32', '--ec', '2', '--est', '2', '--etf', '1', '-c', '--query_transform', 'gru'])
        assert Gs.Query.transform == 'gru'
    finally:
        Gs.Query.transform = old
    _, metrics = list(result.iter_epoch_test())[-1]
    assert np.isfinite([metrics.HitRatio_at10, metrics.NDCG_at10, metrics.MAP_at10]).all()
    result_dir = tmp_path / 'Results' / 'Synth-Tiny-RawGnn-2IHGNNLayer-O3-emb32'
    saved = sorted(n for n in os.listdir(result_dir) if n.startswith('checkpoint_'))
    assert saved
    state = torch.load(os.path.join(result_dir, saved[-1]), map_location='cpu')['model']
    assert [tuple(state[k].shape) for k in gref.KEYS] == [(96, 32), (96, 32), (96,), (96,)]
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev())
    m = build_model(ds, 'ihgnn', 2, 3, 32)
    m.load_state_dict(state)
    with pytest.raises(RuntimeError):
        build_model(ds, 'ihgnn', 2, 3, 32, None).load_state_dict(state)
    # ``python -m ihgnn_amd.Search`` with the same flags answers from that checkpoint, and the order of a search's words matters
    import io
    from ihgnn_amd import Search
    searches = [(3, [1, 2, 5]), (3, [5, 2, 1]), (-1, [7]), (0, [])]
    printed = io.StringIO()
    try:
        assert Search.main(['--ds', 'Synth/Tiny/', '--gnns', '2', '--fo', '3', '--emb', '32', '--query_transform', 'gru', '--cp', 'latest', '--k', '5'],
                           lines=[f'{u}\t{" ".join(map(str, ws))}\n' for u, ws in searches], out=printed) == 0
    finally:
        Gs.Query.transform = old
    with torch.no_grad():
        m.save_features_for_test()
        items, scores = m.search(torch.tensor([u for u, _ in searches]), words=np.asarray([x for _, ws in searches for x in ws], np.int64),
                                 offsets=np.cumsum([0] + [len(ws) for _, ws in searches[:-1]]).astype(np.int64), k=5)
        m.clear_saved_feature()
    got = printed.getvalue().splitlines()
    assert got == [Search.format_answer(a, b) for a, b in zip(items.cpu().tolist(), scores.cpu().tolist())]
    assert got[0] != got[1]
