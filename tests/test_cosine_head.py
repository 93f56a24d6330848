"""GPU: the cosine-similarity HEM head (``Gs.Prediction.use_cosine_similarity``; ``hem_cosine_fwd/bwd_kernel`` in csrc/tail.hip, the cosine instantiations of
csrc/eval.hip, ``ops.hem_score / hem_bce_loss / score_topk(..., cosine=True)``, ``RawGnn``, the loops, the recorded step, ``--cosine``) against
``torch.cosine_similarity`` in float64 on the CPU, a float64 restatement (``tests/cosine_reference.py``, held to the reference by ``tests/test_cosine_head_host.py``)
and the reference's own numbers (fixture F14, ``tests/golden/make_golden_cosine.py``).

Bars: RTOL = 1e-5 of the reference tensor's largest magnitude (``tests/test_gpu_parity.py:16-27``); RTOL_SUM = 2e-6 where two of our own paths differ by summation
order only.  A float32 torch evaluation of the tail recipe on the CPU sits at 3e-7 from float64."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cosine_reference as cref
import query_transform_reference as qref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RTOL = 1e-5
RTOL_SUM = 2e-6
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device('cuda:0')


def as64(a):
    return a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)


def rel(a, b):
    a, b = as64(a), as64(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class cosine_setting:
    """``Gs.Prediction.use_cosine_similarity`` for the block, put back after it."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        self.old = Gs.Prediction.use_cosine_similarity
        Gs.Prediction.use_cosine_similarity = self.on

    def __exit__(self, *exc):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        Gs.Prediction.use_cosine_similarity = self.old


def build_model(ds, kind, L, order, d):
    from ihgnn_amd.Models import HGCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn
    return RawGnn(dev(), ds, d, IHGNNLayer if kind == 'ihgnn' else HGCNLayer, L, order, False, HemPredictionLayer, 0.5).to(dev())


def dataset_of(w, triples=None):
    from ihgnn_amd.Dataset import GraphDataset
    return GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples if triples is None else triples, device=dev())


def check_top(items, scores, want, k):
    """Rule (5) for one (user, query) pair: the returned scores and the reference scores of the returned items equal the reference's top ``k`` to RTOL, the items are
    distinct, and where the smallest gap inside the reference's top ``k`` exceeds 1e-4 max|score| the list equals the stable descending sort exactly.  -> whether that
    strict comparison applied."""
    order = torch.sort(want, descending=True, stable=True).indices[:k]
    assert rel(scores, want[order]) <= RTOL
    assert rel(want[items], want[order]) <= RTOL
    assert len(set(items.tolist())) == k
    gap = (want[order][:-1] - want[order][1:]).abs().min().item() if k > 1 else 1.0
    if gap > 1e-4 * want.abs().max().item():
        assert items.tolist() == order.tolist()
        return True
    return False


# ---------------------------------------------------------------------------------------------
# 1, 2: the batch tail against float64
# ---------------------------------------------------------------------------------------------
TAIL_CASES = [(32, 3, 70), (64, 3, 70), (50, 3, 70), (128, 8, 33), (256, 2, 70), (7, 1, 5)]
U, Q, I = 30, 12, 40


def tail_inputs(d, n_layers, batch, scaled):
    gen = torch.Generator().manual_seed(1000 * d + 10 * n_layers + batch)
    n = U + Q + I
    layers = [torch.randn(n, d, generator=gen) / np.sqrt(d) for _ in range(n_layers)]
    if scaled:
        row = 10 ** (2 * torch.rand(n, 1, generator=gen) - 1)
        layers = [x * row * 0.1 ** l for l, x in enumerate(layers)]
    bias = torch.randn(I, generator=gen)
    u, q, i = (torch.randint(0, c, (batch,), generator=gen) for c in (U, Q, I))
    labels = (torch.rand(batch, generator=gen) < 0.1).float()
    cot = torch.randn(batch, generator=gen)
    return layers, bias, u, q, i, labels, cot


def tail_float64(layers, bias, u, q, i, labels, cot, lam=0.5):
    """scores, loss and the gradients of ``(scores * cot).sum()`` and of the loss, from ``torch.cosine_similarity`` + ``binary_cross_entropy_with_logits`` in float64."""
    out = {}
    for what in ('scores', 'loss'):
        xs = [x.double().requires_grad_(True) for x in layers]
        b = bias.double().requires_grad_(True)
        f = torch.cat(xs, 1)
        scores = torch.cosine_similarity(f[i + U + Q], lam * f[q + U] + (1 - lam) * f[u]) + b[i]
        loss = F.binary_cross_entropy_with_logits(scores, labels.double())
        ((scores * cot.double()).sum() if what == 'scores' else loss).backward()
        out[what] = (scores.detach() if what == 'scores' else loss.detach(), [x.grad for x in xs], b.grad)
    return out


@pytest.mark.parametrize('d,n_layers,batch', TAIL_CASES)
def test_tail_matches_float64(d, n_layers, batch):
    """``ops.hem_score(..., cosine=True)`` and ``ops.hem_bce_loss(..., cosine=True)`` over plain matrices, no holder: half-empty lanes (32), a width off the wave (50),
    eight layers, a batch off the waves per block (33), one layer and fewer columns than lanes (7); rows repeat (30 users, 12 queries, 40 items).  In all but the first
    and last case the rows' magnitudes span two decades and layer l is scaled by 0.1^l."""
    from ihgnn_amd import ops
    layers, bias, u, q, i, labels, cot = tail_inputs(d, n_layers, batch, scaled=(d, n_layers, batch) not in (TAIL_CASES[0], TAIL_CASES[-1]))
    want = tail_float64(layers, bias, u, q, i, labels, cot)
    rows = torch.cat([u, q + U, i + U + Q]).to(dev())
    for what in ('scores', 'loss'):
        xs = [x.to(dev()).requires_grad_(True) for x in layers]
        b = bias.to(dev()).requires_grad_(True)
        if what == 'scores':
            got = ops.hem_score(xs, rows, i.to(dev()), b, 0.5, U + Q, cosine=True)
            got.backward(cot.to(dev()))
        else:
            got = ops.hem_bce_loss(xs, rows, i.to(dev()), labels.to(dev()), b, 0.5, U + Q, cosine=True)
            got.backward()
        ref_out, ref_grads, ref_bias = want[what]
        errs = [rel(got, ref_out)] + [rel(x.grad, g) for x, g in zip(xs, ref_grads)] + [rel(b.grad, ref_bias)]
        print(f'd {d} layers {n_layers} batch {batch} {what}: value {errs[0]:.2e} layer gradients {max(errs[1:-1]):.2e} dbias {errs[-1]:.2e}')
        assert max(errs) <= RTOL, errs


def test_tail_zero_row_and_row_below_eps():
    """One layer; the item rows of the batch: a zero row (cos = 0), a row of norm 2e-9 (torch clamps the norm to 1e-8: a fifth of the unit row's cosine) and two
    ordinary rows, every user and query row used once - scores and every row of the gradient (all finite) equal torch float64's, row by row."""
    from ihgnn_amd import ops
    d = 32
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(U + Q + I, d, generator=gen) / np.sqrt(d)
    x[U + Q + 0] = 0.0
    x[U + Q + 1] *= 2e-9 / float(x[U + Q + 1].norm())
    bias = torch.randn(I, generator=gen)
    u, q, i = torch.tensor([3, 4, 5, 6]), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2, 3])
    cot = torch.tensor([0.7, -1.3, 0.4, 1.1])
    x64 = x.double().requires_grad_(True)
    b64 = bias.double().requires_grad_(True)
    want = torch.cosine_similarity(x64[i + U + Q], 0.5 * x64[q + U] + 0.5 * x64[u]) + b64[i]
    (want * cot.double()).sum().backward()
    assert torch.isfinite(x64.grad).all()
    m1, a1 = (0.5 * x64[q + U] + 0.5 * x64[u])[1].detach(), x64[U + Q + 1].detach()
    assert float(want[0] - b64[0]) == 0.0                                # cos = 0 ...
    assert abs(float(want[1] - b64[1]) - float(a1.norm()) / 1e-8 * float(a1 @ m1 / (a1.norm() * m1.norm()))) <= 1e-12 and abs(float(a1.norm()) / 1e-8 - 0.2) <= 1e-6     # ... and 0.2 cos
    xg, bg = x.to(dev()).requires_grad_(True), bias.to(dev()).requires_grad_(True)
    got = ops.hem_score([xg], torch.cat([u, q + U, i + U + Q]).to(dev()), i.to(dev()), bg, 0.5, U + Q, cosine=True)
    got.backward(cot.to(dev()))
    assert torch.isfinite(xg.grad).all()
    assert rel(got, want) <= RTOL and rel(bg.grad, b64.grad) <= RTOL
    touched = torch.cat([u, q + U, i + U + Q])
    for r in touched.tolist():
        scale = float(x64.grad[r].abs().max())
        if scale == 0.0:
            assert float(xg.grad[r].abs().max()) == 0.0, r
        else:
            assert rel(xg.grad[r], x64.grad[r]) <= RTOL, r
    rest = torch.ones(U + Q + I, dtype=torch.bool)
    rest[touched] = False
    assert float(xg.grad[rest.to(dev())].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# 3: the models against F14
# ---------------------------------------------------------------------------------------------
F14_CASES = (('ihgnn_o3_d32', 'ihgnn'), ('hgcn_d64', 'hgcn'))


def f14():
    return np.load(os.path.join(GOLDEN, 'f14_cosine.npz'))


def small_dataset():
    from ihgnn_amd.Dataset import GraphDataset
    w = np.load(os.path.join(GOLDEN, 'f2_small_workload.npz'))
    Uc, Qc, Ic, V = (int(x) for x in w['counts'])
    return w, GraphDataset.from_arrays(Uc, Qc, Ic, V, w['bag_words'], w['bag_offsets'], w['triples'], device=dev())


def adam_excess_against_fixture(z, prefix, got, g64, p64):
    """The stepped parameter against the entries F14 keeps of the reference's, as a multiple of ``qref.adam_allowance`` at RTOL (``tests/test_query_transform.py``)."""
    allowed = qref.adam_allowance(g64, p64, RTOL)
    got = as64(got)
    if prefix + '.full' in z.files:
        return float((np.abs(got - z[prefix + '.full'].astype(np.float64)) / allowed).max())
    return float((np.abs(got[::8] - z[prefix + '.rows8'].astype(np.float64)) / allowed[::8]).max())


@pytest.mark.parametrize('path', ['forward', 'bce_loss'])
@pytest.mark.parametrize('tag,kind', F14_CASES)
def test_f14_models_match_reference(tag, kind, path):
    """Scores, loss, every gradient (through ``kept()``'s digests) and the parameters after one Adam step of F14's models on both call paths, against the reference and the
    float64 restatement; ``top_items`` against the reference's all-item scores of the 12 test logs by rule (5), and the ranking metrics of the logs it applies to."""
    from ihgnn_amd.Helpers.Metrics import Metrics
    z = f14()
    w, ds = small_dataset()
    pre = tag + '.'
    L, order, d, _ = (int(v) for v in z[pre + 'cfg'])
    sd = qref.fixture_state(z, tag)
    with cosine_setting():
        m = build_model(ds, kind, L, order, d)
        assert list(sd) == list(m.state_dict())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        # evaluation of the initial parameters
        uq = torch.from_numpy(z['test.uq']).to(dev())
        with torch.no_grad():
            m.save_features_for_test()
            items, scores = m.top_items(uq[:, 0], uq[:, 1], 10)
            dense = m.score_all_items(uq[:, 0], uq[:, 1])
            m.clear_saved_feature()
        assert rel(dense, z[pre + 'all_scores']) <= RTOL
        ends = np.cumsum(z['test.items_len'])
        strict = 0
        for k in range(len(ends)):
            if check_top(items[k].cpu().long(), scores[k].cpu(), torch.from_numpy(z[pre + 'all_scores'][k]), 10):
                strict += 1
                truth = z['test.items_flat'][ends[k] - z['test.items_len'][k]:ends[k]].tolist()
                got = Metrics.from_top_indices(items[k].tolist(), truth, None, True)
                np.testing.assert_allclose([got.HitRatio_at10, got.NDCG_at10, got.MAP_at10], z[pre + 'metrics_per_log'][k], atol=1e-9)
        assert strict >= 0.8 * len(ends), strict
        # one training step
        u, q, i = (torch.from_numpy(z[pre + k]).to(dev()) for k in 'uqi')
        flags = torch.from_numpy(z[pre + 'flags']).to(dev())
        if path == 'forward':
            opt = torch.optim.Adam(m.parameters(), 1e-3, weight_decay=0)
            got_scores = m(u, q, i)
            loss = torch.nn.BCEWithLogitsLoss()(got_scores, flags)
            assert rel(got_scores, z[pre + 'scores']) <= RTOL
        else:
            from ihgnn_amd.optim import Adam
            opt = Adam(m.parameters(), 1e-3, weight_decay=0)
            loss = m.bce_loss(u, q, i, flags)
        loss.backward()
    step64 = cref.model_step(sd, w['triples'], w['counts'], w['bag_words'] + 1, w['bag_offsets'], kind, L, order, z[pre + 'u'], z[pre + 'q'], z[pre + 'i'], z[pre + 'flags'])
    print(f'{tag} {path}: loss {loss.item():.7f} reference {float(z[pre + "loss"]):.7f}')
    assert abs(loss.item() - float(z[pre + 'loss'])) <= RTOL * abs(float(z[pre + 'loss']))
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        e_ref, e_64 = qref.fixture_error(z, pre + 'grad.' + n, p.grad), rel(p.grad, step64['grads'][n])
        print(f'   grad {n}: reference {e_ref:.2e} float64 {e_64:.2e}')
        assert e_ref <= RTOL and e_64 <= RTOL, n
    opt.step()
    for n, p in m.named_parameters():
        e_ref = adam_excess_against_fixture(z, pre + 'adam.' + n, p, step64['grads'][n], step64['adam'][n])
        e_64 = qref.adam_excess(p, step64['grads'][n], step64['adam'][n], RTOL)
        assert e_ref <= 1.0 and e_64 <= 1.0, (n, e_ref, e_64)


# ---------------------------------------------------------------------------------------------
# 4: every route into the tail
# ---------------------------------------------------------------------------------------------
ROUTE_MODELS = [('ihgnn', 2, 3, 64), ('hgcn', 2, 1, 32)]


def step_gradients(m, batch):
    m.zero_grad(set_to_none=True)
    loss = m.bce_loss(*batch)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize('kind,L,order,d', ROUTE_MODELS)
def test_routes_into_the_tail_agree(kind, L, order, d):
    """One step of ``bce_loss`` + backward with the embedding tables read in place against X0 assembled (``IHG_NODE_TABLES`` 1 / 0) and with the last layer evaluated at
    the batch rows only against everywhere: loss and every gradient to RTOL_SUM; the first form also against the float64 restatement to RTOL."""
    from ihgnn_amd import ops, profiler, synth
    w = synth.draw(60, 20, 80, 25, 500)
    ds = dataset_of(w)
    batch = next(iter(ds.sample_batches(40, 1, seed=9)))
    torch.manual_seed(11)
    with cosine_setting():
        m = build_model(ds, kind, L, order, d)
        runs = {}
        for tables, rows_only in ((True, True), (False, True), (True, False)):
            ops.NODE_TABLES, m.batch_rows_only_last_layer = tables, rows_only
            try:
                profiler.start()
                runs[tables, rows_only] = step_gradients(m, batch)
                profiler.stop()
                assert {'hem_cosine_fwd', 'hem_cosine_bwd'} <= set(profiler.summary()) and 'hem_score_fwd' not in profiler.summary()
            finally:
                ops.NODE_TABLES, m.batch_rows_only_last_layer = True, True
                profiler.stop()
    l0, g0 = runs[True, True]
    for other in ((False, True), (True, False)):
        l1, g1 = runs[other]
        assert abs(l1.item() - l0.item()) <= RTOL_SUM * abs(l0.item())
        for k in g0:
            assert rel(g1[k], g0[k]) <= RTOL_SUM, (other, k, rel(g1[k], g0[k]))
    u, q, i, y = (v.cpu().numpy() for v in batch)
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    want = cref.model_step(sd, w.triples, (w.user_count, w.query_count, w.item_count), w.bag_words + 1, w.bag_offsets, kind, L, order, u, q, i, y.astype(np.float64))
    assert abs(l0.item() - want['loss']) <= RTOL * abs(want['loss'])
    for k in g0:
        assert rel(g0[k], want['grads'][k]) <= RTOL, (k, rel(g0[k], want['grads'][k]))


@pytest.mark.parametrize('kind,L,order,d', ROUTE_MODELS)
def test_compact_layout_with_isolated_batch_nodes(kind, L, order, d, monkeypatch):
    """Two thirds of every node type in no hyperedge; the batch names isolated users, queries and items.  Under ``IHG_COMPACT_NODES=1`` their rows above layer 0 do not
    exist (negative ``rows_upper``): they add zeros to the head's sums and their layer-0 squares still count in the norms.  Loss and every gradient against the
    every-node-a-row layout to RTOL_SUM and against float64 to RTOL."""
    from ihgnn_amd import layout as layout_mod, synth
    w = synth.draw(60, 20, 80, 25, 500)
    g = np.random.default_rng(4)
    counts = (w.user_count, w.query_count, w.item_count)
    live = [g.choice(n, n // 3, replace=False) for n in counts]
    triples = np.stack([g.choice(live[k], 400) for k in range(3)], 1)
    B = 90
    u, q, i = (torch.from_numpy(g.integers(0, n, B)) for n in counts)
    for ids, alive in zip((u, q, i), live):
        assert len(set(ids.tolist()) - set(alive.tolist())) >= 1 and len(set(ids.tolist()) & set(alive.tolist())) >= 1
    y = torch.from_numpy((g.random(B) < 0.3).astype(np.float32))
    batch = tuple(t.to(dev()) for t in (u, q, i, y))
    results, models = {}, {}
    with cosine_setting():
        for compact in (False, True):
            monkeypatch.setattr(layout_mod, 'COMPACT_NODES', '1' if compact else '0')
            ds = dataset_of(w, triples)
            assert bool(getattr(ds.hypergraph.layout, 'compact', False)) == compact
            torch.manual_seed(7)
            models[compact] = build_model(ds, kind, L, order, d)
        models[True].load_state_dict(models[False].state_dict())
        for compact in (False, True):
            results[compact] = step_gradients(models[compact], batch)
    (l0, g0), (l1, g1) = results[False], results[True]
    sd = {k: v.detach().cpu().numpy() for k, v in models[False].state_dict().items()}
    want = cref.model_step(sd, triples, counts, w.bag_words + 1, w.bag_offsets, kind, L, order, u.numpy(), q.numpy(), i.numpy(), y.numpy().astype(np.float64))
    print(f'compact {kind}: loss {l1.item():.7f} plain {l0.item():.7f} float64 {want["loss"]:.7f}')
    assert abs(l1.item() - l0.item()) <= RTOL_SUM * abs(l0.item()) and abs(l1.item() - want['loss']) <= RTOL * abs(want['loss'])
    for k in g0:
        print(f'   {k}: against the plain layout {rel(g1[k], g0[k]):.2e}, float64 {rel(g1[k], want["grads"][k]):.2e}')
        assert rel(g1[k], g0[k]) <= RTOL_SUM and rel(g1[k], want['grads'][k]) <= RTOL and rel(g0[k], want['grads'][k]) <= RTOL, k


# ---------------------------------------------------------------------------------------------
# 5: score_topk(..., cosine=True) against float64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim,n_items,n_pairs', [(64, 257, 5), (36, 31, 40), (128, 7, 3), (150, 333, 21), (7, 90, 9), (624, 300, 70), (625, 300, 70), (1264, 530, 37),
                                                (192, 70001, 97)])
def test_score_topk_cosine_matches_float64(dim, n_items, n_pairs):
    """Row magnitudes over six decades: the cosine ranking differs from the dot product's for every pair (asserted).  Per pair rule (5); the strict comparison must
    apply to at least 80 % of the pairs (the reference's own scores give 86 - 100 %)."""
    from ihgnn_amd import ops
    Uc, Qc = 50, 20
    gen = torch.Generator().manual_seed(dim + n_items)
    feats = torch.randn(Uc + Qc + n_items, dim, generator=gen) / np.sqrt(dim)
    feats *= 10 ** (6 * torch.rand(Uc + Qc + n_items, 1, generator=gen) - 3)
    bias = 0.1 * torch.randn(n_items, generator=gen)
    users = torch.randint(0, Uc, (n_pairs,), generator=gen)
    queries = torch.randint(0, Qc, (n_pairs,), generator=gen)
    k = min(10, n_items)
    items, scores = ops.score_topk(feats.to(dev()), users.to(dev()), queries.to(dev()), Uc, Uc + Qc, bias.to(dev()), 0.5, k, cosine=True)
    items, scores = items.cpu().long(), scores.cpu()
    f64 = feats.double()
    want = cref.all_item_scores(f64, users, queries, Uc, Uc + Qc, bias.double())
    dot = (0.5 * f64[queries + Uc] + 0.5 * f64[users]) @ f64[Uc + Qc:].t() + bias.double()
    strict = 0
    for c in range(n_pairs):
        assert torch.sort(dot[c], descending=True, stable=True).indices[:k].tolist() != torch.sort(want[c], descending=True, stable=True).indices[:k].tolist()
        strict += check_top(items[c], scores[c], want[c], k)
    print(f'dim {dim} items {n_items} pairs {n_pairs}: strict comparison on {strict} of {n_pairs} pairs')
    assert strict >= 0.8 * n_pairs, (strict, n_pairs)


def test_score_topk_cosine_ties_in_ascending_item_order():
    """Six items with identical rows and bias, placed in the top ten of every pair, come out in ascending id; where all six are in the reference's top ten the whole list
    equals the stable descending sort."""
    from ihgnn_amd import ops
    Uc, Qc, Ic, D = 9, 5, 300, 96
    gen = torch.Generator().manual_seed(5)
    feats = torch.randn(Uc + Qc + Ic, D, generator=gen) / 8
    bias = 0.1 * torch.randn(Ic, generator=gen)
    dup = [17, 3, 250, 131, 64, 65]
    feats[Uc + Qc + torch.tensor(dup)] = feats[Uc + Qc + 17] * 3          # (the scale does not move a cosine: the bias puts them in the top ten)
    bias[torch.tensor(dup)] = 2.0
    users, queries = torch.arange(Uc), torch.arange(Uc) % Qc
    items, _ = ops.score_topk(feats.to(dev()), users.to(dev()), queries.to(dev()), Uc, Uc + Qc, bias.to(dev()), 0.5, 10, cosine=True)
    want = cref.all_item_scores(feats.double(), users, queries, Uc, Uc + Qc, bias.double())
    for c in range(Uc):
        got = items[c].tolist()
        tied = [x for x in got if x in dup]
        assert tied == sorted(dup)                                        # all six (bias 2 against cosines within +-1 and biases of 0.1 sigma), in ascending order
        order = torch.sort(want[c], descending=True, stable=True).indices[:10]
        rest = want[c][order][6:]
        if (rest[:-1] - rest[1:]).min().item() > 1e-3:                    # (no near-tie among the other four)
            assert got == order.tolist()


# ---------------------------------------------------------------------------------------------
# 6: the evaluation loop
# ---------------------------------------------------------------------------------------------
def test_evaluation_loop_scores_with_the_cosine_head(tmp_path):
    """``test_and_get_avg_metrics`` with the setting on runs ``_evaluate_batched`` (``score_topk_cosine`` in the profile): its average is the average of the per-log
    metrics of ``top_items``, and those equal per-log ``Metrics.calculate_on_all_items(model(u, q, None), ...)`` under rule (5)."""
    from ihgnn_amd import profiler, synth
    from ihgnn_amd.Dataset import GraphDataset, TestSearchLogDataLoader
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    from ihgnn_amd.Helpers.Metrics import Metrics
    from ihgnn_amd.Helpers.TrainTestHelper import test_and_get_avg_metrics
    w = synth.draw(80, 25, 120, 30, 900, eval_logs=60)
    paths = synth.write_files(w, str(tmp_path))
    ds = GraphDataset(paths['fn_graph_info'], paths['fn_queries_multihot'], paths['fn_train_data'], PpsHyperGraph, 10, 0, dev())
    loader = TestSearchLogDataLoader(paths['fn_test_data'], ds, dev())
    torch.manual_seed(1)
    with cosine_setting():
        m = build_model(ds, 'ihgnn', 2, 3, 32)
        profiler.start()
        _, avg, _ = test_and_get_avg_metrics(m, ds, loader)
        profiler.stop()
        assert 'score_topk_cosine' in profiler.summary() and 'score_topk' not in profiler.summary()
        uq = torch.tensor([(lg[0], lg[1]) for lg in loader.logs], device=dev())
        ours, theirs, every = [], [], []
        with torch.no_grad():
            m.save_features_for_test()
            items, scores = m.top_items(uq[:, 0], uq[:, 1], 10)
            for k, (users, queries, truth, flags, all1) in enumerate(loader):
                dense = m(users, queries, None)
                mine = Metrics.from_top_indices(items[k].tolist(), truth, flags, all1)
                every.append((mine.HitRatio_at10, mine.NDCG_at10, mine.MAP_at10))
                if check_top(items[k].cpu().long(), scores[k].cpu(), dense.cpu().double(), 10):
                    ref_m = Metrics.calculate_on_all_items(dense, truth, flags, all1)
                    ours.append(every[-1])
                    theirs.append((ref_m.HitRatio_at10, ref_m.NDCG_at10, ref_m.MAP_at10))
            m.clear_saved_feature()
    assert len(ours) >= 0.8 * len(loader.logs), (len(ours), len(loader.logs))
    np.testing.assert_allclose(np.mean(ours, 0), np.mean(theirs, 0), atol=1e-9)
    np.testing.assert_allclose([avg.HitRatio_at10, avg.NDCG_at10, avg.MAP_at10], np.mean(every, 0), atol=1e-9)


# ---------------------------------------------------------------------------------------------
# 7 - 9: recorded step, driver, two ranks
# ---------------------------------------------------------------------------------------------
def test_recorded_step_equals_the_eager_step_and_notices_a_flip():
    """A cosine model's step recorded by ``CapturedTrainingStep`` and replayed equals the eager step over four steps (losses 1e-6, parameters 1e-6: the bar of
    ``test_gat_recorded_step_equals_the_eager_step``); the head is baked into the recording - after the setting flips, ``stale()`` says so."""
    from ihgnn_amd import synth
    from ihgnn_amd.captured_step import CapturedTrainingStep
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.optim import Adam
    ds = dataset_of(synth.draw(300, 40, 200, 50, 4000, seed=21, distribution='powerlaw'))
    batches = list(ds.sample_batches(100, 4, seed=5))
    kept_step = []

    def run(recorded):
        torch.manual_seed(7)
        m = build_model(ds, 'ihgnn', 2, 3, 64)
        opt = Adam(m.parameters(), 1e-3, weight_decay=0)
        step = CapturedTrainingStep(m, opt, batches[0][0].shape[0], warmup_batch=batches[0]) if recorded else None
        losses = []
        for u, q, i, y in batches:
            if recorded:
                losses.append(step.step(u, q, i, y).item())
            else:
                loss = m.bce_loss(u, q, i, y)
                loss.backward(); opt.step(); opt.zero_grad()
                losses.append(loss.item())
        kept_step.append(step)
        return losses, {k: v.clone() for k, v in m.state_dict().items()}

    with cosine_setting():
        l0, p0 = run(False)
        l1, p1 = run(True)
        step = kept_step[-1]
        assert not step.stale() and not step.stale(full=True)
        Gs.Prediction.use_cosine_similarity = False
        assert step.stale() and step.stale(full=True)
        with pytest.raises(RuntimeError):
            step.step(*batches[0])
        # the dot-product step on the same model and batches is a different step: the comparison above is not vacuous
        torch.manual_seed(7)
        other = build_model(ds, 'ihgnn', 2, 3, 64).bce_loss(*batches[0]).item()
    np.testing.assert_allclose(l1, l0, rtol=1e-6)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 1e-6, k
    assert abs(other - l0[0]) > 1e-3 * abs(l0[0])


def test_driver_with_the_cosine_flag(tmp_path, monkeypatch):
    """``--cosine`` through the driver: three epochs on a tiny corpus end with finite metrics and a recorded-or-eager decision, the log names the head, and a following
    ``main()`` without the flag scores with the dot product again."""
    from ihgnn_amd import Main as driver, synth
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    w = synth.draw(60, 20, 80, 25, 500, seed=4, eval_logs=30)
    synth.write_files(w, str(tmp_path / 'Data' / 'Synth' / 'Tiny'))
    monkeypatch.chdir(tmp_path)
    old = Gs.Prediction.use_cosine_similarity
    try:
        hist = driver.main(['--ds', 'Synth/Tiny/', '--gnn', 'IHGNN', '--gnns', '2', '--fo', '3', '--emb', '32', '--seed', '3', '--cosine', '--ec', '3', '--est', '2', '--etf', '1'])
        assert Gs.Prediction.use_cosine_similarity is True
        assert [e for e, _ in hist.iter_epoch_test()] == [2, 3]
        for _, metrics in hist.iter_epoch_test():
            assert np.isfinite([metrics.HitRatio_at10, metrics.NDCG_at10, metrics.MAP_at10]).all()
        assert hist.training_step_recorded in (True, False)
        log = open(tmp_path / 'Results' / 'Synth-Tiny-RawGnn-2IHGNNLayer-O3-emb32' / 'train_log.txt', encoding='utf-8').read()
        assert 'head cosine similarity' in log
        driver.main(['--ds', 'Synth/Tiny/', '--gnn', 'IHGNN', '--gnns', '2', '--fo', '3', '--emb', '32', '--seed', '3', '--ec', '1', '--est', '1', '--etf', '1'])
        assert Gs.Prediction.use_cosine_similarity is False
        log = open(tmp_path / 'Results' / 'Synth-Tiny-RawGnn-2IHGNNLayer-O3-emb32' / 'train_log.txt', encoding='utf-8').read()
        assert 'head dot product' in log
    finally:
        Gs.Prediction.use_cosine_similarity = old


def test_two_ranks_exchange_the_cosine_cotangents():
    """``tools/two_rank_check.py --sync cotangent --cosine`` as a child process: two replicas on GPU 0 over gloo exchange the cosine head's row gradients (the layout of the
    dot-product head's: ``distributed.py`` is unchanged), stay bitwise identical and equal the one-rank run on the union batch by the tool's own bar."""
    r = subprocess.run([sys.executable, 'tools/two_rank_check.py', '--ranks', '2', '--sync', 'cotangent', '--backend', 'gloo', '--device', '0', '--cosine'], cwd=REPO,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'OK' in r.stdout and 'DIVERGED' not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
