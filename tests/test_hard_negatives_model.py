"""GPU: hard negatives through the model (``RawGnn.hard_negative_loss`` over the fused batch tail, ``ops.hard_negative_loss`` on the module path, the compact layout,
tables read in place, a batch beyond one combine launch, the recorded step, the training loop, the driver).

The yardstick is the step the project already has: the hard-negative step on a pool batch against ``bce_loss`` / ``ranking_loss`` on the batch COMPACTED by the returned
selection (the positives, then every positive's selected candidates in rank order - ``collate_fn``'s layout with k negatives).  Workload and bars are
``tests/test_loss_model.py``'s: 2e-6 on the loss and RTOL = 1e-5 of the reference tensor's largest magnitude on every gradient (the two steps differ in the order their
row gradients are combined and in nothing else).  The selection itself is held to the module path's scores up to that margin: every selected score >= every unselected
score of its group - RTOL max|score|, for every group."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_loss_model import RTOL, RTOL_SUM, build_model, dataset_of, dev, rel, workload

pytestmark = pytest.mark.gpu

KINDS = ('bce', 'bpr', 'softmax')
P, M, K = 40, 24, 10


class setting:
    """``Gs.Prediction.use_cosine_similarity``, ``Gs.Training.loss`` and ``Gs.Training.negative_pool`` for the block, put back after it."""

    def __init__(self, cosine=False, loss='bce', pool=0):
        self.new = (bool(cosine), loss, int(pool))

    def __enter__(self):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        self.old = (Gs.Prediction.use_cosine_similarity, Gs.Training.loss, Gs.Training.negative_pool)
        Gs.Prediction.use_cosine_similarity, Gs.Training.loss, Gs.Training.negative_pool = self.new

    def __exit__(self, *exc):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        Gs.Prediction.use_cosine_similarity, Gs.Training.loss, Gs.Training.negative_pool = self.old


def pool_batch(ds, positives, pool, seed):
    """``(users, queries, items)`` of ``positives`` positives of the corpus followed by ``pool`` distinct random candidates for each (``collate_fn``'s layout)."""
    g = np.random.default_rng(seed)
    pos = ds.pos_triples[g.integers(0, len(ds), positives)]
    cand = np.stack([g.choice(ds.item_count, pool, replace=False) for _ in range(positives)])
    users = np.concatenate([pos[:, 0], np.repeat(pos[:, 0], pool)])
    queries = np.concatenate([pos[:, 1], np.repeat(pos[:, 1], pool)])
    items = np.concatenate([pos[:, 2], cand.reshape(-1)])
    return tuple(torch.from_numpy(a.astype(np.int64)).to(dev()) for a in (users, queries, items))


def compacted(batch, positives, selected):
    """The batch cut down to the positives and every positive's selected candidates, rank order; and its labels."""
    keep = selected.shape[1]
    out = tuple(torch.cat([t[:positives], t[positives:].view(positives, -1).gather(1, selected).reshape(-1)]) for t in batch)
    labels = torch.cat([torch.ones(positives), torch.zeros(positives * keep)]).to(dev())
    return out, labels


def gradients(m, loss):
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def hard_step(m, batch, positives, keep, kind=None):
    m.zero_grad(set_to_none=True)
    loss, selected = m.hard_negative_loss(*batch, positives, keep, kind, return_selected=True)
    assert selected.dtype == torch.int64 and not selected.requires_grad and tuple(selected.shape) == (positives, keep)
    return gradients(m, loss) + (selected,)


def plain_step(m, batch, labels, positives, kind):
    """The step as it was before hard negatives, on a batch with k negatives per positive."""
    m.zero_grad(set_to_none=True)
    return gradients(m, m.bce_loss(*batch, labels) if kind == 'bce' else m.ranking_loss(*batch, positives, kind))


def assert_selection_within_margin(m, batch, positives, selected):
    with torch.no_grad():
        scores = m(*batch)
    cand = scores[positives:].view(positives, -1)
    chosen = torch.zeros_like(cand, dtype=torch.bool).scatter_(1, selected, True)
    assert bool((chosen.sum(1) == selected.shape[1]).all())                       # distinct positions, in every group
    margin = RTOL * float(scores.abs().max())
    worst_in = torch.where(chosen, cand, torch.full_like(cand, float('inf'))).min(1).values
    best_out = torch.where(chosen, torch.full_like(cand, float('-inf')), cand).max(1).values
    assert bool((worst_in >= best_out - margin).all()), float((best_out - worst_in).max())
    picked = cand.gather(1, selected)
    assert bool((picked[:, :-1] >= picked[:, 1:] - margin).all())                 # best first


def assert_same_step(hard, plain, what, loss_bar=2e-6, grad_bar=RTOL):
    (l0, g0), (l1, g1) = hard, plain
    assert abs(l0.item() - l1.item()) <= loss_bar * abs(l1.item()), (what, l0.item(), l1.item())
    for name in g1:
        assert rel(g0[name], g1[name]) <= grad_bar, (what, name, rel(g0[name], g1[name]))


# ---------------------------------------------------------------------------------------------
# the hard-negative step is the existing step on the compacted batch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cosine', [False, True])
@pytest.mark.parametrize('gnn', ['ihgnn', 'hgcn', 'gcn', 'gat'])
def test_fused_step_equals_the_plain_step_on_the_compacted_batch(gnn, cosine, kind):
    from ihgnn_amd import ops, profiler
    ds = dataset_of(workload(), pairwise=gnn in ('gcn', 'gat'))
    batch = pool_batch(ds, P, M, seed=9)
    torch.manual_seed(11)
    with setting(cosine=cosine):
        m = build_model(ds, gnn)
        assert m.supports_fused_tail()
        profiler.start()
        try:
            l0, g0, selected = hard_step(m, batch, P, K, kind)
        finally:
            profiler.stop()
        assert ('hem_cosine_fwd' if cosine else 'hem_score_fwd') in profiler.summary()
        assert_selection_within_margin(m, batch, P, selected)
        small, labels = compacted(batch, P, selected)
        plain = plain_step(m, small, labels, P, kind)
        assert_same_step((l0, g0), plain, (gnn, cosine, kind))
        # the module route: the same launch on the model's own scores.  Its selection is held to the same margin and its step to the plain step on ITS compaction;
        # where both routes select alike (their scores differ in rounding at most: only a near-tie at the k-th place could part them) the two steps are compared directly
        m.zero_grad(set_to_none=True)
        loss, again = ops.hard_negative_loss(m(*batch), P, K, kind, return_selected=True)
        l1, g1 = gradients(m, loss)
        assert_selection_within_margin(m, batch, P, again)
        if torch.equal(again, selected):
            assert_same_step((l0, g0), (l1, g1), (gnn, cosine, kind, 'module route'))
        else:
            small, labels = compacted(batch, P, again)
            plain = plain_step(m, small, labels, P, kind)
        assert_same_step((l1, g1), plain, (gnn, cosine, kind, 'module route against the plain step'))
        with setting(cosine=cosine, loss=kind):                                    # kind=None reads the setting at the call: the same step
            l2, g2, selected2 = hard_step(m, batch, P, K)
        assert torch.equal(l0, l2) and torch.equal(selected, selected2)
        for name in g0:
            assert torch.equal(g0[name], g2[name]), name
    print(f'{gnn} cosine={cosine} {kind}: loss {l0.item():.7f}')


@pytest.mark.parametrize('kind', KINDS)
def test_compact_layout_with_isolated_batch_nodes(kind, monkeypatch):
    """Two thirds of every node type in no hyperedge; the batch names isolated users, queries and items.  Under ``IHG_COMPACT_NODES=1`` the hard-negative step equals the
    plain step on the compacted batch, and the every-node-a-row layout's hard-negative step to RTOL_SUM where both select alike."""
    from ihgnn_amd import layout as layout_mod
    w = workload()
    g = np.random.default_rng(4)
    counts = (w.user_count, w.query_count, w.item_count)
    live = [g.choice(n, n // 3, replace=False) for n in counts]
    triples = np.stack([g.choice(live[k], 400) for k in range(3)], 1)
    positives, pool, keep = 30, 12, 3
    pu, pq = (g.integers(0, n, positives) for n in counts[:2])
    u, q = (torch.from_numpy(np.concatenate([p, np.repeat(p, pool)])) for p in (pu, pq))
    i = torch.from_numpy(np.concatenate([g.integers(0, counts[2], positives)] + [g.choice(counts[2], pool, replace=False) for _ in range(positives)]))
    for ids, alive in zip((u, q, i), live):
        assert len(set(ids.tolist()) - set(alive.tolist())) >= 1 and len(set(ids.tolist()) & set(alive.tolist())) >= 1
    batch = tuple(t.to(dev()) for t in (u, q, i))
    models = {}
    for compact in (False, True):
        monkeypatch.setattr(layout_mod, 'COMPACT_NODES', '1' if compact else '0')
        ds = dataset_of(w, triples)
        assert bool(getattr(ds.hypergraph.layout, 'compact', False)) == compact
        torch.manual_seed(7)
        models[compact] = build_model(ds, 'ihgnn')
    models[True].load_state_dict(models[False].state_dict())
    l0, g0, s0 = hard_step(models[False], batch, positives, keep, kind)
    l1, g1, s1 = hard_step(models[True], batch, positives, keep, kind)
    assert_selection_within_margin(models[True], batch, positives, s1)
    small, labels = compacted(batch, positives, s1)
    assert_same_step((l1, g1), plain_step(models[True], small, labels, positives, kind), ('compact', kind))
    with torch.no_grad():                                                        # no gradient wanted: the plain tail on the public matrices, the same loss
        quiet = models[True].hard_negative_loss(*batch, positives, keep, kind)
    assert abs(quiet.item() - l1.item()) <= RTOL_SUM * abs(l1.item())
    if torch.equal(s0, s1):
        assert_same_step((l1, g1), (l0, g0), ('compact against plain layout', kind), RTOL_SUM, RTOL_SUM)


@pytest.mark.parametrize('kind', KINDS)
def test_tables_in_place_and_batch_rows_only(kind):
    from ihgnn_amd import ops
    ds = dataset_of(workload())
    batch = pool_batch(ds, P, M, seed=9)
    torch.manual_seed(11)
    m = build_model(ds, 'ihgnn', d=64)
    for tables, rows_only in ((True, True), (False, True), (True, False)):
        ops.NODE_TABLES, m.batch_rows_only_last_layer = tables, rows_only
        try:
            l0, g0, selected = hard_step(m, batch, P, K, kind)
            small, labels = compacted(batch, P, selected)
            plain = plain_step(m, small, labels, P, kind)
        finally:
            ops.NODE_TABLES, m.batch_rows_only_last_layer = True, True
        assert_selection_within_margin(m, batch, P, selected)
        assert_same_step((l0, g0), plain, (tables, rows_only, kind))


@pytest.mark.parametrize('kind', ['bce', 'bpr'])
def test_a_batch_beyond_one_combine_launch(kind):
    """P = 43, M = 256: 3 P (1 + M) = 33,153 row gradients, just above the 32,768 of one combine launch - the step runs on the chunked scatter paths."""
    from ihgnn_amd import ops
    positives, pool = 43, 256
    assert 3 * positives * (1 + pool) > ops.SCATTER_CHUNK_ROWS >= 3 * (positives - 1) * (1 + pool)
    from ihgnn_amd import synth
    ds = dataset_of(synth.draw(60, 20, 300, 25, 500))                             # (test_loss_model's workload with a catalogue that holds a pool of 256)
    batch = pool_batch(ds, positives, pool, seed=3)
    torch.manual_seed(11)
    m = build_model(ds, 'ihgnn')
    l0, g0, selected = hard_step(m, batch, positives, K, kind)
    assert_selection_within_margin(m, batch, positives, selected)
    small, labels = compacted(batch, positives, selected)
    assert_same_step((l0, g0), plain_step(m, small, labels, positives, kind), (kind, 'chunked'))


# ---------------------------------------------------------------------------------------------
# recorded step
# ---------------------------------------------------------------------------------------------
def test_recorded_step_equals_the_eager_step_and_notices_a_flip():
    """Four replays of a step recorded under a pool equal four eager hard-negative steps bit for bit, in the loss and in every parameter; pool and kept count are baked
    into the recording - after either flips, ``stale()`` says so and ``step()`` refuses."""
    from ihgnn_amd import synth
    from ihgnn_amd.captured_step import CapturedTrainingStep
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.optim import Adam
    ds = dataset_of(synth.draw(300, 40, 200, 50, 4000, seed=21, distribution='powerlaw'))
    positives, pool = 100, 20
    batches = [pool_batch(ds, positives, pool, seed=s) for s in range(4)]
    labels = torch.zeros(positives * (1 + pool), device=dev())
    kept_step = []

    def run(recorded):
        torch.manual_seed(7)
        m = build_model(ds, 'ihgnn', d=64)
        opt = Adam(m.parameters(), 1e-3, weight_decay=0)
        step = CapturedTrainingStep(m, opt, positives * (1 + pool), warmup_batch=batches[0] + (labels,), positives=positives) if recorded else None
        losses = []
        for u, q, i in batches:
            if recorded:
                losses.append(step.step(u, q, i, labels, positives=positives).clone())
            else:
                loss = m.hard_negative_loss(u, q, i, positives, Gs.random_negative_sample_size)
                loss.backward(); opt.step(); opt.zero_grad()
                losses.append(loss.detach().clone())
        kept_step.append(step)
        return losses, {k: v.clone() for k, v in m.state_dict().items()}

    with setting(loss='bpr', pool=pool):
        l0, p0 = run(False)
        l1, p1 = run(True)
        step = kept_step[-1]
        assert step.pool == pool and step.keep == Gs.random_negative_sample_size
        assert not step.stale() and not step.stale(full=True)
        with pytest.raises(ValueError, match='positives'):
            step.step(*batches[0], labels, positives=50)
        Gs.Training.negative_pool = 0
        assert step.stale() and step.stale(full=True)
        with pytest.raises(RuntimeError, match='baked into the recording'):
            step.step(*batches[0], labels)
        Gs.Training.negative_pool = pool + 1
        assert step.stale()
        Gs.Training.negative_pool = pool
        assert not step.stale()
        old = Gs.random_negative_sample_size
        Gs.random_negative_sample_size = old - 1
        try:
            assert step.stale()
        finally:
            Gs.random_negative_sample_size = old
        # the plain bpr step on the first ten candidates is a different step: the comparison below is not vacuous
        torch.manual_seed(7)
        first_ten = torch.arange(10, device=dev()).expand(positives, 10)
        other = build_model(ds, 'ihgnn', d=64).ranking_loss(*compacted(batches[0], positives, first_ten)[0], positives, 'bpr').item()
    print(f'eager losses {[x.item() for x in l0]}, replayed {[x.item() for x in l1]}')
    for a, b in zip(l0, l1):
        assert torch.equal(a, b)
    for name in p0:
        assert torch.equal(p1[name], p0[name]), name
    assert abs(other - l0[0].item()) > 1e-3 * abs(l0[0].item())


# ---------------------------------------------------------------------------------------------
# the training loop, the device loader
# ---------------------------------------------------------------------------------------------
def test_training_loop_takes_the_hard_negative_step(monkeypatch):
    """``train_and_get_avg_loss`` under ``Gs.Training.negative_pool``: the fused step where the fused tail runs (``model.training_loss`` is called under the hard-negative
    objective and no other; the per-objective methods are not the loop's route), the module path with ``ops.objective_loss`` where it does not, and the same average
    loss either way to 1e-4."""
    from torch.utils.data import DataLoader
    from ihgnn_amd import _lib, ops
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Helpers.ProcessController import ProcessController
    from ihgnn_amd.Helpers.TrainTestHelper import train_and_get_avg_loss
    from ihgnn_amd.Models import RawGnn
    from ihgnn_amd.optim import Adam
    import random
    ds = dataset_of(workload())
    ds.rand_neg_sample_size = M                                                  # (Main builds the dataset with the pool size)
    calls = {'hard': 0, 'other': 0, 'op': 0}                                      # calls of model.training_loss, of a per-objective method, of ops.objective_loss
    seen = []                                                                    # the objective of every one of them
    real_loss, real_op = RawGnn.training_loss, ops.objective_loss

    def model_loss(self, users, queries, items, objective, *a, **k):
        calls['hard'] += 1
        seen.append(objective)
        return real_loss(self, users, queries, items, objective, *a, **k)

    def op_loss(scores, objective, *a, **k):
        calls['op'] += 1
        seen.append(objective)
        return real_op(scores, objective, *a, **k)

    monkeypatch.setattr(RawGnn, 'training_loss', model_loss)
    monkeypatch.setattr(ops, 'objective_loss', op_loss)
    for name in ('bce_loss', 'ranking_loss', 'hard_negative_loss'):
        monkeypatch.setattr(RawGnn, name, lambda self, *a, **k: calls.__setitem__('other', calls['other'] + 1))
    averages = []
    with setting(loss='bce', pool=M):
        for fused in (True, False):
            random.seed(3); torch.manual_seed(3)
            m = build_model(ds, 'ihgnn')
            if not fused:
                monkeypatch.setattr(m, 'supports_fused_tail', lambda: False, raising=False)
            opt = Adam(m.parameters(), 1e-3, weight_decay=0)
            loader = DataLoader(ds, 100, shuffle=False, collate_fn=GraphDataset.collate_fn)
            pc = ProcessController(1, 1, 10, 10, None, None)
            next(iter(pc))
            avg, _ = train_and_get_avg_loss(m, opt, torch.nn.BCEWithLogitsLoss(), ds, loader, pc, dev(), record_step='off')
            averages.append(avg)
            assert calls['other'] == 0 and len(loader) >= 4 and (calls['hard'] == len(loader) and calls['op'] == 0 if fused else calls['op'] == len(loader)), calls
            # no other objective ran: every step's is the BCE over 100 positives and the best ten of their 24 candidates each
            keep = Gs.random_negative_sample_size
            assert len(seen) == len(loader) and all((o.kind, o.positives, o.pool, o.keep) == (_lib.HARD_NEGATIVE_KINDS['bce'], 100, M, keep) for o in seen), [o.key() for o in seen]
            calls.update(hard=0, op=0)
            seen.clear()
        ds.rand_neg_sample_size = 10                                             # a loader that draws no pool is refused, not trained on
        with pytest.raises(ValueError, match='negative_pool'):
            train_and_get_avg_loss(m, opt, torch.nn.BCEWithLogitsLoss(), ds, loader, pc, dev(), record_step='off')
    # (not a parity bar - the routes are held to one above: the same batches through both routes train alike)
    assert np.isfinite(averages).all() and abs(averages[0] - averages[1]) <= 1e-4 * abs(averages[1]), averages


def test_device_batches_draw_a_pool_from_the_pool_kernel():
    """More than 16 negatives per positive come from ``ihg_sample_pool`` with the seed and counter ``ihg_sample_negatives`` gets: the batch's items are the reference
    stream's, and up to 16 the batches keep their bits."""
    import hard_negatives_reference as H
    import logged_negatives_reference as L
    from ihgnn_amd.Dataset import DeviceBatchLoader
    ds = dataset_of(workload())
    for k, draw in ((40, H.pool_draw), (16, L.sample_negatives)):
        ds.rand_neg_sample_size = k
        loader = DeviceBatchLoader(ds, 100, seed=2)
        loader.set_epoch(3)
        for b, (p_u, p_q, p_i, p_f, n_u, n_q, n_i, n_f) in enumerate(loader):
            n = int(p_u.shape[0])
            want = draw(2 * 7919, (3 << 32) + b, n, ds.item_count, k)
            assert torch.equal(n_i.cpu().view(n, k), torch.from_numpy(want.copy())), (k, b)
            assert torch.equal(n_u, p_u.repeat_interleave(k)) and torch.equal(n_q, p_q.repeat_interleave(k)) and int(n_f.sum()) == 0
            if b == 1:
                break


# ---------------------------------------------------------------------------------------------
# the driver (child processes, each under its own time limit)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loader', ['device_sampling', 'dataloader'])
def test_driver_trains_on_hard_negatives(loader, tmp_path):
    """``python -m ihgnn_amd.Main ... --hard_negatives 40 --loss bpr`` in a child process, batches drawn on the device (M > 16: the pool kernel) or by the ``DataLoader``:
    two epochs on a tiny corpus; the log names pool and kept counts, the average loss is finite and decreases, metrics are written."""
    from ihgnn_amd import synth
    w = synth.draw(60, 20, 80, 25, 2000, seed=4, eval_logs=30)
    synth.write_files(w, str(tmp_path / 'Data' / 'Synth' / 'Tiny'))
    command = [sys.executable, '-m', 'ihgnn_amd.Main', '--ds', 'Synth/Tiny/', '--gnn', 'IHGNN', '--gnns', '2', '--fo', '3', '--emb', '32', '--seed', '3', '--loss', 'bpr',
               '--hard_negatives', '40', '--ec', '2', '--est', '1', '--etf', '1', '--sm'] + (['--device_sampling'] if loader == 'device_sampling' else [])
    r = subprocess.run(command, cwd=str(tmp_path), capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', '')))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / 'Results' / 'Synth-Tiny-RawGnn-2IHGNNLayer-O3-emb32'
    logs = [f for f in os.listdir(out) if f.endswith('_train_log.txt')]
    metrics = [f for f in os.listdir(out) if f.endswith('_metrics.txt')]
    assert len(logs) == 1 and len(metrics) == 1
    log = open(out / logs[0], encoding='utf-8').read()
    assert '| loss bpr |' in log and 'hard negatives: the best 10 of a pool of 40' in log
    losses = [float(x) for x in re.findall(r'average loss \S*?(\d+\.\d+)', log)]
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[1] < losses[0], losses
    text = open(out / metrics[0], encoding='utf-8').read()
    assert 'Epoch 1 Avg loss' in text and 'Epoch 2 Avg loss' in text and 'Best' in text
