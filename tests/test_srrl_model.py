"""The HIP Srrl model against fixture F15 (the reference's model on the CPU, ``tests/golden/f15_srrl.npz``): PS and KG batches (scores, loss, every gradient, the Adam
step), both sides of ``Gs.Srrl.KG_loss``, the all-item scores, ``top_items`` and the metrics of the 12 test logs, the 24-step training curve replayed through the
training loop's step functions, and a driver run in a child process.  Bars: the project's 1e-5 (largest deviation relative to the reference's largest magnitude),
the metrics within 0.002 and the curve within 1e-4 (F10's bars)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import query_transform_reference as qref
import srrl_reference as sref
from conftest import GOLDEN, REPO
from ihgnn_amd import synth

pytestmark = pytest.mark.gpu

BAR = 1e-5
MODES = ('tail-company-batch', 'head-company-batch', 'query-company-batch')


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def f15():
    return np.load(os.path.join(GOLDEN, 'f15_srrl.npz'))


@pytest.fixture(scope='module')
def workload():
    return synth.draw(40, 20, 50, 30, 300, seed=11, eval_logs=12)


@pytest.fixture()
def kg_setting():
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    old = (Gs.Srrl.KG_loss, Gs.Srrl.uni_weight, Gs.Srrl.regularization)
    yield Gs
    Gs.Srrl.KG_loss, Gs.Srrl.uni_weight, Gs.Srrl.regularization = old


def state(z):
    return {k[3:]: z[k] for k in z.files if k.startswith('sd.')}


def build(w, z):
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Models import Srrl
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev())
    model = Srrl(ds, 32, None, 0.5).to(dev())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state(z).items()})
    return ds, model


def rel(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    return sref.rel(got, want)


def cuda(a):
    return torch.from_numpy(np.asarray(a)).to(dev())


def kg_batch(z, pre):
    return (cuda(z[pre + 'positive']), cuda(z[pre + 'negative']), cuda(z[pre + 'weight']), MODES[int(z[pre + 'mode'])], cuda(z[pre + 'tails']), cuda(z[pre + 'heads']),
            cuda(z[pre + 'queries']))


@pytest.mark.parametrize('kg_on', (True, False))
def test_ps_batch_scores_loss_gradients_and_adam_step(f15, workload, kg_setting, kg_on):
    from ihgnn_amd.optim import Adam
    kg_setting.Srrl.KG_loss = kg_on
    pre = 'ps.' if kg_on else 'ps_nokg.'
    _, model = build(workload, f15)
    opt = Adam(model.parameters(), 1e-3, weight_decay=0)
    u, q, i, flags = (cuda(f15[pre + n]) for n in ('u', 'q', 'i', 'flags'))
    scores = model(u, q, i)
    assert rel(scores, f15[pre + 'scores']) <= BAR
    model.zero_grad(set_to_none=True)
    loss = model.bce_loss(u, q, i, flags)
    assert abs(float(loss.detach()) - float(f15[pre + 'loss'])) <= BAR
    loss.backward()
    reached = {k[len(pre) + 5:] for k in f15.files if k.startswith(pre + 'grad.')}
    assert {n for n, p in model.named_parameters() if p.grad is not None} == reached
    for name, p in model.named_parameters():
        if name in reached:
            assert rel(p.grad, f15[pre + 'grad.' + name]) <= BAR, name
    if kg_on:
        step = sref.ps_step(state(f15), (workload.bag_words + 1, workload.bag_offsets), f15[pre + 'u'], f15[pre + 'q'], f15[pre + 'i'], f15[pre + 'flags'], True)
        opt.step()
        for name, p in model.named_parameters():
            if name in reached:
                assert qref.adam_excess(p, step['grads'][name], step['adam'][name], BAR) <= 1.0, name
            else:
                assert np.array_equal(p.detach().cpu().numpy(), state(f15)[name]), name   # a parameter the step does not reach stays


@pytest.mark.parametrize('m', (0, 1, 2))
def test_kg_batch_scores_loss_and_gradients(f15, workload, kg_setting, m):
    from ihgnn_amd import ops
    _, model = build(workload, f15)
    pre = f'kg{m}.'
    positive, negative, weight, mode, tails, heads, queries = kg_batch(f15, pre)
    neg = model.trainkg((positive, negative, tails, heads, queries), mode=mode, positive_mode=False)
    pos = model.trainkg((positive, tails, heads, queries), mode=mode, positive_mode=True)
    assert tuple(pos.shape) == f15[pre + 'pos'].shape and tuple(neg.shape) == f15[pre + 'neg'].shape
    assert rel(pos, f15[pre + 'pos']) <= BAR and rel(neg, f15[pre + 'neg']) <= BAR
    loss = ops.kg_loss(pos.view(-1), neg, weight)
    assert abs(float(loss.detach()) - float(f15[pre + 'loss'])) <= BAR
    loss.backward()
    reached = {k[len(pre) + 5:] for k in f15.files if k.startswith(pre + 'grad.')}
    assert {n for n, p in model.named_parameters() if p.grad is not None} == reached
    for name, p in model.named_parameters():
        if name in reached:
            assert rel(p.grad, f15[pre + 'grad.' + name]) <= BAR, (mode, name)
    # the uniform weighting: against float64
    model.zero_grad(set_to_none=True)
    uniform = ops.kg_loss(model.trainkg((positive, tails, heads, queries), mode=mode, positive_mode=True).view(-1),
                          model.trainkg((positive, negative, tails, heads, queries), mode=mode, positive_mode=False), None)
    want = sref.kg_step(state(f15), (workload.bag_words + 1, workload.bag_offsets), f15[pre + 'positive'], f15[pre + 'negative'], f15[pre + 'weight'], f15[pre + 'tails'],
                        f15[pre + 'heads'], f15[pre + 'queries'], mode, uni_weight=True)
    assert abs(float(uniform.detach()) - want['loss']) <= BAR


def test_all_item_scores_top_items_and_metrics(f15, workload, kg_setting):
    from ihgnn_amd.Helpers.Metrics import Metrics
    ds, model = build(workload, f15)
    uq = f15['test.uq']
    lens = f15['test.items_len']
    starts = np.concatenate([[0], np.cumsum(lens)])
    users, queries = cuda(uq[:, 0]), cuda(uq[:, 1])
    with torch.no_grad():
        model.save_features_for_test()
        try:
            # the generic loop's contract: one pair against all items
            rows = torch.stack([model(users[c:c + 1].expand(ds.item_count), queries[c:c + 1].expand(ds.item_count), None) for c in range(len(uq))])
            top, top_scores = model.top_items(users, queries, 10)
            deep = model.top_items(users, queries, ds.item_count)[0]
        finally:
            model.clear_saved_feature()
    assert rel(rows, f15['test.all_scores']) <= BAR
    want_items, want_scores = sref.topk(rows.cpu().numpy(), 10)
    assert np.array_equal(top.cpu().numpy(), want_items) and np.array_equal(top_scores.cpu().numpy().astype(np.float64), want_scores)
    assert np.array_equal(top.cpu().numpy(), sref.topk(f15['test.all_scores'], 10)[0])           # (no near-tie in the fixture's top eleven)
    assert np.array_equal(np.sort(deep.cpu().numpy(), axis=1), np.tile(np.arange(ds.item_count), (len(uq), 1)))
    per_log = []
    for c, row in enumerate(top.cpu().tolist()):
        m = Metrics.from_top_indices(row, f15['test.items_flat'][starts[c]:starts[c + 1]].tolist(), None, True)
        per_log.append((m.HitRatio_at10, m.NDCG_at10, m.MAP_at10))
    assert np.abs(np.array(per_log) - f15['test.metrics_per_log']).max() <= 0.002
    assert np.abs(np.array(per_log).mean(0) - f15['test.metrics']).max() <= 0.002
    with pytest.raises(RuntimeError, match='save_features_for_test'):
        model.top_items(users, queries, 10)


def test_top_items_chunks_give_the_same_ranking(f15, workload, kg_setting, monkeypatch):
    srrl_module = sys.modules['ihgnn_amd.Models.Srrl']
    ds, model = build(workload, f15)
    users, queries = cuda(f15['test.uq'][:, 0]), cuda(f15['test.uq'][:, 1])
    with torch.no_grad():
        model.save_features_for_test()
        whole = model.top_items(users, queries, 10)
        assert model.evaluation_chunk_pairs(ds.item_count) >= 12            # one chunk
        row_bytes = 4 * (2 * 32 + 32 + 2 * 32 + 1) + 2 * 4 + 8              # hidden and output rows of ps_mlp_ui and ps_mlp_pred, their two inverse norms, the item index
        monkeypatch.setattr(srrl_module, 'EVALUATION_TEMPORARY_BYTES', 5 * row_bytes * ds.item_count)
        assert model.evaluation_chunk_pairs(ds.item_count) == 5             # 12 pairs in chunks of 5, 5 and 2
        parts = model.top_items(users, queries, 10)
        model.clear_saved_feature()
    assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])


def test_training_curve_replayed_from_the_stored_batches(f15, workload, kg_setting):
    """The 24 steps of F15 - 12 KG steps cycling the modes, 12 PS steps - through the training loop's own step functions, from the stored batches."""
    from ihgnn_amd.Helpers.TrainTestHelper import srrl_kg_step, srrl_ps_step
    from ihgnn_amd.optim import Adam
    _, model = build(workload, f15)
    opt = Adam(model.parameters(), 1e-3, weight_decay=0)
    losses = []
    for s in range(12):
        batch = kg_batch(f15, f'curve.kg{s}.')
        assert batch[3] == MODES[s % 3]
        losses.append(float(srrl_kg_step(model, opt, tuple(t.cpu() if torch.is_tensor(t) else t for t in batch), dev())))
    for s in range(12):
        u, q, i, flags = (torch.from_numpy(f15[f'curve.ps{s}.{n}']) for n in ('u', 'q', 'i', 'flags'))
        empty = torch.zeros(0, dtype=torch.long)
        losses.append(float(srrl_ps_step(model, opt, (u, q, i, flags, empty, empty, empty, torch.zeros(0)), dev())))
    deviation = np.abs(np.array(losses) - f15['curve.loss'])
    print('curve deviation per step:', ' '.join(f'{d:.1e}' for d in deviation))
    assert deviation.max() <= 1e-4


def test_driver_trains_and_evaluates_in_a_child_process(tmp_path):
    """``python -m ihgnn_amd.Main --model Srrl`` on a written dataset: two epochs, one evaluation, finite losses and metrics in the log."""
    import re
    w = synth.draw(60, 20, 80, 25, 501, seed=4, eval_logs=30)
    synth.write_files(w, str(tmp_path / 'Data' / 'Synth' / 'Tiny'))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    proc = subprocess.run([sys.executable, '-m', 'ihgnn_amd.Main', '--model', 'Srrl', '--ds', 'Synth/Tiny/', '--emb', '32', '--ec', '2', '--est', '2', '--etf', '1', '--seed', '5'],
                          cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    result_dir = tmp_path / 'Results' / 'Synth-Tiny-Srrl-emb32'
    log = open(result_dir / 'train_log.txt', encoding='utf-8').read()
    kg = [float(x) for x in re.findall(r'avg loss  KG->  ([0-9.naninf-]+)', log)]
    ps = [float(x) for x in re.findall(r'avg loss ([0-9.naninf-]+)  <-PS', log)]
    assert len(kg) == 2 and len(ps) == 2 and np.isfinite(kg + ps).all()
    assert 'usable search logs' in log and 'model Srrl' in log
    assert len(re.findall(r'evaluation done in', log)) == 2             # the test set and the validation set, once
    shown = re.findall(r'(\d\.\d{4})\s+(\d\.\d{4})\s+(\d\.\d{4})', log)      # HR@10 NDCG@10 MAP@10 rows (Metrics.to_string)
    assert len(shown) >= 2 and all(0.0 <= float(v) <= 1.0 for row in shown for v in row)
