#!/usr/bin/env python3
"""Generate ``f15_srrl.npz``: the reference's Srrl baseline (CDboyOne/IHGNN, ``Models/Srrl.py``, ``SrrlDataset.py``, ``Helpers/TrainTestHelper.py:160-257``) run on the CPU
as written, on the small workload (F2's), d = 32.

Here-only tooling, like ``make_golden_cosine.py`` (same stubs for ``torch_sparse`` and ``dgl``, written here from their documented semantics): it needs the reference
checkout, is never imported by tests, ``bench.py`` or the product, and contains no reference code.  The reference seeds nothing; every seed below is set by this harness.
The file holds data only.

  sd.*             the model's state dict (``cfg`` = d, the seed used - the first from 1500 on without a near-tie in a test log's top eleven -, negatives)
  paths.<table>.*  ``MetaPaths``' six dictionaries, flattened in dictionary order: ``keys`` [n, 2], ``members`` (flat), ``lens`` [n]
  weights          every positive's subsampling weight
  kg<m>.*          one KG batch per mode m = 0 (tail) / 1 (head) / 2 (query): ``positive`` [B, 3], ``negative`` [B, k], ``weight`` [B], ``tails`` / ``heads`` / ``queries``
                   [B, 1], the scores ``pos`` [B, 1] and ``neg`` [B, k], the ``loss`` and ``grad.<parameter>`` for every parameter the step reaches
  ps.* / ps_nokg.* a PS batch of 64 rows (``u``, ``q``, ``i``, ``flags``) with ``scores``, BCE ``loss``, ``grad.<parameter>``; ``ps`` also ``adam.<parameter>`` after one Adam
                   step (lr 1e-3); ``ps_nokg``: the same batch under ``Gs.Srrl.KG_loss = False``
  test.*           the 12 test logs (``uq``, ``items_flat``, ``items_len``), the reference's all-item scores ``all_scores`` [12, I], HR / NDCG / MAP@10 per log and averaged
  curve.*          24 training steps from the stored parameters (Adam, lr 1e-3): 12 KG steps cycling the modes, then 12 PS steps; every batch as the reference's loaders
                   produced it (``kg<s>.*`` as above without scores, ``ps<s>.u / q / i / flags``) and ``loss`` [24]

    python tests/golden/make_golden_srrl.py            # rewrites tests/golden/f15_srrl.npz
"""
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('IHGNN_REFERENCE') or os.path.join(os.path.dirname(REPO), 'reference')      # the reference checkout: beside this one unless named
sys.dont_write_bytecode = True


def _install_stubs():
    ts = types.ModuleType('torch_sparse')

    class SparseTensor:
        def __init__(self, t):
            self.t = t

        @classmethod
        def from_torch_sparse_coo_tensor(cls, t):
            return cls(t)

        def coalesce(self):
            return SparseTensor(self.t.coalesce())

    ts.SparseTensor = SparseTensor
    ts.matmul = lambda a, b: torch.sparse.mm(a.t, b)
    sys.modules['torch_sparse'] = ts
    dgl = types.ModuleType('dgl')                                        # (imported by the reference's GnnLayers; no GAT layer is built here)
    dgl.graph = lambda *a, **k: None
    dgl.ops = types.SimpleNamespace()
    sys.modules['dgl'] = dgl


_install_stubs()
sys.path.insert(0, REFERENCE)
sys.path.insert(1, REPO)
sys.path.insert(2, os.path.join(REPO, 'tests'))

from torch.utils.data import DataLoader                                 # noqa: E402
from Dataset import GraphDataset, TestSearchLogDataLoader               # noqa: E402  (reference)
from Helpers.Graph import PpsHyperGraph                                 # noqa: E402  (reference)
from Helpers.GlobalSettings import Gs                                   # noqa: E402  (reference)
from Helpers.Metrics import Metrics                                     # noqa: E402  (reference)
from Models.Srrl import Srrl                                            # noqa: E402  (reference)
from SrrlDataset import MetaPaths, OneShotIterator, SrrlDatasetKG       # noqa: E402  (reference)

from ihgnn_amd import synth                                             # noqa: E402  (this repo)
import srrl_reference as sref                                           # noqa: E402  (this repo: the float64 restatement)

CPU = torch.device('cpu')
torch.set_num_threads(4)
D, SEED, NEGATIVES, KG_BATCH, PS_BATCH, CURVE_BATCH = 32, 1500, 10, 48, 64, 32
MODES = ('tail-company-batch', 'head-company-batch', 'query-company-batch')
TABLES = ('positive_heads', 'positive_queries', 'positive_tails', 'negative_heads', 'negative_queries', 'negative_tails')
BAR = 2e-6


def seed_all(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def sd_numpy(module):
    return {k: v.detach().cpu().numpy().copy() for k, v in module.state_dict().items()}


def kg_loaders(meta, batch):
    return [DataLoader(SrrlDatasetKG(meta, NEGATIVES, mode), batch, True, collate_fn=SrrlDatasetKG.collate_fn) for mode in MODES]


def kg_batch_arrays(pre, batch):
    positive, negative, weight, mode, tails, heads, queries = batch
    return {pre + 'positive': positive.numpy(), pre + 'negative': negative.numpy(), pre + 'weight': weight.numpy(), pre + 'tails': tails.numpy(),
            pre + 'heads': heads.numpy(), pre + 'queries': queries.numpy(), pre + 'mode': np.int64(MODES.index(mode))}


def reference_kg_loss(model, batch):
    positive, negative, weight, mode, tails, heads, queries = batch
    neg = model.trainkg((positive, negative, tails, heads, queries), mode=mode, positive_mode=False)
    pos = model.trainkg((positive, tails, heads, queries), mode=mode, positive_mode=True)
    ln, lp = torch.nn.functional.logsigmoid(-neg).mean(dim=1), torch.nn.functional.logsigmoid(pos).squeeze(dim=1)
    loss = (-(weight * lp).sum() / weight.sum() - (weight * ln).sum() / weight.sum()) / 2
    return pos, neg, loss


def clear_ranking(all_scores):
    """No near-tie among the top eleven of any log (gaps above 1e-4 of the score range): the metric comparison must not rest on one."""
    for row in np.asarray(all_scores, np.float64):
        ranked = np.sort(row)[::-1]
        if not (ranked[:10] - ranked[1:11]).min() > 1e-4 * (ranked[0] - ranked[-1]):
            return False
    return True


def main():
    assert Gs.Srrl.KG_loss and not Gs.Srrl.uni_weight and Gs.Srrl.regularization == 0
    w = synth.draw(40, 20, 50, 30, 300, seed=11, eval_logs=12)          # make_golden.small_workload(): tests/golden/f2_small_workload.npz
    pth = synth.write_files(w, '/tmp/ihgnn_golden_small_f15')
    ds = GraphDataset(pth['fn_graph_info'], pth['fn_queries_multihot'], pth['fn_train_data'], PpsHyperGraph, NEGATIVES, 0, CPU)
    bags = (w.bag_words + 1, w.bag_offsets)
    out = {'cfg': np.array([D, SEED, NEGATIVES], np.int64)}

    # the first seed from SEED on whose parameters rank no test log on a near-tie (checked again, on the reference's own scores, below)
    test_pairs = [(a, b) for a, b, _ in w.test_logs]
    for seed in range(SEED, SEED + 50):
        seed_all(seed)
        model = Srrl(ds, D, None, 0.5)
        sd = sd_numpy(model)
        if clear_ranking(sref.all_item_scores(sd, bags, [a for a, _ in test_pairs], [b for _, b in test_pairs]).numpy()):
            break
    else:
        raise AssertionError('no seed without a near-tie')
    out['cfg'] = np.array([D, seed, NEGATIVES], np.int64)
    out.update({'sd.' + k: v for k, v in sd.items()})

    meta = MetaPaths(ds)
    assert [tuple(int(x) for x in t) for t in w.triples.tolist()] == [tuple(t) for t in meta.positive_interactions]
    for name in TABLES:
        table = getattr(meta, name)
        out[f'paths.{name}.keys'] = np.array(list(table.keys()), np.int64).reshape(-1, 2)
        out[f'paths.{name}.members'] = np.array([x for members in table.values() for x in members], np.int64)
        out[f'paths.{name}.lens'] = np.array([len(members) for members in table.values()], np.int64)
    kg_set = SrrlDatasetKG(meta, NEGATIVES, MODES[0])
    out['weights'] = np.array([float(kg_set[n][2]) for n in range(len(kg_set))], np.float32)

    # one KG batch per mode
    seed_all(SEED + 1)
    for m, loader in enumerate(kg_loaders(meta, KG_BATCH)):
        batch = next(iter(loader))
        model.zero_grad(set_to_none=True)
        pos, neg, loss = reference_kg_loss(model, batch)
        loss.backward()
        pre = f'kg{m}.'
        arrays = kg_batch_arrays(pre, batch)
        step = sref.kg_step(sd, bags, batch[0], batch[1], batch[2], batch[4], batch[5], batch[6], batch[3])
        worst = max(sref.rel(pos.detach(), step['pos']), sref.rel(neg.detach(), step['neg']), abs(loss.item() - step['loss']))
        for name, p in model.named_parameters():
            assert (p.grad is None) == (step['grads'][name] is None), name
            if p.grad is not None:
                worst = max(worst, sref.rel(p.grad, step['grads'][name]))
                arrays[pre + 'grad.' + name] = p.grad.numpy().copy()
        assert worst <= BAR, (MODES[m], worst)
        arrays.update({pre + 'pos': pos.detach().numpy(), pre + 'neg': neg.detach().numpy(), pre + 'loss': np.float64(loss.item())})
        out.update(arrays)
        print(f'F15 KG {MODES[m]}: loss {loss.item():.6f}, restatement within {worst:.1e}')

    # one PS batch, with and without the KG rows
    seed_all(SEED + 2)
    u, q, i = torch.randint(0, ds.user_count, (PS_BATCH,)), torch.randint(0, ds.query_count, (PS_BATCH,)), torch.randint(0, ds.item_count, (PS_BATCH,))
    flags = (torch.rand(PS_BATCH) < 0.3).float()
    for pre, kg_on in (('ps.', True), ('ps_nokg.', False)):
        Gs.Srrl.KG_loss = kg_on
        fresh = Srrl(ds, D, None, 0.5)
        fresh.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        opt = torch.optim.Adam(fresh.parameters(), 1e-3, weight_decay=0)
        scores = fresh(u, q, i)
        loss = torch.nn.BCEWithLogitsLoss()(scores, flags)
        loss.backward()
        step = sref.ps_step(sd, bags, u, q, i, flags, kg_on)
        worst = max(sref.rel(scores.detach(), step['scores']), abs(loss.item() - step['loss']))
        grads = {}
        for name, p in fresh.named_parameters():
            assert (p.grad is None) == (step['grads'][name] is None), name
            if p.grad is not None:
                worst = max(worst, sref.rel(p.grad, step['grads'][name]))
                grads[name] = p.grad.numpy().copy()
        assert worst <= BAR, (pre, worst)
        out.update({pre + 'grad.' + k: v for k, v in grads.items()})
        out.update({pre + 'u': u.numpy(), pre + 'q': q.numpy(), pre + 'i': i.numpy(), pre + 'flags': flags.numpy(), pre + 'scores': scores.detach().numpy(),
                    pre + 'loss': np.float64(loss.item())})
        if kg_on:
            opt.step()
            import query_transform_reference as qref
            stepped = sd_numpy(fresh)
            assert max(qref.adam_excess(stepped[n], step['grads'][n], step['adam'][n], BAR) for n in grads) <= 1.0
            out.update({pre + 'adam.' + k: stepped[k] for k in grads})
        print(f'F15 {pre[:-1]}: loss {loss.item():.6f}, restatement within {worst:.1e}')
    Gs.Srrl.KG_loss = True

    # evaluation of the stored parameters over the workload's test logs
    test = TestSearchLogDataLoader(pth['fn_test_data'], ds, CPU)
    total, per_log, all_scores, uq = Metrics(), [], [], []
    with torch.no_grad():
        model.save_features_for_test()
        for users, queries, items, _, all1 in test:
            s = model(users, queries, None)
            mm = Metrics.calculate_on_all_items(s, items, None, all1)
            total.add_to_self(mm)
            per_log.append((mm.HitRatio_at10, mm.NDCG_at10, mm.MAP_at10))
            all_scores.append(s.numpy().copy())
            uq.append((int(users[0]), int(queries[0])))
        model.clear_saved_feature()
    assert len(per_log) == 12 and uq == [(a, b) for a, b, _ in w.test_logs]
    all_scores = np.stack(all_scores)
    assert sref.rel(all_scores, sref.all_item_scores(sd, bags, [a for a, _ in uq], [b for _, b in uq])) <= BAR
    assert clear_ranking(all_scores), 'near-tie in the top eleven: pick another seed'
    avg = total.divide_and_get_new(len(per_log))
    out.update({'test.uq': np.array(uq, np.int64), 'test.items_flat': np.array([x for _, _, it in w.test_logs for x in it], np.int64),
                'test.items_len': np.array([len(it) for _, _, it in w.test_logs], np.int64), 'test.all_scores': all_scores,
                'test.metrics_per_log': np.array(per_log, np.float64), 'test.metrics': np.array([avg.HitRatio_at10, avg.NDCG_at10, avg.MAP_at10], np.float64)})
    print(f'F15 evaluation: HR/NDCG/MAP@10 {out["test.metrics"]}')

    # 24 steps: 12 KG steps cycling the modes, then 12 PS steps
    seed_all(SEED + 3)
    fresh = Srrl(ds, D, None, 0.5)
    fresh.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    opt = torch.optim.Adam(fresh.parameters(), 1e-3, weight_decay=0)
    kg_iterator = OneShotIterator(*kg_loaders(meta, CURVE_BATCH))
    losses = []
    for s in range(12):
        batch = kg_iterator.next()
        out.update(kg_batch_arrays(f'curve.kg{s}.', batch))
        opt.zero_grad()
        _, _, loss = reference_kg_loss(fresh, batch)
        losses.append(loss.item())
        loss.backward()
        opt.step()
    ps_data = DataLoader(ds, CURVE_BATCH, shuffle=True, collate_fn=GraphDataset.collate_fn)
    ps_loader = (batch for _ in range(2) for batch in ps_data)              # (an epoch of the 300 positives is 10 batches: the curve runs into a second one)
    for s in range(12):
        p_u, p_q, p_i, p_f, n_u, n_q, n_i, n_f = next(ps_loader)
        users, queries, items, labels = torch.cat([p_u, n_u]), torch.cat([p_q, n_q]), torch.cat([p_i, n_i]), torch.cat([p_f, n_f]).float()
        out.update({f'curve.ps{s}.u': users.numpy(), f'curve.ps{s}.q': queries.numpy(), f'curve.ps{s}.i': items.numpy(), f'curve.ps{s}.flags': labels.numpy()})
        opt.zero_grad()
        loss = torch.nn.BCEWithLogitsLoss()(fresh(users, queries, items).float(), labels)
        losses.append(loss.item())
        loss.backward()
        opt.step()
    assert np.isfinite(losses).all()
    out['curve.loss'] = np.array(losses, np.float64)
    print('F15 curve:', ' '.join(f'{x:.4f}' for x in losses))

    path = os.path.join(HERE, 'f15_srrl.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 1 << 20, os.path.getsize(path)
    print(f'{os.path.getsize(path):>9d}  f15_srrl.npz')


if __name__ == '__main__':
    main()
