#!/usr/bin/env python3
"""Generate ``f14_cosine.npz``: the reference (CDboyOne/IHGNN) run on CPU with ``Gs.Prediction.use_cosine_similarity = True`` - the HEM head scores
``torch.cosine_similarity(item_feature, m_uq) + items_bias`` (``Models/PredictionLayers.py:38-40``).

Here-only tooling, like ``make_golden_query_transform.py`` (same stubs for ``torch_sparse`` and ``dgl``, written here from their documented semantics): it needs the
reference checkout, is never imported by tests, ``bench.py`` or the product, and contains no reference code.  The reference seeds nothing; every seed below is set by
this harness, and the parameters themselves are stored.  The file holds data only.

  head.*           ``HemPredictionLayer.forward`` on stored random inputs (70 rows of width 96; row magnitudes over two decades, one zero item row and one of norm
                   2e-9): user / query / item features, item indices, the bias, the scores
  <case>.*         whole ``RawGnn`` models on the small workload (F2's) - IHGNN order 3 x 2 layers d = 32, HGCN x 2 layers d = 64: parameters (by the seed in ``.cfg``),
                   a batch, scores, BCE loss, every parameter gradient, the parameters after one Adam step (lr 1e-3).  A gradient or stepped parameter of more than
                   1024 elements is kept in the manner of F13: every 8th row (``.rows8``) and the float64 row and column sums (``.rowsum`` / ``.colsum``); smaller ones
                   whole (``.full``).  For the workload's 12 test logs (``test.uq`` / ``test.items_flat`` / ``test.items_len``): the reference's all-item scores of the
                   initial parameters (``.all_scores`` [12, I]), its HR / NDCG / MAP@10 per log (``.metrics_per_log``) and their average (``.metrics``).

    python tests/golden/make_golden_cosine.py            # rewrites tests/golden/f14_cosine.npz
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

from Dataset import GraphDataset, TestSearchLogDataLoader               # noqa: E402  (reference)
from Helpers.Graph import PpsHyperGraph                                 # noqa: E402  (reference)
from Helpers.GlobalSettings import Gs                                   # noqa: E402  (reference)
from Helpers.Metrics import Metrics                                     # noqa: E402  (reference)
from Models import RawGnn, IHGNNLayer, HGCNLayer, HemPredictionLayer    # noqa: E402  (reference)

from ihgnn_amd import synth                                             # noqa: E402  (this repo)
import cosine_reference as cref                                         # noqa: E402  (this repo: the float64 restatement)

CPU = torch.device('cpu')
torch.set_num_threads(4)
# (tag, layer kind, layers, order, d, seed)
MODEL_CASES = (('ihgnn_o3_d32', 'ihgnn', 2, 3, 32, 1435), ('hgcn_d64', 'hgcn', 2, 1, 64, 1465))
BATCH = 64


def seed_all(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def sd_numpy(module):
    return {k: v.detach().cpu().numpy().copy() for k, v in module.state_dict().items()}


def kept(prefix, value):
    """A tensor as the fixture keeps it (the module docstring): whole, or every 8th row + row / column sums."""
    v = np.asarray(value)
    if v.size <= 1024 or v.ndim != 2:
        return {prefix + '.full': v}
    return {prefix + '.rows8': v[::8].copy(), prefix + '.rowsum': v.astype(np.float64).sum(1), prefix + '.colsum': v.astype(np.float64).sum(0)}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))


def small_dataset():
    w = synth.draw(40, 20, 50, 30, 300, seed=11, eval_logs=12)          # make_golden.small_workload(): tests/golden/f2_small_workload.npz
    pth = synth.write_files(w, '/tmp/ihgnn_golden_small_f14')
    return w, pth, GraphDataset(pth['fn_graph_info'], pth['fn_queries_multihot'], pth['fn_train_data'], PpsHyperGraph, 10, 0, CPU)


def head_case(out):
    seed_all(1400)
    rows, width, items = 70, 96, 40
    head = HemPredictionLayer(width, 0.5, items)
    scale = lambda: 10 ** (2 * torch.rand(rows, 1) - 1)
    user, query, item = (torch.randn(rows, width) / width ** 0.5 * scale() for _ in range(3))
    item[3] = 0.0                                                        # below eps: cos = 0
    item[4] *= 2e-9 / float(item[4].norm())                              # norm 2e-9: the clamp makes it 0.2 of a unit row
    idx = torch.randint(0, items, (rows,))
    with torch.no_grad():
        scores = head(user, query, item, idx)
    want = cref.hem_cosine(user.double(), query.double(), item.double(), head.items_bias.detach().double()[idx])
    assert rel(scores.numpy(), want.numpy()) <= 2e-6
    out.update({'head.user': user.numpy(), 'head.query': query.numpy(), 'head.item': item.numpy(), 'head.indices': idx.numpy(),
                'head.bias': head.items_bias.detach().numpy().copy(), 'head.scores': scores.numpy(), 'head.lam': np.float64(0.5)})
    print(f'F14 head: restatement within {rel(scores.numpy(), want.numpy()):.1e}')


def model_case(out, tag, kind, L, order, d, seed, w, pth, ds):
    layer_t = IHGNNLayer if kind == 'ihgnn' else HGCNLayer
    seed_all(seed)
    m = RawGnn(CPU, ds, d, layer_t, L, order, False, HemPredictionLayer, 0.5)
    with torch.no_grad():                                               # (as F13: values a tenth of the reference's unit normal, so that the cosine is not drowned by the bias)
        m.prediction_layer.items_bias.normal_(0, 0.1)
    sd = sd_numpy(m)
    pre = f'{tag}.'
    counts = (w.user_count, w.query_count, w.item_count)
    # evaluation of the initial parameters over the workload's test logs
    test = TestSearchLogDataLoader(pth['fn_test_data'], ds, CPU)
    total, per_log, all_scores, uq = Metrics(), [], [], []
    with torch.no_grad():
        m.save_features_for_test()
        for users, queries, items, _, all1 in test:
            s = m(users, queries, None)
            mm = Metrics.calculate_on_all_items(s, items, None, all1)
            total.add_to_self(mm)
            per_log.append((mm.HitRatio_at10, mm.NDCG_at10, mm.MAP_at10))
            all_scores.append(s.numpy().copy())
            uq.append((int(users[0]), int(queries[0])))
        m.clear_saved_feature()
    assert len(per_log) == 12 and uq == [(u, q) for u, q, _ in w.test_logs]
    avg = total.divide_and_get_new(len(per_log))
    all64 = cref.model_all_item_scores(sd, w.triples, counts, w.bag_words + 1, w.bag_offsets, kind, L, order, [u for u, _ in uq], [q for _, q in uq])
    assert rel(np.stack(all_scores), all64.numpy()) <= 2e-6
    # one training step
    u = torch.randint(0, ds.user_count, (BATCH,)); q = torch.randint(0, ds.query_count, (BATCH,)); i = torch.randint(0, ds.item_count, (BATCH,))
    flags = (torch.rand(BATCH) < 0.3).float()
    step64 = cref.model_step(sd, w.triples, counts, w.bag_words + 1, w.bag_offsets, kind, L, order, u, q, i, flags)
    opt = torch.optim.Adam(m.parameters(), 1e-3, weight_decay=0)
    scores = m(u, q, i)
    loss = torch.nn.BCEWithLogitsLoss()(scores, flags)
    loss.backward()
    assert all(p.grad is not None for p in m.parameters()) and np.isfinite(loss.item())
    grads = {n: p.grad.numpy().copy() for n, p in m.named_parameters()}
    opt.step()
    stepped = sd_numpy(m)
    worst = max([rel(step64['scores'].numpy(), scores.detach().numpy()), abs(step64['loss'] - loss.item())] + [rel(step64['grads'][n].numpy(), g) for n, g in grads.items()])
    assert worst <= 2e-6, (tag, worst)
    import query_transform_reference as qref
    assert max(qref.adam_excess(v, step64['grads'][n], step64['adam'][n], 2e-6) for n, v in stepped.items()) <= 1.0, tag
    out.update({pre + 'sd.' + k: v for k, v in sd.items()})
    for n, g in grads.items():
        out.update(kept(pre + 'grad.' + n, g))
    for k, v in stepped.items():
        out.update(kept(pre + 'adam.' + k, v))
    out.update({pre + 'u': u.numpy(), pre + 'q': q.numpy(), pre + 'i': i.numpy(), pre + 'flags': flags.numpy(), pre + 'scores': scores.detach().numpy(),
                pre + 'loss': np.float64(loss.item()), pre + 'cfg': np.array([L, order, d, seed], np.int64), pre + 'all_scores': np.stack(all_scores),
                pre + 'metrics_per_log': np.array(per_log, np.float64), pre + 'metrics': np.array([avg.HitRatio_at10, avg.NDCG_at10, avg.MAP_at10], np.float64)})
    print(f'F14 {tag}: seed {seed}, loss {loss.item():.6f}, restatement within {worst:.1e}, HR/NDCG/MAP@10 {out[pre + "metrics"]}')


def main():
    Gs.Prediction.use_cosine_similarity = True
    out = {}
    head_case(out)
    w, pth, ds = small_dataset()
    out.update({'test.uq': np.array([(u, q) for u, q, _ in w.test_logs], np.int64), 'test.items_flat': np.array([x for _, _, it in w.test_logs for x in it], np.int64),
                'test.items_len': np.array([len(it) for _, _, it in w.test_logs], np.int64)})
    for tag, kind, L, order, d, seed in MODEL_CASES:
        model_case(out, tag, kind, L, order, d, seed, w, pth, ds)
    path = os.path.join(HERE, 'f14_cosine.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 1 << 20, os.path.getsize(path)
    print(f'{os.path.getsize(path):>9d}  f14_cosine.npz')


if __name__ == '__main__':
    main()
