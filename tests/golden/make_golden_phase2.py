#!/usr/bin/env python3
"""Generate ``f12_phase2.npz``: the reference's IHGNNLayer with ``phase2_attention=True`` (CDboyOne/IHGNN ``Models/GnnLayers.py:156-236``) run on CPU.

Here-only tooling, like ``make_golden_gat.py`` (same stubs for ``torch_sparse`` and ``dgl``, written here from their documented semantics): it needs the reference
checkout, is never imported by tests, ``bench.py`` or the product, and contains no reference code.

THE REFERENCE IS RUN PATCHED, because as written this branch cannot be constructed: ``IHGNNLayer._FakeDataset`` offers ``.Graph`` and ``.NodeCount``, while
``GATLayer.__init__`` - which the branch hands that object to - reads ``dataset.graph2d.Adjacency`` and ``dataset.node_count`` (``GnnLayers.py:62, 90``), so the
constructor dies with ``AttributeError: '_FakeDataset' object has no attribute 'graph2d'``.  This harness replaces ``IHGNNLayer._FakeDataset`` by a class that ALSO
exposes those two names (``_PatchedFakeDataset`` below) and changes nothing else; no line of the reference is edited or copied.  With that the branch runs: the
"fake" graph has ``N + E`` vertices and an edge hyperedge -> member node per incidence, ``fake_gat`` transforms ``cat([h, Ef])`` with ONE Linear, scores every edge,
normalises per node and sums.  Backward works under LeakyReLU only: under ReLU / Tanh the in-place ``squeeze_`` of ``GnnLayers.py:111`` makes autograd refuse, as in
F11 - those cases are stored with ``has_grad = 0`` and the test takes their gradients from its float64 restatement.

The reference seeds nothing; every seed below is set by this harness.  The file holds data only: the reference's outputs and the small seeded inputs.  A second run
reproduces the inputs bit for bit and the outputs to about 1e-7 (torch's threaded CPU sums).

    python tests/golden/make_golden_phase2.py            # rewrites tests/golden/f12_phase2.npz
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


class _Graph:
    def __init__(self, src, dst, num_nodes):
        self.src, self.dst, self.num_nodes = src.long(), dst.long(), int(num_nodes)


def _edge_softmax(g, scores):
    s = scores.reshape(-1)
    top = torch.full((g.num_nodes,), -float('inf'), dtype=s.dtype).scatter_reduce(0, g.dst, s, 'amax', include_self=True)
    e = torch.exp(s - top[g.dst])
    den = torch.zeros(g.num_nodes, dtype=s.dtype).index_add(0, g.dst, e)
    return (e / den[g.dst]).reshape(scores.shape)


def _u_mul_e_sum(g, x, a):
    return torch.zeros(g.num_nodes, x.shape[1], dtype=x.dtype).index_add(0, g.dst, x[g.src] * a.reshape(-1, 1))


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
    dgl = types.ModuleType('dgl')
    dgl.graph = lambda data, num_nodes, device=None: _Graph(data[0], data[1], num_nodes)
    dgl.ops = types.SimpleNamespace(edge_softmax=_edge_softmax, u_mul_e_sum=_u_mul_e_sum)
    sys.modules['dgl'] = dgl


_install_stubs()
sys.path.insert(0, REFERENCE)
sys.path.insert(1, REPO)

import torch.nn as nn                                                   # noqa: E402

from Dataset import GraphDataset                                        # noqa: E402  (reference)
from Helpers.Graph import PpsHyperGraph                                 # noqa: E402  (reference)
from Helpers.GlobalSettings import Gs, Gsv                              # noqa: E402  (reference)
from Models import RawGnn, IHGNNLayer, HemPredictionLayer               # noqa: E402  (reference)

from ihgnn_amd import synth                                             # noqa: E402  (this repo)


class _PatchedFakeDataset:
    """``IHGNNLayer._FakeDataset`` plus the two attribute names ``GATLayer.__init__`` reads (see the module docstring)."""

    def __init__(self, adjacency, node_count):
        self.Graph = self.graph2d = IHGNNLayer._FakeGraph(adjacency)
        self.NodeCount = self.node_count = node_count


IHGNNLayer._FakeDataset = _PatchedFakeDataset

CPU = torch.device('cpu')
torch.set_num_threads(4)
ACTIVATIONS = {'leaky_relu': (nn.LeakyReLU, 'leaky_relu'), 'relu': (nn.ReLU, 'relu'), 'tanh': (nn.Tanh, 'tanh')}
HEADS = {'concat': Gsv.concat, 'product': Gsv.product}

# (tag, graph, d, order, head, activation): the layer cases of the GPU test - orders 1 / 2 / 3, both heads, the three activations, d in {8, 32, 64}
# (d = 64 on the tiny graph at order 1: the aggregation weight and its gradient are 3 / 6 / 7 d^2 floats each, and the file stays well under 1 MB)
LAYER_CASES = (
    ('tiny_o1_d8_concat_leaky', 'tiny', 8, 1, 'concat', 'leaky_relu'),
    ('tiny_o2_d8_product_tanh', 'tiny', 8, 2, 'product', 'tanh'),
    ('tiny_o3_d32_product_leaky', 'tiny', 32, 3, 'product', 'leaky_relu'),
    ('tiny_o1_d64_product_leaky', 'tiny', 64, 1, 'product', 'leaky_relu'),
    ('tiny_o1_d64_concat_tanh', 'tiny', 64, 1, 'concat', 'tanh'),
    ('small_o3_d32_concat_leaky', 'small', 32, 3, 'concat', 'leaky_relu'),
    ('small_o2_d32_product_relu', 'small', 32, 2, 'product', 'relu'),
    ('small_o3_d8_concat_tanh', 'small', 8, 3, 'concat', 'tanh'),
    ('small_o1_d8_product_leaky', 'small', 8, 1, 'product', 'leaky_relu'),
    ('small_o2_d8_concat_relu', 'small', 8, 2, 'concat', 'relu'),
    ('small_o2_d8_concat_leaky', 'small', 8, 2, 'concat', 'leaky_relu'),
)


def seed_all(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def sd_numpy(module, prefix='sd.'):
    return {prefix + k: v.detach().cpu().numpy().copy() for k, v in module.state_dict().items()}


def dataset_for(which):
    if which == 'tiny':
        pth = {k: os.path.join(HERE, 'f1_data', v) for k, v in dict(fn_graph_info='graph_info.txt', fn_queries_multihot='queries_multihot.txt',
                                                                      fn_train_data='train_data.csv').items()}
    else:
        pth = synth.write_files(synth.draw(40, 20, 50, 30, 300, seed=11, eval_logs=12), '/tmp/ihgnn_golden_small_phase2')      # make_golden.small_workload()
    return GraphDataset(pth['fn_graph_info'], pth['fn_queries_multihot'], pth['fn_train_data'], PpsHyperGraph, 10, 0, CPU)


def main():
    out = {}
    for tag, which, d, order, head, act in LAYER_CASES:
        Gs.Gnn.gat_head, Gs.Gnn.gat_activation = HEADS[head], ACTIVATIONS[act]
        ds = dataset_for(which)
        seed_all(1200 + d + order)
        layer = IHGNNLayer(CPU, ds, d, d, order, True)
        x = torch.randn(ds.node_count, d, requires_grad=True)
        y = layer(x)
        cot = torch.randn_like(y)
        out.update({f'{tag}.{k}': v for k, v in sd_numpy(layer).items()})
        out.update({f'{tag}.x': x.detach().numpy(), f'{tag}.y': y.detach().numpy(), f'{tag}.cot': cot.numpy()})
        try:
            y.backward(cot)
        except RuntimeError as exc:
            # the in-place squeeze of GnnLayers.py:111 under ReLU / Tanh, as in make_golden_gat.py: only the forward exists there
            assert 'inplace' in str(exc), exc
            out[f'{tag}.has_grad'] = np.int64(0)
            continue
        out[f'{tag}.has_grad'] = np.int64(1)
        out[f'{tag}.dx'] = x.grad.numpy()
        for name, p in layer.named_parameters():
            out[f'{tag}.grad.{name}'] = p.grad.numpy().copy()
    # seeded construction: the initial weights for both heads and all three activations (d = 16, order 3)
    ds = dataset_for('tiny')
    for head in HEADS:
        for act in ACTIVATIONS:
            Gs.Gnn.gat_head, Gs.Gnn.gat_activation = HEADS[head], ACTIVATIONS[act]
            seed_all(1212)
            out.update({f'init.{head}.{act}.{k}': v for k, v in sd_numpy(IHGNNLayer(CPU, ds, 16, 16, 3, True), '').items()})
    # model level: RawGnn with two IHGNN layers, order 3, attention on (the reference's defaults: concatenation, LeakyReLU) on the small workload
    Gs.Gnn.gat_head, Gs.Gnn.gat_activation = Gsv.concat, ACTIVATIONS['leaky_relu']
    ds = dataset_for('small')
    seed_all(1277)
    m = RawGnn(CPU, ds, 16, IHGNNLayer, 2, 3, True, HemPredictionLayer, 0.5)
    out.update({f'model.{k}': v for k, v in sd_numpy(m).items()})
    u = torch.randint(0, ds.user_count, (64,)); q = torch.randint(0, ds.query_count, (64,)); i = torch.randint(0, ds.item_count, (64,))
    flags = (torch.rand(64) < 0.3).float()
    scores = m(u, q, i)
    loss = torch.nn.BCEWithLogitsLoss()(scores, flags)
    loss.backward()
    assert all(p.grad is not None for p in m.parameters()) and np.isfinite(loss.item())
    out.update({f'model.grad.{n}': p.grad.numpy().copy() for n, p in m.named_parameters()})
    out.update({'model.u': u.numpy(), 'model.q': q.numpy(), 'model.i': i.numpy(), 'model.flags': flags.numpy(),
                'model.scores': scores.detach().numpy(), 'model.loss': np.float64(loss.item())})
    path = os.path.join(HERE, 'f12_phase2.npz')
    np.savez_compressed(path, **out)
    print(f'{os.path.getsize(path):>9d}  f12_phase2.npz')


if __name__ == '__main__':
    main()
