"""GATLayer on the host: construction against the reference (fixture F11, tests/golden/make_golden_gat.py), the mirrored CSR positions of the pairwise
graph, and the driver's layer check.  No GPU needed."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

CPU = torch.device('cpu')
ACTIVATIONS = {'leaky_relu': (nn.LeakyReLU, 'leaky_relu'), 'relu': (nn.ReLU, 'relu'), 'tanh': (nn.Tanh, 'tanh')}


def tiny_dataset(graph_type=None):
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.Graph import Pps2DGraph
    d = os.path.join(GOLDEN, 'f1_data')
    return GraphDataset(os.path.join(d, 'graph_info.txt'), os.path.join(d, 'queries_multihot.txt'), os.path.join(d, 'train_data.csv'),
                        graph_type or Pps2DGraph, 10, 0, CPU)


class _settings:
    """Gs.Gnn / Gs.graph_completeness for one block, restored afterwards."""

    def __init__(self, head=None, activation=None, completeness=None):
        self.new = (head, activation, completeness)

    def __enter__(self):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        self.old = (Gs.Gnn.gat_head, Gs.Gnn.gat_activation, Gs.graph_completeness)
        head, act, mode = self.new
        if head is not None:
            Gs.Gnn.gat_head = head
        if act is not None:
            Gs.Gnn.gat_activation = act
        if mode is not None:
            Gs.graph_completeness = mode

    def __exit__(self, *exc):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        Gs.Gnn.gat_head, Gs.Gnn.gat_activation, Gs.graph_completeness = self.old


def test_gat_settings_default_to_the_reference():
    """The reference's last assignments win (GlobalSettings.py:59-66): concatenation head, LeakyReLU."""
    from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
    assert Gs.Gnn.gat_head == Gsv.concat == 'concatenation'
    assert Gs.Gnn.gat_activation == (nn.LeakyReLU, 'leaky_relu')


@pytest.mark.parametrize('head', ['concat', 'product'])
@pytest.mark.parametrize('act', ['leaky_relu', 'relu', 'tanh'])
def test_gat_layer_construction_matches_reference(head, act):
    """Keys, shapes and the seeded initial weights are the reference's, bit for bit (construction order: Linear, xavier_uniform_ with the activation's gain,
    then feature_transform)."""
    from ihgnn_amd.Helpers.GlobalSettings import Gsv
    from ihgnn_amd.Models import GATLayer
    z = np.load(os.path.join(GOLDEN, 'f11_gat.npz'))
    ds = tiny_dataset()
    with _settings({'concat': Gsv.concat, 'product': Gsv.product}[head], ACTIVATIONS[act]):
        torch.manual_seed(1111)
        layer = GATLayer(CPU, ds, 16, 16)
    pre = f'init.{head}.{act}.'
    want = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    got = layer.state_dict()
    assert list(got) == ['feature_aggregate.0.weight', 'feature_aggregate.0.bias', 'feature_transform.weight', 'feature_transform.bias']
    assert set(got) == set(want)
    for k, v in got.items():
        assert tuple(v.shape) == want[k].shape, k
        np.testing.assert_array_equal(v.numpy(), want[k], err_msg=k)
    assert tuple(got['feature_aggregate.0.weight'].shape) == ((1, 32) if head == 'concat' else (1, 16))


def test_gat_layer_refuses_unknown_settings():
    from ihgnn_amd.Models import GATLayer
    ds = tiny_dataset()
    with _settings(head='sum'), pytest.raises(ValueError, match='head'):
        GATLayer(CPU, ds, 8, 8)
    with _settings(activation=(nn.Sigmoid, 'sigmoid')), pytest.raises(ValueError, match='activation'):
        GATLayer(CPU, ds, 8, 8)
    with _settings(activation=(nn.ReLU, 'tanh')), pytest.raises(ValueError, match='activation'):
        GATLayer(CPU, ds, 8, 8)


@pytest.mark.parametrize('which', ['tiny', 'small'])
@pytest.mark.parametrize('mode', ['uqi', 'uq', 'ui', 'qi'])
def test_pair_layout_mirror_is_the_reverse_edge(which, mode):
    """mirror[p] of entry (v, u) is the position of (u, v): an involution that swaps row and column, on every completeness mode, with and without self loops."""
    from ihgnn_amd.layout import PairLayout
    if which == 'tiny':
        triples, (U, Q, I) = tiny_dataset().pos_triples, (5, 4, 6)
    else:
        w = np.load(os.path.join(GOLDEN, 'f2_small_workload.npz'))
        triples, (U, Q, I) = w['triples'], (40, 20, 50)
    for loops in (False, True):
        lay = PairLayout(triples, U, Q, I, CPU, completeness=mode, self_loops=loops)
        m = lay.mirror_host.astype(np.int64)
        ptr, ids = lay.csr.ptr_host.astype(np.int64), lay.csr.ids_host.astype(np.int64)
        rows = np.repeat(np.arange(U + Q + I), np.diff(ptr))
        assert m.shape == ids.shape and lay.csr.nnz > 0
        np.testing.assert_array_equal(m[m], np.arange(m.shape[0]))
        np.testing.assert_array_equal(rows[m], ids)
        np.testing.assert_array_equal(ids[m], rows)
        assert torch.equal(lay.mirror.cpu(), torch.from_numpy(lay.mirror_host))


def test_pair_layout_split_plan_names_the_row_of_every_segment():
    from ihgnn_amd.layout import PairLayout
    w = np.load(os.path.join(GOLDEN, 'f2_small_workload.npz'))
    lay = PairLayout(w['triples'], 40, 20, 50, CPU, heavy_threshold=4)
    csr = lay.csr
    assert csr.n_heavy > 0
    rows, segptr = csr.heavy_rows.numpy(), csr.heavy_segptr.numpy()
    want = np.repeat(rows, np.diff(segptr))
    np.testing.assert_array_equal(csr.seg_row.numpy(), want)
    ptr = csr.ptr_host
    assert (csr.seg_begin.numpy() >= ptr[want]).all() and (csr.seg_end.numpy() <= ptr[want + 1]).all()


def test_driver_accepts_gat(tmp_path, monkeypatch):
    """``--gnn GAT`` passes the driver's layer check (it stops at the next one: this host has no GPU path)."""
    from ihgnn_amd import Main
    monkeypatch.chdir(tmp_path)
    with pytest.raises(RuntimeError, match='no CPU path'):
        Main.main(['--gnn', 'GAT', '--device', 'cpu'])
    from ihgnn_amd.Helpers.ArgsParser import build_parser
    assert 'GAT are not part' not in build_parser().format_help()


def test_pair_layout_mirror_refuses_a_repeated_pair():
    """A CSR that lists a (row, column) pair twice has reverse entries for every entry, but not one-to-one: refused, not left with unwritten mirror slots."""
    from ihgnn_amd.layout import Csr, PairLayout
    lay = PairLayout.__new__(PairLayout)
    lay.node_count, lay.device, lay._mirror = 2, CPU, None
    lay.csr = Csr(np.array([0, 2, 4], np.int32), np.array([1, 1, 0, 0], np.int32), CPU)
    with pytest.raises(ValueError, match='more than once'):
        lay.mirror_host
    lay.csr = Csr(np.array([0, 1, 1], np.int32), np.array([1], np.int32), CPU)
    with pytest.raises(ValueError, match='not symmetric'):
        lay.mirror_host
