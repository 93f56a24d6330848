"""IHGNNLayer with phase-2 attention on the host: construction against the reference (fixture F12, tests/golden/make_golden_phase2.py), the position map
of the node <- hyperedge incidence, and the driver's flag.  No GPU needed."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

CPU = torch.device('cpu')
ACTIVATIONS = {'leaky_relu': (nn.LeakyReLU, 'leaky_relu'), 'relu': (nn.ReLU, 'relu'), 'tanh': (nn.Tanh, 'tanh')}
KEYS = ['feature_interactor.aggregation.weight', 'feature_interactor.aggregation.bias', 'fake_gat.feature_aggregate.0.weight', 'fake_gat.feature_aggregate.0.bias',
        'fake_gat.feature_transform.weight', 'fake_gat.feature_transform.bias', 'feature_transform.weight', 'feature_transform.bias']


def tiny_dataset():
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    d = os.path.join(GOLDEN, 'f1_data')
    return GraphDataset(os.path.join(d, 'graph_info.txt'), os.path.join(d, 'queries_multihot.txt'), os.path.join(d, 'train_data.csv'), PpsHyperGraph, 10, 0, CPU)


class _settings:
    """Gs.Gnn head / activation for one block, restored afterwards."""

    def __init__(self, head=None, activation=None):
        self.new = (head, activation)

    def __enter__(self):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        self.old = (Gs.Gnn.gat_head, Gs.Gnn.gat_activation)
        head, act = self.new
        if head is not None:
            Gs.Gnn.gat_head = head
        if act is not None:
            Gs.Gnn.gat_activation = act

    def __exit__(self, *exc):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        Gs.Gnn.gat_head, Gs.Gnn.gat_activation = self.old


@pytest.mark.parametrize('head', ['concat', 'product'])
@pytest.mark.parametrize('act', ['leaky_relu', 'relu', 'tanh'])
def test_phase2_layer_construction_matches_reference(head, act):
    """Keys, shapes and the seeded initial weights are the reference's, bit for bit (construction order: interactor, fake_gat - its feature_aggregate re-drawn
    by xavier_uniform_ with the activation's gain, then its feature_transform -, feature_transform)."""
    from ihgnn_amd.Helpers.GlobalSettings import Gsv
    from ihgnn_amd.Models import IHGNNLayer
    z = np.load(os.path.join(GOLDEN, 'f12_phase2.npz'))
    ds = tiny_dataset()
    with _settings({'concat': Gsv.concat, 'product': Gsv.product}[head], ACTIVATIONS[act]):
        torch.manual_seed(1212)
        layer = IHGNNLayer(CPU, ds, 16, 16, 3, True)
    pre = f'init.{head}.{act}.'
    want = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    got = layer.state_dict()
    assert list(got) == KEYS
    assert set(got) == set(want)
    for k, v in got.items():
        assert tuple(v.shape) == want[k].shape, k
        np.testing.assert_array_equal(v.numpy(), want[k], err_msg=k)
    assert tuple(got['fake_gat.feature_aggregate.0.weight'].shape) == ((1, 32) if head == 'concat' else (1, 16))
    assert layer.attention_phase2 is True and layer.reads_cotangent_rows_only() is False


def test_layer_without_attention_keeps_its_keys():
    from ihgnn_amd.Models import IHGNNLayer
    layer = IHGNNLayer(CPU, tiny_dataset(), 8, 8, 1, False)
    assert list(layer.state_dict()) == [k for k in KEYS if not k.startswith('fake_gat.')]
    assert layer.attention_phase2 is False and layer.reads_cotangent_rows_only() is True


def test_raw_gnn_gives_every_layer_a_fake_gat():
    """``RawGnn`` forwards the keyword to every layer; the layers above the first are first-order.  The key set is F12's model case."""
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    z = np.load(os.path.join(GOLDEN, 'f12_phase2.npz'))
    m = RawGnn(CPU, tiny_dataset(), 16, IHGNNLayer, 2, 3, True, HemPredictionLayer, 0.5)
    want = {k[len('model.sd.'):]: z[k].shape for k in z.files if k.startswith('model.sd.')}
    got = m.state_dict()
    assert {k for k in got if k.startswith('gnn_')} == {k for k in want if k.startswith('gnn_')}
    for k in got:
        if k.startswith('gnn_'):
            assert tuple(got[k].shape) == want[k], k
    assert [layer.feature_interaction_order for layer in m.gnns] == [3, 1] and all(hasattr(layer, 'fake_gat') for layer in m.gnns)


def test_phase2_layer_refuses_unknown_settings():
    from ihgnn_amd.Models import IHGNNLayer
    ds = tiny_dataset()
    with _settings(head='sum'), pytest.raises(ValueError, match='head'):
        IHGNNLayer(CPU, ds, 8, 8, 2, True)
    with _settings(activation=(nn.Sigmoid, 'sigmoid')), pytest.raises(ValueError, match='activation'):
        IHGNNLayer(CPU, ds, 8, 8, 2, True)
    with _settings(activation=(nn.ReLU, 'tanh')), pytest.raises(ValueError, match='activation'):
        IHGNNLayer(CPU, ds, 8, 8, 2, True)
    # the settings are not read with the attention off
    with _settings(head='sum'):
        IHGNNLayer(CPU, ds, 8, 8, 2, False)
    from ihgnn_amd import ops
    x = torch.zeros(1, 4)
    with pytest.raises(ValueError, match='head'):
        ops.hyper_attention(x, x, None, x, x, head='sum')
    with pytest.raises(ValueError, match='activation'):
        ops.hyper_attention(x, x, None, x, x, activation='sigmoid')


def _layouts():
    from ihgnn_amd.layout import IncidenceLayout
    w = np.load(os.path.join(GOLDEN, 'f2_small_workload.npz'))
    U, Q, I, _ = (int(x) for x in w['counts'])
    small = w['triples']
    repeated = np.concatenate([small, small[::3], small[::7]])                # every third triple twice, every seventh once more
    return {'tiny': tiny_dataset().hypergraph.layout,
            'small': IncidenceLayout(small, U, Q, I, CPU),
            'small_split': IncidenceLayout(small, U, Q, I, CPU, heavy_threshold=4),
            'multiplicities': IncidenceLayout(repeated, U, Q, I, CPU, edge_multiplicity='1'),
            'compact': IncidenceLayout(small[small[:, 0] < U - 5], U, Q, I, CPU, compact_nodes='1')}


@pytest.mark.parametrize('which', ['tiny', 'small', 'small_split', 'multiplicities', 'compact'])
def test_member_ids_are_the_position_map(which):
    """``member_csr.ids[p] = 3 e + type(v)`` for entry p = (v, e) of ``node_csr``: a permutation of ``[0, 3 E)`` - what lets the attention's backward write every
    entry's weight at its slot of an edge-major ``[E, 3]`` table - that lands on the slot of ``i3`` holding v."""
    lay = _layouts()[which]
    e = lay.edge_count
    pos = lay.member_csr.ids_host.astype(np.int64)
    ids = lay.node_csr.ids_host.astype(np.int64)
    assert pos.shape == (3 * e,) and e > 0
    np.testing.assert_array_equal(np.sort(pos), np.arange(3 * e))
    np.testing.assert_array_equal(pos // 3, ids)
    rows = np.repeat(np.arange(lay.node_count), np.diff(lay.node_csr.ptr_host.astype(np.int64)))
    np.testing.assert_array_equal(lay.i3_host.reshape(-1)[pos], rows)
    if which == 'multiplicities':
        assert lay.edge_weight is not None and float(lay.edge_weight.max()) >= 2 and e < lay.hyperedge_count
    if which == 'small_split':
        assert lay.node_csr.n_heavy > 0
        np.testing.assert_array_equal(lay.node_csr.seg_row.numpy(), np.repeat(lay.node_csr.heavy_rows.numpy(), np.diff(lay.node_csr.heavy_segptr.numpy())))
    if which == 'compact':
        assert lay.compact and lay.node_count < lay.public_node_count


def test_driver_parses_phase2(tmp_path, monkeypatch):
    from ihgnn_amd import Main
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    assert parse_args([]).phase2 is False and parse_args(['--phase2']).phase2 is True
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match='phase2'):
        Main.main(['--gnn', 'HGCN', '--phase2', '--device', 'cpu'])
    with pytest.raises(RuntimeError, match='no CPU path'):                     # past the flag's checks: this host has no GPU path
        Main.main(['--phase2', '--device', 'cpu'])


def test_recorded_step_refuses_a_model_with_attention():
    """The training loop takes a ValueError from the recording as "train eagerly" (TrainTestHelper.train_and_get_avg_loss)."""
    from ihgnn_amd.captured_step import CapturedTrainingStep
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    from ihgnn_amd.optim import Adam
    m = RawGnn(CPU, tiny_dataset(), 8, IHGNNLayer, 1, 2, True, HemPredictionLayer, 0.5)
    with pytest.raises(ValueError, match='phase-2 attention'):
        CapturedTrainingStep(m, Adam(m.parameters(), 1e-3), 4)
