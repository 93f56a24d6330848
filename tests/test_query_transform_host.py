"""CPU: the query transform ``Gs.Query.transform == 'activation'`` (``Models/EmbeddingLayers.py:40-44, 83-84``) - the float64 restatement the GPU tests measure against
(``tests/query_transform_reference.py``) held to the reference's own numbers (fixture F13, ``tests/golden/make_golden_query_transform.py``) at 2e-6, the bar of
``tests/test_oracle_golden.py``; the command line, the settings and the module's state dict."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import query_transform_reference as qref
from conftest import GOLDEN

BAR = 2e-6
CPU = torch.device('cpu')
MODEL_CASES = (('ihgnn_o3_d32', 'ihgnn', 2, 3, 32), ('ihgnn_o2_d64', 'ihgnn', 2, 2, 64), ('hgcn_d64', 'hgcn', 2, 1, 64))
ACTS = ('relu', 'tanh')


def f13():
    return np.load(os.path.join(GOLDEN, 'f13_query_transform.npz'))


def small():
    return np.load(os.path.join(GOLDEN, 'f2_small_workload.npz'))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class query_settings:
    """``Gs.Query`` set for the block, put back after it."""

    def __init__(self, transform, activation=nn.ReLU):
        self.new = (transform, activation)

    def __enter__(self):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        self.old = (Gs.Query.transform, Gs.Query.transform_activation)
        Gs.Query.transform, Gs.Query.transform_activation = self.new

    def __exit__(self, *exc):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        Gs.Query.transform, Gs.Query.transform_activation = self.old


def test_f13_covers_what_the_issue_lists():
    z = f13()
    for act in ACTS:
        assert f'emb.{act}.queries' in z.files and f'emb.{act}.picked' in z.files
        for tag, *_ in MODEL_CASES:
            assert f'{tag}.{act}.loss' in z.files and (f'{tag}.{act}.grad.{qref.W_KEY}.rows8' in z.files or f'{tag}.{act}.grad.{qref.W_KEY}.full' in z.files)
            assert float(z[f'{tag}.{act}.margin']) > 0                   # no ReLU mask bit of a model case is within fp32 rounding of the kink
    c = np.load(os.path.join(GOLDEN, 'f13_query_transform_curve.npz'))
    assert len(c['curve.losses']) == 48 and c['curve.metrics'].shape == (3,)


@pytest.mark.parametrize('act', ACTS)
def test_restatement_matches_the_reference_embedding_layer(act):
    """``EmbeddingLayer(None, None, None)``, ``embed_query(indices)`` and the gradients of every parameter under the stored cotangents."""
    z, w = f13(), small()
    pre = f'emb.{act}.'
    sd = {k[len(pre) + 3:]: qref.t64(z[k]).requires_grad_(True) for k in z.files if k.startswith(pre + 'sd.')}
    wq, bq = sd['query_transform.0.weight'], sd['query_transform.0.bias']
    _, _, y = qref.query_rows(sd['embedding_bag_vocabulary.weight'], w['bag_words'] + 1, w['bag_offsets'], wq, bq, act)
    users, items = sd['embedding_user.weight'][1:], sd['embedding_item.weight'][1:]
    assert rel(y.detach(), z[pre + 'queries']) <= BAR and rel(users.detach(), z[pre + 'users']) == 0 and rel(items.detach(), z[pre + 'items']) == 0
    ((users * qref.t64(z[pre + 'cot_users'])).sum() + (y * qref.t64(z[pre + 'cot_queries'])).sum() + (items * qref.t64(z[pre + 'cot_items'])).sum()).backward()
    for k, v in sd.items():
        assert rel(v.grad, z[pre + 'grad.' + k]) <= BAR, k
        v.grad = None
    # indexed: the reference transforms the picked rows (EmbeddingLayers.py:80-84) - the same rows of the transformed table
    _, _, y = qref.query_rows(sd['embedding_bag_vocabulary.weight'], w['bag_words'] + 1, w['bag_offsets'], wq, bq, act)
    picked = y[torch.from_numpy(z[pre + 'indices'])]
    assert rel(picked.detach(), z[pre + 'picked']) <= BAR
    picked.backward(qref.t64(z[pre + 'cot_picked']))
    for k in ('embedding_bag_vocabulary.weight', 'query_transform.0.weight', 'query_transform.0.bias'):
        assert rel(sd[k].grad, z[pre + 'picked_grad.' + k]) <= BAR, k


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('tag,kind,L,order,d', MODEL_CASES)
def test_restatement_matches_the_reference_models(tag, kind, L, order, d, act):
    """Scores, BCE loss and every parameter gradient of the whole model at 2e-6; the parameters after one Adam step within that bar carried through the step."""
    z, w = f13(), small()
    pre = f'{tag}.{act}.'
    assert tuple(int(v) for v in z[pre + 'cfg'][:3]) == (L, order, d)
    step = qref.model_step(qref.fixture_state(z, tag), w['triples'], w['counts'], w['bag_words'] + 1, w['bag_offsets'], kind, L, order, act,
                           z[pre + 'u'], z[pre + 'q'], z[pre + 'i'], z[pre + 'flags'])
    assert rel(step['scores'], z[pre + 'scores']) <= BAR and abs(step['loss'] - float(z[pre + 'loss'])) <= BAR
    assert abs(step['min_margin'] - float(z[pre + 'margin'])) <= 1e-9
    for k, g in step['grads'].items():
        assert qref.fixture_error(z, pre + 'grad.' + k, g) <= BAR, k
        # the stepped parameters: within what a gradient that holds BAR may move Adam's first step (qref.adam_allowance: the step is steep where |g| is near eps, and
        # there the reference's own fp32 rounding of g shows) - the entries F13 keeps, one by one
        assert qref.fixture_adam_excess(z, pre + 'adam.' + k, g, step['adam'][k], BAR) <= 1.0, k


def test_flags_parse_default_and_reach_the_settings():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
    a = parse_args([])
    assert (a.query_transform, a.query_activation) == (Gsv.mean, 'relu')
    b = parse_args(['--query_transform', 'activation', '--query_activation', 'tanh'])
    assert (b.query_transform, b.query_activation) == (Gsv.activation, 'tanh')
    for bad in (['--query_transform', 'rnn'], ['--query_activation', 'gelu']):
        with pytest.raises(SystemExit):
            parse_args(bad)
    with query_settings(Gsv.mean):
        driver.apply_query_settings(b)
        assert Gs.Query.transform == Gsv.activation and Gs.Query.transform_activation is nn.Tanh
        driver.apply_query_settings(parse_args(['--query_transform', 'activation']))
        assert Gs.Query.transform == Gsv.activation and Gs.Query.transform_activation is nn.ReLU
        driver.apply_query_settings(a)
        assert Gs.Query.transform == Gsv.mean
    assert Gs.Query.transform == Gsv.mean and Gs.Query.transform_activation is nn.ReLU         # the defaults, as the reference's last assignments


def small_dataset():
    from ihgnn_amd.Dataset import GraphDataset
    w = small()
    U, Q, I, V = (int(x) for x in w['counts'])
    return GraphDataset.from_arrays(U, Q, I, V, w['bag_words'], w['bag_offsets'], w['triples'], device=CPU)


def test_rnn_and_unknown_activations_are_refused():
    from ihgnn_amd.Helpers.GlobalSettings import Gsv
    from ihgnn_amd.Models.EmbeddingLayers import EmbeddingLayer
    ds = small_dataset()
    with query_settings(Gsv.rnn):
        with pytest.raises(NotImplementedError):
            EmbeddingLayer(ds, 8)
    for act in (nn.Sigmoid, nn.LeakyReLU, nn.GELU):
        with query_settings(Gsv.activation, act):
            with pytest.raises(NotImplementedError):
                EmbeddingLayer(ds, 8)
    with query_settings('something else'):
        with pytest.raises((NotImplementedError, ValueError)):
            EmbeddingLayer(ds, 8)
    with query_settings(Gsv.mean):
        assert not hasattr(EmbeddingLayer(ds, 8), 'query_transform')


@pytest.mark.parametrize('act', [nn.ReLU, nn.Tanh])
def test_activation_model_has_the_reference_state_dict(act):
    """Key names, order and shapes of an activation model equal F13's (the reference's); construction draws what the reference draws: the ``mean`` model built from
    the same seed has the same embedding tables (the Linear is created after them) and different layers."""
    from ihgnn_amd.Helpers.GlobalSettings import Gsv
    from ihgnn_amd.Models import HGCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn
    z = f13()
    ds = small_dataset()
    for tag, kind, L, order, d in MODEL_CASES:
        want = qref.fixture_state(z, tag)
        with query_settings(Gsv.activation, act):
            torch.manual_seed(3)
            m = RawGnn(CPU, ds, d, IHGNNLayer if kind == 'ihgnn' else HGCNLayer, L, order, False, HemPredictionLayer, 0.5)
        got = m.state_dict()
        assert list(got) == list(want), tag
        assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in want.items()}, tag
        assert isinstance(m.embeddings.query_transform[0], nn.Linear) and isinstance(m.embeddings.query_transform[1], act)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in want.items()})                  # a reference checkpoint loads
        with query_settings(Gsv.mean):
            torch.manual_seed(3)
            plain = RawGnn(CPU, ds, d, IHGNNLayer if kind == 'ihgnn' else HGCNLayer, L, order, False, HemPredictionLayer, 0.5)
        assert qref.W_KEY not in plain.state_dict()
