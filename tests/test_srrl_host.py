"""The Srrl baseline without a GPU: fixture F15 (``tests/golden/f15_srrl.npz``, the reference's model run on the CPU; ``make_golden_srrl.py``) against the float64
restatement ``tests/srrl_reference.py`` within 2e-6, the restatement's hand-written block backward against autograd, the KG batches' host code against the fixture
exactly, the model's state dict, the driver's switches and refusals, and the new symbols of the C ABI."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import srrl_reference as sref
from conftest import GOLDEN, REPO
from ihgnn_amd import _lib, synth

BAR = 2e-6
MODES = ('tail-company-batch', 'head-company-batch', 'query-company-batch')
TABLES = ('positive_heads', 'positive_queries', 'positive_tails', 'negative_heads', 'negative_queries', 'negative_tails')
NEW_SYMBOLS = ('ihg_cat_linear_max_width', 'ihg_cat_linear_workspace_bytes', 'ihg_cat_linear_fwd', 'ihg_cat_linear_bwd', 'ihg_rows_dot_fwd', 'ihg_rows_dot_bwd', 'ihg_kg_loss',
               'ihg_rows_topk')


@pytest.fixture(scope='module')
def f15():
    return np.load(os.path.join(GOLDEN, 'f15_srrl.npz'))


@pytest.fixture(scope='module')
def workload():
    return synth.draw(40, 20, 50, 30, 300, seed=11, eval_logs=12)


def state(z):
    return {k[3:]: z[k] for k in z.files if k.startswith('sd.')}


def dataset(w):
    from ihgnn_amd.Dataset import GraphDataset
    return GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=torch.device('cpu'))


def test_f15_kg_batches_against_float64(f15, workload):
    sd, bags = state(f15), (workload.bag_words + 1, workload.bag_offsets)
    for m, mode in enumerate(MODES):
        pre = f'kg{m}.'
        assert int(f15[pre + 'mode']) == m
        step = sref.kg_step(sd, bags, f15[pre + 'positive'], f15[pre + 'negative'], f15[pre + 'weight'], f15[pre + 'tails'], f15[pre + 'heads'], f15[pre + 'queries'], mode)
        assert sref.rel(f15[pre + 'pos'], step['pos']) <= BAR and sref.rel(f15[pre + 'neg'], step['neg']) <= BAR and abs(float(f15[pre + 'loss']) - step['loss']) <= BAR
        reached = {k[len(pre) + 5:] for k in f15.files if k.startswith(pre + 'grad.')}
        assert reached == {k for k, g in step['grads'].items() if g is not None} and reached
        for name in reached:
            assert sref.rel(f15[pre + 'grad.' + name], step['grads'][name]) <= BAR, (mode, name)


def test_f15_ps_batches_against_float64(f15, workload):
    import query_transform_reference as qref
    sd, bags = state(f15), (workload.bag_words + 1, workload.bag_offsets)
    for pre, kg_on in (('ps.', True), ('ps_nokg.', False)):
        step = sref.ps_step(sd, bags, f15[pre + 'u'], f15[pre + 'q'], f15[pre + 'i'], f15[pre + 'flags'], kg_on)
        assert sref.rel(f15[pre + 'scores'], step['scores']) <= BAR and abs(float(f15[pre + 'loss']) - step['loss']) <= BAR
        reached = {k[len(pre) + 5:] for k in f15.files if k.startswith(pre + 'grad.')}
        assert reached == {k for k, g in step['grads'].items() if g is not None}
        assert ('g_u.aggregation.0.weight' in reached) == kg_on and not any(k.startswith('KG.embedding_user') or k.startswith('KG.embedding_item') for k in reached)
        for name in reached:
            assert sref.rel(f15[pre + 'grad.' + name], step['grads'][name]) <= BAR, (pre, name)
            if kg_on:
                assert qref.adam_excess(f15[pre + 'adam.' + name], step['grads'][name], step['adam'][name], BAR) <= 1.0, name


def test_f15_all_item_scores_and_their_ranking(f15, workload):
    sd, bags = state(f15), (workload.bag_words + 1, workload.bag_offsets)
    uq = f15['test.uq']
    assert [tuple(r) for r in uq.tolist()] == [(u, q) for u, q, _ in workload.test_logs]
    want = sref.all_item_scores(sd, bags, uq[:, 0], uq[:, 1]).numpy()
    assert sref.rel(f15['test.all_scores'], want) <= BAR
    for row in f15['test.all_scores'].astype(np.float64):                # what the generator asserted: no near-tie among the top eleven
        ranked = np.sort(row)[::-1]
        assert (ranked[:10] - ranked[1:11]).min() > 1e-4 * (ranked[0] - ranked[-1])
    assert np.array_equal(sref.topk(f15['test.all_scores'], 10)[0], sref.topk(want, 10)[0])
    assert f15['test.metrics_per_log'].shape == (12, 3) and np.allclose(f15['test.metrics_per_log'].mean(0), f15['test.metrics'])


@pytest.mark.parametrize('normalize,leaky', [(True, True), (True, False), (False, True)])
def test_block_backward_restates_autograd(normalize, leaky):
    """The hand-written gradients of ``srrl_reference.block_backward`` (what the kernel tests compare with) are torch's autograd of the same modules in float64,
    below F.normalize's eps too (one zero row, one of norm 1e-13)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(9, 12, generator=g, dtype=torch.float64)
    x[2] = 0.0
    x[5] *= 1e-13 / x[5].norm()
    w, b, dy = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((7, 12), (7,), (9, 7)))
    xl, wl, bl = (t.clone().requires_grad_(True) for t in (x, w, b))
    z = (F.normalize(xl, dim=-1) if normalize else xl) @ wl.t() + bl
    y = F.leaky_relu(z, 0.01) if leaky else z
    y.backward(dy)
    fwd = sref.block_forward(x.numpy(), w.numpy(), b.numpy(), normalize, leaky)
    assert np.abs(fwd['y'] - y.detach().numpy()).max() <= 1e-12
    got = sref.block_backward(x.numpy(), w.numpy(), dy.numpy(), fwd['y'], normalize, leaky)
    for mine, theirs in ((got['dw'], wl.grad), (got['dbias'], bl.grad), (got['dx'], xl.grad)):
        assert np.abs(mine - theirs.numpy()).max() <= 1e-12 * max(1.0, float(theirs.abs().max()))


def test_kg_loss_and_topk_restatements():
    g = torch.Generator().manual_seed(6)
    pos, neg, w = torch.randn(7, generator=g), torch.randn(7, 3, generator=g), torch.rand(7, generator=g) + 0.1
    ref = sref.kg_loss(pos, neg, w)
    want = (-(w.double() * F.logsigmoid(pos.double())).sum() / w.double().sum() - (w.double() * F.logsigmoid(-neg.double()).mean(1)).sum() / w.double().sum()) / 2
    assert abs(ref['loss'] - float(want)) <= 1e-14
    assert abs(sref.kg_loss(pos, neg)['loss'] - float((-F.logsigmoid(pos.double()).mean() - F.logsigmoid(-neg.double()).mean(1).mean()) / 2)) <= 1e-14
    items, best = sref.topk(np.array([[1.0, 3.0, 3.0, 0.0, 3.0]]), 4)
    assert items.tolist() == [[1, 2, 4, 0]] and best.tolist() == [[3.0, 3.0, 3.0, 1.0]]
    assert sref.topk(np.array([[2.0, 5.0]]), 3)[0].tolist() == [[1, 0, -1]]


def test_meta_paths_and_weights_equal_the_fixture(f15, workload):
    from ihgnn_amd.SrrlDataset import MetaPaths, SrrlDatasetKG
    meta = MetaPaths(dataset(workload))
    assert meta.positive_interactions == [tuple(t) for t in workload.triples.tolist()]
    for name in TABLES:
        table = getattr(meta, name)
        assert np.array_equal(np.array(list(table.keys()), np.int64).reshape(-1, 2), f15[f'paths.{name}.keys']), name
        assert np.array_equal(np.array([x for members in table.values() for x in members], np.int64), f15[f'paths.{name}.members']), name
        assert np.array_equal(np.array([len(members) for members in table.values()], np.int64), f15[f'paths.{name}.lens']), name
    kg = SrrlDatasetKG(meta, 10, MODES[0])
    assert len(kg) == len(workload.triples)
    assert np.array_equal(np.array([float(kg.subsampling_weight(n)) for n in range(len(kg))], np.float32), f15['weights'])
    first = {}
    for u, q, _ in meta.positive_interactions:                           # 4 on first sight, + 1 afterwards
        first[(u, q)] = first.get((u, q), 3) + 1
    assert kg.head_query_frequency == first and min(first.values()) == 4
    with pytest.raises(NotImplementedError):
        SrrlDatasetKG(meta, 10, MODES[0], only_use_random_negative_sample=False)


def test_kg_samples_lie_in_their_sets_and_collate_keeps_the_layout(workload):
    from torch.utils.data import DataLoader
    from ihgnn_amd.SrrlDataset import MetaPaths, OneShotIterator, SrrlDatasetKG
    random.seed(3); np.random.seed(3); torch.manual_seed(3)
    meta = MetaPaths(dataset(workload))
    kg = SrrlDatasetKG(meta, 10, MODES[1])
    for n in range(len(kg)):
        positive, negatives, weight, mode, tail, head, query = kg[n]
        u, q, i = positive.tolist()
        assert (u, q, i) == meta.positive_interactions[n] and mode == MODES[1] and weight.shape == (1,)
        assert int(tail) in meta.positive_tails[(u, q)] and int(head) in meta.positive_heads[(q, i)] and int(query) in meta.positive_queries[(u, i)]
        assert negatives.dtype == torch.int64 and negatives.shape == (10,) and 0 <= int(negatives.min()) and int(negatives.max()) < workload.item_count
    loaders = [DataLoader(SrrlDatasetKG(meta, 10, mode), 32, True, collate_fn=SrrlDatasetKG.collate_fn) for mode in MODES]
    it = OneShotIterator(*loaders)
    for step in range(7):
        positive, negatives, weight, mode, tails, heads, queries = it.next()
        assert mode == MODES[step % 3] and positive.shape == (32, 3) and negatives.shape == (32, 10) and weight.shape == (32,)
        assert tails.shape == heads.shape == queries.shape == (32, 1)
    assert it.step == 7


def test_state_dict_keys_and_shapes_equal_the_fixture(f15, workload):
    from ihgnn_amd.Models import HemPredictionLayer, Srrl
    torch.manual_seed(0)
    model = Srrl(dataset(workload), 32, None, 0.5)
    want = state(f15)
    got = model.state_dict()
    assert list(got.keys()) == list(want.keys())
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: v.shape for k, v in want.items()}
    assert model.PS.embedding_bag_vocabulary is None
    for table in (model.KG.embedding_user, model.KG.embedding_item, model.KG.embedding_bag_vocabulary, model.PS.embedding_user, model.PS.embedding_item):
        assert torch.allclose(table.weight.norm(dim=1), torch.ones(table.weight.shape[0]), atol=1e-6)         # row-normalised tables
    assert all(float(p.detach().abs().max()) == 0.0 for n, p in model.named_parameters() if n.endswith('bias'))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in want.items()})
    with pytest.raises(NotImplementedError):
        Srrl(dataset(workload), 32, HemPredictionLayer, 0.5)


def test_driver_accepts_the_model_and_refuses_what_cannot_apply(monkeypatch):
    from ihgnn_amd import Main
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Models import IHGNNLayer, Srrl, parse_model_type
    args = parse_args(['--model', 'Srrl'])
    assert parse_model_type[args.model] is Srrl and parse_model_type['srrl'] is Srrl
    assert Main.result_directory('Synth/Tiny/', 2, IHGNNLayer, 3, 32, Srrl) == os.path.join('Results', 'Synth-Tiny-Srrl-emb32')
    assert Main.result_directory('Synth/Tiny/', 2, IHGNNLayer, 3, 32) == os.path.join('Results', 'Synth-Tiny-RawGnn-2IHGNNLayer-O3-emb32')
    assert (Gs.Srrl.KG_loss, Gs.Srrl.uni_weight, Gs.Srrl.regularization) == (True, False, 0) and Gs.negative_sample_size == 10
    Main.check_srrl_settings(args, 1)
    with pytest.raises(NotImplementedError, match='single process'):
        Main.check_srrl_settings(args, 2)
    with pytest.raises(NotImplementedError, match='record_step'):
        Main.check_srrl_settings(parse_args(['--model', 'Srrl', '--record_step', 'on']), 1)
    with pytest.raises(NotImplementedError, match='device_sampling'):
        Main.check_srrl_settings(parse_args(['--model', 'Srrl', '--device_sampling']), 1)
    with pytest.raises(ValueError, match='phase2'):
        Main.check_srrl_settings(parse_args(['--model', 'Srrl', '--phase2']), 1)
    monkeypatch.setattr(Gs, 'batch_size', 3000)                          # 3000 x 11 rows > 32768
    with pytest.raises(ValueError, match='32768'):
        Main.check_srrl_settings(args, 1)
    monkeypatch.setattr(Gs, 'batch_size', 2978)                          # 32758 rows: fine
    Main.check_srrl_settings(args, 1)
    monkeypatch.setattr(Gs, 'embedding_size', 129)                       # concatenated rows of 258 floats: beyond the block kernels' 256
    with pytest.raises(ValueError, match='--emb 129'):
        Main.check_srrl_settings(args, 1)
    monkeypatch.setattr(Gs, 'embedding_size', 128)
    Main.check_srrl_settings(args, 1)


def test_new_symbols_are_declared_exported_and_the_abi_version_stays():
    header = open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 37 and _lib.load().ihg_abi_version() == 37
    assert 'srrl.hip' in [os.path.basename(p) for p in __import__('ihgnn_amd.build', fromlist=['SOURCES']).SOURCES]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    ok, INV, WS = ctypes.c_void_p(16), _lib.ERR_INVALID, _lib.ERR_WORKSPACE
    width = int(lib.ihg_cat_linear_max_width())
    assert width == 256

    def fwd(wa=32, wb=32, m=32, n=32, rep_b=1, act=_lib.ACT_LEAKY_RELU, ld_out=None, p=ok):
        return lib.ihg_cat_linear_fwd(p, wa, wa, None, 1, p, wb, wb, None, rep_b, p, wa + wb, None, m, 1, act, p, m if ld_out is None else ld_out, p, n, None)

    def bwd(wa=32, wb=32, m=32, n=32, ws=ok, ws_bytes=1 << 40, dw=ok, p=ok):
        return lib.ihg_cat_linear_bwd(p, m, p, m, p, wa, wa, None, 1, p, wb, wb, None, 1, p, p, wa + wb, m, 1, _lib.ACT_LEAKY_RELU, dw, wa + wb, None, None, wa, None, wb, n, ws,
                                      ws_bytes, None)
    for bad in (dict(wa=0), dict(m=0), dict(n=-1), dict(rep_b=0), dict(wa=width, wb=1), dict(m=width + 1), dict(act=1), dict(act=7), dict(n=33, rep_b=10), dict(ld_out=31),
                dict(p=None)):
        assert fwd(**bad) == INV, bad
    assert fwd(n=0, p=None) == _lib.OK                                   # no rows: nothing to do
    assert bwd(dw=None) == INV and bwd(p=None) == INV and bwd(ws=None) == INV and bwd(ws=ctypes.c_void_p(8)) == INV
    assert bwd(ws_bytes=int(lib.ihg_cat_linear_workspace_bytes(32, 64, 32)) - 1) == WS and 'workspace too small' in _lib.last_error()
    assert int(lib.ihg_cat_linear_workspace_bytes(32, 64, 32)) == 4 * (64 * (32 * 64 + 32) + 32 * 64)
    assert int(lib.ihg_cat_linear_workspace_bytes(32, width + 1, 32)) == -1 and int(lib.ihg_cat_linear_workspace_bytes(-1, 64, 32)) == -1
    assert lib.ihg_rows_dot_fwd(ok, 32, ok, 32, 10, ok, 33, 32, None) == INV and lib.ihg_rows_dot_fwd(None, 32, None, 32, 1, None, 0, 32, None) == _lib.OK
    assert lib.ihg_rows_dot_bwd(None, ok, 32, ok, 32, 1, ok, 32, ok, 32, 5, 32, None) == INV and lib.ihg_rows_dot_bwd(ok, ok, 32, ok, 32, 1, ok, 31, None, 0, 5, 32, None) == INV
    assert lib.ihg_kg_loss(ok, ok, 10, None, 0, 10, ok, ok, ok, 10, None) == INV and lib.ihg_kg_loss(ok, ok, 9, None, 5, 10, ok, ok, ok, 10, None) == INV
    assert lib.ihg_kg_loss(ok, ok, 10, None, 5, 10, None, ok, ok, 10, None) == INV
    for k in (0, 129):
        assert lib.ihg_rows_topk(ok, 50, 4, 50, k, ok, ok, None) == INV and '1 .. 128' in _lib.last_error()
    assert lib.ihg_rows_topk(ok, 49, 4, 50, 10, ok, ok, None) == INV and lib.ihg_rows_topk(ok, 50, 4, 50, 10, None, ok, None) == INV
    assert lib.ihg_rows_topk(None, 50, 0, 50, 10, None, None, None) == _lib.OK


def test_new_ops_refuse_cpu_tensors():
    from ihgnn_amd import ops
    x, w = torch.zeros(4, 8), torch.zeros(5, 16)
    for call in (lambda: ops.cat_linear(x, x, w, None), lambda: ops.rows_dot(x, x), lambda: ops.kg_loss(torch.zeros(4), torch.zeros(4, 3)), lambda: ops.rows_topk(x, 2),
                 lambda: ops.bce_with_logits(torch.zeros(4), torch.zeros(4)), lambda: ops.gather_rows(x, torch.zeros(2, dtype=torch.long)),
                 lambda: ops.scatter_row_gradients(x, torch.zeros(4, dtype=torch.long), 3)):
        with pytest.raises(_lib.IhgnnHipError, match='no CPU path'):
            call()


def test_product_still_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(REPO, 'ihgnn_amd')):
        for fn in files:
            if fn.endswith(('.py', '.hip', '.hpp', '.h')):
                assert 'oracle' not in open(os.path.join(root, fn)).read(), fn
