"""GPU: the GAT attention (csrc/gat.hip + K7, ``ops.gat_attention``, ``GATLayer``) against the reference (fixture F11, tests/golden/make_golden_gat.py) and
against a float64 restatement of ``GnnLayers.py:98-115`` kept in this file."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RTOL = 1e-5
ROW_RTOL = 1e-5
HEADS = {'concat': 'concatenation', 'product': 'product'}
ACTIVATIONS = {'leaky_relu': (nn.LeakyReLU, 'leaky_relu'), 'relu': (nn.ReLU, 'relu'), 'tanh': (nn.Tanh, 'tanh')}


def dev():
    return torch.device('cuda:0')


def rel(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def row_rel(a, b, floor=1e-3):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    mag = np.abs(b).max(1)
    keep = mag > floor * max(mag.max(), 1e-30)
    if not keep.any():
        return 0.0
    return float((np.abs(a - b).max(1)[keep] / mag[keep]).max())


class settings:
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


_ACT64 = {'leaky_relu': lambda t: torch.nn.functional.leaky_relu(t, 0.01), 'relu': torch.relu, 'tanh': torch.tanh}


def attention64(h, w, c, ptr, ids, head, act):
    """float64 restatement of GnnLayers.py:100-115 over the CSR (entry p of row v, column u: the edge u -> v)."""
    n = h.shape[0]
    ptr = torch.as_tensor(np.asarray(ptr, np.int64))
    src = torch.as_tensor(np.asarray(ids, np.int64))
    dst = torch.repeat_interleave(torch.arange(n), torch.diff(ptr))
    d = h.shape[1]
    w = w.reshape(-1)
    if head == 'concatenation':
        pre = h[src] @ w[:d] + h[dst] @ w[d:] + c.reshape(())
    else:
        pre = (h[src] * h[dst]) @ w + c.reshape(())
    pre.retain_grad() if pre.requires_grad else None
    z = _ACT64[act](pre)
    top = torch.full((n,), -float('inf'), dtype=z.dtype).scatter_reduce(0, dst, z.detach(), 'amax', include_self=True)
    e = torch.exp(z - top[dst])
    den = torch.zeros(n, dtype=z.dtype).index_add(0, dst, e)
    alpha = e / den[dst]
    attention64.pre = pre                                         # (the scores before the activation: their gradient sizes the cancelling sums)
    return torch.zeros(n, d, dtype=h.dtype).index_add(0, dst, alpha[:, None] * h[src]), alpha


def layer64(x, W, b, w, c, ptr, ids, head, act):
    h = x @ W.t() + b
    h.retain_grad() if h.requires_grad else None
    layer64.h = h                                                 # (its gradient: the attention's input gradient, before the transform's)
    return attention64(h, w, c, ptr, ids, head, act)


def pair_layout(seed=5, U=300, Q=40, I=200, E=3000, heavy_threshold=None, completeness='uqi', isolated=0):
    from ihgnn_amd import synth
    from ihgnn_amd.layout import PairLayout
    w = synth.draw(U, Q, I, 10, E, seed=seed, distribution='powerlaw', exponent=1.1)
    triples = w.triples
    if isolated:
        # the last `isolated` users / items take part in nothing: no edges, an exact zero row
        keep = (triples[:, 0] < U - isolated) & (triples[:, 2] < I - isolated)
        triples = triples[keep]
    return PairLayout(triples, U, Q, I, dev(), completeness=completeness, heavy_threshold=heavy_threshold)


def run_layer_parts(lay, d, head, act, seed, wide=None, c_value=None, zero_w=False):
    """(got y, dx, dW, db, dw, dc) from the HIP path and (the float64 ones) for a layer x W^T + b -> attention on ``lay``."""
    from ihgnn_amd import ops
    g = torch.Generator().manual_seed(seed)
    n = lay.node_count
    wide = wide or d
    x = torch.randn(n, d, generator=g)
    W = torch.randn(d, d, generator=g) / d ** 0.5
    b = torch.randn(d, generator=g) * 0.1
    w = torch.randn(2 * d if head == 'concatenation' else d, generator=g) / d ** 0.5
    if zero_w:
        w.zero_()
    c = torch.full((1,), float(c_value), dtype=torch.float32) if c_value is not None else torch.randn(1, generator=g)
    cot = torch.randn(n, d, generator=g)
    xs = [t.double().requires_grad_(True) for t in (x, W, b, w, c)]
    y64, alpha64 = layer64(*xs, lay.csr.ptr_host, lay.csr.ids_host, head, act)
    y64.backward(cot.double())
    want = [y64.detach()] + [t.grad for t in xs]
    run_layer_parts.dh = layer64.h.grad
    run_layer_parts.dc_scale = float(attention64.pre.grad.abs().sum())      # dc = sum of the scores' gradients, which cancel row by row
    # device: features zero-padded to `wide` columns (weights as zero-padded blocks) when wide > d
    xd = ops.pad_columns(x, wide).to(dev()).requires_grad_(True)
    Wd = ops.pad_square(W, wide).to(dev()).requires_grad_(True)
    bd = ops.pad_vector(b, wide).to(dev()).requires_grad_(True)
    wv = (ops.pad_columns(w.view(2, d), wide).reshape(-1) if head == 'concatenation' else ops.pad_vector(w, wide)).to(dev()).requires_grad_(True)
    cd = c.to(dev()).requires_grad_(True)
    h = xd @ Wd.t() + bd
    h.retain_grad()
    y = ops.gat_attention(h, lay, wv, cd, head, act)
    y.backward(ops.pad_columns(cot, wide).to(dev()))
    dwv = wv.grad.cpu()
    if wide != d:
        dwv = dwv.view(2, wide)[:, :d].reshape(-1) if head == 'concatenation' else dwv[:d]
        assert float(y.detach()[:, d:].abs().max()) == 0.0 and float(xd.grad[:, d:].abs().max()) == 0.0
    got = [y.detach()[:, :d].cpu(), xd.grad[:, :d].cpu(), Wd.grad[:d, :d].cpu(), bd.grad[:d].cpu(), dwv, cd.grad.cpu()]
    run_layer_parts.dh_got = h.grad[:, :d].cpu()
    return got, want, alpha64.detach()


# ---------------------------------------------------------------------------------------------
# F11: against the reference
# ---------------------------------------------------------------------------------------------
F11_CASES = [('tiny_uqi_d8_concat_leaky', 'tiny', 8, 'uqi', 'concat', 'leaky_relu'), ('tiny_qi_d8_product_tanh', 'tiny', 8, 'qi', 'product', 'tanh'),
             ('small_uqi_d64_concat_leaky', 'small', 64, 'uqi', 'concat', 'leaky_relu'), ('small_uqi_d64_product_leaky', 'small', 64, 'uqi', 'product', 'leaky_relu'),
             ('small_ui_d32_concat_relu', 'small', 32, 'ui', 'concat', 'relu'), ('small_qi_d32_product_relu', 'small', 32, 'qi', 'product', 'relu'),
             ('small_uqi_d32_concat_tanh', 'small', 32, 'uqi', 'concat', 'tanh'), ('small_ui_d8_product_leaky', 'small', 8, 'ui', 'product', 'leaky_relu')]


def f11_dataset(which):
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.Graph import Pps2DGraph
    if which == 'tiny':
        d = os.path.join(GOLDEN, 'f1_data')
        return GraphDataset(os.path.join(d, 'graph_info.txt'), os.path.join(d, 'queries_multihot.txt'), os.path.join(d, 'train_data.csv'), Pps2DGraph, 10, 0, dev())
    w = np.load(os.path.join(GOLDEN, 'f2_small_workload.npz'))
    U, Q, I, V = (int(x) for x in w['counts'])
    return GraphDataset.from_arrays(U, Q, I, V, w['bag_words'], w['bag_offsets'], w['triples'], graph_type=Pps2DGraph, device=dev())


@pytest.mark.parametrize('tag,which,d,mode,head,act', F11_CASES)
def test_f11_gat_layer_matches_reference(tag, which, d, mode, head, act):
    """y, dx and every parameter gradient of GATLayer against the reference's (DGL's two ops restated in torch, make_golden_gat.py).  Under ReLU / Tanh the
    reference's in-place squeeze (GnnLayers.py:111) leaves it without a backward: there the gradients are held against the float64 restatement."""
    from ihgnn_amd.Helpers.GlobalSettings import Gsv
    from ihgnn_amd.Models import GATLayer
    z = np.load(os.path.join(GOLDEN, 'f11_gat.npz'))
    with settings({'concat': Gsv.concat, 'product': Gsv.product}[head], ACTIVATIONS[act], mode):
        ds = f11_dataset(which)
        layer = GATLayer(dev(), ds, d, d)
    layer.load_state_dict({k[len(tag) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f'{tag}.sd.')})
    layer.to(dev())
    x = torch.from_numpy(z[f'{tag}.x']).to(dev()).requires_grad_(True)
    y = layer(x)
    cot = torch.from_numpy(z[f'{tag}.cot'])
    y.backward(cot.to(dev()))
    assert rel(y, z[f'{tag}.y']) <= RTOL
    if int(z[f'{tag}.has_grad']):
        assert rel(x.grad, z[f'{tag}.dx']) <= RTOL
        for name, p in layer.named_parameters():
            assert rel(p.grad, z[f'{tag}.grad.{name}']) <= RTOL, name
        return
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    x64 = torch.from_numpy(z[f'{tag}.x']).double().requires_grad_(True)
    lay = layer.graph
    y64, _ = layer64(x64, sd['feature_transform.weight'], sd['feature_transform.bias'], sd['feature_aggregate.0.weight'], sd['feature_aggregate.0.bias'],
                     lay.csr.ptr_host, lay.csr.ids_host, HEADS[head], act)
    assert rel(y64, z[f'{tag}.y']) <= 1e-6                     # (the restatement is the reference's forward)
    y64.backward(cot.double())
    assert rel(x.grad, x64.grad) <= RTOL
    for name, p in layer.named_parameters():
        if name == 'feature_aggregate.0.bias':
            assert abs(float(p.grad) - float(sd[name].grad)) <= RTOL * float(attention64.pre.grad.abs().sum()), name      # (a cancelling sum, as below)
        else:
            assert rel(p.grad, sd[name].grad) <= RTOL, name


def test_f11_gat_model_matches_reference():
    from ihgnn_amd.Helpers.Graph import Pps2DGraph
    from ihgnn_amd.Models import GATLayer, HemPredictionLayer, RawGnn
    z = np.load(os.path.join(GOLDEN, 'f11_gat.npz'))
    ds = f11_dataset('small')
    assert ds.graph_type is Pps2DGraph
    m = RawGnn(dev(), ds, 16, GATLayer, 2, 1, False, HemPredictionLayer, 0.5).to(dev())
    sd = {k[len('model.sd.'):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('model.sd.')}
    assert set(sd) == set(m.state_dict())
    m.load_state_dict(sd)
    u, q, i = (torch.from_numpy(z[f'model.{k}']).to(dev()) for k in 'uqi')
    scores = m(u, q, i)
    loss = torch.nn.BCEWithLogitsLoss()(scores, torch.from_numpy(z['model.flags']).to(dev()))
    loss.backward()
    assert rel(scores, z['model.scores']) <= RTOL and abs(loss.item() - float(z['model.loss'])) <= 1e-6
    for name, p in m.named_parameters():
        want = z[f'model.grad.{name}']
        if name.endswith('feature_aggregate.0.bias') and abs(float(want.reshape(-1)[0])) < 1e-9:
            # the score bias of the last layer: every row's scores share it and its gradient cancels to rounding noise (reference: 1e-13) - held absolutely
            assert abs(float(p.grad)) <= 1e-9, name
            continue
        assert rel(p.grad, want) <= 2e-5, name


# ---------------------------------------------------------------------------------------------
# against the float64 restatement: widths, split rows, edge cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,wide', [(32, 32), (64, 64), (128, 128), (256, 256), (96, 128), (30, 30)])
@pytest.mark.parametrize('head', ['concatenation', 'product'])
@pytest.mark.parametrize('split', [False, True])
def test_gat_attention_matches_float64(d, wide, head, split):
    """Power-law pair graph with isolated nodes, split rows forced (threshold 8) or not (threshold above every row); padded 96 -> 128 runs the zero-padded
    attention vector; 30 runs the 4-byte path.  Isolated nodes: exact zero output and input gradient."""
    lay = pair_layout(seed=d, heavy_threshold=8 if split else 1 << 30, isolated=7)
    assert (lay.csr.n_heavy > 0) == split
    deg = np.diff(lay.csr.ptr_host)
    assert (deg == 0).sum() >= 7
    got, want, _ = run_layer_parts(lay, d, head, 'leaky_relu', seed=d + 3, wide=wide)
    names = ('y', 'dx', 'dW', 'db', 'dw')
    for name, a, b in zip(names, got, want):
        assert rel(a, b) <= RTOL, (name, rel(a, b))
    # per row: the output, and the attention's input gradient dh (dx = dh W adds the test's own fp32 torch matmul, held to RTOL above).  The product head's dh
    # rows at d >= 96 sum w * (ds + ds[mirror]) h_u over terms that cancel, 1.0 - 1.2e-5 per row here: held to RTOL over the tensor above; per row at d = 128
    # on the C3 graph (test_gat_on_the_c3_pair_graph)
    assert row_rel(got[0], want[0]) <= ROW_RTOL
    if head == 'concatenation' or wide <= 64:
        assert row_rel(run_layer_parts.dh_got, run_layer_parts.dh) <= ROW_RTOL
    # dc sums the scores' gradients, which cancel inside every row (sum alpha (d alpha - c) = 0): held to RTOL of the sum of their magnitudes
    assert abs(float(got[5]) - float(want[5])) <= RTOL * run_layer_parts.dc_scale
    iso = torch.from_numpy(deg == 0)
    assert float(got[0][iso].abs().max()) == 0.0 and float(got[1][iso].abs().max()) == 0.0


@pytest.mark.parametrize('head', ['concatenation', 'product'])
@pytest.mark.parametrize('act', ['leaky_relu', 'relu', 'tanh'])
def test_gat_attention_edge_cases(head, act):
    """Rows of length 1 (alpha = 1), all-equal scores (w = 0: alpha = 1 / degree), scores around +-80 and around 100 - exp(100) overflows fp32 on its own, so under
    LeakyReLU / ReLU every row's softmax depends on the row maximum being subtracted first."""
    lay = pair_layout(seed=9, heavy_threshold=16, completeness='ui')
    deg = np.diff(lay.csr.ptr_host)
    assert (deg == 1).any() and lay.csr.n_heavy > 0
    for c_value, zero_w in ((None, False), (0.3, True), (80.0, False), (-80.0, False), (100.0, False)):
        got, want, alpha64 = run_layer_parts(lay, 32, head, act, seed=17, c_value=c_value, zero_w=zero_w)
        assert abs(float(got[5]) - float(want[5])) <= RTOL * max(run_layer_parts.dc_scale, 1e-6), c_value
        for name, a, b in zip(('y', 'dx', 'dW', 'db', 'dw'), got, want):
            if float(b.abs().max()) < 1e-12:
                # a gradient that vanishes: equal scores (the softmax absorbs c) or a saturated activation (tanh at 80: 1 - z^2 is 0 in fp32, 1e-69 in fp64)
                assert float(a.abs().max()) <= 1e-6, (c_value, name, a)
                continue
            assert rel(a, b) <= RTOL, (c_value, zero_w, name, rel(a, b))
    # alpha itself: 1 on rows of length 1, 1 / degree under equal scores, rows summing to one
    g = torch.Generator().manual_seed(3)
    h = torch.randn(lay.node_count, 32, generator=g).to(dev())
    for zero_w in (False, True):
        w = torch.zeros(64 if head == 'concatenation' else 32, device=dev()) if zero_w else torch.randn(64 if head == 'concatenation' else 32, generator=g).to(dev())
        alpha = gat_alpha(h, lay, w, torch.full((1,), 80.0, device=dev()), head, act)
        rows = np.repeat(np.arange(lay.node_count), deg)
        sums = np.bincount(rows, weights=alpha.astype(np.float64), minlength=lay.node_count)
        assert np.abs(sums[deg > 0] - 1).max() <= 1e-6
        assert (alpha[np.repeat(deg == 1, deg)] == 1.0).all()
        if zero_w:
            np.testing.assert_allclose(alpha, 1.0 / deg[rows], rtol=2e-7)


def gat_alpha(h, lay, w, c, head, act):
    """alpha of every entry from the forward launch itself (ihg_gat_attention_fwd)."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    csr = lay.csr
    n, d = h.shape
    z, alpha, am = (torch.empty(max(csr.nnz, 1), device=dev()) for _ in range(3))
    wsb = int(lib.ihg_gat_workspace_bytes(n, csr.n_segments, d, ops.GAT_HEADS[head]))
    ws = torch.empty(wsb // 4 + 4, device=dev())
    _lib.check(lib.ihg_gat_attention_fwd(ops._ptr(h), d, ops._ptr(csr.ptr), ops._ptr(csr.ids), ops._ptr(lay.mirror), ops._ptr(csr.row_order), n, d, ops._ptr(w),
                                         ops._ptr(c), ops.GAT_HEADS[head], ops.GAT_ACTIVATIONS[act], *ops._split_row_args(csr), ops._ptr(z), ops._ptr(alpha), ops._ptr(am),
                                         ops._ptr(ws), wsb, ops._stream()), 'fwd')
    a = alpha.cpu().numpy()[:csr.nnz]
    np.testing.assert_array_equal(am.cpu().numpy()[:csr.nnz][lay.mirror_host], a)       # the mirrored copy is the same numbers at the reverse positions
    return a


@pytest.mark.parametrize('head', ['concatenation', 'product'])
def test_gat_attention_is_bitwise_reproducible(head):
    lay = pair_layout(seed=4, heavy_threshold=8)
    outs = []
    for _ in range(2):
        got, _, _ = run_layer_parts(lay, 64, head, 'leaky_relu', seed=5)
        outs.append(got)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def attention64_device(h, w, c, src, dst, n, head, act, chunk=1 << 20):
    """The float64 restatement of ``attention64`` run with torch ops on the device, in chunks of entries under activation checkpointing: at C3 an
    ``[nnz, d]`` float64 tensor is 12 GB, here at most ``chunk`` rows of one exist at a time.  Returns (out, alpha, scores before the activation)."""
    from torch.utils.checkpoint import checkpoint
    nnz, d = int(src.shape[0]), int(h.shape[1])
    spans = [(i, min(i + chunk, nnz)) for i in range(0, nnz, chunk)]
    if head == 'concatenation':
        pre = (h @ w[:d])[src] + (h @ w[d:])[dst] + c.reshape(())
    else:
        pre = torch.cat([checkpoint(lambda hh, ww, s0, s1: (hh[s0] * hh[s1]) @ ww, h, w, src[a:b], dst[a:b], use_reentrant=False) for a, b in spans])
        pre = pre + c.reshape(())
    pre.retain_grad()
    z = _ACT64[act](pre)
    top = torch.full((n,), -float('inf'), dtype=z.dtype, device=z.device).scatter_reduce(0, dst, z.detach(), 'amax', include_self=True)
    e = torch.exp(z - top[dst])
    den = torch.zeros(n, dtype=z.dtype, device=z.device).index_add(0, dst, e)
    alpha = e / den[dst]
    out = torch.zeros(n, d, dtype=h.dtype, device=h.device)
    for a, b in spans:
        out = out.index_add(0, dst[a:b], checkpoint(lambda hh, al, s0: al[:, None] * hh[s0], h, alpha[a:b], src[a:b], use_reentrant=False))
    return out, alpha, pre


@pytest.mark.parametrize('head', ['concatenation', 'product'])
def test_gat_on_the_c3_pair_graph(head):
    """The C3-size pair graph (N = 376 k, nnz = 12.1 M, the default split-row plan: about 2,000 split rows, up to thousands of entries each) at d = 128, forward AND
    backward against the float64 restatement over the whole graph (torch float64 on the device, chunked): the output and the input gradient on 300 sampled
    rows plus the 20 heaviest at ROW_RTOL, the attention-vector gradient at RTOL, the score bias's gradient (a sum over all 12 M scores) at RTOL of the sum of its
    terms' magnitudes, and alpha of every non-empty row summing to one."""
    from ihgnn_amd import ops, synth
    from ihgnn_amd.layout import PairLayout
    w = synth.draw_config('C3')
    lay = PairLayout(w.triples, w.user_count, w.query_count, w.item_count, dev())
    csr = lay.csr
    assert csr.n_heavy > 1000 and csr.max_row_len > 10 * csr.heavy_threshold
    n, d = lay.node_count, 128
    g = torch.Generator().manual_seed(13)
    h0 = torch.randn(n, d, generator=g) * 0.5
    w0 = torch.randn(2 * d if head == 'concatenation' else d, generator=g) / d ** 0.5
    c0 = torch.randn(1, generator=g)
    cot = torch.randn(n, d, generator=g).to(dev())
    h, wv, c = (t.to(dev()).requires_grad_(True) for t in (h0, w0, c0))
    y = ops.gat_attention(h, lay, wv, c, head, 'leaky_relu')
    y.backward(cot)
    alpha = gat_alpha(h.detach(), lay, wv.detach(), c.detach(), head, 'leaky_relu')
    deg = np.diff(csr.ptr_host.astype(np.int64))
    rows_of = np.repeat(np.arange(n), deg)
    sums = np.bincount(rows_of, weights=alpha.astype(np.float64), minlength=n)
    assert np.abs(sums[deg > 0] - 1).max() <= 1e-6
    h64, w64, c64 = (t.to(dev()).double().requires_grad_(True) for t in (h0, w0, c0))
    src = csr.ids.long()
    dst = torch.repeat_interleave(torch.arange(n, device=dev()), torch.from_numpy(deg).to(dev()))
    y64, _, pre64 = attention64_device(h64, w64, c64, src, dst, n, head, 'leaky_relu')
    y64.backward(cot.double())
    rng = np.random.default_rng(1)
    pick = torch.from_numpy(np.unique(np.concatenate([rng.choice(np.nonzero(deg > 0)[0], 300, replace=False), np.argsort(-deg)[:20]])))
    assert row_rel(y.detach().cpu()[pick], y64.detach().cpu()[pick]) <= ROW_RTOL
    assert row_rel(h.grad.cpu()[pick], h64.grad.cpu()[pick]) <= ROW_RTOL
    assert rel(wv.grad, w64.grad) <= RTOL
    assert abs(float(c.grad) - float(c64.grad)) <= RTOL * float(pre64.grad.abs().sum())


# ---------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------
def gat_dataset(seed=21):
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.Graph import Pps2DGraph
    w = synth.draw(300, 40, 200, 50, 4000, seed=seed, distribution='powerlaw')
    return GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, graph_type=Pps2DGraph,
                                    device=dev())


def test_gat_bce_step_matches_the_plain_loss():
    """``bce_loss`` (fused batch tail) of a 2-layer GAT model equals ``BCEWithLogitsLoss(model(u, q, i))`` in loss and every gradient, and the layer gradients of
    the plain path hold the float64 model."""
    from ihgnn_amd.Models import GATLayer, HemPredictionLayer, RawGnn
    ds = gat_dataset()
    u, q, i, y = next(iter(ds.sample_batches(80, 1, seed=3)))
    torch.manual_seed(5)
    m = RawGnn(dev(), ds, 64, GATLayer, 2, 1, False, HemPredictionLayer, 0.5).to(dev())
    loss = m.bce_loss(u, q, i, y)
    loss.backward()
    fused = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    plain = torch.nn.BCEWithLogitsLoss()(m(u, q, i), y.float())
    plain.backward()
    assert abs(loss.item() - plain.item()) <= 1e-6 * max(1.0, abs(plain.item()))
    for k, p in m.named_parameters():
        assert grad_close(fused[k], p.grad), k
    # float64: the same model restated (embeddings -> two GAT layers -> HEM over the batch rows)
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    x0 = m.embeddings.all_nodes().detach().cpu().double().requires_grad_(True)
    lay = m.gnns[0].graph
    feats = [x0]
    for l in range(2):
        p = f'gnn_{l}.'
        feats.append(layer64(feats[-1], sd[p + 'feature_transform.weight'], sd[p + 'feature_transform.bias'], sd[p + 'feature_aggregate.0.weight'],
                             sd[p + 'feature_aggregate.0.bias'], lay.csr.ptr_host, lay.csr.ids_host, 'concatenation', 'leaky_relu')[0])
    f = torch.cat(feats, 1)
    uu, qq, ii = u.cpu(), q.cpu() + ds.query_start_index_in_graph, i.cpu() + ds.item_start_index_in_graph
    s = ((0.5 * f[qq] + 0.5 * f[uu]) * f[ii]).sum(1) + sd['prediction_layer.items_bias'][i.cpu()]
    l64 = torch.nn.BCEWithLogitsLoss()(s, y.cpu().double())
    l64.backward()
    assert abs(loss.item() - l64.item()) <= 1e-5 * abs(l64.item())
    for k in ('gnn_0.feature_aggregate.0.weight', 'gnn_0.feature_aggregate.0.bias', 'gnn_1.feature_aggregate.0.bias', 'gnn_1.feature_transform.weight',
              'prediction_layer.items_bias'):
        assert grad_close(fused[k], sd[k].grad), k


def grad_close(a, b):
    """RTOL - except for a score bias whose gradient cancels to rounding noise (every score of a row shares it and the softmax absorbs it: the sum over
    a row of alpha (d alpha - c) is zero, and so is the layer's gradient when the row's scores share their sign): there, both are below 1e-9."""
    b = b.detach().cpu().double()
    if b.numel() == 1 and float(b.abs()) < 1e-9:
        return float(a.detach().abs().max()) < 1e-9
    return rel(a, b) <= RTOL


def test_gat_recorded_step_equals_the_eager_step():
    """A GAT training step recorded by CapturedTrainingStep and replayed equals the eager step over four steps (losses 1e-6, parameters 1e-6)."""
    from ihgnn_amd.captured_step import CapturedTrainingStep
    from ihgnn_amd.Models import GATLayer, HemPredictionLayer, RawGnn
    from ihgnn_amd.optim import Adam
    ds = gat_dataset()
    batches = list(ds.sample_batches(100, 4, seed=5))

    def run(recorded):
        torch.manual_seed(7)
        m = RawGnn(dev(), ds, 64, GATLayer, 2, 1, False, HemPredictionLayer, 0.5).to(dev())
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
        return losses, {k: v.clone() for k, v in m.state_dict().items()}

    l0, p0 = run(False)
    l1, p1 = run(True)
    np.testing.assert_allclose(l1, l0, rtol=1e-6)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 1e-6, k


def test_gat_driver_epoch(tmp_path, monkeypatch):
    """The driver with ``--gnn GAT`` on a small synthetic corpus: two epochs train and test with finite metrics, eager and recorded alike."""
    import random
    from ihgnn_amd import Main as driver, synth
    w = synth.draw(200, 30, 150, 40, 3000, seed=8, eval_logs=40)
    synth.write_files(w, str(tmp_path / 'Data' / 'Synth' / 'Tiny'))
    monkeypatch.chdir(tmp_path)
    args = ['--ds', 'Synth/Tiny/', '--gnn', 'GAT', '--gnns', '2', '--emb', '32', '--ec', '2', '--est', '2', '--etf', '1', '--record_step']
    random.seed(11); torch.manual_seed(11)
    eager = driver.main(args + ['off'])
    random.seed(11); torch.manual_seed(11)
    recorded = driver.main(args + ['on'])
    (_, m_e), (_, m_r) = list(eager.iter_epoch_test())[-1], list(recorded.iter_epoch_test())[-1]
    for m in (m_e, m_r):
        assert np.isfinite([m.HitRatio_at10, m.NDCG_at10, m.MAP_at10]).all()
    assert abs(m_e.NDCG_at10 - m_r.NDCG_at10) <= 2e-3 and abs(m_e.HitRatio_at10 - m_r.HitRatio_at10) <= 2e-3
    assert eager.training_step_recorded is False and recorded.training_step_recorded is True
    assert os.path.isdir(tmp_path / 'Results' / 'Synth-Tiny-RawGnn-2GATLayer-emb32')


def test_gat_layer_launches_only_library_kernels(tmp_path):
    """GATLayer's forward + backward at d = 64 (its node transform included; both heads) under a kernel trace: every kernel after the marker launch is one of
    the library's."""
    import csv
    import glob
    import shutil
    import subprocess
    import sys
    profiler_exe = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    if not os.path.exists(profiler_exe):
        pytest.skip('rocprofv3 not available')
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'gat_trace.py'
    script.write_text(f'''
import sys
sys.path.insert(0, {repo!r})
import torch
from ihgnn_amd import _lib, ops, synth
from ihgnn_amd.Dataset import GraphDataset
from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
from ihgnn_amd.Helpers.Graph import Pps2DGraph
from ihgnn_amd.Models import GATLayer
dev = torch.device('cuda:0')
w = synth.draw(300, 40, 200, 50, 3000, seed=5, distribution='powerlaw', exponent=1.1)
ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, graph_type=Pps2DGraph, device=dev)
torch.manual_seed(1)
layers = []
for head in (Gsv.concat, Gsv.product):
    Gs.Gnn.gat_head = head
    layers.append(GATLayer(dev, ds, 64, 64).to(dev))
x = torch.randn(ds.node_count, 64, device=dev).requires_grad_(True)
cot = torch.randn(ds.node_count, 64, device=dev)
marker = torch.empty(8, dtype=torch.int64, device=dev)
for rep in range(3):
    if rep == 2:                                               # the marker: a library launch the layer never makes
        torch.cuda.synchronize()
        _lib.check(_lib.load().ihg_sample_negatives(1, 0, 4, 100, 2, ops._ptr(marker), ops._stream()), 'marker')
    for layer in layers:
        layer.zero_grad(set_to_none=True)                      # (no accumulation into earlier gradients: autograd keeps the library's tensors)
        x.grad = None
        layer(x).backward(cot)
torch.cuda.synchronize()
print('gat done')
''')
    out = str(tmp_path / 'trace')
    r = subprocess.run([profiler_exe, '--kernel-trace', '--output-format', 'csv', '-d', out, '--', sys.executable, str(script)], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0 and 'gat done' in r.stdout, r.stderr[-2000:]
    files = glob.glob(os.path.join(out, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no kernel trace written'
    rows = sorted(csv.DictReader(open(files[0])), key=lambda x: int(x['Start_Timestamp']))
    names = [x['Kernel_Name'] for x in rows]
    marks = [k for k, n in enumerate(names) if 'sample_negatives_kernel' in n]
    assert len(marks) == 1, marks
    last = names[marks[0] + 1:]                                  # the two layers' forward + backward
    foreign = [n for n in last if 'at::native' in n or '__amd_rocclr' in n or 'elementwise_kernel' in n]
    assert not foreign, foreign
    short = sorted({n.split('(')[0] for n in last})
    for want in ('attn_project_kernel', 'attn_softmax_kernel', 'gat_row_dot_kernel', 'node_segment_sum_kernel', 'gat_softmax_bwd_kernel', 'gat_source_sums_kernel',
                 'gat_symmetrize_kernel', 'gat_param_partials_kernel', 'gat_param_finish_kernel', 'attn_node_grad_kernel'):
        assert any(want in n for n in last), (want, short)
    gat = {n for n in short if 'gat_' in n or 'attn_' in n or 'node_segment_sum' in n or 'heavy_finish' in n}
    assert len(short) > len(gat), short                          # the node transform's kernels (forward, input and weight gradients) are in the window too
