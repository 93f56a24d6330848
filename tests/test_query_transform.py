"""GPU: the query transform ``Gs.Query.transform == 'activation'`` (``ihg_rows_linear_act_fwd/bwd`` in csrc/dense.hip, the four query-row producers of
``ihgnn_amd.ops``, ``EmbeddingLayer.query_transform``, ``--query_transform``) against a float64 restatement (``tests/query_transform_reference.py``, held to the
reference by ``tests/test_query_transform_host.py``) and the reference's own numbers (fixture F13, ``tests/golden/make_golden_query_transform.py``).

Bars: RTOL = 1e-5 of the tensor's largest magnitude (DESIGN section 5's contract), per row as well (``row_rel``); a loss 1e-4; ranking metrics +- 0.002.

The ReLU kink.  ``dz = dy * [z > 0]``: where the float64 ``z`` is within fp32 rounding of zero an fp32 evaluation may land on the other side and the gradient moves by a
whole ``dy`` entry.  The kernel tests remove that ambiguity from their INPUTS: ``tau[q, j] = (d + longest bag + 8) 2^-23 (sum_k |m_k W_jk| + |b_j|)`` is the worst-case
rounding of the fp32 path, computed from the float64 operands alone (``kink_threshold``); the cotangent is set to zero at the entries with ``|z| < tau``, and at most
1 % of the entries may be such (asserted).  F13's model cases were generated on seeds for which no query pre-activation is that close (the stored margin)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import query_transform_reference as qref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RTOL = 1e-5
ROW_RTOL = 1e-5
LOSS_RTOL = 1e-4
ACTS = {'relu': nn.ReLU, 'tanh': nn.Tanh}
MODEL_CASES = (('ihgnn_o3_d32', 'ihgnn', 2, 3, 32), ('ihgnn_o2_d64', 'ihgnn', 2, 2, 64), ('hgcn_d64', 'hgcn', 2, 1, 64))
EMB = 'embeddings.'


def dev():
    return torch.device('cuda:0')


def as64(a):
    return a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)


def rel(a, b):
    a, b = as64(a), as64(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def row_rel(a, b, floor=1e-3):
    """Largest per-row relative error over the rows of ``b`` (the reference) above ``floor`` of its largest row; the floor may leave out at most 5 % of the rows."""
    a, b = as64(a), as64(b)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    mag = np.abs(b).max(1)
    keep = mag > floor * max(mag.max(), 1e-30)
    assert int((~keep).sum()) <= 0.05 * max(len(keep), 1), int((~keep).sum())
    return float((np.abs(a - b).max(1)[keep] / mag[keep]).max()) if keep.any() else 0.0


class query_settings:
    """``Gs.Query`` set for the block, put back after it."""

    def __init__(self, act):
        self.act = act

    def __enter__(self):
        from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
        self.old = (Gs.Query.transform, Gs.Query.transform_activation)
        Gs.Query.transform, Gs.Query.transform_activation = (Gsv.mean, nn.ReLU) if self.act is None else (Gsv.activation, ACTS[self.act])

    def __exit__(self, *exc):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        Gs.Query.transform, Gs.Query.transform_activation = self.old


class arithmetic:
    """``IHG_INTERACT_ARITH`` for the block (read by the library at every call)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = os.environ.get('IHG_INTERACT_ARITH')
        if self.mode == 'f32':
            os.environ['IHG_INTERACT_ARITH'] = 'f32'
        else:
            os.environ.pop('IHG_INTERACT_ARITH', None)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop('IHG_INTERACT_ARITH', None)
        else:
            os.environ['IHG_INTERACT_ARITH'] = self.old


def f13():
    return np.load(os.path.join(GOLDEN, 'f13_query_transform.npz'))


def small():
    return np.load(os.path.join(GOLDEN, 'f2_small_workload.npz'))


def dataset_from_npz(w):
    from ihgnn_amd.Dataset import GraphDataset
    U, Q, I, V = (int(x) for x in w['counts'])
    return GraphDataset.from_arrays(U, Q, I, V, w['bag_words'], w['bag_offsets'], w['triples'], device=dev())


def synth_dataset(seed=21, counts=(300, 40, 200, 50, 4000), **kw):
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    w = synth.draw(*counts, seed=seed, distribution='powerlaw', **kw)
    return w, GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev())


def build_model(ds, kind, L, order, d, act):
    from ihgnn_amd.Models import HGCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn
    with query_settings(act):
        return RawGnn(dev(), ds, d, IHGNNLayer if kind == 'ihgnn' else HGCNLayer, L, order, False, HemPredictionLayer, 0.5).to(dev())


# ---------------------------------------------------------------------------------------------
# the kernels: forward, dW, db, dm against float64
# ---------------------------------------------------------------------------------------------
def bags(rows, vocab, rng, empty_every=7):
    """Random bags of 0 .. 6 words (bags 3, 10, 17, ... empty - the one-row case is a real mean; ``vocab == 1``: every word is the one word)."""
    lens = rng.integers(1, 7, rows)
    lens[3::empty_every] = 0
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return rng.integers(0, vocab, int(lens.sum())).astype(np.int64), offsets


def transform_case(d, rows, act, seed, vocab=50):
    """Operands, float64 results and the masked cotangent of one kernel case."""
    from ihgnn_amd import ops
    rng = np.random.default_rng(seed)
    words, offsets = bags(rows, vocab, rng)
    table = torch.from_numpy((rng.standard_normal((vocab + 1, d)) * 0.5).astype(np.float32))
    wq = torch.from_numpy((rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32))
    bq = torch.from_numpy((rng.standard_normal(d) * 0.2).astype(np.float32))
    t64, w64, b64 = (v.double().requires_grad_(True) for v in (table, wq, bq))
    m, z, y = qref.query_rows(t64, words + 1, offsets, w64, b64, act)
    m.retain_grad()
    cot = torch.from_numpy(rng.standard_normal((rows, d)).astype(np.float32))
    masked = 0.0
    if act == 'relu':
        near = z.detach().abs() < qref.kink_threshold(m.detach(), w64.detach(), b64.detach(), qref.longest_bag(words, offsets))
        masked = float(near.double().mean())
        assert masked <= 0.01, masked                                    # the cap: at most 1 % of the entries may be taken out
        cot = cot.masked_fill(near, 0.0)
    y.backward(cot.double())
    bag = ops.BagLayout(words + 1, offsets, vocab + 1, dev())
    return dict(bag=bag, table=table, wq=wq, bq=bq, cot=cot, y=y.detach(), m=m.detach(), dm=m.grad, dw=w64.grad, db=b64.grad, dtable=t64.grad, masked=masked)


@pytest.mark.parametrize('arith', ['split', 'f32'])
@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('rows', [1, 63, 1000, 26000])
@pytest.mark.parametrize('d', [32, 64, 128, 256, 96, 30])
def test_transform_kernels_match_float64(d, rows, act, arith):
    """``ops.bag_mean(table, bag, wq, bq, act)``: y, dW, db and (through the bag mean's backward, which consumes dm) the word table's gradient; dm itself from the raw
    entry point.  Empty bags (every 7th from the fourth: ``y = act(b)``) are in every case of 63 rows and more; one row: a one-row GEMM on a real mean (the one-row
    EMPTY bag is in ``test_transform_edge_cases``).  Per row as well: y and dm always, dW from 63 rows (with one row a ReLU unit that is off leaves a zero row of dW),
    the word table's gradient from 1,000 rows (below that most of the 51 words are in no bag: zero rows)."""
    from ihgnn_amd import _lib, ops
    c = transform_case(d, rows, act, seed=1000 * d + rows)
    with arithmetic(arith):
        table, wq, bq = (c[k].to(dev()).requires_grad_(True) for k in ('table', 'wq', 'bq'))
        y = ops.bag_mean(table, c['bag'], wq, bq, act)
        y.backward(c['cot'].to(dev()))
        # dm: the raw backward on the same operands
        lib = _lib.load()
        means = ops.bag_mean(table.detach(), c['bag'])
        dm, dw, db = torch.empty_like(means), torch.empty_like(wq), torch.empty_like(bq)
        ws = ops._workspace(int(lib.ihg_node_linear_workspace_bytes(d)), dev())
        cot = c['cot'].to(dev())
        _lib.check(lib.ihg_rows_linear_act_bwd(ops._ptr(cot), d, ops._ptr(y.detach()), d, ops._ptr(means), d, ops._ptr(wq.detach()), d, ops.QUERY_ACTIVATIONS[act],
                                               ops._ptr(dw), d, ops._ptr(db), ops._ptr(dm), d, rows, ops._ptr(ws), ws.numel() * 4, d, ops._stream()), 'bwd')
    errs = dict(y=rel(y, c['y']), dw=rel(wq.grad, c['dw']), db=rel(bq.grad, c['db']), dm=rel(dm, c['dm']), dtable=rel(table.grad, c['dtable']))
    print(f'd {d} rows {rows} {act} {arith}: ' + ' '.join(f'{k} {v:.2e}' for k, v in errs.items()) + f' | masked {c["masked"]:.4f}')
    assert torch.equal(dw, wq.grad) and torch.equal(db, bq.grad)        # the op and the raw call: the same launches
    for k, v in errs.items():
        assert v <= RTOL, (k, v)
    assert row_rel(y, c['y']) <= ROW_RTOL and row_rel(dm, c['dm']) <= ROW_RTOL
    if rows >= 63:
        assert row_rel(wq.grad, c['dw']) <= ROW_RTOL
    if rows >= 1000:
        assert row_rel(table.grad, c['dtable']) <= ROW_RTOL


@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('d', [64, 128, 30])
def test_transform_writes_a_column_slice(d, act):
    """``out`` as a column slice of a wider matrix (the feature matrix of ``RawGnn.propagate``): the same bits as the contiguous output, nothing outside the slice."""
    from ihgnn_amd import _lib, ops
    c = transform_case(d, 777, act, seed=5 + d)
    lib = _lib.load()
    table, wq, bq = (c[k].to(dev()) for k in ('table', 'wq', 'bq'))
    y = ops.bag_mean(table, c['bag'], wq, bq, act)
    means = ops.bag_mean(table, c['bag'])
    wide = torch.full((777, 3 * d + 4), 7.0, device=dev())
    out = wide[:, d + 4:2 * d + 4]
    ws = ops._workspace(int(lib.ihg_node_linear_workspace_bytes(d)), dev())
    _lib.check(lib.ihg_rows_linear_act_fwd(ops._ptr(means), d, ops._ptr(wq), d, ops._ptr(bq), ops.QUERY_ACTIVATIONS[act], ops._ptr(out), wide.stride(0), 777, ops._ptr(ws),
                                           ws.numel() * 4, d, ops._stream()), 'fwd')
    assert torch.equal(out, y)
    assert float((wide[:, :d + 4] - 7.0).abs().max()) == 0.0 and float((wide[:, 2 * d + 4:] - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_transform_edge_cases(act):
    """99 of 100 bags empty (``y = act(b)`` in those rows; they still count in ``db``, not in ``dW`` nor in the table's gradient), and a one-word vocabulary (every
    non-empty bag has the same mean)."""
    from ihgnn_amd import ops
    d = 64
    rng = np.random.default_rng(3)
    wq = torch.from_numpy((rng.standard_normal((d, d)) / 8).astype(np.float32))
    bq = torch.from_numpy(rng.standard_normal(d).astype(np.float32))
    table = torch.from_numpy(rng.standard_normal((3, d)).astype(np.float32))
    words, offsets = np.array([2], np.int64), np.zeros(100, np.int64)     # table rows: the last bag holds word row 2, every other bag is empty
    cot = torch.from_numpy(rng.standard_normal((100, d)).astype(np.float32))
    t64, w64, b64 = (v.double().requires_grad_(True) for v in (table, wq, bq))
    _, z, y64 = qref.query_rows(t64, words, offsets, w64, b64, act)
    if act == 'relu':
        assert float(z.detach().abs().min()) > 1e-4                      # (nowhere near the kink)
    y64.backward(cot.double())
    tg, wg, bg = (v.to(dev()).requires_grad_(True) for v in (table, wq, bq))
    y = ops.bag_mean(tg, ops.BagLayout(words, offsets, 3, dev()), wg, bg, act)
    y.backward(cot.to(dev()))
    want = qref.ACTIVATIONS[act](bq.double())
    assert rel(y[:99], want.expand(99, d)) <= RTOL and rel(y, y64) <= RTOL
    for got, ref64 in ((wg.grad, w64.grad), (bg.grad, b64.grad), (tg.grad, t64.grad)):
        assert rel(got, ref64) <= RTOL
    assert float(tg.grad[:2].abs().max()) == 0.0
    # one query, no word at all (the id list of its bag layout is empty): y = act(b), db = dy * act'(y), dW = 0, no gradient to the table
    tg, wg, bg = (v.to(dev()).requires_grad_(True) for v in (table, wq, bq))
    y = ops.bag_mean(tg, ops.BagLayout(np.zeros(0, np.int64), np.zeros(1, np.int64), 3, dev()), wg, bg, act)
    y.backward(cot[:1].to(dev()))
    slope = (want > 0).double() if act == 'relu' else 1 - want ** 2
    assert rel(y, want.view(1, d)) <= RTOL and rel(bg.grad, cot[0].double() * slope) <= RTOL
    assert float(wg.grad.abs().max()) == 0.0 and float(tg.grad.abs().max()) == 0.0
    # a one-word vocabulary
    c = transform_case(d, 500, act, seed=8, vocab=1)
    table, wq, bq = (c[k].to(dev()).requires_grad_(True) for k in ('table', 'wq', 'bq'))
    y = ops.bag_mean(table, c['bag'], wq, bq, act)
    y.backward(c['cot'].to(dev()))
    for got, want in ((y, c['y']), (wq.grad, c['dw']), (bq.grad, c['db']), (table.grad, c['dtable'])):
        assert rel(got, want) <= RTOL


def test_transform_is_bitwise_reproducible_and_checks_its_arguments():
    from ihgnn_amd import _lib, ops
    runs = []
    c = transform_case(128, 5000, 'tanh', seed=12)
    for _ in range(3):
        table, wq, bq = (c[k].to(dev()).requires_grad_(True) for k in ('table', 'wq', 'bq'))
        y = ops.bag_mean(table, c['bag'], wq, bq, 'tanh')
        y.backward(c['cot'].to(dev()))
        runs.append((y.detach().clone(), wq.grad.clone(), bq.grad.clone(), table.grad.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0]))
    with pytest.raises(ValueError):
        ops.bag_mean(c['table'].to(dev()), c['bag'], c['wq'].to(dev()), c['bq'].to(dev()), 'gelu')
    lib = _lib.load()
    x = torch.zeros(4, 32, device=dev())
    ws = ops._workspace(int(lib.ihg_node_linear_workspace_bytes(32)), dev())
    assert lib.ihg_rows_linear_act_fwd(ops._ptr(x), 32, ops._ptr(x), 32, None, 7, ops._ptr(x), 32, 4, ops._ptr(ws), ws.numel() * 4, 32, ops._stream()) == -1
    assert lib.ihg_rows_linear_act_fwd(ops._ptr(x), 32, ops._ptr(x), 32, None, 1, ops._ptr(x), 32, 4, ops._ptr(ws), 64, 32, ops._stream()) == -3


# ---------------------------------------------------------------------------------------------
# the layer and the models against F13
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_f13_embedding_layer_matches_reference(act):
    """``forward(None, None, None)``, ``all_nodes()``, ``embed_query(indices)`` and every parameter's gradient under F13's cotangents."""
    from ihgnn_amd.Models.EmbeddingLayers import EmbeddingLayer
    z = f13()
    ds = dataset_from_npz(small())
    pre = f'emb.{act}.'
    with query_settings(act):
        emb = EmbeddingLayer(ds, 32)
    sd = {k[len(pre) + 3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre + 'sd.')}
    assert list(sd) == list(emb.state_dict())
    emb.load_state_dict(sd)
    emb.to(dev())
    u, q, it = emb(None, None, None)
    assert rel(q, z[pre + 'queries']) <= RTOL and row_rel(q, z[pre + 'queries']) <= ROW_RTOL
    assert torch.equal(u.cpu(), torch.from_numpy(z[pre + 'users'])) and torch.equal(it.cpu(), torch.from_numpy(z[pre + 'items']))
    cots = [torch.from_numpy(z[pre + f'cot_{k}']).to(dev()) for k in ('users', 'queries', 'items')]
    ((u * cots[0]).sum() + (q * cots[1]).sum() + (it * cots[2]).sum()).backward()
    split = {n: p.grad.clone() for n, p in emb.named_parameters()}
    for n, g in split.items():
        assert rel(g, z[pre + 'grad.' + n]) <= RTOL, n
    emb.zero_grad(set_to_none=True)
    x = emb.all_nodes()                                                  # the same rows as one op
    assert torch.equal(x, torch.cat([u, q, it]).detach())
    x.backward(torch.cat(cots))
    for n, p in emb.named_parameters():
        assert rel(p.grad, z[pre + 'grad.' + n]) <= RTOL, n
    emb.zero_grad(set_to_none=True)
    picked = emb.embed_query(torch.from_numpy(z[pre + 'indices']).to(dev()))
    assert rel(picked, z[pre + 'picked']) <= RTOL
    picked.backward(torch.from_numpy(z[pre + 'cot_picked']).to(dev()))
    for n in ('embedding_bag_vocabulary.weight', 'query_transform.0.weight', 'query_transform.0.bias'):
        assert rel(emb.get_parameter(n).grad, z[pre + 'picked_grad.' + n]) <= RTOL, n


def adam_excess_against_fixture(z, prefix, got, g64, p64):
    """The stepped parameter against the entries F13 keeps of the reference's (whole, or every 8th row), as a multiple of ``qref.adam_allowance`` at RTOL: Adam's first
    step is steep where ``|g|`` is near eps, and a gradient that holds RTOL may move it by that much (the allowance comes from the float64 gradient alone)."""
    allowed = qref.adam_allowance(g64, p64, RTOL)
    got = as64(got)
    if prefix + '.full' in z.files:
        return float((np.abs(got - z[prefix + '.full'].astype(np.float64)) / allowed).max())
    return float((np.abs(got[::8] - z[prefix + '.rows8'].astype(np.float64)) / allowed[::8]).max())


@pytest.mark.parametrize('path', ['forward', 'bce_loss'])
@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('tag,kind,L,order,d', MODEL_CASES)
def test_f13_models_match_reference(tag, kind, L, order, d, act, path):
    """Scores, loss, every gradient and the parameters after one Adam step of F13's whole models, on both call paths: ``forward`` + ``BCEWithLogitsLoss`` (torch's Adam,
    as the reference's driver) and ``bce_loss`` (the fused batch tail; the library's Adam).  Every gradient against the float64 restatement as well, and the stepped
    parameters against the reference's and the float64 step within what the gradient's bar allows through Adam's first step (``qref.adam_allowance``)."""
    z, w = f13(), small()
    pre = f'{tag}.{act}.'
    ds = dataset_from_npz(w)
    m = build_model(ds, kind, L, order, d, act)
    sd = qref.fixture_state(z, tag)
    assert list(sd) == list(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    u, q, i = (torch.from_numpy(z[pre + k]).to(dev()) for k in 'uqi')
    flags = torch.from_numpy(z[pre + 'flags']).to(dev())
    if path == 'forward':
        opt = torch.optim.Adam(m.parameters(), 1e-3, weight_decay=0)
        scores = m(u, q, i)
        loss = torch.nn.BCEWithLogitsLoss()(scores, flags)
        assert rel(scores, z[pre + 'scores']) <= RTOL
    else:
        from ihgnn_amd.optim import Adam
        opt = Adam(m.parameters(), 1e-3, weight_decay=0)
        loss = m.bce_loss(u, q, i, flags)
    loss.backward()
    step64 = qref.model_step(sd, w['triples'], w['counts'], w['bag_words'] + 1, w['bag_offsets'], kind, L, order, act, z[pre + 'u'], z[pre + 'q'], z[pre + 'i'], z[pre + 'flags'])
    print(f'{tag} {act} {path}: loss {loss.item():.7f} reference {float(z[pre + "loss"]):.7f}')
    assert abs(loss.item() - float(z[pre + 'loss'])) <= LOSS_RTOL * abs(float(z[pre + 'loss']))
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        e_ref, e_64 = qref.fixture_error(z, pre + 'grad.' + n, p.grad), rel(p.grad, step64['grads'][n])
        print(f'   grad {n}: reference {e_ref:.2e} float64 {e_64:.2e}')
        assert e_ref <= RTOL and e_64 <= RTOL, n
    opt.step()
    for n, p in m.named_parameters():
        e_ref = adam_excess_against_fixture(z, pre + 'adam.' + n, p, step64['grads'][n], step64['adam'][n])
        e_64 = qref.adam_excess(p, step64['grads'][n], step64['adam'][n], RTOL)
        print(f'   adam {n}: largest error over its allowance: against the reference {e_ref:.2e}, against float64 {e_64:.2e} | plain relative to the reference '
              f'{qref.fixture_error(z, pre + "adam." + n, p):.2e}')
        assert e_ref <= 1.0 and e_64 <= 1.0, n


@pytest.mark.parametrize('path', ['module_calls', 'fused_step'])
def test_f13_training_curve_and_ranking_metrics(path):
    """48 Adam steps of the reference with the ReLU transform (F13's curve: IHGNN order 3 x 2 layers, d = 64, F10's workload) replayed on both call paths: losses to 1e-4,
    HR / NDCG / MAP@10 within 0.002."""
    from ihgnn_amd.Helpers.Metrics import Metrics
    c = np.load(os.path.join(GOLDEN, 'f13_query_transform_curve.npz'))
    w = np.load(os.path.join(GOLDEN, 'f10_workload.npz'))
    L, order, d, _ = (int(v) for v in c['curve.cfg'])
    ds = dataset_from_npz(w)
    m = build_model(ds, 'ihgnn', L, order, d, str(c['curve.act']))
    sd = {k[len('curve.sd.'):]: torch.from_numpy(c[k]) for k in c.files if k.startswith('curve.sd.')}
    assert list(sd) == list(m.state_dict())
    m.load_state_dict(sd)
    if path == 'fused_step':
        from ihgnn_amd.optim import Adam
        opt = Adam(m.parameters(), 1e-3, weight_decay=0)
    else:
        opt = torch.optim.Adam(m.parameters(), 1e-3, weight_decay=0)
    lossf = torch.nn.BCEWithLogitsLoss()
    losses = []
    for b in c['curve.batches']:
        u, q, i, fl = (torch.from_numpy(b[k].astype(np.int64)).to(dev()) for k in range(4))
        loss = m.bce_loss(u, q, i, fl.float()) if path == 'fused_step' else lossf(m(u, q, i), fl.float())
        loss.backward(); opt.step(); opt.zero_grad()
        losses.append(loss.item())
    print(f'F13 curve {path}: worst loss deviation {float(np.abs(np.array(losses) / c["curve.losses"] - 1).max()):.2e}')
    np.testing.assert_allclose(losses, c['curve.losses'], rtol=LOSS_RTOL)
    ends = np.cumsum(w['test_items_len'])
    acc = Metrics()
    with torch.no_grad():
        m.save_features_for_test()
        for k, (uu, qq) in enumerate(w['test_uq']):
            items = w['test_items_flat'][ends[k] - w['test_items_len'][k]:ends[k]].tolist()
            one = torch.tensor([int(uu)], device=dev()).expand(ds.item_count)
            oneq = torch.tensor([int(qq)], device=dev()).expand(ds.item_count)
            acc.add_to_self(Metrics.calculate_on_all_items(m(one, oneq, None), items, None, True))
        m.clear_saved_feature()
    avg = acc.divide_and_get_new(len(w['test_uq']))
    got = np.array([avg.HitRatio_at10, avg.NDCG_at10, avg.MAP_at10])
    print(f'F13 curve {path}: HR/NDCG/MAP@10 {got} reference {c["curve.metrics"]}')
    np.testing.assert_allclose(got, c['curve.metrics'], atol=2e-3)
    digest = np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in m.state_dict().values()])
    np.testing.assert_allclose(digest[:, 1], c['curve.final_digest'][:, 1], rtol=2e-5)


# ---------------------------------------------------------------------------------------------
# step forms
# ---------------------------------------------------------------------------------------------
def step_gradients(m, batch):
    m.zero_grad(set_to_none=True)
    loss = m.bce_loss(*batch)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def float64_gradients(m, w, triples, kind, L, order, act, batch):
    u, q, i, y = (v.cpu().numpy() for v in batch)
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    return qref.model_step(sd, triples, (w.user_count, w.query_count, w.item_count), w.bag_words + 1, w.bag_offsets, kind, L, order, act, u, q, i, y.astype(np.float64))


@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('kind,L,order,d', [('ihgnn', 2, 3, 128), ('hgcn', 2, 1, 64), ('ihgnn', 2, 2, 256), ('ihgnn', 1, 3, 32)])
def test_step_reads_the_tables_in_place_with_the_transform(kind, L, order, d, act):
    """With ``IHG_NODE_TABLES`` on (the first layer and the batch tail read the tables and the transformed query rows in place; the transform's backward runs on the
    complete ``d_query``) and off (X0 assembled): loss and every gradient agree bit for bit - the criterion of ``test_training_step_reads_the_embedding_tables_in_place``
    - and hold the float64 model.  Every parameter, the transform's included, receives a gradient."""
    from ihgnn_amd import ops, profiler
    w, ds = synth_dataset(seed=33, counts=(150, 30, 110, 40, 2500))
    batch = next(iter(ds.sample_batches(60, 1, seed=9)))
    torch.manual_seed(11)
    m = build_model(ds, kind, L, order, d, act)
    results = []
    for tables in (True, False):
        ops.NODE_TABLES = tables
        try:
            profiler.start()
            results.append(step_gradients(m, batch) + (None,))
            profiler.stop()
            results[-1] = results[-1][:2] + (profiler.summary(),)
        finally:
            ops.NODE_TABLES = True
            profiler.stop()
    (l1, g1, s1), (l0, g0, s0) = results
    assert {'bag_mean_fwd', 'query_transform_fwd', 'query_transform_bwd', 'bag_mean_bwd'} <= set(s1) and {'query_transform_fwd', 'query_transform_bwd'} <= set(s0)
    assert torch.equal(l1, l0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    want = float64_gradients(m, w, w.triples, kind, L, order, act, batch)
    assert abs(l1.item() - want['loss']) <= LOSS_RTOL * abs(want['loss'])
    for k in g1:
        print(f'{kind} d {d} {act} {k}: {rel(g1[k], want["grads"][k]):.2e}')
        assert rel(g1[k], want['grads'][k]) <= RTOL, k
    assert float(g1[EMB + 'query_transform.0.weight'].abs().max()) > 0


@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_step_on_a_compact_layout_with_multiplicities(act, monkeypatch):
    """A layout that leaves the isolated nodes out and keeps a repeated (user, query, item) once with its multiplicity (config C5's kind) against the every-node-a-row,
    one-row-per-interaction model on the same weights, and both against float64."""
    from ihgnn_amd import layout as layout_mod, synth
    from ihgnn_amd.Dataset import GraphDataset
    w = synth.draw(300, 40, 200, 50, 4000, seed=21)
    g = np.random.default_rng(4)
    live = [g.choice(n, n // 3, replace=False) for n in (300, 40, 200)]     # two thirds of every type in no hyperedge; half of the triples repeated
    base = np.stack([g.choice(live[k], 3000) for k in range(3)], 1)
    triples = np.concatenate([base, base[:1500]])
    models, batch = {}, None
    for collapsed in (False, True):
        monkeypatch.setattr(layout_mod, 'COMPACT_NODES', '1' if collapsed else '0')
        monkeypatch.setattr(layout_mod, 'EDGE_MULTIPLICITY', '1' if collapsed else '0')
        ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, triples, device=dev())
        lay = ds.hypergraph.layout
        assert bool(getattr(lay, 'compact', False)) == collapsed and (lay.edge_weight is not None) == collapsed
        if batch is None:
            batch = next(iter(ds.sample_batches(80, 1, seed=5)))
        torch.manual_seed(7)
        models[collapsed] = build_model(ds, 'ihgnn', 2, 3, 64, act)
    models[True].load_state_dict(models[False].state_dict())
    l0, g0 = step_gradients(models[False], batch)
    l1, g1 = step_gradients(models[True], batch)
    want = float64_gradients(models[False], w, triples, 'ihgnn', 2, 3, act, batch)
    assert abs(l1.item() - l0.item()) <= 2e-6 * abs(l0.item()) and abs(l1.item() - want['loss']) <= LOSS_RTOL * abs(want['loss'])
    for k in g0:
        print(f'compact {act} {k}: against the plain layout {rel(g1[k], g0[k]):.2e}, float64 {rel(g1[k], want["grads"][k]):.2e}')
        assert rel(g1[k], g0[k]) <= RTOL and rel(g1[k], want['grads'][k]) <= RTOL and rel(g0[k], want['grads'][k]) <= RTOL, k


@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_step_at_a_padded_width(act):
    """d = 96 runs at 128: the transform at 96 on the any-width kernels, its rows padded with exact zeros; every layer output's padding columns are exactly zero and the
    gradients hold the float64 96-wide model."""
    w, ds = synth_dataset(seed=33, counts=(150, 30, 110, 40, 2500))
    batch = next(iter(ds.sample_batches(60, 1, seed=9)))
    torch.manual_seed(3)
    m = build_model(ds, 'ihgnn', 2, 3, 96, act)
    assert m.compute_width == 128
    with torch.no_grad():
        for x in m.propagate_layers():
            assert x.shape[1] == 128 and float(x[:, 96:].abs().max()) == 0.0
        assert m.propagate().shape[1] == 3 * 96
    l, g = step_gradients(m, batch)
    want = float64_gradients(m, w, w.triples, 'ihgnn', 2, 3, act, batch)
    assert abs(l.item() - want['loss']) <= LOSS_RTOL * abs(want['loss'])
    for k in g:
        assert g[k].shape == want['grads'][k].shape and rel(g[k], want['grads'][k]) <= RTOL, k


@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('kind', ['gcn', 'gat', 'phase2'])
def test_other_layer_kinds_with_the_transform(kind, act):
    """GCN and GAT (the pairwise graph) and IHGNN with phase-2 attention over transformed query rows: X0's query rows are the float64 transform's; a step gives every
    parameter a finite gradient; and the transform's own gradients - W_q, b_q, the word table - are the float64 transform's backward of the cotangent that reached
    the query rows of X0 (captured from the step itself).  Repeatable bit for bit."""
    from ihgnn_amd.Helpers.Graph import Pps2DGraph
    from ihgnn_amd.Models import GATLayer, GCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn
    w, ds = synth_dataset(seed=33, counts=(150, 30, 110, 40, 2500))
    if kind != 'phase2':
        ds.graph_type = Pps2DGraph
    torch.manual_seed(2)
    with query_settings(act):
        if kind == 'phase2':
            m = RawGnn(dev(), ds, 32, IHGNNLayer, 2, 3, True, HemPredictionLayer, 0.5).to(dev())
        else:
            m = RawGnn(dev(), ds, 32, GCNLayer if kind == 'gcn' else GATLayer, 2, 1, False, HemPredictionLayer, 0.5).to(dev())
    u, q, i, y = next(iter(ds.sample_batches(60, 1, seed=9)))
    emb, seen = m.embeddings, []
    plain_all_nodes = emb.all_nodes

    def capturing(out=None):
        x = plain_all_nodes(out)
        if x.requires_grad:
            x.retain_grad()
            seen.append(x)
        return x
    emb.all_nodes = capturing
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        del seen[:]
        loss = torch.nn.BCEWithLogitsLoss()(m(u, q, i), y.float())
        loss.backward()
        assert len(seen) == 1 and np.isfinite(loss.item())
        runs.append((loss.item(), {k: p.grad.clone() for k, p in m.named_parameters()}, seen[0].detach().clone(), seen[0].grad.clone()))
    assert runs[0][0] == runs[1][0] and all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
    _, grads, x0, dx0 = runs[0]
    assert all(torch.isfinite(g).all() for g in grads.values()) and set(grads) == {k for k, _ in m.named_parameters()}
    U, Q = ds.user_count, ds.query_count
    sd = {k: qref.t64(v).requires_grad_(True) for k, v in m.state_dict().items() if k.startswith(EMB)}
    _, _, y64 = qref.query_rows(sd[EMB + 'embedding_bag_vocabulary.weight'], w.bag_words + 1, w.bag_offsets, sd[qref.W_KEY], sd[qref.B_KEY], act)
    assert rel(x0[U:U + Q], y64) <= RTOL
    y64.backward(dx0[U:U + Q].cpu().double())
    for k in (qref.W_KEY, qref.B_KEY, EMB + 'embedding_bag_vocabulary.weight'):
        print(f'{kind} {act} {k}: {rel(grads[k], sd[k].grad):.2e}')
        assert rel(grads[k], sd[k].grad) <= RTOL, k


# ---------------------------------------------------------------------------------------------
# evaluation, recorded step, two ranks, kernel trace, driver
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_evaluation_features_and_top_items(act):
    """``save_features_for_test`` (every layer writes its column slice of one matrix - the transform writes the query rows of the first) equals the autograd path's
    features and the float64 model's; ``top_items`` over them equals the ranking of ``score_all_items`` of the float64 features."""
    w, ds = synth_dataset(seed=33, counts=(150, 30, 110, 40, 2500))
    torch.manual_seed(5)
    m = build_model(ds, 'ihgnn', 2, 3, 64, act)
    taped = m.propagate().detach()
    with torch.no_grad():
        m.save_features_for_test()
        feats = m._saved_output_feature
        assert torch.equal(feats, taped)                                 # the column-slice write of propagate() against the autograd path
        sd = {k: qref.t64(v) for k, v in m.state_dict().items()}
        from oracle import ihgnn_ref as ref
        g64 = ref.HyperGraph(w.triples, w.user_count, w.query_count, w.item_count, dtype=torch.float64)
        f64 = torch.cat(qref.model_features(sd, g64, w.bag_words + 1, w.bag_offsets, 'ihgnn', 2, 3, act), 1)
        assert rel(feats, f64) <= RTOL
        users = torch.arange(0, 40, device=dev()); queries = torch.arange(0, 40, device=dev()) % ds.query_count
        items, scores = m.top_items(users, queries, 10)
        lam = m.prediction_layer.lambda_muq
        mixed = lam * f64[queries.cpu() + ds.query_start_index_in_graph] + (1 - lam) * f64[users.cpu()]
        all64 = mixed @ f64[ds.item_start_index_in_graph:].t() + sd['prediction_layer.items_bias']
        top64 = all64.topk(10, dim=1)
        assert rel(scores, top64.values) <= RTOL
        # ranks may swap only between items whose float64 scores are within the bar of each other
        same = items.cpu().long() == top64.indices
        swapped = torch.gather(all64, 1, items.cpu().long())
        assert bool((same | ((swapped - top64.values).abs() <= RTOL * all64.abs().max())).all())
        assert rel(m.score_all_items(users, queries), all64) <= RTOL
        m.clear_saved_feature()


@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_recorded_step_equals_the_eager_step_with_the_transform(act):
    """``CapturedTrainingStep`` over 8 batches is bitwise the eager step (losses, parameters); every parameter, ``query_transform`` included, receives a gradient -
    the recording refuses a model with a parameter that gets none."""
    from ihgnn_amd.captured_step import CapturedTrainingStep
    from ihgnn_amd.optim import Adam
    w, ds = synth_dataset(seed=21)
    batches = list(ds.sample_batches(100, 8, seed=5))

    def run(recorded):
        torch.manual_seed(7)
        m = build_model(ds, 'ihgnn', 2, 3, 64, act)
        opt = Adam(m.parameters(), 1e-3, weight_decay=0)
        step = CapturedTrainingStep(m, opt, batches[0][0].shape[0], warmup_batch=batches[0]) if recorded else None
        losses = []
        for u, q, i, y in batches:
            if step is not None:
                losses.append(step.step(u, q, i, y).item())
            else:
                loss = m.bce_loss(u, q, i, y)
                loss.backward()
                assert all(p.grad is not None for p in m.parameters())
                opt.step(); opt.zero_grad()
                losses.append(loss.item())
        return losses, {k: v.clone() for k, v in m.state_dict().items()}

    l0, p0 = run(False)
    l1, p1 = run(True)
    assert l0 == l1
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    assert not torch.equal(p0[EMB + 'query_transform.0.weight'], build_model(ds, 'ihgnn', 2, 3, 64, act).state_dict()[EMB + 'query_transform.0.weight'])


def test_two_ranks_on_one_gpu_with_the_transform(tmp_path):
    """``python -m ihgnn_amd.Main --query_transform activation`` as two ranks on GPU 0 over gloo: the checkpoints of a ``cotangent`` run and a ``flat`` run agree (as in
    ``test_driver_with_two_ranks_on_one_gpu``), hold the transform's parameters, and ``check_replicas()`` - which the training loop asks after every epoch under the cotangent exchange (all-reduced over the
    ranks; anything but 0 is logged as drift by the chief) - returned 0."""
    import socket
    import subprocess
    import sys
    from ihgnn_amd import synth
    w = synth.draw(60, 20, 80, 25, 501, seed=4, eval_logs=30)
    synth.write_files(w, str(tmp_path / 'Data' / 'Synth' / 'Tiny'))
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    states = {}
    for sync in ('cotangent', 'flat'):
        with socket.socket() as sock:
            sock.bind(('127.0.0.1', 0))
            port = sock.getsockname()[1]
        procs = []
        for rank in range(2):
            env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), IHG_DIST_BACKEND='gloo',
                       HSA_ENABLE_IPC_MODE_LEGACY='0', PYTHONPATH=repo + os.pathsep + os.environ.get('PYTHONPATH', ''))
            procs.append(subprocess.Popen([sys.executable, '-m', 'ihgnn_amd.Main', '--ds', 'Synth/Tiny/', '--gnn', 'IHGNN', '--gnns', '2', '--fo', '3', '--emb', '32', '--ec', '2',
                                           '--est', '2', '--etf', '1', '-c', '--device', '0', '--grad_sync', sync, '--seed', '3', '--query_transform', 'activation',
                                           '--query_activation', 'tanh'], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = [p.communicate(timeout=600)[0] for p in procs]
        assert all(p.returncode == 0 for p in procs), outs[0][-3000:] + outs[1][-3000:]
        assert 'query transform activation (Tanh)' in outs[0]
        assert 'replicas drifted apart' not in outs[0] + outs[1]         # check_replicas() == 0 after both epochs
        result_dir = tmp_path / 'Results' / 'Synth-Tiny-RawGnn-2IHGNNLayer-O3-emb32'
        saved = sorted(n for n in os.listdir(result_dir) if n.startswith('checkpoint_'))
        states[sync] = torch.load(os.path.join(result_dir, saved[-1]), map_location='cpu')['model']
        for n in saved:
            os.remove(os.path.join(result_dir, n))
    assert EMB + 'query_transform.0.weight' in states['flat'] and EMB + 'query_transform.0.bias' in states['flat']
    for name, value in states['cotangent'].items():
        assert torch.isfinite(value).all()
        assert float((value - states['flat'][name]).abs().max()) <= 1e-3, name


def test_step_with_the_transform_launches_only_library_kernels(tmp_path):
    """Training steps (d = 128, 2 layers, order 3; tables read in place; ReLU and Tanh models) under a kernel trace: between two Adam launches every kernel is one
    of the library's, the transform's forward and backward among them."""
    import csv
    import glob
    import shutil
    import subprocess
    import sys
    profiler_exe = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    if not os.path.exists(profiler_exe):
        pytest.skip('rocprofv3 not available')
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'transform_trace.py'
    script.write_text(f'''
import sys
sys.path.insert(0, {repo!r})
import torch
import torch.nn as nn
from ihgnn_amd import ops, synth
from ihgnn_amd.Dataset import GraphDataset
from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
from ihgnn_amd.optim import Adam
dev = torch.device('cuda:0')
w = synth.draw(300, 40, 200, 50, 4000, seed=21, distribution='powerlaw')
ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev)
batches = list(ds.sample_batches(100, 6, seed=5))
for act in (nn.ReLU, nn.Tanh):
    Gs.Query.transform, Gs.Query.transform_activation = Gsv.activation, act
    torch.manual_seed(1)
    m = RawGnn(dev, ds, 128, IHGNNLayer, 2, 3, False, HemPredictionLayer, 0.5).to(dev)
    m.batch_rows_only_last_layer = False                       # (as tools/step_launches.py, whose trace test_training_step_launches_no_framework_kernels reads)
    opt = Adam(m.parameters(), 1e-3, weight_decay=0)
    for u, q, i, y in batches:
        loss = m.bce_loss(u, q, i, y)
        ops.backward(loss)                                       # (the training loop's call: the root gradient is a cached one, not a fill per step)
        opt.step(); opt.zero_grad()
torch.cuda.synchronize()
print('steps done')
''')
    out = str(tmp_path / 'trace')
    r = subprocess.run([profiler_exe, '--kernel-trace', '--output-format', 'csv', '-d', out, '--', sys.executable, str(script)], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0 and 'steps done' in r.stdout, r.stderr[-2000:]
    files = glob.glob(os.path.join(out, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no kernel trace written'
    rows = sorted(csv.DictReader(open(files[0])), key=lambda x: int(x['Start_Timestamp']))
    adam = [k for k, x in enumerate(rows) if 'adam_kernel' in x['Kernel_Name']]
    assert len(adam) >= 12
    for a, b in ((adam[3], adam[4]), (adam[-3], adam[-2])):               # a steady-state step of either model: everything after one Adam launch up to the next
        step = [x['Kernel_Name'] for x in rows[a + 1:b + 1]]
        foreign = [n for n in step if 'at::native' in n or '__amd_rocclr' in n or 'elementwise_kernel' in n]
        assert not foreign, foreign
        short = sorted({n.split('(')[0] for n in step})
        # the transform's launches: forward on the split row GEMM with the activation in its epilogue (d = 128, default arithmetic), backward dm row GEMM + weight gradient
        assert sum('row_gemm_split_kernel<128, false, ' in n and 'false, 0>' not in n for n in step) == 1, short
        assert sum('row_gemm_kernel<128, 0, ' in n and '0, 0>' not in n for n in step) == 1 and sum('dense_weight_grad_act_kernel' in n for n in step) == 1, short


def test_driver_epoch_with_the_transform_writes_a_checkpoint_that_reloads(tmp_path, monkeypatch):
    """Two driver epochs with ``--query_transform activation --query_activation tanh``: finite metrics, a checkpoint with the transform's keys that loads into a fresh
    activation model; the settings are put back afterwards."""
    import random
    from ihgnn_amd import Main as driver, synth
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    w = synth.draw(200, 30, 150, 40, 3000, seed=8, eval_logs=40)
    synth.write_files(w, str(tmp_path / 'Data' / 'Synth' / 'Tiny'))
    monkeypatch.chdir(tmp_path)
    old = (Gs.Query.transform, Gs.Query.transform_activation)
    try:
        random.seed(11); torch.manual_seed(11)
        result = driver.main(['--ds', 'Synth/Tiny/', '--gnns', '2', '--fo', '3', '--emb', '32', '--ec', '2', '--est', '2', '--etf', '1', '-c', '--query_transform', 'activation',
                              '--query_activation', 'tanh'])
        assert Gs.Query.transform == 'activation' and Gs.Query.transform_activation is nn.Tanh
    finally:
        Gs.Query.transform, Gs.Query.transform_activation = old
    _, metrics = list(result.iter_epoch_test())[-1]
    assert np.isfinite([metrics.HitRatio_at10, metrics.NDCG_at10, metrics.MAP_at10]).all()
    result_dir = tmp_path / 'Results' / 'Synth-Tiny-RawGnn-2IHGNNLayer-O3-emb32'
    saved = sorted(n for n in os.listdir(result_dir) if n.startswith('checkpoint_'))
    assert saved
    state = torch.load(os.path.join(result_dir, saved[-1]), map_location='cpu')['model']
    assert tuple(state[EMB + 'query_transform.0.weight'].shape) == (32, 32) and tuple(state[EMB + 'query_transform.0.bias'].shape) == (32,)
    from ihgnn_amd.Dataset import GraphDataset
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev())
    m = build_model(ds, 'ihgnn', 2, 3, 32, 'tanh')
    m.load_state_dict(state)
    with pytest.raises(RuntimeError):
        build_model(ds, 'ihgnn', 2, 3, 32, None).load_state_dict(state)   # (a mean model has no such keys)
