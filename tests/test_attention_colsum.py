"""The finish launches of the two attention backwards (``ihg_gat_finish_bwd``, ``ihg_phase2_finish_bwd``) called directly, against float64 numpy: the
fixed-order column sums of the parameter gradients (``p2_colsum_partials_kernel`` + ``p2_colsum_finish_kernel`` under phase 2; ``gat_param_partials_kernel`` +
``gat_param_finish_kernel`` under GAT, whose move to phase 2's pair these cases are ready for) and the node-row gradient, at
the smallest shapes that reach every path of the column-sum kernels.

Rows n in {1, 511, 512, 513, 1025}: one partial block, the 512-row block boundary from both sides, a third block of one row (phase 2: the hyperedge
count, over 513 node rows).  Widths d in {3, 32, 255, 256}: fewer columns than the narrowest thread row; 32 threads on a row with 8 row slices; 256 threads on a
row with the bias column in the same pass; the bias column alone in a second pass.  Both heads; one case with a row stride above d.

Bars (derived, not tuned).  A sum of n products added in ANY order carries at most n roundings on any term (one from its product, at most n - 1 from the
additions above it), so it is within ``n eps`` (eps = 2^-24, to first order) of the exact sum, relative to the sum of the terms' magnitudes.  The three-term
scalar of phase 2's hyperedge pass adds two roundings, the exact 1/2 of GAT's product head none: ``|got - exact| <= (n + 4) 2^-24 sum_r |term_r|`` covers every
order a kernel could take, the terms being ``|s_r x_rc|``, ``(|s_r0| + |s_r1| + |s_r2|) |x_rc|`` or ``|x y|``.  ``test_bound_holds_for_a_sequential_sum`` shows,
without a GPU, that a plain float32 evaluation passes it at every shape: a failing GPU case is a wrong kernel, not a tight bar.  An entry of ``dh`` is two
products and two additions at the most: ``4 * 2^-24`` of the sum of the magnitudes of its terms."""
import functools

import numpy as np
import pytest

EPS = 2.0 ** -24
N_ROWS = (1, 511, 512, 513, 1025)
DIMS = (3, 32, 255, 256)
HEADS = ('concatenation', 'product')
P2_NODES = 513
CASES = [(n, d, head, 0) for n in N_ROWS for d in DIMS for head in HEADS] + [(513, 32, head, 4) for head in HEADS]


def padded(rng, rows, d, pad):
    """``[rows, d]`` random float32 as a view of a ``[rows, d + pad]`` array (row stride d + pad)."""
    return rng.standard_normal((rows, d + pad)).astype(np.float32)[:, :d]


def column_sum(scalars, x, y=None, factor=1.0):
    """``(exact, sum of the terms' magnitudes)`` per column of ``factor sum_r (sum_t scalars[r, t]) x[r, c]`` - or of ``factor sum_r x y`` - in float64."""
    x = x.astype(np.float64)
    if y is not None:
        terms = factor * x * y.astype(np.float64)
        return terms.sum(0), np.abs(terms).sum(0)
    s = scalars.astype(np.float64)
    return factor * (s.sum(1)[:, None] * x).sum(0), factor * (np.abs(s).sum(1)[:, None] * np.abs(x)).sum(0)


@functools.lru_cache(maxsize=None)
def gat_case(n, d, head, pad):
    """Inputs of ``ihg_gat_finish_bwd`` and, per output, ``(exact, bound)`` in float64."""
    rng = np.random.RandomState(1000 * n + d + (7 if head == 'product' else 0) + pad)
    h, b, dh0 = padded(rng, n, d, pad), padded(rng, n, d, pad), padded(rng, n, d, pad)
    ns = rng.standard_normal((n, 2)).astype(np.float32)
    w = rng.standard_normal(2 * d if head == 'concatenation' else d).astype(np.float32)
    w64, ns64 = w.astype(np.float64), ns.astype(np.float64)
    bias, bias_mag = column_sum(ns[:, 1:], np.ones((n, 1), np.float32))
    if head == 'concatenation':
        src, src_mag = column_sum(ns[:, :1], h)
        dst, dst_mag = column_sum(ns[:, 1:], h)
        dw, dw_mag = np.concatenate([src, dst]), np.concatenate([src_mag, dst_mag])
        terms = [dh0.astype(np.float64), ns64[:, :1] * w64[None, :d], ns64[:, 1:] * w64[None, d:]]
    else:
        dw, dw_mag = column_sum(None, h, b, 0.5)
        terms = [dh0.astype(np.float64), w64[None, :] * b.astype(np.float64)]
    want = {'dweight': (dw, (n + 4) * EPS * dw_mag), 'dbias': (bias, (n + 4) * EPS * bias_mag),
            'dh': (sum(terms), 4 * EPS * sum(np.abs(t) for t in terms))}
    return dict(h=h, b=b, dh0=dh0, node_sums=ns, weight=w), want


@functools.lru_cache(maxsize=None)
def phase2_case(e, d, head, pad):
    """Inputs of ``ihg_phase2_finish_bwd`` (``e`` hyperedge rows, ``P2_NODES`` node rows) and, per output, ``(exact, bound)`` in float64."""
    n = P2_NODES
    rng = np.random.RandomState(1000 * e + d + (7 if head == 'product' else 0) + pad + 500000)
    h, ef, b = padded(rng, n, d, pad), padded(rng, e, d, pad), padded(rng, n, d, pad)
    ns = rng.standard_normal((n, 2)).astype(np.float32)
    ds_edge = rng.standard_normal((e, 3)).astype(np.float32)
    w = rng.standard_normal(2 * d if head == 'concatenation' else d).astype(np.float32)
    w64, ns64 = w.astype(np.float64), ns.astype(np.float64)
    bias, bias_mag = column_sum(ns[:, 1:], np.ones((n, 1), np.float32))
    if head == 'concatenation':
        src, src_mag = column_sum(ds_edge, ef)
        dst, dst_mag = column_sum(ns[:, 1:], h)
        dw, dw_bound = np.concatenate([src, dst]), np.concatenate([(e + 4) * EPS * src_mag, (n + 4) * EPS * dst_mag])
        terms = [ns64[:, 1:] * w64[None, d:]]
    else:
        dw, dw_mag = column_sum(None, h, b)
        dw_bound = (n + 4) * EPS * dw_mag
        terms = [w64[None, :] * b.astype(np.float64)]
    want = {'dweight': (dw, dw_bound), 'dbias': (bias, (n + 4) * EPS * bias_mag), 'dh': (sum(terms), 4 * EPS * sum(np.abs(t) for t in terms))}
    return dict(h=h, ef=ef, b=b, node_sums=ns, ds_edge=ds_edge, weight=w), want


def check(tag, got, want):
    for name, (exact, bound) in want.items():
        err = np.abs(got[name].astype(np.float64).reshape(exact.shape) - exact)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f'{tag} {name}: largest error / bound = {worst:.3f}')
        assert (err <= bound).all(), (tag, name, worst)


def sequential_column_sum(scalars, x, y=None, factor=1.0):
    """The column sums in float32, rows added one after the other."""
    acc = np.zeros(x.shape[1], np.float32)
    if y is None:
        s = scalars[:, 0].copy()
        for t in range(1, scalars.shape[1]):
            s = s + scalars[:, t]
    for r in range(x.shape[0]):
        acc = acc + (x[r] * y[r] if y is not None else s[r] * x[r])
    return acc * np.float32(factor)


@pytest.mark.parametrize('n,d,head,pad', CASES)
def test_bound_holds_for_a_sequential_sum(n, d, head, pad):
    """The bars themselves: float32 numpy, rows in sequence (the longest chain of additions any order has), passes them at every shape of both layers."""
    for layer, (inp, want) in (('gat', gat_case(n, d, head, pad)), ('phase2', phase2_case(n, d, head, pad))):
        ns, w = inp['node_sums'], inp['weight']
        one = np.ones((ns.shape[0], 1), np.float32)
        got = {'dbias': sequential_column_sum(ns[:, 1:], one)}
        if head == 'product':
            got['dweight'] = sequential_column_sum(None, inp['h'], inp['b'], 0.5 if layer == 'gat' else 1.0)
            got['dh'] = w[None, :] * inp['b']
        else:
            src = sequential_column_sum(ns[:, :1], inp['h']) if layer == 'gat' else sequential_column_sum(inp['ds_edge'], inp['ef'])
            got['dweight'] = np.concatenate([src, sequential_column_sum(ns[:, 1:], inp['h'])])
            got['dh'] = ns[:, 1:] * w[None, d:]
            if layer == 'gat':
                got['dh'] = ns[:, :1] * w[None, :d] + got['dh']
        if layer == 'gat':
            got['dh'] = inp['dh0'] + got['dh']
        check(f'{layer} sequential n={n} d={d} {head}', got, want)


def on_device(a):
    """The array on the GPU with its row stride kept (a column view of the padded allocation)."""
    import torch
    base = a.base if a.base is not None and a.ndim == 2 and a.base.shape[1] > a.shape[1] else a
    return torch.from_numpy(np.ascontiguousarray(base)).cuda()[:, :a.shape[1]] if a.ndim == 2 else torch.from_numpy(a).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize('n,d,head,pad', CASES)
def test_gat_finish_bwd_matches_float64(n, d, head, pad):
    import torch
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    inp, want = gat_case(n, d, head, pad)
    t = {k: on_device(v) for k, v in inp.items()}
    code = ops.GAT_HEADS[head]
    product = head == 'product'
    wsb = int(lib.ihg_gat_workspace_bytes(n, 0, d, code))
    ws = torch.empty(wsb // 4 + 4, device='cuda')
    runs = []
    for _ in range(2):
        dh = torch.empty(n, d + pad, device='cuda')[:, :d]
        dh.copy_(t['dh0'])
        dweight, dbias = torch.full_like(t['weight'], float('nan')), torch.full((1,), float('nan'), device='cuda')
        _lib.check(lib.ihg_gat_finish_bwd(ops._ptr(t['h']), d + pad, ops._ptr(t['b']) if product else None, d + pad if product else 0, ops._ptr(t['node_sums']),
                                          ops._ptr(t['weight']), code, n, d, ops._ptr(dh), d + pad, ops._ptr(dweight), ops._ptr(dbias), ops._ptr(ws), wsb,
                                          ops._stream()), 'ihg_gat_finish_bwd')
        runs.append({'dweight': dweight.cpu().numpy(), 'dbias': dbias.cpu().numpy(), 'dh': dh.cpu().numpy()})
    for name in runs[0]:
        assert runs[0][name].tobytes() == runs[1][name].tobytes(), name
    check(f'gat n={n} d={d} {head} pad={pad}', runs[0], want)


@pytest.mark.gpu
@pytest.mark.parametrize('e,d,head,pad', CASES)
def test_phase2_finish_bwd_matches_float64(e, d, head, pad):
    import torch
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    n = P2_NODES
    inp, want = phase2_case(e, d, head, pad)
    t = {k: on_device(v) for k, v in inp.items()}
    code = ops.GAT_HEADS[head]
    product = head == 'product'
    wsb = int(lib.ihg_phase2_workspace_bytes(n, e, 0, d, code))
    ws = torch.empty(wsb // 4 + 4, device='cuda')
    runs = []
    for _ in range(2):
        dh = torch.full((n, d + pad), float('nan'), device='cuda')[:, :d]
        dweight, dbias = torch.full_like(t['weight'], float('nan')), torch.full((1,), float('nan'), device='cuda')
        _lib.check(lib.ihg_phase2_finish_bwd(ops._ptr(t['h']), d + pad, ops._ptr(t['ef']), d + pad, ops._ptr(t['b']) if product else None, d + pad if product else 0,
                                             ops._ptr(t['node_sums']), ops._ptr(t['ds_edge']), ops._ptr(t['weight']), code, n, e, d, ops._ptr(dh), d + pad,
                                             ops._ptr(dweight), ops._ptr(dbias), ops._ptr(ws), wsb, ops._stream()), 'ihg_phase2_finish_bwd')
        runs.append({'dweight': dweight.cpu().numpy(), 'dbias': dbias.cpu().numpy(), 'dh': dh.cpu().numpy()})
    for name in runs[0]:
        assert runs[0][name].tobytes() == runs[1][name].tobytes(), name
    check(f'phase2 e={e} d={d} {head} pad={pad}', runs[0], want)
