"""The cosine head of the batch tail (``hem_cosine_fwd_kernel`` / ``hem_cosine_bwd_kernel``, ``csrc/tail.hip``) through ``ihg_hem_cosine_fwd`` / ``ihg_hem_cosine_bwd``
on their own, in the three call forms of ``test_update_tail.py::test_hem_score_kernels_match_float64``: every layer in one numbering (host ``grad_scale``); the layers
above layer 0 in a numbering of their own with -1 for users, queries, items and both user and query of a row (``grad_scale`` x a device scalar); the same with layer 0
read from three typed tables.  Every score, every entry of the guarded ``stats`` buffer (the three sums; the fourth float 0) and every entry of the row gradients -
width L d + 4, the bias column checked, the columns behind it and the guard rows still sentinel - is held to the float64 reference within the bound counted beside it
(``tests/update_tail_reference.py``); ``tests/test_cosine_tail_host.py`` holds a float32 evaluation in the kernels' order to the same bounds.  The first batch rows
are the edges: a zero item row and a zero mixed row (gradient terms exactly 0, everything finite), a norm below 1e-8 (the clamped value divides), an item whose
layer-0 row is its only nonzero one, user and query both isolated above layer 0.  Every source is compared with its copy after the launches."""
import ctypes

import numpy as np
import pytest
import torch

import update_tail_reference as R
from test_attention_kernels import Guarded
from test_cosine_tail_host import BATCHES, DIMS, FORMS, LAMBDAS, LAYERS, reference_of, scales_of
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

SENTINEL = 12345.678
GUARD_ROWS = 2
WORST = {}                               # entry point -> worst error / bound (recorded in DESIGN.md section 5)


@pytest.fixture(scope='module', autouse=True)
def _report_worst_ratios():
    yield
    for name in sorted(WORST):
        print(f'worst error / bound: {name}: {WORST[name]:.3f}')


def _run(n_layers, dim, batch, form, lam, seed):
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    n_u, n_q, n_i, n_up = R.COSINE_TAIL_NODES
    what = f'L = {n_layers}, d = {dim}, B = {batch}, {form}, lam = {lam}'
    case = R.cosine_tail_case(n_layers, dim, batch, form, seed)
    want, ds = reference_of(case, form, lam)
    width = n_layers * dim
    cols = n_layers * (dim + 1) + 3                                         # every layer's buffer has this many columns: one row stride for the call
    layer0, above = case['layers'][0], case['layers'][1:]
    buffers = []
    if form == 'typed':
        tables = []
        for lo, hi, pad in ((0, n_u, 1), (n_u, n_u + n_q, 0), (n_u + n_q, n_u + n_q + n_i, 1)):      # rows 1.. of a user and an item table, the query rows
            t = torch.full((pad + hi - lo, dim + 2), SENTINEL, dtype=torch.float32, device=dev())
            t[pad:, :dim] = torch.from_numpy(layer0[lo:hi])
            tables.append((t, pad))
        buffers += [t for t, _ in tables]
        layer0_rows = (ctypes.c_void_p * 3)(*[t[pad:].data_ptr() for t, pad in tables])
        typed0 = (layer0_rows, dim + 2, (ctypes.c_int64 * 4)(0, n_u, n_u + n_q, n_u + n_q + n_i))
        first = tables[1][0].data_ptr()                                     # (slot 0 of the layer list is replaced by the typed rows)
    else:
        buf0 = torch.full((layer0.shape[0], cols), SENTINEL, dtype=torch.float32, device=dev())
        buf0[:, 1:1 + dim] = torch.from_numpy(layer0)
        buffers.append(buf0)
        typed0 = (None, 0, None)
        first = buf0[:, 1:].data_ptr()
    buf_up = torch.full((above[0].shape[0] if above else 1, cols), SENTINEL, dtype=torch.float32, device=dev())
    ups = []
    for l, x in enumerate(above, start=1):
        v = buf_up[:, 1 + l * (dim + 1): 1 + l * (dim + 1) + dim]
        v.copy_(torch.from_numpy(x))
        ups.append(v.data_ptr())
    buffers.append(buf_up)
    ptrs = (ctypes.c_void_p * n_layers)(first, *ups)
    to = lambda x: None if x is None else torch.from_numpy(x).to(dev())
    rows, rows_upper, items, bias, dscores = (to(case[k]) for k in ('rows', 'rows_upper', 'items', 'bias', 'dscores'))
    scale, device_scale = scales_of(form)
    device_scalar = None if device_scale is None else torch.tensor(device_scale, dtype=torch.float32, device=dev())
    sources = buffers + [t for t in (rows, rows_upper, items, bias, dscores, device_scalar) if t is not None]
    copies = [t.clone() for t in sources]

    scores, stats = Guarded(batch), Guarded(4 * batch)
    assert stats.view.data_ptr() % 16 == 0
    rc = lib.ihg_hem_cosine_fwd(ptrs, n_layers, cols, dim, *typed0, ops._ptr(rows), ops._ptr(rows_upper), ops._ptr(items), ops._ptr(bias), lam, ops._ptr(scores.view),
                                ops._ptr(stats.view), batch, ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.OK, f'{what}: ihg_hem_cosine_fwd returned {rc}: {_lib.last_error()}'
    scores.assert_guards(what)
    stats.assert_guards(what)
    stats_before = stats.buf.clone()
    rowgrad = torch.full((GUARD_ROWS + 3 * batch + GUARD_ROWS, width + 4), SENTINEL, dtype=torch.float32, device=dev())
    payload = rowgrad[GUARD_ROWS:GUARD_ROWS + 3 * batch]
    rc = lib.ihg_hem_cosine_bwd(ptrs, n_layers, cols, dim, *typed0, ops._ptr(rows), ops._ptr(rows_upper), ops._ptr(dscores), ops._ptr(stats.view), ops._ptr(device_scalar),
                                scale, lam, ops._ptr(payload), width + 4, batch, ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.OK, f'{what}: ihg_hem_cosine_bwd returned {rc}: {_lib.last_error()}'
    assert torch.equal(stats.buf.view(torch.int32), stats_before.view(torch.int32)), f'{what}: the backward wrote into stats'
    for t, c in zip(sources, copies):
        assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t, c.view(torch.int32) if c.dtype == torch.float32 else c), f'{what}: a source was written'
    assert bool((rowgrad[:GUARD_ROWS] == SENTINEL).all()) and bool((rowgrad[GUARD_ROWS + 3 * batch:] == SENTINEL).all()), f'{what}: rows around rowgrad were written'
    assert bool((payload[:, width + 1:] == SENTINEL).all()), f'{what}: columns behind the bias column were written'
    st = stats.view.view(batch, 4).cpu().numpy()
    assert (st[:, 3] == 0).all(), f'{what}: the fourth float of a stats row is not 0'
    got = payload[:, :width + 1].cpu().numpy().reshape(3, batch, width + 1)
    worst = R.assert_cosine_tail_within_bounds(scores.view.cpu().numpy(), st, got, want, ds, what)
    for name, w in zip(('ihg_hem_cosine_fwd scores', 'ihg_hem_cosine_fwd stats', 'ihg_hem_cosine_bwd row gradients'), worst):
        WORST[name] = max(WORST.get(name, 0.0), w)


@pytest.mark.parametrize('dim', DIMS)
@pytest.mark.parametrize('n_layers', LAYERS)
def test_hem_cosine_kernels_match_float64_per_entry(n_layers, dim):
    """1, 2, 5 and 8 layers x widths 1 ... 256 (one lane, a partial pass over the lanes, one pass, a second partial one, four) x batches of 1, 63, 65 rows x the three
    call forms, lam = 0, 0.3, 1 in rotation so that every pair occurs over the cases."""
    i = DIMS.index(dim)
    for j, batch in enumerate(BATCHES):
        for k, form in enumerate(FORMS):
            _run(n_layers, dim, batch, form, LAMBDAS[(i + j + k) % 3], i + k)


def test_a_batch_of_one_row_meets_every_edge():
    """One row, L = 5, d = 33, each edge in turn (the seed names it) in the two forms that have isolated nodes."""
    for seed in range(len(R.COSINE_TAIL_EDGES)):
        for form in ('upper', 'typed'):
            _run(5, 33, 1, form, 0.3, seed)
