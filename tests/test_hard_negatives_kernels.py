"""``ihg_sample_pool`` and ``ihg_hard_negative_loss`` (``csrc/tail.hip``) through the C ABI, into guarded, NaN-prefilled buffers: the pool bit for bit against the sequential
definition, the loss launch against the verdicts ``tests/hard_negatives_reference.py`` states (the ones ``tests/test_hard_negatives_host.py`` holds the float32 emulation
to, on the same cases) - the selection exactly, ``dscores`` fully written and +0.0 off the selection, loss and ``dscores`` within the float64 bounds on the compacted
scores - bitwise repeatable, guards intact, k = M against ``ihg_ranking_loss``, bad arguments refused with nothing written."""
import numpy as np
import pytest
import torch

import hard_negatives_reference as H
import loss_reference as R

pytestmark = pytest.mark.gpu

GUARD = 8                                                   # words either side of every output


def dev():
    return torch.device('cuda:0')


def guarded(n, dtype, fill):
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev())
    t[:GUARD], t[-GUARD:] = -7, -7
    return t


def intact(*buffers):
    return all(bool((b[:GUARD] == -7).all() and (b[-GUARD:] == -7).all()) for b in buffers)


# ---------------------------------------------------------------------------------------------
# the pool
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', H.POOL_ROWS)
def test_sample_pool_equals_the_sequential_definition(rows):
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    seed, counter = 7919 * 5 + 2, (3 << 32) + 41
    for r, m, n_items in H.POOL_CASES:
        if r != rows:
            continue
        out = guarded(rows * m, torch.int64, -1)
        status = lib.ihg_sample_pool(seed, counter, rows, n_items, m, ops._ptr(out[GUARD:]), ops._stream())
        torch.cuda.synchronize()
        assert status == 0 and intact(out), (rows, m, n_items)
        want = torch.from_numpy(H.pool_draw(seed, counter, rows, n_items, m).copy())
        assert torch.equal(out[GUARD:-GUARD].view(rows, m).cpu(), want), (rows, m, n_items)


def test_sample_pool_op_prefix_and_refusals():
    """``ops.sample_pool``: the launch; its first 16 columns are ``ihg_sample_negatives``' bits; a refusal writes nothing."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    got = ops.sample_pool(99, 7, 65, 1000, 40, device=dev())
    assert got.shape == (65, 40) and got.dtype == torch.int64
    assert torch.equal(got.cpu(), torch.from_numpy(H.pool_draw(99, 7, 65, 1000, 40).copy()))
    few = torch.empty(65, 16, dtype=torch.int64, device=dev())
    assert lib.ihg_sample_negatives(99, 7, 65, 1000, 16, ops._ptr(few), ops._stream()) == 0
    assert torch.equal(few, got[:, :16])
    assert ops.sample_pool(99, 7, 0, 1000, 40, device=dev()).shape == (0, 40)
    out = guarded(65 * 40, torch.int64, -1)
    for m, n_items in ((0, 1000), (257, 1000), (40, 39)):
        assert lib.ihg_sample_pool(99, 7, 65, n_items, m, ops._ptr(out[GUARD:]), ops._stream()) == _lib.ERR_INVALID
        with pytest.raises(_lib.IhgnnHipError, match='ihg_sample_pool'):
            ops.sample_pool(99, 7, 65, n_items, m, device=dev())
    torch.cuda.synchronize()
    assert intact(out) and bool((out[GUARD:-GUARD] == -1).all())


# ---------------------------------------------------------------------------------------------
# the loss launch
# ---------------------------------------------------------------------------------------------
def launch(kind, scores, positives, pool, keep):
    """-> ``(status, loss float32, dscores float32 numpy, selected int32 numpy [P, keep], guards intact)``; ``scores``: numpy float32 or None (a null pointer)."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    n = max(int(positives) * (1 + int(pool)), 1) if scores is None else scores.shape[0]
    rows = min(max(int(positives), 1), 4096) * min(max(int(keep), 1), 256)
    s = None if scores is None else torch.from_numpy(scores.copy()).to(dev())
    out = guarded(n, torch.float32, float('nan'))
    loss = guarded(1, torch.float32, float('nan'))
    selected = guarded(rows, torch.int32, -1)
    status = lib.ihg_hard_negative_loss(ops._ptr(s), positives, pool, keep, kind, ops._ptr(loss[GUARD:]), ops._ptr(out[GUARD:]), ops._ptr(selected[GUARD:]), ops._stream())
    torch.cuda.synchronize()
    ok = intact(out, loss, selected)
    return status, loss.cpu().numpy()[GUARD], out.cpu().numpy()[GUARD:-GUARD], selected.cpu().numpy()[GUARD:-GUARD], ok


@pytest.fixture(scope='module')
def worst():
    """The worst ``error / bound`` per kind and output over the module's cases, printed once at the end (DESIGN §8 quotes one run's figures)."""
    table = {}
    yield table
    for key in sorted(table):
        print(f'ihg_hard_negative_loss {key[0]} {key[1]}: worst error / bound {table[key]:.3f}')


@pytest.mark.parametrize('kind', sorted(H.KINDS))
@pytest.mark.parametrize('design', H.DESIGNS)
def test_selection_loss_and_gradient_meet_every_verdict(kind, design, worst):
    for d, P, M, k in H.CASES:
        if d != design:
            continue
        s = H.scores_of(d, P, M, k)
        status, loss, ds, selected, ok = launch(H.KINDS[kind], s, P, M, k)
        assert status == 0 and ok, (kind, d, P, M, k)
        ratios = H.verdicts(kind, d, s, P, M, k, loss, ds, selected.reshape(P, k))
        print(f'{kind} {d} P={P} M={M} k={k}: error / bound {ratios}')
        for name, ratio in ratios.items():
            worst[(kind, name)] = max(worst.get((kind, name), 0.0), ratio)
        status2, loss2, ds2, selected2, ok2 = launch(H.KINDS[kind], s, P, M, k)
        assert status2 == 0 and ok2
        assert loss.tobytes() == loss2.tobytes() and ds.tobytes() == ds2.tobytes() and selected.tobytes() == selected2.tobytes(), f'{kind} {d} P={P} M={M} k={k}: two launches differ'


@pytest.mark.parametrize('kind', sorted(R.KINDS))
def test_the_whole_pool_kept_agrees_with_the_ranking_loss(kind):
    """k = M: every candidate is a negative, so ``ihg_ranking_loss`` on the same scores is the same objective in another order of summation - both within the float64
    bounds of the same reference, and ``selected`` a permutation of the pool in score order."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    for P, M in ((17, 11), (16, 256), (33, 64)):
        s = H.scores_of('randn8', P, M, M)
        status, loss, ds, selected, ok = launch(R.KINDS[kind], s, P, M, M)
        assert status == 0 and ok
        selected = selected.reshape(P, M)
        assert (np.sort(selected, 1) == np.arange(M)).all()
        t = torch.from_numpy(s.copy()).to(dev())
        plain_loss, plain_ds = torch.empty((), device=dev()), torch.empty_like(t)
        assert lib.ihg_ranking_loss(ops._ptr(t), P, M, R.KINDS[kind], ops._ptr(plain_loss), ops._ptr(plain_ds), ops._stream()) == 0
        ref = R.reference(kind, s, P, M)                                       # (in pool order: the objective does not depend on the order of a group's negatives)
        for got_loss, got_ds in ((float(loss), ds), (float(plain_loss.cpu()), plain_ds.cpu().numpy())):
            assert abs(got_loss - ref['loss']) <= ref['bound_loss'], (kind, P, M)
            assert (np.abs(got_ds.astype(np.float64) - ref['ds']) <= ref['bound_ds']).all(), (kind, P, M)


def test_bad_arguments_leave_the_buffers_alone():
    from ihgnn_amd import _lib
    s = H.scores_of('randn1', 2, 11, 10)
    table = [(1, s, 2, 11, 0), (1, s, 2, 11, 12), (1, s, 2, 257, 10), (1, s, 0, 11, 10), (3, s, 2, 11, 10), (-1, s, 2, 11, 10), (2, None, 2, 11, 10),
             (0, s, (1 << 31) // 12 + 1, 11, 10)]
    for kind, scores, positives, pool, keep in table:
        status, loss, ds, selected, ok = launch(kind, scores, positives, pool, keep)
        assert status == _lib.ERR_INVALID and 'ihg_hard_negative_loss' in _lib.last_error(), (kind, positives, pool, keep)
        assert ok and np.isnan(loss) and np.isnan(ds).all() and (selected == -1).all(), (kind, positives, pool, keep)


@pytest.mark.parametrize('kind', sorted(H.KINDS))
def test_op_is_the_launch_and_differentiates(kind):
    """``ops.hard_negative_loss``: the launch's loss and selection, and a backward that is ``dscores`` times the upstream gradient; a non-contiguous view is read as its
    values."""
    from ihgnn_amd import ops
    P, M, k = 17, 65, 10
    s = H.scores_of('randn8', P, M, k)
    _, loss, ds, selected, _ = launch(H.KINDS[kind], s, P, M, k)
    t = torch.from_numpy(s.copy()).to(dev()).requires_grad_()
    got, picked = ops.hard_negative_loss(t, P, k, kind, return_selected=True)
    (got * 3.0).backward()
    assert got.detach().cpu().numpy().tobytes() == loss.tobytes()
    assert picked.dtype == torch.int64 and not picked.requires_grad and (picked.cpu().numpy() == selected.reshape(P, k)).all()
    assert torch.equal(t.grad.cpu(), torch.from_numpy(ds) * 3.0)
    wide = torch.from_numpy(np.stack([s, s + 1], 1)).to(dev())
    assert ops.hard_negative_loss(wide[:, 0], P, k, kind).cpu().numpy().tobytes() == loss.tobytes()
    with pytest.raises(ValueError, match='rows'):
        ops.hard_negative_loss(t, P + 1, k, kind)
