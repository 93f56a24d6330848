"""``ihg_ranking_loss`` (``csrc/tail.hip``) through the C ABI, into guarded, NaN-prefilled buffers, for both kinds: per entry against float64 within the bounds that
``tests/loss_reference.py`` derives (the verdicts ``tests/test_loss_host.py`` holds the float32 emulation to, on the same cases), bitwise repeatable, guards intact,
bad arguments refused with nothing written."""
import ctypes

import numpy as np
import pytest
import torch

import loss_reference as R

pytestmark = pytest.mark.gpu

GUARD = 8                                                   # floats either side of dscores and of the loss


def dev():
    return torch.device('cuda:0')


def launch(kind, scores, positives, k):
    """-> ``(status, loss float32, dscores float32 numpy, guards intact)``; ``scores``: numpy float32 or None (a null pointer)."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    n = max(int(positives) * (1 + int(k)), 1) if scores is None else scores.shape[0]
    s = None if scores is None else torch.from_numpy(scores).to(dev())
    out = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=dev())
    loss = torch.full((1 + 2 * GUARD,), float('nan'), dtype=torch.float32, device=dev())
    out[:GUARD], out[-GUARD:], loss[:GUARD], loss[-GUARD:] = -7.0, -7.0, -7.0, -7.0
    status = lib.ihg_ranking_loss(ops._ptr(s), positives, k, kind, ops._ptr(loss[GUARD:]), ops._ptr(out[GUARD:]), ops._stream())
    torch.cuda.synchronize()
    out, loss = out.cpu().numpy(), loss.cpu().numpy()
    intact = bool((out[:GUARD] == -7).all() and (out[-GUARD:] == -7).all() and (loss[:GUARD] == -7).all() and (loss[-GUARD:] == -7).all())
    return status, loss[GUARD], out[GUARD:-GUARD], intact


@pytest.fixture(scope='module')
def worst():
    """The worst ``error / bound`` per kind and output over the module's cases, printed once at the end (DESIGN §8 quotes one run's figures)."""
    table = {}
    yield table
    for key in sorted(table):
        print(f'ihg_ranking_loss {key[0]} {key[1]}: worst error / bound {table[key]:.3f}')


@pytest.mark.parametrize('kind', sorted(R.KINDS))
@pytest.mark.parametrize('design', R.DESIGNS)
def test_matches_float64_within_the_derived_bounds(kind, design, worst):
    for d, P, k in R.CASES:
        if d != design:
            continue
        s = R.scores_of(d, P, k)
        status, loss, ds, intact = launch(R.KINDS[kind], s, P, k)
        assert status == 0 and intact, (kind, d, P, k)
        ratios = R.verdicts(kind, d, s, P, k, loss, ds)
        print(f'{kind} {d} P={P} k={k}: error / bound {ratios}')
        for name, ratio in ratios.items():
            worst[(kind, name)] = max(worst.get((kind, name), 0.0), ratio)
        status2, loss2, ds2, intact2 = launch(R.KINDS[kind], s, P, k)
        assert status2 == 0 and intact2
        assert loss.tobytes() == loss2.tobytes() and ds.tobytes() == ds2.tobytes(), f'{kind} {d} P={P} k={k}: two launches differ'


@pytest.mark.parametrize('kind', sorted(R.KINDS))
def test_huge_scores_stay_finite_and_balanced(kind):
    for P, k in R.HUGE_SHAPES:
        s = R.scores_of('huge', P, k)
        status, loss, ds, intact = launch(R.KINDS[kind], s, P, k)
        assert status == 0 and intact
        R.verdicts(kind, 'huge', s, P, k, loss, ds)


def test_bad_arguments_leave_the_buffers_alone():
    from ihgnn_amd import _lib
    s = R.scores_of('randn1', 4, 3)
    table = [(1, s, 0, 3), (1, s, -1, 3), (1, s, 4, 0), (1, s, 4, -2), (0, s, 4, 3), (3, s, 4, 3), (-1, s, 4, 3), (2, None, 4, 3),
             (2, s, (1 << 31) // 4, 3), (1, s, 1 << 40, 1)]
    for kind, scores, positives, k in table:
        status, loss, ds, intact = launch(kind, scores, positives, k)
        assert status == _lib.ERR_INVALID and 'ihg_ranking_loss' in _lib.last_error(), (kind, positives, k)
        assert intact and np.isnan(loss) and np.isnan(ds).all(), (kind, positives, k)
    lib = _lib.load()
    ok = torch.zeros(16, device=dev())
    from ihgnn_amd import ops
    assert lib.ihg_ranking_loss(ops._ptr(ok), 4, 3, 1, None, ops._ptr(ok), ops._stream()) == _lib.ERR_INVALID
    assert lib.ihg_ranking_loss(ops._ptr(ok), 4, 3, 1, ops._ptr(ok), None, ops._stream()) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert float(ok.abs().sum()) == 0.0


@pytest.mark.parametrize('kind', sorted(R.KINDS))
def test_op_is_the_launch_and_differentiates(kind):
    """``ops.ranking_loss``: the launch's loss, and a backward that is ``dscores`` times the upstream gradient; a non-contiguous view is read as its values."""
    from ihgnn_amd import ops
    P, k = 65, 10
    s = R.scores_of('randn8', P, k)
    _, loss, ds, _ = launch(R.KINDS[kind], s, P, k)
    t = torch.from_numpy(s).to(dev()).requires_grad_()
    got = ops.ranking_loss(t, P, kind)
    (got * 3.0).backward()
    assert got.detach().cpu().numpy().tobytes() == loss.tobytes()
    assert torch.equal(t.grad.cpu(), torch.from_numpy(ds) * 3.0)
    wide = torch.from_numpy(np.stack([s, s + 1], 1)).to(dev())
    assert ops.ranking_loss(wide[:, 0], P, kind).cpu().numpy().tobytes() == loss.tobytes()
    with pytest.raises(ValueError, match='rows'):
        ops.ranking_loss(t, P + 1, kind)
