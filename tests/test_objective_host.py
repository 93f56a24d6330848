"""The training objective's one description (``ops.Objective``) without a GPU: what ``ops.training_objective`` makes of every setting (``--loss``, ``--hard_negatives``),
its ``key()`` - what a recorded step compares per replay -, the refusal of a pool the batch does not carry, and the one launch each objective makes (a recorder in the
library's place: the entry point and its arguments)."""
import itertools

import pytest
import torch

KINDS = {'bce': 0, 'bpr': 1, 'softmax': 2}
P, K, POOL, KEEP = 100, 10, 20, 10


class settings:
    """``Gs.Training.loss`` / ``Gs.Training.negative_pool`` / ``Gs.random_negative_sample_size`` for the block, put back after it."""

    def __init__(self, loss='bce', pool=0, keep=KEEP):
        self.new = (loss, pool, keep)

    def __enter__(self):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        self.old = (Gs.Training.loss, Gs.Training.negative_pool, Gs.random_negative_sample_size)
        Gs.Training.loss, Gs.Training.negative_pool, Gs.random_negative_sample_size = self.new

    def __exit__(self, *exc):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        Gs.Training.loss, Gs.Training.negative_pool, Gs.random_negative_sample_size = self.old


@pytest.mark.parametrize('loss,pool', list(itertools.product(sorted(KINDS), (0, POOL))))
def test_training_objective_under_each_setting(loss, pool):
    from ihgnn_amd import ops
    per_positive = pool or K
    with settings(loss, pool):
        o = ops.training_objective(P * (1 + per_positive), P)
    if loss == 'bce' and not pool:
        assert (o.kind, o.positives, o.pool, o.keep, o.selected) == (0, None, None, None, None)
        assert not o.grouped and not o.hard and o.label == 'bce_with_logits'
    else:
        assert (o.kind, o.positives, o.pool, o.keep, o.selected) == (KINDS[loss], P, per_positive, KEEP if pool else None, None)
        assert o.grouped and o.hard == bool(pool) and o.label == ('hard_negative_loss' if pool else 'ranking_loss')
    assert o.key() == (o.kind, o.positives, o.pool, o.keep) and hash(o.key()) is not None


def test_key_tells_the_objectives_apart():
    """``key()`` differs whenever the kind, (over groups) the positives, the pool or the kept count differs - and not with the positives under the plain BCE, which does
    not look at them (a recorded BCE step is not stale for them)."""
    from ihgnn_amd import ops
    keys = {}
    for loss, pool, keep, positives in itertools.product(sorted(KINDS), (0, POOL, 2 * POOL), (KEEP, KEEP - 1), (P, P // 2)):
        with settings(loss, pool, keep):
            rows = P * (1 + K) * (1 + POOL) * (1 + 2 * POOL) if not pool else positives * (1 + pool)      # (without a pool: rows that split into either number of groups)
            key = ops.training_objective(rows, positives).key()
        grouped = loss != 'bce' or pool
        what = (loss, positives if grouped else None, pool if pool else (rows // positives - 1 if grouped else None), keep if pool else None)
        assert keys.setdefault(key, what) == what, (key, what, keys[key])          # equal keys: equal in everything a recording holds
    assert len(keys) == len(set(keys.values())) == 1 + 2 * 2 + 3 * 2 * 2 * 2    # plain BCE; bpr / softmax x positives; three kinds x two pools x kept counts x positives
    with settings('bce'):
        assert ops.training_objective(1100, None).key() == ops.training_objective(1100, 100).key() == ops.training_objective(1100, 7).key() == ops.bce_objective().key()


def test_training_objective_refuses_what_the_batch_does_not_carry():
    from ihgnn_amd import ops
    with settings('bce', POOL):
        with pytest.raises(ValueError, match='negative_pool = 20, but the loader drew 1000 negatives for 100 positives'):
            ops.training_objective(P * (1 + K), P)
        with pytest.raises(ValueError, match='carry a pool of 10'):
            ops.training_objective(P * (1 + K), P)
        with pytest.raises(ValueError, match='needs positives='):
            ops.training_objective(P * (1 + POOL), None)
    with settings('bpr'):
        with pytest.raises(ValueError, match='needs positives='):
            ops.training_objective(P * (1 + K), None)
        with pytest.raises(ValueError, match='rows'):
            ops.training_objective(P * (1 + K) + 1, P)
    with settings('softmax', POOL, POOL + 1):
        with pytest.raises(ValueError, match='keep'):
            ops.training_objective(P * (1 + POOL), P)
    with pytest.raises(ValueError, match='positives'):
        ops.Objective('bpr')                                                     # a loss over groups without its groups


class Recorder:
    """In the library's place: every entry point returns ``OK`` and leaves its name and arguments (pointers as integers)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name,) + tuple(getattr(a, 'value', a) for a in args)) or 0


@pytest.mark.parametrize('case', ['bce', 'ranking', 'hard'])
def test_launch_calls_one_entry_point_with_its_arguments(case, monkeypatch):
    """The smallest shapes that tell the arguments apart: the BCE over n = 3 scores; a ranking loss over P = 2, k = 1; hard negatives over P = 2, pool = 2, keep = 1."""
    from ihgnn_amd import _lib, ops
    lib = Recorder()
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    monkeypatch.setattr(ops, '_stream', lambda: None)
    objective, n = {'bce': (ops.bce_objective(), 3), 'ranking': (ops.ranking_objective(4, 2, 'softmax'), 4), 'hard': (ops.hard_negative_objective(6, 2, 1, 'bpr'), 6)}[case]
    scores, labels, loss, dscores = torch.zeros(n), torch.zeros(n), torch.zeros(()), torch.zeros(n)
    objective.launch(scores, labels if case == 'bce' else None, loss, dscores)
    s, y, l, d = (t.data_ptr() for t in (scores, labels, loss, dscores))
    assert len({s, y, l, d}) == 4
    if case == 'bce':
        assert lib.calls == [('ihg_bce_with_logits', s, y, 3, l, d, None)] and objective.selected is None
    elif case == 'ranking':
        assert lib.calls == [('ihg_ranking_loss', s, 2, 1, 2, l, d, None)] and objective.selected is None
    else:
        picked = objective.selected
        assert picked.dtype == torch.int32 and tuple(picked.shape) == (2, 1)
        assert lib.calls == [('ihg_hard_negative_loss', s, 2, 2, 1, 1, l, d, picked.data_ptr(), None)]
