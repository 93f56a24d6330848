"""The ranking losses (``--loss bpr | softmax``) without a GPU: the float32 emulation of ``ihg_ranking_loss`` is held to the verdicts the GPU file holds the kernel to, on
the same cases (``tests/loss_reference.py``), each mutation of it misses a named case, and the host side - the flag, the setting, the Srrl refusal, the host check of
the batch's grouping, the entry's argument checks (which come before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import loss_reference as R
from conftest import REPO


@pytest.mark.parametrize('kind', sorted(R.KINDS))
def test_emulation_meets_every_verdict(kind):
    worst = {}
    for design, P, k in R.CASES:
        s = R.scores_of(design, P, k)
        for name, ratio in R.verdicts(kind, design, s, P, k, *R.emulate(kind, s, P, k)).items():
            worst[name] = max(worst.get(name, 0.0), ratio)
    for P, k in R.HUGE_SHAPES:
        s = R.scores_of('huge', P, k)
        R.verdicts(kind, 'huge', s, P, k, *R.emulate(kind, s, P, k))
    print(f'{kind}: worst error / bound of the emulation {worst}')
    assert all(0 < ratio <= 1 for ratio in worst.values())


def test_cases_cover_the_ladder():
    shapes = {(p, k) for _, p, k in R.CASES}
    assert {(p, 10) for p in (1, 2, 63, 64, 65, 1023, 1024, 1025)} <= shapes
    assert {(p, k) for p in (1, 65) for k in (1, 2, 10, 15, 16, 17, 33, 100)} <= shapes
    assert {('equal', p, k) for p in (1, 64) for k in (1, 15)} <= set(R.CASES)
    assert all((d, 65, 10) in R.CASES for d in R.DESIGNS)


def test_designs_are_what_they_say():
    P, k = 65, 10
    for design, sign in (('ahead60', 1), ('behind60', -1)):
        s = R.scores_of(design, P, k).astype(np.float64)
        gap = sign * (s[:P, None] - s[P:].reshape(P, k))
        assert gap.min() >= 60 - 1e-4 and gap.min() <= 60 + 1e-4
    s = R.scores_of('tie', P, k)
    assert ((s[P:].reshape(P, k) == s[:P, None]).sum(1) >= 1).all()
    assert set(np.abs(R.scores_of('huge', P, k))) == {np.float32(1e4)}
    # the float64 values are the formulas' (autograd of the torch composition in float64)
    for kind in R.KINDS:
        s = R.scores_of('randn8', P, k)
        t = torch.from_numpy(s).double().requires_grad_()
        loss = R.torch_loss(kind, t, P)
        loss.backward()
        ref = R.reference(kind, s, P, k)
        assert abs(float(loss.detach()) - ref['loss']) <= 1e-12 * abs(ref['loss'])
        assert np.abs(t.grad.numpy() - ref['ds']).max() <= 1e-14


@pytest.mark.parametrize('mutation', R.MUTATIONS)
def test_mutation_misses_its_case(mutation):
    assert R.MUTATION_CASES[mutation]
    for kind, design, P, k in R.MUTATION_CASES[mutation]:
        assert (design, P, k) in R.CASES
        s = R.scores_of(design, P, k)
        R.verdicts(kind, design, s, P, k, *R.emulate(kind, s, P, k))                 # the unmutated scheme passes this very case
        with pytest.raises(AssertionError):
            R.verdicts(kind, design, s, P, k, *R.emulate(kind, s, P, k, mutation))


def test_loss_flag_and_setting():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    assert Gs.Training.loss == 'bce'
    assert parse_args([]).loss == 'bce'
    for name in ('bce', 'bpr', 'softmax'):
        assert parse_args(['--loss', name]).loss == name
    with pytest.raises(SystemExit):
        parse_args(['--loss', 'hinge'])
    try:
        driver.apply_training_settings(parse_args(['--loss', 'softmax']))
        assert Gs.Training.loss == 'softmax'
        driver.apply_training_settings(parse_args([]))                           # a run without the flag trains on the BCE, whatever ran before it in this process
        assert Gs.Training.loss == 'bce'
        with pytest.raises(ValueError):
            driver.apply_training_settings(type('Args', (), {'loss': 'hinge'})())
    finally:
        Gs.Training.loss = 'bce'


def test_srrl_refuses_a_ranking_loss():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    driver.check_srrl_settings(parse_args(['--model', 'Srrl']), 1)
    driver.check_srrl_settings(parse_args(['--model', 'Srrl', '--loss', 'bce']), 1)
    for name in ('bpr', 'softmax'):
        with pytest.raises(NotImplementedError, match='--loss'):
            driver.check_srrl_settings(parse_args(['--model', 'Srrl', '--loss', name]), 1)


def test_grouping_is_checked_on_the_host():
    """``B % positives == 0`` and ``B / positives - 1 >= 1``, before any launch: CPU tensors get as far as the check and no further."""
    from ihgnn_amd import _lib, ops
    for args, pair, pool in (((1100, 100, 'bpr'), (100, 1), 10), ((1600, 100, 'softmax'), (100, 2), 15), ((4, 2, _lib.LOSS_KINDS['softmax']), (2, 2), 1)):
        o = ops.ranking_objective(*args)
        assert (o.positives, o.kind) == pair and o.pool == pool and o.keep is None
    for rows, positives in ((1100, 99), (100, 100), (7, 0), (7, -1), (3, 2)):
        with pytest.raises(ValueError, match='rows'):
            ops.ranking_objective(rows, positives, 'bpr')
        with pytest.raises(ValueError, match='rows'):
            ops.ranking_loss(torch.zeros(rows), positives, 'bpr')
    for kind in ('bce', 'hinge', 0, 3, None):
        with pytest.raises(ValueError, match='kind'):
            ops.ranking_objective(4, 2, kind)
    with pytest.raises(ValueError, match='vector'):
        ops.ranking_loss(torch.zeros(2, 2), 2, 'bpr')
    with pytest.raises(_lib.IhgnnHipError, match='GPU tensor'):
        ops.ranking_loss(torch.zeros(4), 2, 'bpr')                                # (grouped correctly: refused for what it is, a CPU tensor - there is no fall-back)


def test_entry_refuses_bad_arguments_before_any_launch():
    from ihgnn_amd import _lib
    lib = _lib.load()
    ws = ctypes.c_void_p(16)
    assert lib.ihg_ranking_loss(ws, 0, 10, 1, ws, ws, None) == _lib.ERR_INVALID and 'positives' in _lib.last_error()
    assert lib.ihg_ranking_loss(ws, 100, 0, 1, ws, ws, None) == _lib.ERR_INVALID and 'k >= 1' in _lib.last_error()
    assert lib.ihg_ranking_loss(ws, 100, 10, 0, ws, ws, None) == _lib.ERR_INVALID and 'kind' in _lib.last_error()
    assert lib.ihg_ranking_loss(ws, 100, 10, 3, ws, ws, None) == _lib.ERR_INVALID and 'kind' in _lib.last_error()
    assert lib.ihg_ranking_loss(ws, (1 << 31) // 11 + 1, 10, 2, ws, ws, None) == _lib.ERR_INVALID and 'INT32_MAX' in _lib.last_error()
    assert lib.ihg_ranking_loss(ws, 1, (1 << 31) - 1, 2, ws, ws, None) == _lib.ERR_INVALID and 'INT32_MAX' in _lib.last_error()
    for args in ((None, 100, 10, 1, ws, ws), (ws, 100, 10, 1, None, ws), (ws, 100, 10, 1, ws, None)):
        assert lib.ihg_ranking_loss(*args, None) == _lib.ERR_INVALID and 'null pointer' in _lib.last_error()
    header = open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read()
    assert '#define IHG_LOSS_BPR 1' in header and '#define IHG_LOSS_SOFTMAX 2' in header and _lib.LOSS_KINDS == {'bpr': 1, 'softmax': 2}


def test_model_refuses_bce_as_a_ranking_loss():
    """``RawGnn.ranking_loss`` reads ``Gs.Training.loss`` when no kind is given and refuses ``'bce'`` (labels are needed) before it touches the model."""
    from ihgnn_amd.Models import RawGnn
    stub = object.__new__(RawGnn)
    index = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match='bce_loss'):
        RawGnn.ranking_loss(stub, index, index, index, 2)
    with pytest.raises(ValueError, match='bce_loss'):
        RawGnn.ranking_loss(stub, index, index, index, 2, 'bce')
    with pytest.raises(ValueError, match='rows'):
        RawGnn.ranking_loss(stub, index, index, index, 3, 'bpr')
