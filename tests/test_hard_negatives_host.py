"""Hard negatives (``--hard_negatives M``) without a GPU: the float32 emulation of ``ihg_hard_negative_loss`` is held to the verdicts the GPU file holds the kernel to, on
the same cases (``tests/hard_negatives_reference.py``), each mutation of it misses a named verdict, the pool stream's properties, and the host side - both entries'
argument checks (which come before any launch), the symbols, the flag, the settings, the host check of the batch's grouping."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hard_negatives_reference as H
import logged_negatives_reference as L
from conftest import REPO


# ---------------------------------------------------------------------------------------------
# the emulation and its mutations
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sorted(H.KINDS))
def test_emulation_meets_every_verdict(kind):
    worst = {}
    for design, P, M, k in H.CASES:
        s = H.scores_of(design, P, M, k)
        for name, ratio in H.verdicts(kind, design, s, P, M, k, *H.emulate(kind, s, P, M, k)).items():
            worst[name] = max(worst.get(name, 0.0), ratio)
    print(f'{kind}: worst error / bound of the emulation {worst}')
    assert all(0 < ratio <= 1 for ratio in worst.values())


def test_cases_cover_the_ladder():
    shapes = {(p, m, k) for _, p, m, k in H.CASES}
    assert {p for p, _, _ in shapes} == {1, 2, 15, 16, 17, 33, 1025}
    assert {m for _, m, _ in shapes} == {2, 11, 63, 64, 65, 128, 255, 256}
    for m in H.M_LADDER:
        assert {k for _, mm, k in shapes if mm == m} >= {k for k in (1, 10, m - 1, m) if 1 <= k <= m}
    assert set(H.DESIGNS) == {d for d, *_ in H.CASES} and set(H.DESIGNS) >= set(H.R.DESIGNS) | {'tiek', 'bits'}
    assert 24 <= len(shapes) <= 60
    assert all(k <= m <= 256 for _, m, k in shapes)


def test_designs_are_what_they_say():
    P, M, k = 17, 65, 10
    s = H.scores_of('tiek', P, M, k)
    cand = s[P:].reshape(P, M)
    assert (cand[0] == cand[0, 0]).all() and (H.select(s, P, M, k)[0] == np.arange(k)).all()      # a whole group equal: the lowest positions win
    straddling = 0
    for p in range(P):
        ordered = np.sort(cand[p])[::-1]
        straddling += ordered[k - 1] == ordered[k]
    assert straddling == P                                                   # every group has equal scores either side of the k-th place
    bits = H.scores_of('bits', P, M, k)[P:].view(np.uint32)
    for pattern in (0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000):
        assert (bits == pattern).any(), hex(pattern)
    # the key order: -NaN < -inf < -1 < -0 < +0 < 1 < +inf < +NaN, strictly
    ladder = np.array([0xFFC00000, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000, 0x7F800000, 0x7FC00000], np.uint32).view(np.float32)
    keys = H.score_keys(ladder).astype(np.int64)
    assert (np.diff(keys) > 0).all()
    finite = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    assert (np.argsort(H.score_keys(finite), kind='stable') == np.argsort(finite, kind='stable')).all()
    # the compaction is collate_fn's layout: the BCE's float64 values are autograd's on it
    sel = H.select(H.scores_of('randn8', P, M, k), P, M, k)
    small = H.compact(H.scores_of('randn8', P, M, k), P, M, sel)
    assert small.shape == (P * (1 + k),) and (small[P:].reshape(P, k)[:, :-1] >= small[P:].reshape(P, k)[:, 1:]).all()
    t = torch.from_numpy(small).double().requires_grad_()
    y = torch.cat([torch.ones(P), torch.zeros(P * k)]).double()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(t, y)
    loss.backward()
    ref = H.bce_reference(small, P, k)
    assert abs(float(loss.detach()) - ref['loss']) <= 1e-12 * abs(ref['loss']) and np.abs(t.grad.numpy() - ref['ds']).max() <= 1e-14


@pytest.mark.parametrize('mutation', H.MUTATIONS)
def test_mutation_misses_its_verdict(mutation):
    assert H.MUTATION_CASES[mutation]
    for (kind, design, P, M, k), word in H.MUTATION_CASES[mutation]:
        assert (design, P, M, k) in H.CASES
        s = H.scores_of(design, P, M, k)
        H.verdicts(kind, design, s, P, M, k, *H.emulate(kind, s, P, M, k))        # the unmutated scheme passes this very case
        with pytest.raises(AssertionError, match=word):
            H.verdicts(kind, design, s, P, M, k, *H.emulate(kind, s, P, M, k, mutation))


# ---------------------------------------------------------------------------------------------
# the pool stream
# ---------------------------------------------------------------------------------------------
def test_pool_stream_prefix_and_sample_negatives():
    seed, counter = 7919 * 3 + 1, (5 << 32) + 17
    for n_items in (256, 257, 1000, 2 ** 40):
        full = H.pool_draw(seed, counter, 65, n_items, 256)
        assert ((full >= 0) & (full < n_items)).all()
        assert all(len(set(row.tolist())) == 256 for row in full)
        for c in (1, 16, 17, 64, 65):
            assert (H.pool_draw(seed, counter, 65, n_items, c) == full[:, :c]).all(), (n_items, c)
        for c in (1, 10, 16):
            assert (L.sample_negatives(seed, counter, 65, n_items, c) == full[:, :c]).all(), (n_items, c)
    assert (np.sort(H.pool_draw(seed, counter, 65, 256, 256), 1) == np.arange(256)).all()      # m = n_items: a permutation of the catalogue
    assert (np.sort(H.pool_draw(seed, counter, 5, 50, 50), 1) == np.arange(50)).all()


def test_chunked_draw_is_the_sequential_draw_and_the_chunk_check_matters():
    seed, counter = 11, 4
    for n_items, m in ((256, 256), (257, 256), (1000, 256), (50, 50), (2 ** 40, 65), (17, 16), (65, 64)):
        want = H.pool_draw(seed, counter, 9, n_items, m)
        assert (H.pool_draw_chunked(seed, counter, 9, n_items, m) == want).all(), (n_items, m)
    # without the earlier-lane check a value that repeats inside one chunk is accepted twice: rows lose their distinctness and leave the sequential stream
    broken = H.pool_draw_chunked(seed, counter, 9, 256, 256, mutation='chunk_duplicate_accepted')
    assert (broken != H.pool_draw(seed, counter, 9, 256, 256)).any() and any(len(set(row.tolist())) < 256 for row in broken)


def test_pool_draws_are_uniform():
    """Chi-square of the first column and of all columns over 100 items, 20,000 rows x 20 draws at a fixed seed.  99 degrees of freedom: the 99.9 % critical value is
    148.2.  (Columns of one row are distinct, which makes the pooled counts slightly MORE even than independent draws: the bar stays valid.)"""
    n_items, rows, m = 100, 20000, 20
    draws = H.pool_draw(2024, 1, rows, n_items, m)
    critical = 148.2
    for sample in (draws[:, 0], draws[:, m - 1], draws.reshape(-1)):
        counts = np.bincount(sample, minlength=n_items)
        expected = sample.shape[0] / n_items
        chi2 = float(((counts - expected) ** 2 / expected).sum())
        print(f'chi-square over {sample.shape[0]} draws: {chi2:.1f}')
        assert chi2 < critical


# ---------------------------------------------------------------------------------------------
# the entries' refusals, the symbols
# ---------------------------------------------------------------------------------------------
def test_sample_pool_refuses_bad_arguments_before_any_launch():
    from ihgnn_amd import _lib
    lib = _lib.load()
    out = ctypes.c_void_p(16)
    for m, n_items in ((0, 100), (-1, 100), (257, 1000), (11, 10), (1, 0)):
        assert lib.ihg_sample_pool(1, 2, 5, n_items, m, out, None) == _lib.ERR_INVALID, (m, n_items)
        assert 'ihg_sample_pool' in _lib.last_error() and '1 <= m <= min(256, n_items)' in _lib.last_error()
    assert lib.ihg_sample_pool(1, 2, 5, 100, 20, None, None) == _lib.ERR_INVALID and 'ihg_sample_pool: null pointer' in _lib.last_error()
    assert lib.ihg_sample_pool(1, 2, 0, 100, 20, None, None) == _lib.OK                      # no rows: nothing to write, nothing launched


def test_hard_negative_loss_refuses_bad_arguments_before_any_launch():
    from ihgnn_amd import _lib
    lib = _lib.load()
    ws = ctypes.c_void_p(16)
    call = lambda *a: lib.ihg_hard_negative_loss(*a, None)
    for pool, keep in ((20, 0), (20, -3), (20, 21), (257, 10), (0, 0)):
        assert call(ws, 100, pool, keep, 1, ws, ws, ws) == _lib.ERR_INVALID and '1 <= keep <= pool <= 256' in _lib.last_error(), (pool, keep)
    assert call(ws, 0, 20, 10, 1, ws, ws, ws) == _lib.ERR_INVALID and 'positives >= 1' in _lib.last_error()
    for kind in (-1, 3, 7):
        assert call(ws, 100, 20, 10, kind, ws, ws, ws) == _lib.ERR_INVALID and 'kind' in _lib.last_error()
    assert call(ws, (1 << 31) // 257 + 1, 256, 10, 0, ws, ws, ws) == _lib.ERR_INVALID and 'INT32_MAX' in _lib.last_error()
    assert call(ws, 1 << 40, 2, 1, 2, ws, ws, ws) == _lib.ERR_INVALID and 'INT32_MAX' in _lib.last_error()
    for args in ((None, 100, 20, 10, 1, ws, ws, ws), (ws, 100, 20, 10, 1, None, ws, ws), (ws, 100, 20, 10, 1, ws, None, ws), (ws, 100, 20, 10, 1, ws, ws, None)):
        assert call(*args) == _lib.ERR_INVALID and 'ihg_hard_negative_loss: null pointer' in _lib.last_error()


def test_symbols_are_declared_and_exported_and_the_abi_stays():
    from ihgnn_amd import _lib
    lib = _lib.load()
    assert lib.ihg_abi_version() == 37 and _lib.ABI_VERSION == 37
    header = open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read()
    for name in ('ihg_sample_pool', 'ihg_hard_negative_loss'):
        assert re.search(r'^int ' + name + r'\(', header, re.M) and name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and hasattr(lib, name), f'{name} declared but not exported'
    assert '#define IHG_LOSS_BCE 0' in header and _lib.HARD_NEGATIVE_KINDS == {'bce': 0, 'bpr': 1, 'softmax': 2} == H.KINDS
    assert _lib.POOL_MAX == H.POOL_MAX == 256


# ---------------------------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------------------------
def test_objective_is_checked_on_the_host():
    from ihgnn_amd import _lib, ops
    o = ops.hard_negative_objective(100 * 51, 100, 10, 'bpr')
    assert (o.positives, o.pool, o.keep, o.kind, o.selected) == (100, 50, 10, 1, None)
    assert ops.hard_negative_objective(6, 2, 2, 'bce').kind == 0 and ops.hard_negative_objective(6, 2, 1, 2).kind == 2
    for rows, positives in ((5100, 99), (100, 100), (7, 0), (7, -1)):
        with pytest.raises(ValueError, match='rows'):
            ops.hard_negative_objective(rows, positives, 1, 'bpr')
        with pytest.raises(ValueError, match='rows'):
            ops.hard_negative_loss(torch.zeros(rows), positives, 1, 'bpr')
    for keep in (0, -1, 51):
        with pytest.raises(ValueError, match='keep'):
            ops.hard_negative_objective(5100, 100, keep, 'bpr')
    with pytest.raises(ValueError, match='256'):
        ops.hard_negative_objective(2 * 258, 2, 10, 'bpr')
    for kind in ('hinge', 3, -1, None, True):
        with pytest.raises(ValueError, match='kind'):
            ops.hard_negative_objective(6, 2, 1, kind)
    with pytest.raises(ValueError, match='vector'):
        ops.hard_negative_loss(torch.zeros(3, 2), 2, 1, 'bpr')
    with pytest.raises(_lib.IhgnnHipError, match='GPU tensor'):
        ops.hard_negative_loss(torch.zeros(6), 2, 1, 'bpr')                      # (grouped correctly: refused for what it is, a CPU tensor - there is no fall-back)


def test_model_checks_the_grouping_before_it_touches_the_model():
    from ihgnn_amd.Models import RawGnn
    stub = object.__new__(RawGnn)
    index = torch.zeros(6, dtype=torch.int64)
    with pytest.raises(ValueError, match='rows'):
        RawGnn.hard_negative_loss(stub, index, index, index, 4, 1)
    with pytest.raises(ValueError, match='keep'):
        RawGnn.hard_negative_loss(stub, index, index, index, 2, 3)               # kind=None reads Gs.Training.loss: 'bce' is legal here
    with pytest.raises(ValueError, match='kind'):
        RawGnn.hard_negative_loss(stub, index, index, index, 2, 1, 'hinge')


def test_flag_and_settings():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    assert Gs.Training.negative_pool == 0 and parse_args([]).hard_negatives == 0
    assert parse_args(['--hard_negatives', '50']).hard_negatives == 50
    with pytest.raises(SystemExit):
        parse_args(['--hard_negatives', 'many'])
    kept = Gs.random_negative_sample_size
    try:
        driver.apply_training_settings(parse_args(['--hard_negatives', '50', '--loss', 'bpr']))
        assert Gs.Training.negative_pool == 50 and Gs.Training.loss == 'bpr'
        driver.apply_training_settings(parse_args([]))                           # a run without the flag draws no pool, whatever ran before it in this process
        assert Gs.Training.negative_pool == 0 and Gs.Training.loss == 'bce'
        driver.apply_training_settings(parse_args(['--hard_negatives', '256']))
        assert Gs.Training.negative_pool == 256
        for bad in (str(kept), str(kept - 1), '1', '257', '-4'):
            with pytest.raises(ValueError, match='--hard_negatives'):
                driver.apply_training_settings(parse_args(['--hard_negatives', bad]))
            assert Gs.Training.negative_pool == 256                              # a refusal assigns nothing
        with pytest.raises(ValueError, match='--logged_negatives'):
            driver.apply_training_settings(parse_args(['--hard_negatives', '50', '--logged_negatives', '2']))
    finally:
        Gs.Training.loss, Gs.Training.negative_pool = 'bce', 0
    driver.check_srrl_settings(parse_args(['--model', 'Srrl']), 1)
    with pytest.raises(NotImplementedError, match='--hard_negatives'):
        driver.check_srrl_settings(parse_args(['--model', 'Srrl', '--hard_negatives', '50']), 1)


def test_recording_needs_positives_under_a_pool():
    """The recording reads the pool when it is made and refuses, before it touches the model, a batch it cannot group."""
    from ihgnn_amd.captured_step import CapturedTrainingStep
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.optim import Adam
    w = torch.nn.Parameter(torch.zeros(2))
    opt = Adam([w], 1e-3)
    Gs.Training.negative_pool = 50
    try:
        with pytest.raises(ValueError, match='positives'):
            CapturedTrainingStep(torch.nn.Linear(1, 1), opt, 5100)
        with pytest.raises(ValueError, match='pool of 20'):
            CapturedTrainingStep(torch.nn.Linear(1, 1), opt, 2100, positives=100)
    finally:
        Gs.Training.negative_pool = 0
