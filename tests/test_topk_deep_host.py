"""No GPU: the host side of rankings deeper than ten - ``Metrics`` at further cutoffs against ``tests/topk_reference.py`` (itself held to the pinned oracle at
K = 10), their accumulation and formatting, ``--cutoffs``, and the argument checks of ``ihg_score_topk_deep``, which answer before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import topk_reference as tref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_case(rng, n_items, n_truth, graded):
    scores = torch.tensor(rng.standard_normal(n_items))                   # float64, no ties
    order = tref.ranking(scores, n_items).tolist()
    # truth: some items of the top ranks (so that a graded case always has a hit: the reference divides by the hits' ideal DCG) and some from anywhere
    truth = sorted(set(order[:3][:max(1, n_truth // 2)]) | set(rng.choice(n_items, n_truth, replace=False).tolist()))
    flags = [int(f) for f in rng.integers(1, 4, len(truth))] if graded else None
    return scores, truth, flags


def test_reference_at_ten_equals_the_pinned_oracle():
    from oracle import ihgnn_ref as ref
    rng = np.random.default_rng(3)
    for trial in range(40):
        scores, truth, flags = random_case(rng, 300, int(rng.integers(1, 15)), graded=bool(trial % 2))
        assert tref.ranking_metrics(scores, truth, flags, 10) == ref.ranking_metrics(scores, truth, flags)


@pytest.mark.parametrize('cutoff', [10, 20, 128])
def test_metrics_at_a_cutoff_equal_the_reference(cutoff):
    from ihgnn_amd.Helpers.Metrics import Metrics
    rng = np.random.default_rng(cutoff)
    for trial in range(40):
        graded = bool(trial % 2)
        scores, truth, flags = random_case(rng, 400, int(rng.integers(1, 40)), graded)
        top = tref.ranking(scores, 128).tolist()                          # ONE list at the largest cutoff; every cutoff reads a prefix
        want = tref.ranking_metrics(scores, truth, flags, cutoff)
        m = Metrics.from_top_indices(top, truth, flags if graded else [1] * len(truth), not graded, cutoff)
        np.testing.assert_allclose((m.HitRatio_at10, m.NDCG_at10, m.MAP_at10), want, rtol=0, atol=1e-12)
        both = Metrics.at_cutoffs(top, truth, flags if graded else [1] * len(truth), not graded, (cutoff,))
        ten = Metrics.from_top_indices(top[:10], truth, flags if graded else [1] * len(truth), not graded)
        assert (both.HitRatio_at10, both.NDCG_at10, both.MAP_at10) == (ten.HitRatio_at10, ten.NDCG_at10, ten.MAP_at10)
        np.testing.assert_allclose(both.extra[cutoff], want, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        Metrics.from_top_indices(list(range(200)), [1], None, True, 129)


def test_accumulation_and_formatting_with_and_without_extras():
    from ihgnn_amd.Helpers.Metrics import Metrics
    # without extras: the strings of the reference's class, byte for byte
    a, b = Metrics(0.5, 0.25, 0.125), Metrics(0.25, 0.5, 0.0625)
    a.add_to_self(b)
    avg = a.divide_and_get_new(2)
    assert (avg.HitRatio_at10, avg.NDCG_at10, avg.MAP_at10) == (0.375, 0.375, 0.09375) and avg.extra == {}
    assert Metrics.title == 'HitRatio@10 NDCG@10 MAP@10'
    assert avg.to_string() == str(avg) == 'HitRatio@10 NDCG@10 MAP@10\n0.3750      0.3750  0.0938'
    assert avg.to_string(no_title=True) == '0.3750 0.3750 0.0938'
    assert avg.to_highlight_string() == 'HitRatio@10 NDCG@10 MAP@10\n\033[0;41m0.3750      0.3750  0.0938\033[0m'
    # with extras: carried through the sum and the division, appended as further lines; the @10 lines and the title-less form are as above
    c = Metrics(0.5, 0.25, 0.125, {20: (0.5, 0.5, 0.25), 100: (1.0, 0.75, 0.5)})
    d = Metrics(0.25, 0.5, 0.0625, {20: (0.25, 0.25, 0.25), 100: (0.5, 0.25, 0.25)})
    total = Metrics()
    total.add_to_self(c)
    total.add_to_self(d)
    assert total.extra == {20: (0.75, 0.75, 0.5), 100: (1.5, 1.0, 0.75)}
    mean = total.divide_and_get_new(2)
    assert mean.extra == {20: (0.375, 0.375, 0.25), 100: (0.75, 0.5, 0.375)}
    assert (mean.HitRatio_at10, mean.NDCG_at10, mean.MAP_at10) == (0.375, 0.375, 0.09375)
    assert mean.to_string(no_title=True) == '0.3750 0.3750 0.0938'
    lines = mean.to_string().split('\n')
    assert '\n'.join(lines[:2]) == avg.to_string()
    assert lines[2].split() == ['HitRatio@20', 'NDCG@20', 'MAP@20'] and lines[3].split() == ['0.3750', '0.3750', '0.2500']
    assert lines[4].split() == ['HitRatio@100', 'NDCG@100', 'MAP@100'] and lines[5].split() == ['0.7500', '0.5000', '0.3750'] and len(lines) == 6
    assert mean.to_highlight_string().split('\n')[1] == avg.to_highlight_string().split('\n')[1]


def test_cutoffs_flag():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    assert parse_args([]).cutoffs == ()
    assert parse_args(['--cutoffs', '20,50,100']).cutoffs == (20, 50, 100)
    assert parse_args(['--cutoffs', '128, 11,11']).cutoffs == (11, 128)
    for bad in ('5', '129', '20,ten', '10', '20;50'):
        with pytest.raises(SystemExit):
            parse_args(['--cutoffs', bad])
    old = Gs.Evaluation.extra_cutoffs
    try:
        driver.apply_evaluation_settings(parse_args(['--cutoffs', '100,20']))
        assert Gs.Evaluation.extra_cutoffs == (20, 100)
        driver.apply_evaluation_settings(parse_args([]))                  # a run without the flag reports @10 alone, whatever ran before it in this process
        assert Gs.Evaluation.extra_cutoffs == ()
    finally:
        Gs.Evaluation.extra_cutoffs = old


def test_entry_points_are_declared_in_header_and_binding():
    from ihgnn_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('ihg_score_topk_max_k', 'ihg_score_topk_deep_workspace_bytes', 'ihg_score_topk_deep'):
        assert re.search(r'\b' + name + r'\s*\(', text) and name in _lib.SIGNATURES and hasattr(lib, name), name
    # ihg_score_topk's arguments, then the head and the pass counts in front of the stream
    base = _lib.SIGNATURES['ihg_score_topk'][1]
    assert _lib.SIGNATURES['ihg_score_topk_deep'] == (ctypes.c_int, base[:-1] + [ctypes.c_int32, ctypes.c_void_p] + base[-1:])
    assert _lib.load().ihg_score_topk_max_k() == 128
    assert _lib.ABI_VERSION == 37 == _lib.load().ihg_abi_version()        # entry points were added, none changed


def test_bad_arguments_are_refused_before_any_launch():
    """This runs where there is no GPU: an answer at all means that nothing was launched."""
    from ihgnn_amd import _lib
    from ihgnn_amd.Models import RawGnn
    lib = _lib.load()
    ws = ctypes.c_void_p(4096)                                            # a non-null, 16-byte aligned address that is never dereferenced
    top = lambda dim, n_items, k, n_pairs=1, feats=ws, space=ws, nbytes=1 << 40, cosine=0, passes=None: lib.ihg_score_topk_deep(
        feats, 2000, dim, 0, 0, n_items, ws, ws, ws, 0.5, n_pairs, k, ws, ws, space, nbytes, cosine, passes, None)
    for cosine in (0, 1):
        for k in (0, 129, -1):
            assert top(64, 1000, k, cosine=cosine) == _lib.ERR_INVALID
            assert 'ihg_score_topk_deep' in _lib.last_error() and '128' in _lib.last_error()
    assert top(RawGnn.MAX_SCORED_WIDTH + 1, 1000, 128) == _lib.ERR_INVALID and str(RawGnn.MAX_SCORED_WIDTH) in _lib.last_error()
    assert top(64, 0, 128) == _lib.ERR_INVALID and top(64, 1000, 128, feats=None) == _lib.ERR_INVALID and top(2001, 1000, 128) == _lib.ERR_INVALID
    # a short workspace: refused like its siblings' (the code the header gives that cause), its own name in the message
    need = lib.ihg_score_topk_deep_workspace_bytes(1, 1000, 64, 128)
    for short in (dict(nbytes=16), dict(nbytes=need - 1), dict(space=None), dict(space=ctypes.c_void_p(4100))):
        assert top(64, 1000, 128, **short) == _lib.ERR_WORKSPACE and 'ihg_score_topk_deep' in _lib.last_error()
    assert top(64, 1000, 128, n_pairs=0) == _lib.OK                        # an empty call launches nothing
    for n_pairs, n_items, dim in ((1, 1000, 64), (4096, 120000, 384), (37, 70001, 192), (70, 300, 1264)):
        for k in (1, 10, 128):
            assert lib.ihg_score_topk_deep_workspace_bytes(n_pairs, n_items, dim, k) >= lib.ihg_score_topk_workspace_bytes(n_pairs, n_items, dim) > 0
    assert lib.ihg_score_topk_deep_workspace_bytes(1, 1000, 64, 129) == 0 == lib.ihg_score_topk_deep_workspace_bytes(1, 1000, 64, 0)
