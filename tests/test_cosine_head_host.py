"""No GPU: the cosine-similarity HEM head (``Gs.Prediction.use_cosine_similarity``) - the float64 restatement (``tests/cosine_reference.py``) against the reference's
own numbers (fixture F14, ``tests/golden/make_golden_cosine.py``), the ``--cosine`` flag, the three entry points' declarations and their argument checks."""
import ctypes
import os
import re

import numpy as np
import torch

import cosine_reference as cref
import query_transform_reference as qref
from conftest import GOLDEN, REPO

BAR = 2e-6                                                               # test_oracle_golden.py's bar for a float64 restatement against the reference's float32
MODEL_CASES = (('ihgnn_o3_d32', 'ihgnn'), ('hgcn_d64', 'hgcn'))


def f14():
    return np.load(os.path.join(GOLDEN, 'f14_cosine.npz'))


def small():
    return np.load(os.path.join(GOLDEN, 'f2_small_workload.npz'))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_restatement_reproduces_the_reference_head():
    """F14's ``HemPredictionLayer.forward``: scores to 2e-6, the zero item row gives the bare bias (cos = 0) and the row of norm 2e-9 a fifth of its unit row's cosine;
    the closed-form row gradients are autograd's of ``torch.cosine_similarity`` in float64."""
    z = f14()
    user, query, item = (qref.t64(z['head.' + k]) for k in ('user', 'query', 'item'))
    idx = torch.from_numpy(z['head.indices'])
    bias = qref.t64(z['head.bias'])[idx]
    got = cref.hem_cosine(user, query, item, bias, float(z['head.lam']))
    assert rel(got, z['head.scores']) <= BAR
    assert float(item[3].norm()) == 0.0 and abs(float(got[3] - bias[3])) == 0.0
    shrink = float(item[4].norm()) / cref.EPS                            # the clamp divides by eps, not by the norm: the row counts for norm / eps of a unit row
    assert abs(shrink - 0.2) <= 1e-6
    m = 0.5 * query + 0.5 * user
    unit = float((item[4] / item[4].norm()) @ (m[4] / m[4].norm()))
    assert abs(float(got[4] - bias[4]) - shrink * unit) <= 1e-12
    u, q, a = (t.clone().requires_grad_(True) for t in (user, query, item))
    ds = torch.linspace(-1, 1, user.shape[0], dtype=torch.float64)
    ((torch.cosine_similarity(a, 0.5 * q + 0.5 * u) + bias) * ds).sum().backward()
    for mine, theirs in zip(cref.row_gradients(user, query, item, ds), (u.grad, q.grad, a.grad)):
        assert torch.isfinite(mine).all() and rel(mine, theirs) <= 1e-12


def test_restatement_reproduces_the_reference_models():
    """Every array of F14's two models: scores, loss, every gradient, the Adam-stepped parameters, the all-item scores of the 12 test logs and their metrics."""
    from ihgnn_amd.Helpers.Metrics import Metrics
    z, w = f14(), small()
    ends = np.cumsum(z['test.items_len'])
    for tag, kind in MODEL_CASES:
        pre = tag + '.'
        L, order, d, _ = (int(v) for v in z[pre + 'cfg'])
        sd = qref.fixture_state(z, tag)
        step = cref.model_step(sd, w['triples'], w['counts'], w['bag_words'] + 1, w['bag_offsets'], kind, L, order, z[pre + 'u'], z[pre + 'q'], z[pre + 'i'], z[pre + 'flags'])
        assert rel(step['scores'], z[pre + 'scores']) <= BAR and abs(step['loss'] - float(z[pre + 'loss'])) <= BAR
        for n in sd:
            assert qref.fixture_error(z, pre + 'grad.' + n, step['grads'][n]) <= BAR, (tag, n)
            assert qref.fixture_adam_excess(z, pre + 'adam.' + n, step['grads'][n], step['adam'][n], BAR) <= 1.0, (tag, n)
        all64 = cref.model_all_item_scores(sd, w['triples'], w['counts'], w['bag_words'] + 1, w['bag_offsets'], kind, L, order, z['test.uq'][:, 0], z['test.uq'][:, 1])
        assert rel(all64, z[pre + 'all_scores']) <= BAR
        per_log = []
        for k in range(len(ends)):
            items = z['test.items_flat'][ends[k] - z['test.items_len'][k]:ends[k]].tolist()
            m = Metrics.calculate_on_all_items(torch.from_numpy(z[pre + 'all_scores'][k]), items, None, True)
            per_log.append((m.HitRatio_at10, m.NDCG_at10, m.MAP_at10))
        np.testing.assert_allclose(per_log, z[pre + 'metrics_per_log'], atol=1e-12)
        np.testing.assert_allclose(np.mean(per_log, 0), z[pre + 'metrics'], atol=1e-12)


def test_cosine_flag_sets_and_clears_the_setting():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    assert parse_args(['--cosine']).cosine is True and parse_args([]).cosine is False
    old = Gs.Prediction.use_cosine_similarity
    try:
        driver.apply_prediction_settings(parse_args(['--cosine']))
        assert Gs.Prediction.use_cosine_similarity is True
        driver.apply_prediction_settings(parse_args([]))                 # a run without the flag gets the dot product, whatever ran before it in this process
        assert Gs.Prediction.use_cosine_similarity is False
    finally:
        Gs.Prediction.use_cosine_similarity = old


def test_entry_points_are_declared_in_header_and_binding():
    from ihgnn_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('ihg_hem_cosine_fwd', 'ihg_hem_cosine_bwd', 'ihg_score_topk_cosine'):
        assert re.search(r'\b' + name + r'\s*\(', text) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES['ihg_score_topk_cosine'] == _lib.SIGNATURES['ihg_score_topk']
    assert _lib.ABI_VERSION == 37 == _lib.load().ihg_abi_version()


def test_bad_arguments_return_invalid_and_launch_nothing():
    """As their siblings: every check answers ``IHG_ERR_INVALID`` with a message before any launch (this runs where there is no GPU)."""
    from ihgnn_amd import _lib
    from ihgnn_amd.Models import RawGnn
    lib = _lib.load()
    ws = ctypes.c_void_p(4096)                                           # a non-null, 16-byte aligned address that is never dereferenced
    odd = ctypes.c_void_p(4100)
    layers9 = (ctypes.c_void_p * 9)(*[4096] * 9)
    fwd = lambda layers, n, ld, dim, l0, ld0, tb, rows, items, bias, scores, stats, batch: lib.ihg_hem_cosine_fwd(layers, n, ld, dim, l0, ld0, tb, rows, None, items, bias, 0.5,
                                                                                                                    scores, stats, batch, None)
    bwd = lambda layers, n, ld, dim, l0, ld0, tb, rows, dscores, stats, rowgrad, ldg, batch: lib.ihg_hem_cosine_bwd(layers, n, ld, dim, l0, ld0, tb, rows, None, dscores, stats, None,
                                                                                                                     1.0, 0.5, rowgrad, ldg, batch, None)
    for n_layers, ld, dim in ((9, 4, 4), (0, 4, 4), (2, 3, 4), (2, 4, 0)):
        assert fwd(layers9, n_layers, ld, dim, None, 0, None, ws, ws, ws, ws, ws, 5) == _lib.ERR_INVALID
        assert 'ihg_hem_cosine_fwd' in _lib.last_error()
        assert bwd(layers9, n_layers, ld, dim, None, 0, None, ws, ws, ws, ws, 64, 5) == _lib.ERR_INVALID
        assert 'ihg_hem_cosine_bwd' in _lib.last_error()
    assert fwd(None, 2, 4, 4, None, 0, None, ws, ws, ws, ws, ws, 5) == _lib.ERR_INVALID
    assert fwd(layers9, 2, 4, 4, None, 0, None, ws, ws, ws, ws, ws, -1) == _lib.ERR_INVALID
    assert fwd(layers9, 2, 4, 4, layers9, 4, None, ws, ws, ws, ws, ws, 5) == _lib.ERR_INVALID          # typed layer 0 without its type ranges
    assert fwd(layers9, 2, 4, 4, None, 0, None, ws, ws, ws, ws, None, 5) == _lib.ERR_INVALID           # no stats buffer
    assert fwd(layers9, 2, 4, 4, None, 0, None, ws, ws, ws, ws, odd, 5) == _lib.ERR_INVALID            # stats rows are 16 bytes, read and written whole
    assert 'aligned' in _lib.last_error()
    assert fwd(layers9, 2, 4, 4, None, 0, None, None, ws, ws, ws, ws, 5) == _lib.ERR_INVALID
    holes = (ctypes.c_void_p * 2)(4096, None)
    assert fwd(holes, 2, 4, 4, None, 0, None, ws, ws, ws, ws, ws, 5) == _lib.ERR_INVALID and 'null layer' in _lib.last_error()
    assert bwd(layers9, 2, 4, 4, None, 0, None, ws, ws, ws, ws, 7, 5) == _lib.ERR_INVALID              # rowgrad rows shorter than 2 x 4
    assert bwd(layers9, 2, 4, 4, None, 0, None, ws, ws, None, ws, 12, 5) == _lib.ERR_INVALID
    assert bwd(layers9, 2, 4, 4, None, 0, None, ws, None, ws, ws, 12, 5) == _lib.ERR_INVALID
    assert bwd(layers9, 2, 4, 4, layers9, 3, (ctypes.c_int64 * 4)(0, 1, 2, 3), ws, ws, ws, ws, 12, 5) == _lib.ERR_INVALID    # layer 0's row stride below dim
    assert fwd(layers9, 8, 4, 4, None, 0, None, ws, ws, ws, ws, ws, 0) == _lib.OK and bwd(layers9, 8, 4, 4, None, 0, None, ws, ws, ws, ws, 64, 0) == _lib.OK     # an empty batch launches nothing
    # ihg_score_topk_cosine: ihg_score_topk's checks, its own name in the message
    top = lambda dim, n_items, k, n_pairs=1, feats=ws, space=ws, nbytes=1 << 40: lib.ihg_score_topk_cosine(feats, 2000, dim, 0, 0, n_items, ws, ws, ws, 0.5, n_pairs, k, ws, ws, space,
                                                                                                            nbytes, None)
    assert top(RawGnn.MAX_SCORED_WIDTH + 1, 10, 10) == _lib.ERR_INVALID
    assert 'ihg_score_topk_cosine' in _lib.last_error() and str(RawGnn.MAX_SCORED_WIDTH) in _lib.last_error()
    assert top(64, 10, 11) == _lib.ERR_INVALID and top(64, 0, 10) == _lib.ERR_INVALID and top(64, 10, 10, feats=None) == _lib.ERR_INVALID
    assert top(2001, 10, 10) == _lib.ERR_INVALID                          # row stride below the width
    assert top(64, 10, 10, nbytes=16) == _lib.ERR_WORKSPACE and top(64, 10, 10, space=None) == _lib.ERR_WORKSPACE
    assert top(64, 10, 10, n_pairs=0) == _lib.OK
