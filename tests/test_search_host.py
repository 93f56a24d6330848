"""The host side of the search API, where there is no GPU: the two entry points are declared, every bad argument of ``ihg_search_topk`` is refused before a launch,
``RawGnn.search`` checks what it is given on the host, ``ops.pack_item_mask`` packs the words the kernel reads, and ``tests/search_reference.py`` agrees with
``ranking_reference``'s own reference on a feature matrix that has the external rows appended."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ranking_reference as R
import search_reference as S
import topk_reference as tref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_in_header_binding_and_library():
    from ihgnn_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('ihg_search_topk_workspace_bytes', 'ihg_search_topk'):
        assert re.search(r'\b' + name + r'\s*\(', text) and name in _lib.SIGNATURES and hasattr(lib, name), name
    # ihg_score_topk_deep's arguments with (query_rows, ld_q, q_dim, item_mask) behind `queries`
    deep = _lib.SIGNATURES['ihg_score_topk_deep'][1]
    assert _lib.SIGNATURES['ihg_search_topk'] == (ctypes.c_int, deep[:9] + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p] + deep[9:])
    assert _lib.SIGNATURES['ihg_search_topk_workspace_bytes'] == _lib.SIGNATURES['ihg_score_topk_deep_workspace_bytes']
    assert _lib.ABI_VERSION == 37 == _lib.load().ihg_abi_version()        # entry points were added, none changed


def test_bad_arguments_are_refused_before_any_launch():
    """This runs where there is no GPU: an answer at all means that nothing was launched."""
    from ihgnn_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)                                             # a non-null, 16-byte aligned address that is never dereferenced

    def call(dim=64, n_items=1000, k=10, n_pairs=1, queries=p, query_rows=None, ld_q=0, q_dim=0, mask=None, space=p, nbytes=1 << 40, cosine=0):
        return lib.ihg_search_topk(p, 2000, dim, 0, 0, n_items, p, p, queries, query_rows, ld_q, q_dim, mask, 0.5, n_pairs, k, p, p, space, nbytes, cosine, None, None)

    def refused(**kw):
        rc = call(**kw)
        return rc == _lib.ERR_INVALID and 'ihg_search_topk' in _lib.last_error()

    assert refused(queries=p, query_rows=p, ld_q=32, q_dim=32)            # both query sources
    assert refused(queries=None, query_rows=None)                          # neither
    for q_dim in (0, -1, 65):
        assert refused(queries=None, query_rows=p, ld_q=64, q_dim=q_dim)
    assert refused(queries=None, query_rows=p, ld_q=31, q_dim=32)
    for cosine in (0, 1):
        for k in (0, -1, 129):
            assert refused(k=k, cosine=cosine) and '128' in _lib.last_error()
    need = lib.ihg_search_topk_workspace_bytes(1, 1000, 64, 128)
    assert need == lib.ihg_score_topk_deep_workspace_bytes(1, 1000, 64, 128) + 16 == R.deep_workspace_bytes(1, 1000, 64) + 16
    for short in (dict(nbytes=16), dict(nbytes=need - 1), dict(space=None), dict(space=ctypes.c_void_p(4100))):
        assert refused(k=128, **short)
    assert refused(dim=1265) and refused(n_items=0) and refused(dim=2001)
    # the same bad arguments with nothing to do are still bad; a good empty call launches nothing
    assert refused(n_pairs=0, queries=None, query_rows=None) and refused(n_pairs=0, k=129)
    assert call(n_pairs=0) == _lib.OK and call(n_pairs=0, queries=None, query_rows=p, ld_q=40, q_dim=32, mask=p) == _lib.OK
    for k in (0, 129):
        assert lib.ihg_search_topk_workspace_bytes(1, 1000, 64, k) == 0


def _stub(user_count=5, query_count=4, item_count=7, vocab_size=9, self_loops=False):
    ds = types.SimpleNamespace(user_count=user_count, query_count=query_count, item_count=item_count, vocab_size=vocab_size)
    layer = types.SimpleNamespace(graph=types.SimpleNamespace(self_loops=self_loops))
    return types.SimpleNamespace(dataset=ds, gnns=[layer])


def test_model_search_checks_its_inputs_on_the_host():
    """``RawGnn._check_search_inputs`` is the first thing ``search`` does: it needs the dataset's counts and the layers' graphs, nothing on a device."""
    from ihgnn_amd.Models import RawGnn
    check = lambda *a, **kw: RawGnn._check_search_inputs(_stub(), *a, **kw)
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    good = dict(users=t(0, -1, 4), queries=None, words=t(0, 8, 3), offsets=t(0, 1, 1), candidates=None)
    w, o = check(**good)
    assert w.tolist() == [0, 8, 3] and o.tolist() == [0, 1, 1]
    assert check(t(0, -1), t(3, 0), None, None, t(0, 6)) == (None, None)
    assert check(t(0, -1), t(3, 0), None, None, torch.ones(7, dtype=torch.bool)) == (None, None)
    bad = [dict(users=t(0, -2, 4)), dict(users=t(0, 5, 4)),                                     # users outside [-1, U)
           dict(words=t(0, 9, 3)), dict(words=t(-1, 8, 3)),                                     # word ids outside [0, V)
           dict(offsets=t(1, 1, 2)), dict(offsets=t(0, 2, 1)), dict(offsets=t(0, 1, 4)), dict(offsets=t(0, 1)),   # offsets: start, order, range, count
           dict(candidates=t(0, 7)), dict(candidates=t(-1)), dict(candidates=torch.ones(6, dtype=torch.bool)),  # candidate ids outside [0, I)
           dict(queries=t(0, 1, 2)),                                                            # both query forms
           dict(words=None, offsets=None),                                                      # neither
           dict(offsets=None)]                                                                  # words without offsets
    for change in bad:
        with pytest.raises(ValueError):
            check(**{**good, **change})
    with pytest.raises(ValueError):
        check(t(0, 1), t(0, 4), None, None, None)                                               # a query outside [0, Q)
    with pytest.raises(NotImplementedError):
        RawGnn._check_search_inputs(_stub(self_loops=True), **good)
    from ihgnn_amd.Models import Srrl
    assert not hasattr(Srrl, 'search')


def test_pair_layout_records_its_self_connections():
    from ihgnn_amd.layout import PairLayout
    triples = np.array([[0, 0, 0], [1, 1, 1]])
    cpu = torch.device('cpu')
    assert PairLayout(triples, 2, 3, 2, cpu, self_loops=True).self_loops is True and PairLayout(triples, 2, 3, 2, cpu).self_loops is False


@pytest.mark.parametrize('n_items', [1, 31, 32, 33, 64, 100])
def test_mask_packing_against_numpy(n_items):
    from ihgnn_amd import ops
    rng = np.random.default_rng(n_items)
    for flags in (rng.random(n_items) < 0.5, np.ones(n_items, bool), np.zeros(n_items, bool), S.mask_pattern('last', n_items), S.mask_pattern('last_of_word', n_items)):
        want = S.pack_mask(flags)
        assert want.shape == ((n_items + 31) // 32,)
        assert all(bool(want[i >> 5] >> (i & 31) & 1) == bool(flags[i]) for i in range(n_items))
        got = ops.pack_item_mask(torch.from_numpy(flags), n_items)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy().view(np.uint32), want)
        ids = torch.from_numpy(np.flatnonzero(flags)[::-1].copy())         # ids in any order, one of them twice
        ids = torch.cat([ids, ids[:1]])
        assert np.array_equal(ops.pack_item_mask(ids, n_items).numpy().view(np.uint32), want)
    with pytest.raises(ValueError):
        ops.pack_item_mask(torch.tensor([n_items]), n_items)
    with pytest.raises(ValueError):
        ops.pack_item_mask(torch.ones(n_items + 1, dtype=torch.bool), n_items)


@pytest.mark.parametrize('cosine', [False, True])
def test_reference_agrees_with_the_ranking_reference_on_appended_rows(cosine):
    """An external row is the row of a query appended to the feature matrix: ``SearchCase.scores64`` is ``topk_reference.all_item_scores`` - the reference of
    ``ranking_reference`` - on that matrix, and the bound's magnitudes equal those of the appended ``RankCase``.  Both sides form the same float64 operands by the
    same elementwise steps and differ only in the order in which a matrix product of another shape adds a score's ``dim`` terms: each sum is within
    ``dim * 2^-53 * sum |m_c a_c|`` of the exact one, so the two are within twice that of each other."""
    for j, (n_pairs, n_items, dim, q_dim) in enumerate(((5, 70, 64, 32), (3, 33, 40, 8), (4, 20, 96, 96))):
        base = R.float_case('randn', n_pairs, n_items, dim, R.LAMS_FLOAT[1 + j % 2])
        ext = np.random.default_rng(j).standard_normal((n_pairs, q_dim)).astype(np.float32)
        case = S.SearchCase(base, ext=ext)
        app = S.appended_case(case)
        bias = torch.cat([app.bias, torch.zeros(n_pairs)])                 # (the appended rows read as items by all_item_scores: dropped again)
        want = tref.all_item_scores(app.features, app.users, app.queries, app.query_row0, app.item_row0, bias, app.lam, cosine)[:, :n_items]
        m, a = torch.from_numpy(case.mixed64()), app.features.double()[app.item_row0:app.item_row0 + n_items]
        if cosine:
            m, a = m / m.norm(dim=1, keepdim=True).clamp_min(tref.EPS), a / a.norm(dim=1, keepdim=True).clamp_min(tref.EPS)
        assert bool(((case.scores64(cosine) - want).abs() <= 2 * dim * 2.0 ** -53 * (m.abs() @ a.abs().t())).all())
        f = app.features.double().numpy()
        mm = app.lam * np.abs(f[app.queries.numpy() + app.query_row0]) + (1 - app.lam) * np.abs(f[app.users.numpy()])
        assert np.array_equal(case.magnitudes()[0], mm)


def test_reference_states_the_anonymous_pair_and_the_mask():
    base = R.float_case('randn', 6, 40, 48, 0.3)
    anon = np.array([True, False, True, False, False, True])
    mask = S.mask_pattern('every_other', 40)
    case = S.SearchCase(base, anon=anon, mask=mask)
    assert case.users.tolist() == [-1, 1, -1, 3, 4, -1]
    f = base.features.double()
    q, u, a = f[base.queries + base.query_row0], f[base.users], f[base.item_row0:]
    for cosine in (False, True):
        s = case.scores64(cosine)
        for c in range(6):
            m = q[c] if anon[c] else base.lam * q[c] + (1 - base.lam) * u[c]                     # PredictionLayers.py:25: `query_feature if user_feature is None`
            want = (torch.cosine_similarity(a, m[None, :], eps=1e-8) if cosine else a @ m) + base.bias.double()
            assert torch.allclose(s[c], want, rtol=1e-13, atol=1e-13)
    mm, t = case.magnitudes()
    assert np.array_equal(mm[anon], np.abs(q.numpy()[anon])) and np.array_equal(mm[~anon], base.magnitudes()[0][~anon])
    # the ranking under the mask: candidates only, the stable order, the -1 tail
    scores, items = S.expected(case, 30, False)
    assert bool((items[:, :20] % 2 == 0).all()) and bool((items[:, 20:] == -1).all()) and bool((scores[:, 20:] == -S.FLT_MAX).all())
    full_s, full_i = R.expected(S.SearchCase(base, anon=anon), 40, False)
    fs, fi = S.filtered_prefix(full_s, full_i, mask, 30)
    assert torch.equal(fi, items) and torch.equal(fs, scores)
    got = S.masked_float_verdict(scores, items, case, 30, False, 'self')
    assert 0 < got < 1                                                     # (float32 of the float64 scores: u |s64|, one term of the bound)
    wrong = items.clone()
    wrong[0, 0] = 1                                                        # an item outside the mask
    with pytest.raises(AssertionError):
        S.masked_float_verdict(scores, wrong, case, 30, False, 'self')
    assert S.SearchCase(base, mask=S.mask_pattern('none', 40)).target(10) == 0
    assert S.pack_mask(S.mask_pattern('last', 33), garbage=True).tolist() == [0, 0xFFFFFFFF]
