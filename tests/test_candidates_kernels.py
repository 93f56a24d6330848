"""``ihg_search_candidates`` (``csrc/candidates.hip``: ``cand_plan_kernel``, ``cand_units_kernel``, ``cand_score_kernel``, ``cand_select_kernel``) through the C ABI, on
the smallest shapes at which each of its mechanisms can go wrong, against ``tests/candidates_reference.py``:

    exact designs   items and scores EQUAL the stable ranking of what each search may rank (integer-valued operands, ``LAMS_EXACT``: every score is exact in plain
                    float32 sums of any order - ``test_candidates_host.py`` confirms it on the emulation for each design used, the three cosine designs included), and
                    EQUAL row c of ``ihg_search_topk_excluding`` called for search c alone with mask = what c may rank: both families are exact there
    float designs   ``candidates_reference.float_verdict`` (the derived bound, per-search ``allowed``), nothing left out
    all_scores      every slot within its bound of float64, ``-inf`` exactly on the gated entries, and the top-k the stable ranking of those very floats, bitwise
    composition     the same removed set as a mask, as exclusion runs and as both gives the same rows bitwise; an exclusion run equal to the candidate run: target 0,
                    ``passes`` 0
    degenerate      a null ``cand_row`` equals the identity ``cand_row``; shared runs equal their copies; ``total = 0``
    always          two launches over 0xFF and 0x3C workspace bytes are bit-equal, every output slot is written, ``passes[c] <= ceil(max(target_c, 1) / 10)``, the ``-1``
                    tail of search c begins at ``target_c``

70 searches (more than one wave of them), 300 items and 2,100 for the long runs, widths 1 .. 1,280 in geometries b (16-byte rows: the vector loads), c and d (the
scalar loads), run lengths 0, 1, 2, k - 1, k, k + 1, 63, 64, 65, CH - 1, CH, CH + 1, 2 CH + 1 and every item in turn.  The harness is ``test_search_kernels.py``'s."""
import numpy as np
import pytest
import torch

import candidates_reference as CR
import ranking_reference as R
import search_reference as S
from test_attention_kernels import Guarded, Source
from test_ranking_kernels import INT_FILL, GuardedInts, Workspace
from test_search_kernels import SearchOperands

pytestmark = pytest.mark.gpu

HEADS = [False, True]
WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst_ratios():
    yield
    for name in sorted(WORST):
        print(f'worst error / bound: {name}: {WORST[name]:.3f}')


class CandidateOperands(SearchOperands):
    """``SearchOperands`` with the candidate CSR and the exclusion CSR of a ``CandidateCase`` on the device."""

    def __init__(self, case, geometry='b', mask_words=None):
        super().__init__(case, geometry, mask_words)
        ptr, flat, self.total = case.cand_csr()
        self.cand_ptr, self.cand_items = Source(torch.from_numpy(ptr)), Source(torch.from_numpy(flat))
        self.cand_row = None if case.cand_row_of is None else Source(torch.from_numpy(case.cand_row_of))
        self.ptr = self.items = self.row = None
        if case.has_lists:
            eptr, eflat = case.csr()
            self.ptr, self.items = Source(torch.from_numpy(eptr)), Source(torch.from_numpy(eflat))
            self.row = None if case.row_of is None else Source(torch.from_numpy(case.row_of))

    def assert_unchanged(self, what):
        super().assert_unchanged(what)
        for src in (self.cand_ptr, self.cand_items, self.cand_row, self.ptr, self.items, self.row):
            if src is not None:
                src.assert_unchanged(what)


def _launch(x, k, cosine, fill, what, with_scores=False):
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    c = x.case
    n_bytes = int(lib.ihg_search_candidates_workspace_bytes(c.n_pairs, x.total, c.dim, k))
    assert n_bytes == CR.workspace_bytes(c.n_pairs, x.total)
    ws = Workspace(n_bytes, fill)
    scores, items, passes = Guarded(c.n_pairs * k), GuardedInts(c.n_pairs * k), GuardedInts(c.n_pairs)
    flat = Guarded(x.total) if with_scores else None
    by_row = x.ext is not None
    excl = (None, None, None, 0) if x.ptr is None else (ops._ptr(x.ptr.t), ops._ptr(x.items.t), None if x.row is None else ops._ptr(x.row.t), len(c.lists))
    rc = lib.ihg_search_candidates(ops._ptr(x.features.view), int(x.features.view.stride(0)), c.dim, c.query_row0, c.item_row0, c.n_items, ops._ptr(x.bias.t),
                                   ops._ptr(x.users.t), None if by_row else ops._ptr(x.queries.t), ops._ptr(x.ext.view) if by_row else None,
                                   int(x.ext.view.stride(0)) if by_row else 0, c.q_dim if by_row else 0, None if x.mask is None else ops._ptr(x.mask.t), *excl,
                                   ops._ptr(x.cand_ptr.t), ops._ptr(x.cand_items.t), None if x.cand_row is None else ops._ptr(x.cand_row.t), len(c.cand), x.total, c.lam,
                                   c.n_pairs, k, ops._ptr(scores.view), ops._ptr(items.view), ops._ptr(flat.arg) if with_scores else None, ops._ptr(ws.view), n_bytes,
                                   int(cosine), ops._ptr(passes.view), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.OK, f'{what}: returned {rc}: {_lib.last_error()}'
    for t in (scores, items, passes, ws) + ((flat,) if with_scores else ()):
        t.assert_guards(what)
    x.assert_unchanged(what)
    out = scores.view.view(c.n_pairs, k).clone(), items.view.view(c.n_pairs, k).clone(), passes.view.clone()
    return out + ((flat.view.clone(),) if with_scores else ())


def _same(a, b):
    return all(torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p, q.view(torch.int32) if q.dtype == torch.float32 else q) for p, q in zip(a[:3], b[:3]))


def _ranked(x, k, cosine, what, with_scores=False):
    """One call twice, over 0xFF and over 0x3C workspace bytes: the same bits, every slot written, and per search ``passes`` within its limit and the tail where it
    belongs."""
    first = _launch(x, k, cosine, 0xFF, what, with_scores)
    second = _launch(x, k, cosine, 0x3C, what + ' (second run)', with_scores)
    assert _same(first, second), f'{what}: two identical calls differ'
    scores, items, passes = (t.cpu() for t in first[:3])
    assert not bool(torch.isnan(scores).any()) and not bool((items == INT_FILL).any()) and not bool((passes == INT_FILL).any()), f'{what}: an output slot was not written'
    if with_scores:
        assert torch.equal(first[3].view(torch.int32), second[3].view(torch.int32)), f'{what}: all_scores of two identical calls differ'
        assert not bool(torch.isnan(first[3]).any()), f'{what}: a slot of all_scores was not written'
    for c, n in enumerate(x.case.targets(k).tolist()):
        limit = (max(n, 1) + CR.TOP - 1) // CR.TOP
        assert 0 <= int(passes[c]) <= limit and (n > 0 or int(passes[c]) == 0), f'{what}: search {c}: passes = {int(passes[c])} beyond ceil(max(target, 1) / 10) = {limit} (target {n})'
        assert bool((items[c, n:] == -1).all()) and bool((scores[c, n:] == -R.FLT_MAX).all()) and bool((items[c, :n] >= 0).all()), \
            f'{what}: search {c}: the -1 tail does not start at target = {n}: {items[c].tolist()}'
    return first


def _excluding_alone(x, k, cosine, what, pairs):
    """``ihg_search_topk_excluding`` (null lists) for every search of ``pairs`` ALONE under the mask of what it may rank."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    c = x.case
    n_bytes = int(lib.ihg_search_topk_excluding_workspace_bytes(1, c.n_items, c.dim, k))
    ws = Workspace(n_bytes, 0xFF)
    scores, items = Guarded(len(pairs) * k), GuardedInts(len(pairs) * k)
    by_row = x.ext is not None
    allowed = c.allowed()
    words = [Source(torch.from_numpy(S.pack_mask(allowed[p]).view(np.int32).copy())) for p in pairs]
    for j, p in enumerate(pairs):
        rc = lib.ihg_search_topk_excluding(ops._ptr(x.features.view), int(x.features.view.stride(0)), c.dim, c.query_row0, c.item_row0, c.n_items, ops._ptr(x.bias.t),
                                           ops._ptr(x.users.t[p:]), None if by_row else ops._ptr(x.queries.t[p:]), ops._ptr(x.ext.view[p:]) if by_row else None,
                                           int(x.ext.view.stride(0)) if by_row else 0, c.q_dim if by_row else 0, ops._ptr(words[j].t), None, None, None, 0, c.lam, 1, k,
                                           ops._ptr(scores.view[j * k:]), ops._ptr(items.view[j * k:]), ops._ptr(ws.view), n_bytes, int(cosine), None, ops._stream())
        assert rc == _lib.OK, f'{what}: search {p} alone: returned {rc}: {_lib.last_error()}'
    torch.cuda.synchronize()
    return scores.view.view(len(pairs), k).clone(), items.view.view(len(pairs), k).clone()


def _check(case, k, cosine, geometry='b', with_scores=False):
    """Every verdict on one case; returns the call's output."""
    what = f'{case.name} k={k} cosine={cosine} geometry {geometry}'
    x = CandidateOperands(case, geometry)
    got = _ranked(x, k, cosine, what, with_scores)
    if case.exact:
        R.ensure_exact(case, cosine)
        CR.assert_exact(got[0], got[1], case, k, cosine, what)
        pairs = list(range(0, case.n_pairs, 5))
        alone = _excluding_alone(x, k, cosine, what, pairs)
        differ = ((got[0][pairs].view(torch.int32) != alone[0].view(torch.int32)) | (got[1][pairs] != alone[1])).any(1).nonzero().flatten().tolist()
        assert not differ, f'{what}: searches {[pairs[j] for j in differ]} differ from ihg_search_topk_excluding for the search alone under its own mask'
    else:
        key = f'float designs, cosine={cosine}'
        WORST[key] = max(WORST.get(key, 0.0), CR.float_verdict(got[0], got[1], case, k, cosine, what))
    return got


@pytest.mark.parametrize('cosine', HEADS)
def test_float_designs_at_every_width(cosine):
    """``randn`` / ``worst`` / ``wide_range`` at widths 1 .. 1,280, every k, the ladder of run lengths in turn; plain, excluded, masked, external-row and anonymous
    searches; ``all_scores`` beside the ranking on every other case (its top-k is then the ranking of those very floats)."""
    for j, (case, k, geometry) in enumerate(CR.float_cases(cosine)):
        got = _check(case, k, cosine, geometry, with_scores=j % 2 == 0)
        if j % 2 == 0:
            what = f'{case.name} k={k} cosine={cosine} all_scores'
            key = f'all_scores, cosine={cosine}'
            WORST[key] = max(WORST.get(key, 0.0), CR.all_scores_verdict(got[3], case, cosine, what))
            want = CR.ranking_of_floats(got[3], case, k)
            assert torch.equal(got[0].cpu().view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1].cpu(), want[1]), \
                f'{what}: the top-k is not the stable ranking of the returned floats'
            plain = _ranked(CandidateOperands(case, geometry), k, cosine, what + ' (null all_scores)')
            assert _same(got, plain), f'{what}: the ranking with all_scores differs from the ranking without'


@pytest.mark.parametrize('cosine', HEADS)
def test_exact_designs_equal_the_reference_and_the_catalogue_kernels(cosine):
    for case, k, geometry in CR.exact_cases(cosine):
        assert case.exact
        _check(case, k, cosine, geometry)


@pytest.mark.parametrize('cosine', HEADS)
def test_one_long_run_beside_empty_ones(cosine):
    """2,100 ids of one search: nine scoring units, thirteen trips of one selecting wave; 69 searches with nothing to rank."""
    case, k, geometry = CR.one_long_run_case(cosine)
    got = _check(case, k, cosine, geometry)
    assert got[2].tolist() == [13 if c == 33 else 0 for c in range(case.n_pairs)]


@pytest.mark.parametrize('cosine', HEADS)
def test_shared_runs_through_cand_row(cosine):
    """Several searches of different users on one run, ``-1`` and an out-of-range row, a run nobody names: the verdict, bit-equality with the call that gives every
    search its own copy of its run, and ``all_scores`` holding the lowest-numbered search's scores (``-inf`` on the run nobody names)."""
    case, k, geometry = CR.shared_runs_case(cosine)
    got = _check(case, k, cosine, geometry, with_scores=True)
    what = f'{case.name} k={k} cosine={cosine}'
    CR.all_scores_verdict(got[3], case, cosine, what)
    own = _ranked(CandidateOperands(CR.copied(case), geometry), k, cosine, what + ' (copies)')
    assert _same(got, own), f'{what}: a shared run and its copies differ'
    plain = _ranked(CandidateOperands(case, geometry), k, cosine, what + ' (null all_scores)')
    assert _same(got, plain), f'{what}: the ranking with all_scores differs from the ranking without'


@pytest.mark.parametrize('cosine', HEADS)
def test_null_cand_row_equals_the_identity(cosine):
    case, k, geometry = CR.float_cases(cosine)[3]
    what = f'{case.name} k={k} cosine={cosine}'
    got = _ranked(CandidateOperands(case, geometry), k, cosine, what)
    same = CR.CandidateCase(case.base, case.cand, cand_rows=np.arange(case.n_pairs), lists=case.lists if case.has_lists else None, anon=case.anon, mask=case.mask,
                            ext=None if case.ext is None else case.ext.numpy())
    assert _same(got, _ranked(CandidateOperands(same, geometry), k, cosine, what + ' (identity cand_row)')), f'{what}: the identity cand_row differs from a null one'


@pytest.mark.parametrize('cosine', HEADS)
def test_mask_exclusion_and_both_remove_the_same(cosine):
    """One removed set X stated three ways - the mask ``~X``, every search excluding X (one shared run), half of X each way - returns the same rows bitwise; and an
    exclusion run equal to the candidate run leaves target 0 and ``passes`` 0."""
    n_items, k = 300, 11
    base = R.float_case('randn', CR.N_PAIRS, n_items, 30, 0.3, seed=3)
    runs = CR.runs_by_length(CR.N_PAIRS, n_items, k, seed=3)
    removed = np.random.default_rng(5).random(n_items) < 0.4
    removed[[0, n_items - 1]] = True
    x_ids = np.flatnonzero(removed)
    shared = np.zeros(CR.N_PAIRS, np.int64)
    by_mask = CR.CandidateCase(base, runs, mask=~removed)
    by_list = CR.CandidateCase(base, runs, lists=[x_ids], rows=shared)
    half = removed & (np.arange(n_items) % 2 == 0)
    by_both = CR.CandidateCase(base, runs, lists=[np.flatnonzero(removed & ~half)], rows=shared, mask=~half)
    assert np.array_equal(by_mask.allowed(), by_list.allowed()) and np.array_equal(by_mask.allowed(), by_both.allowed())
    what = f'{base.name} k={k} cosine={cosine}'
    got = _check(by_mask, k, cosine, 'b')
    assert _same(got, _check(by_list, k, cosine, 'b')), f'{what}: exclusion runs differ from the mask that removes the same items'
    assert _same(got, _check(by_both, k, cosine, 'b')), f'{what}: mask and exclusion together differ from the mask alone'
    nothing = CR.CandidateCase(base, runs, lists=runs)
    assert not nothing.targets(k).any()
    got = _check(nothing, k, cosine, 'c')
    assert not got[2].any() and bool((got[1] == -1).all())


def test_no_candidates_at_all():
    """``total = 0``: every run empty - every row the ``-1`` tail, ``passes`` 0, an empty ``all_scores``."""
    base = R.float_case('randn', CR.N_PAIRS, 300, 64, 0.3)
    case = CR.CandidateCase(base, [[] for _ in range(CR.N_PAIRS)])
    got = _check(case, 10, False, 'b', with_scores=True)
    assert bool((got[1] == -1).all()) and not got[2].any() and got[3].numel() == 0
