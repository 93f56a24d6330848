"""``ihg_search_topk`` (``csrc/eval.hip``: ``search_target_kernel``, ``score_prepare_kernel<COSINE, true>``, ``score_topk_kernel<PB, COSINE, true, true>``,
``merge_deep_kernel<true>``) through the C ABI, each of its three additions over ``ihg_score_topk_deep`` held against that entry point BITWISE wherever the two must
agree, and against the float64 reference of ``tests/search_reference.py`` everywhere else:

    external rows   equal ``ihg_score_topk_deep`` on the feature matrix with the rows appended (zero above ``q_dim``): items, scores and ``passes``.  The rows sit in a
                    sentinel-filled buffer with a row stride beyond ``q_dim``: a read past ``q_dim`` would show
    no user         an all-anonymous call equals the ``lambda = 1`` call under the dot product (``1 q + 0 u = q``); in a mixed call every pair equals ITS call - the
                    ``lambda = 1`` one or the plain one; cosine: the float verdict; exact designs: EQUAL to the stable ranking and float32(float64 scores)
    mask            ``all`` equals the call without a mask; for I <= 128 a masked call equals the unmasked k = 128 ranking with the non-candidates removed, cut at k,
                    then the ``-1`` tail; for larger I the float verdict under the mask; ``passes[c] <= ceil(min(k, candidates) / 10)`` always

As in ``test_ranking_kernels.py``: ``features`` is a column slice of a wider sentinel-filled matrix, the outputs are views into guarded buffers pre-filled so that an
unwritten slot shows, the workspace is exactly as long as the library asks with a guard behind it, and EVERY call runs twice - over a workspace of all-ones bytes (NaN
planes and ``aux``) and over one whose bytes read as finite values - and must come back bitwise equal: the planes of a masked item are never written, and whatever
they hold must not reach a result.  Every source is compared with its copy after the launch."""
import numpy as np
import pytest
import torch

import ranking_reference as R
import search_reference as S
from test_aggregate_kernels import Padded
from test_attention_kernels import Guarded, Source
from test_gpu_parity import dev
from test_ranking_kernels import INT_FILL, GuardedInts, Operands, Workspace, _launch as _deep_launch

pytestmark = pytest.mark.gpu

HEADS = [False, True]
PAIRS = (1, 32, 33, 64, 65)
ITEMS = (1, 9, 10, 11, 31, 32, 33, 100, 128, 129, 300, 4100)
WIDTHS = ((64, 32), (40, 8), (96, 96), (384, 128), (1264, 316))
KS = (1, 10, 11, 50, 128)
WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst_ratios():
    yield
    for name in sorted(WORST):
        print(f'worst error / bound: {name}: {WORST[name]:.3f}')


class SearchOperands:
    """The sources of a ``SearchCase`` on the device; ``mask_words``: the uint32 words to pass (default: the case's mask packed, no mask: a null pointer)."""

    def __init__(self, case, geometry='b', mask_words=None):
        self.case = case
        self.features = Padded(case.features, geometry)
        self.users, self.queries, self.bias = Source(case.users), Source(case.queries), Source(case.bias)
        self.ext = None if case.ext is None else Padded(case.ext, geometry)
        if mask_words is None and case.mask is not None:
            mask_words = S.pack_mask(case.mask)
        self.mask = None if mask_words is None else Source(torch.from_numpy(mask_words.view(np.int32).copy()))
        assert case.ext is None or int(self.ext.view.stride(0)) > case.q_dim

    def with_mask(self, case, mask_words=None):
        """The same device sources under another mask (``case``: this case with that mask)."""
        other = object.__new__(SearchOperands)
        other.__dict__.update(self.__dict__)
        other.case = case
        words = S.pack_mask(case.mask) if mask_words is None and case.mask is not None else mask_words
        other.mask = None if words is None else Source(torch.from_numpy(words.view(np.int32).copy()))
        return other

    def assert_unchanged(self, what):
        for src in (self.features, self.users, self.queries, self.bias, self.ext, self.mask):
            if src is not None:
                src.assert_unchanged(what)


def _launch(x, k, cosine, fill, what):
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    c = x.case
    n_bytes = int(lib.ihg_search_topk_workspace_bytes(c.n_pairs, c.n_items, c.dim, k))
    assert n_bytes == R.deep_workspace_bytes(c.n_pairs, c.n_items, c.dim) + 16
    ws = Workspace(n_bytes, fill)
    scores, items, passes = Guarded(c.n_pairs * k), GuardedInts(c.n_pairs * k), GuardedInts(c.n_pairs)
    by_row = x.ext is not None
    rc = lib.ihg_search_topk(ops._ptr(x.features.view), int(x.features.view.stride(0)), c.dim, c.query_row0, c.item_row0, c.n_items, ops._ptr(x.bias.t), ops._ptr(x.users.t),
                             None if by_row else ops._ptr(x.queries.t), ops._ptr(x.ext.view) if by_row else None, int(x.ext.view.stride(0)) if by_row else 0,
                             c.q_dim if by_row else 0, None if x.mask is None else ops._ptr(x.mask.t), c.lam, c.n_pairs, k, ops._ptr(scores.view), ops._ptr(items.view),
                             ops._ptr(ws.view), n_bytes, int(cosine), ops._ptr(passes.view), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.OK, f'{what}: returned {rc}: {_lib.last_error()}'
    for t in (scores, items, passes, ws):
        t.assert_guards(what)
    x.assert_unchanged(what)
    return scores.view.view(c.n_pairs, k).clone(), items.view.view(c.n_pairs, k).clone(), passes.view.clone()


def _search(x, k, cosine, what):
    """One call twice, over NaN and over finite workspace bytes: the same bits (verdict 5), every slot written, ``passes`` within its limit."""
    first = _launch(x, k, cosine, 0xFF, what)
    second = _launch(x, k, cosine, 0x3C, what + ' (second run)')
    assert _same(first, second), f'{what}: two identical calls differ'
    scores, items, passes = first
    assert not bool(torch.isnan(scores).any()) and not bool((items == INT_FILL).any()), f'{what}: an output slot was not written'
    limit = (x.case.target(k) + R.TOP - 1) // R.TOP
    assert bool(((passes >= 0) & (passes <= limit)).all()), f'{what}: passes {passes.tolist()} beyond ceil(min(k, candidates) / 10) = {limit}'
    n = x.case.target(k)
    assert bool((items[:, n:] == -1).all()) and bool((scores[:, n:] == -R.FLT_MAX).all()) and bool((items[:, :n] >= 0).all()), f'{what}: the -1 tail does not start at min(k, candidates)'
    if x.case.mask is not None and n:
        assert bool(torch.from_numpy(x.case.mask).to(items.device)[items[:, :n].long()].all()), f'{what}: an item outside the mask is returned'
    return first


def _deep(case, k, cosine, what, geometry='b'):
    """``ihg_score_topk_deep`` on a plain ``RankCase`` (the harness of ``test_ranking_kernels.py``)."""
    return _deep_launch(Operands(case, geometry), k, cosine, True, 0xFF, what + ' (ihg_score_topk_deep)')


def _same(a, b, rows=None):
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    return (torch.equal(pick(a[0]).view(torch.int32), pick(b[0]).view(torch.int32)) and torch.equal(pick(a[1]), pick(b[1])) and torch.equal(pick(a[2]), pick(b[2])))


def _with_lam(case, lam):
    out = object.__new__(R.RankCase)
    out.__dict__.update(case.__dict__)
    out.lam, out._scores = float(np.float32(lam)), {}
    return out


def _ext_rows(n_pairs, q_dim, seed):
    """External rows; the last of several is zero (an empty bag)."""
    ext = np.random.default_rng([seed, n_pairs, q_dim]).standard_normal((n_pairs, q_dim)).astype(np.float32)
    if n_pairs > 1:
        ext[-1] = 0
    return ext


def _verdict(got, case, k, cosine, what, key):
    WORST[key] = max(WORST.get(key, 0.0), S.masked_float_verdict(got[0], got[1], case, k, cosine, what))


GRID = [(p, i) for p in PAIRS for i in ITEMS]                             # every (pairs, I) edge at the small width
LADDER = [(1, 100, 40, 8), (33, 300, 40, 8), (65, 129, 96, 96), (32, 4100, 96, 96), (33, 300, 384, 128), (64, 4100, 384, 128), (1, 128, 1264, 316), (33, 129, 1264, 316),
          (65, 300, 1264, 316)]


@pytest.mark.parametrize('cosine', HEADS)
def test_external_rows_equal_the_appended_rows(cosine):
    """Verdict 1 on all 60 (pairs, I) edges at (dim, q_dim) = (64, 32) and on the width ladder: bitwise ``ihg_score_topk_deep`` of the appended matrix, ``passes``
    included; the width ladder also meets the float verdict."""
    shapes = [(p, i, 64, 32) for p, i in GRID] + LADDER
    for j, (n_pairs, n_items, dim, q_dim) in enumerate(shapes):
        base = R.float_case('randn', n_pairs, n_items, dim, R.LAMS_FLOAT[1 + j % 2] if j % 5 else 0.5)
        case = S.SearchCase(base, ext=_ext_rows(n_pairs, q_dim, j))
        k = KS[j % 5]
        what = f'{case.name} k={k} cosine={cosine}'
        geometry = 'bc'[j % 2]
        got = _search(SearchOperands(case, geometry), k, cosine, what)
        want = _deep(S.appended_case(case), k, cosine, what, geometry)
        assert _same(got, want), f'{what}: differs from ihg_score_topk_deep on the appended rows'
        if dim != 64:
            _verdict(got, case, k, cosine, what, f'external rows, cosine={cosine}')


def _anon_positions(n_pairs):
    anon = np.zeros(n_pairs, bool)
    anon[[p for p in (0, 31, 32, n_pairs - 1) if p < n_pairs]] = True
    return anon


@pytest.mark.parametrize('cosine', HEADS)
def test_anonymous_pairs(cosine):
    """Verdict 2: all pairs anonymous, and anonymous pairs at positions 0, 31, 32 and the last of a mixed call, by ``queries`` and by external rows."""
    shapes = [(p, i, 64, 32) for p, i in ((1, 100), (32, 33), (33, 300), (64, 129), (65, 4100), (33, 9), (65, 10))] + [(33, 100, 40, 8), (65, 300, 384, 128), (33, 129, 1264, 316)]
    for j, (n_pairs, n_items, dim, q_dim) in enumerate(shapes):
        base = R.float_case('randn', n_pairs, n_items, dim, 0.3)
        k = KS[(j + 1) % 5]
        for anon in (np.ones(n_pairs, bool), _anon_positions(n_pairs)):
            ext = _ext_rows(n_pairs, q_dim, j) if j % 2 else None
            case = S.SearchCase(base, ext=ext, anon=anon)
            what = f'{case.name} k={k} cosine={cosine}'
            got = _search(SearchOperands(case, 'bc'[j % 2]), k, cosine, what)
            _verdict(got, case, k, cosine, what, f'anonymous, cosine={cosine}')
            plain = S.appended_case(case) if ext is not None else base
            with_user = _deep(plain, k, cosine, what)
            assert _same(got, with_user, np.flatnonzero(~anon)), f'{what}: a pair WITH a user differs from ihg_score_topk_deep'
            if not cosine:
                query_only = _deep(_with_lam(plain, 1.0), k, cosine, what + ' lambda=1')
                assert _same(got, query_only, np.flatnonzero(anon)), f'{what}: an anonymous pair differs from the lambda = 1 call'


@pytest.mark.parametrize('design', ['random', 'mixed_bits', 'row_scales', 'all_equal', 'tied_across', 'one_list_dec'])
def test_anonymous_exact_designs(design):
    """Exact designs (integer operands, power-of-two row scales): EQUAL items and scores for pairs without a user, under the dot product."""
    for j, (n_pairs, n_items) in enumerate(((5, 70), (33, 300), (65, 4100))):
        base = R.exact_case(design, n_pairs, n_items, 64, False, R.LAMS_EXACT[j % 2])
        case = S.SearchCase(base, anon=_anon_positions(n_pairs) if j else np.ones(n_pairs, bool))
        R.ensure_exact(case, False)
        k = KS[(j + 2) % 5]
        what = f'{case.name} k={k}'
        got = _search(SearchOperands(case, 'bc'[j % 2]), k, False, what)
        S.assert_exact(got[0], got[1], case, k, False, what)


def _garbage_words(mask):
    return S.pack_mask(mask, garbage=True)


@pytest.mark.parametrize('cosine', HEADS)
def test_mask_patterns_up_to_128_items(cosine):
    """Verdict 3 for I <= 128: every pattern against the unmasked k = 128 ranking of the same call (it ranks every item) with the non-candidates removed."""
    for j, n_items in enumerate([i for i in ITEMS if i <= 128]):
        n_pairs = PAIRS[j % 5]
        base = R.float_case('randn', n_pairs, n_items, 64, 0.3)
        ext = _ext_rows(n_pairs, 32, j) if j % 2 else None
        anon = _anon_positions(n_pairs) if j % 3 == 0 else None
        free = S.SearchCase(base, ext=ext, anon=anon)
        x = SearchOperands(free, 'bc'[j % 2])
        full = _search(x, 128, cosine, f'{free.name} k=128 cosine={cosine}')
        for p, pattern in enumerate(S.MASK_PATTERNS):
            k = KS[(j + p) % 5]
            mask = S.mask_pattern(pattern, n_items, seed=j)
            case = S.SearchCase(base, ext=ext, anon=anon, mask=mask)
            what = f'{case.name} {pattern} k={k} cosine={cosine}'
            got = _search(x.with_mask(case), k, cosine, what)
            want_s, want_i = S.filtered_prefix(full[0], full[1], mask, k)
            assert torch.equal(got[1].cpu(), want_i) and torch.equal(got[0].cpu().view(torch.int32), want_s.view(torch.int32)), f'{what}: not the filtered unmasked ranking'
            if pattern == 'all':
                assert _same(got, _search(x, k, cosine, what + ' (no mask)')), f'{what}: an all-ones mask differs from no mask'
            if pattern == 'none':
                assert bool((got[2] == 0).all()) and bool((got[1] == -1).all())
            if n_items % 32 and pattern in ('last', 'random10', 'none'):
                again = _search(x.with_mask(case, _garbage_words(mask)), k, cosine, what + ' (garbage past n_items)')
                assert _same(got, again), f'{what}: bits at or past n_items reach the result'


@pytest.mark.parametrize('cosine', HEADS)
def test_mask_patterns_beyond_128_items(cosine):
    """Verdict 3 for I = 129, 300 and 4,100 (more than one item slice, more than one trip of the 256 threads over the mask's 129 words): the float verdict under the
    mask, no masked item in any output, ``all`` bitwise the call without a mask, garbage past ``n_items`` ignored."""
    for j, (n_pairs, n_items, dim, q_dim) in enumerate(((33, 129, 64, 32), (65, 300, 64, 32), (32, 4100, 64, 32), (5, 4100, 384, 128), (64, 300, 40, 8))):
        base = R.float_case('randn', n_pairs, n_items, dim, 0.3)
        ext = _ext_rows(n_pairs, q_dim, j) if j % 2 else None
        anon = _anon_positions(n_pairs) if j % 2 == 0 else None
        x = SearchOperands(S.SearchCase(base, ext=ext, anon=anon), 'bc'[j % 2])
        for p, pattern in enumerate(S.MASK_PATTERNS):
            k = KS[(j + p) % 5]
            mask = S.mask_pattern(pattern, n_items, seed=j)
            case = S.SearchCase(base, ext=ext, anon=anon, mask=mask)
            what = f'{case.name} {pattern} k={k} cosine={cosine}'
            got = _search(x.with_mask(case), k, cosine, what)
            _verdict(got, case, k, cosine, what, f'mask, cosine={cosine}')
            if pattern == 'all':
                assert _same(got, _search(x, k, cosine, what + ' (no mask)')), f'{what}: an all-ones mask differs from no mask'
            if n_items % 32 and pattern in ('first', 'random10', 'all'):
                again = _search(x.with_mask(case, _garbage_words(mask)), k, cosine, what + ' (garbage past n_items)')
                assert _same(got, again), f'{what}: bits at or past n_items reach the result'


@pytest.mark.parametrize('cosine', HEADS)
def test_zero_mixed_row_scores_the_bias(cosine):
    """Verdict 4: an anonymous pair with a zero external row (an empty bag and nobody logged in) has a zero mixed row - every score is the item's bias, under the
    cosine head too (the clamped norm divides a zero dot product) - and the ranking is the stable ranking of the bias; its neighbours are not disturbed."""
    for n_pairs, n_items, k in ((1, 100, 50), (33, 300, 11), (65, 33, 128)):
        base = R.float_case('randn', n_pairs, n_items, 64, 0.3)
        ext = _ext_rows(n_pairs, 32, 7)
        ext[0] = 0
        anon = np.zeros(n_pairs, bool)
        anon[[0, n_pairs - 1]] = True
        case = S.SearchCase(base, ext=ext, anon=anon)
        what = f'{case.name} k={k} cosine={cosine}'
        got = _search(SearchOperands(case), k, cosine, what)
        _verdict(got, case, k, cosine, what, f'zero rows, cosine={cosine}')
        n = min(k, n_items)
        order = torch.sort(base.bias, descending=True, stable=True).indices[:n]
        for c in {0, n_pairs - 1}:
            assert torch.equal(got[1][c, :n].cpu().long(), order) and torch.equal(got[0][c, :n].cpu(), base.bias[order]), f'{what}: pair {c} does not score the bias'


@pytest.mark.parametrize('design', ['all_equal', 'tied_across', 'tie_at_boundary'])
def test_ties_across_a_mask_boundary_ascend_by_item_id(design):
    """Verdict 4: bit-equal scores on both sides of masked items, of word boundaries and of deep-pass boundaries come back in ascending item id (exact designs)."""
    for j, (n_pairs, n_items) in enumerate(((5, 100), (33, 300), (5, 2016))):
        base = R.exact_case(design, n_pairs, n_items, 64, False, 0.5)
        for pattern in ('every_other', 'random10', 'last_partial_word'):
            case = S.SearchCase(base, mask=S.mask_pattern(pattern, n_items, seed=j))
            R.ensure_exact(case, False)
            k = KS[(j + 3) % 5] if pattern != 'every_other' else 128
            what = f'{case.name} {pattern} k={k}'
            got = _search(SearchOperands(case, 'bc'[j % 2]), k, False, what)
            S.assert_exact(got[0], got[1], case, k, False, what)
