"""``ihg_search_topk_excluding`` (``csrc/eval.hip``: ``exclude_target_kernel``, ``score_topk_kernel<PB, COSINE, true, true, true>``, ``merge_deep_kernel<true, true>``)
through the C ABI, on the smallest shapes at which each of its mechanisms can go wrong, against ``tests/exclude_reference.py``:

    exact designs   items and scores EQUAL the stable ranking of what each pair may rank (integer-valued operands: every score is exact in the kernels' arithmetic)
    float designs   the per-pair float verdict (``ranking_reference.score_bound`` unchanged: exclusion changes no score)
    bitwise         row c equals ``ihg_search_topk`` called for pair c ALONE under the mask ``candidates & ~run of c`` - the scores that remain are that entry's bits
    empty lists     with every run empty, and with a null ``excl_ptr``, the whole output equals ``ihg_search_topk``'s, ``passes`` included
    always          two launches (over NaN and over finite workspace bytes) are bit-equal, every output slot is written, ``passes[c] <= ceil(max(target_c, 1) / 10)``,
                    the ``-1`` tail of pair c begins at ``target_c`` and no item of its run is returned

Where an excluded id can sit: a lane meets the ids ``8 r4 + 4 half + x`` of a 32-item tile, so 0, 3, 4, 7, 8 are the edges of the lane halves' groups of four, 31, 32, 33
the tile edge; the first and last id of every wave's run of tiles (at 2,100 items ``eval_slices`` gives two item slices of eight runs of about four tiles) is where a
cursor is positioned or spent; ``n_items - 1`` sits in a partial last tile.  The harness is ``tests/test_search_kernels.py``'s: a column slice of a sentinel-filled
feature matrix, guarded NaN-prefilled outputs, a workspace of exactly the size the library asks with guards behind it, every source compared with its copy."""
import numpy as np
import pytest
import torch

import exclude_reference as E
import ranking_reference as R
import search_reference as S
from test_attention_kernels import Guarded, Source
from test_ranking_kernels import INT_FILL, GuardedInts, Workspace
from test_search_kernels import SearchOperands, _ext_rows, _launch as _search_launch, _same

pytestmark = pytest.mark.gpu

HEADS = [False, True]
KS = (1, 10, 11, 128)
WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst_ratios():
    yield
    for name in sorted(WORST):
        print(f'worst error / bound: {name}: {WORST[name]:.3f}')


def positions(n_pairs, n_items, dim):
    """The ids where a cursor can go wrong (module docstring), ascending and distinct."""
    edges = [i for b, e in R.tile_ranges(n_pairs, n_items, dim) if e > b for i in (32 * b, 32 * e - 1)]
    return sorted({i for i in [0, 3, 4, 7, 8, 31, 32, 33, n_items - 1] + edges if 0 <= i < n_items})


KINDS = ('empty', 'one', 'across_tile_edge', 'all_but_one', 'all', 'top_k', 'top_1', 'more_than_k', 'positions', 'random')


def lists_by_kind(free, k, cosine, kinds=KINDS, seed=0):
    """One run per pair, the kinds in turn - so one 32-pair tile holds runs from empty to every item.  ``free``: the case without lists (its float64 ranking names the
    top-k and the top-1 that a run removes exactly)."""
    n, pos = free.n_items, positions(free.n_pairs, free.n_items, free.dim)
    cand = free.candidates()
    order = torch.sort(free.scores64(cosine)[:, torch.from_numpy(cand)], dim=1, descending=True, stable=True).indices.numpy()
    rng = np.random.default_rng([seed, free.n_pairs, n, k])
    runs = []
    for c in range(free.n_pairs):
        kind = kinds[c % len(kinds)]
        turn = c // len(kinds)
        if kind == 'empty':
            run = []
        elif kind == 'one':
            run = [pos[turn % len(pos)]]
        elif kind == 'across_tile_edge':                                   # consecutive ids over the edge between two tiles (the last one where there are several)
            edge = max(32, (n - 1) // 32 * 32)
            run = [i for i in range(edge - 5, edge + 6) if 0 <= i < n]
        elif kind == 'all_but_one':
            run = [i for i in range(n) if i != pos[-1 - turn % len(pos)]]
        elif kind == 'all':
            run = list(range(n))
        elif kind == 'top_k':
            run = cand[order[c, :k]].tolist()
        elif kind == 'top_1':
            run = cand[order[c, :1]].tolist()
        elif kind == 'more_than_k':
            run = rng.choice(n, size=min(n, k + 5), replace=False).tolist()
        elif kind == 'positions':
            run = pos
        else:
            run = np.flatnonzero(rng.random(n) < 0.3).tolist()
        runs.append(run)
    return runs


class ExcludeOperands(SearchOperands):
    """``SearchOperands`` with the lists of an ``ExcludeCase`` on the device."""

    def __init__(self, case, geometry='b', mask_words=None):
        super().__init__(case, geometry, mask_words)
        ptr, flat = case.csr()
        self.ptr, self.items = Source(torch.from_numpy(ptr)), Source(torch.from_numpy(flat))
        self.row = None if case.row_of is None else Source(torch.from_numpy(case.row_of))

    def assert_unchanged(self, what):
        super().assert_unchanged(what)
        for src in (self.ptr, self.items, self.row):
            if src is not None:
                src.assert_unchanged(what)


def _launch(x, k, cosine, fill, what, lists=True):
    """One call of the entry point; ``lists=False``: a null ``excl_ptr`` (then ``excl_items`` and ``excl_row`` are null too)."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    c = x.case
    n_bytes = int(lib.ihg_search_topk_excluding_workspace_bytes(c.n_pairs, c.n_items, c.dim, k))
    assert n_bytes == R.deep_workspace_bytes(c.n_pairs, c.n_items, c.dim) + 16 + (4 * c.n_pairs + 15) // 16 * 16
    ws = Workspace(n_bytes, fill)
    scores, items, passes = Guarded(c.n_pairs * k), GuardedInts(c.n_pairs * k), GuardedInts(c.n_pairs)
    by_row = x.ext is not None
    excl = (ops._ptr(x.ptr.t), ops._ptr(x.items.t), None if x.row is None else ops._ptr(x.row.t), len(c.lists)) if lists else (None, None, None, 0)
    rc = lib.ihg_search_topk_excluding(ops._ptr(x.features.view), int(x.features.view.stride(0)), c.dim, c.query_row0, c.item_row0, c.n_items, ops._ptr(x.bias.t),
                                       ops._ptr(x.users.t), None if by_row else ops._ptr(x.queries.t), ops._ptr(x.ext.view) if by_row else None,
                                       int(x.ext.view.stride(0)) if by_row else 0, c.q_dim if by_row else 0, None if x.mask is None else ops._ptr(x.mask.t), *excl, c.lam,
                                       c.n_pairs, k, ops._ptr(scores.view), ops._ptr(items.view), ops._ptr(ws.view), n_bytes, int(cosine), ops._ptr(passes.view), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.OK, f'{what}: returned {rc}: {_lib.last_error()}'
    for t in (scores, items, passes, ws):
        t.assert_guards(what)
    x.assert_unchanged(what)
    return scores.view.view(c.n_pairs, k).clone(), items.view.view(c.n_pairs, k).clone(), passes.view.clone()


def _excluding(x, k, cosine, what):
    """One call twice, over NaN and over finite workspace bytes: the same bits, every slot written, and per pair: ``passes`` within its limit, the tail where it
    belongs, nothing of the pair's run in its row."""
    first = _launch(x, k, cosine, 0xFF, what)
    second = _launch(x, k, cosine, 0x3C, what + ' (second run)')
    assert _same(first, second), f'{what}: two identical calls differ'
    scores, items, passes = (t.cpu() for t in first)
    assert not bool(torch.isnan(scores).any()) and not bool((items == INT_FILL).any()) and not bool((passes == INT_FILL).any()), f'{what}: an output slot was not written'
    targets = x.case.targets(k)
    for c, n in enumerate(targets.tolist()):
        limit = (max(n, 1) + R.TOP - 1) // R.TOP
        assert 0 <= int(passes[c]) <= limit and (n > 0 or int(passes[c]) == 0), f'{what}: pair {c}: passes = {int(passes[c])} beyond ceil(max(target, 1) / 10) = {limit} (target {n})'
        assert bool((items[c, n:] == -1).all()) and bool((scores[c, n:] == -R.FLT_MAX).all()) and bool((items[c, :n] >= 0).all()), \
            f'{what}: pair {c}: the -1 tail does not start at target = {n}: {items[c].tolist()}'
        assert not np.isin(items[c, :n].numpy(), x.case.run_of(c)).any(), f'{what}: pair {c}: an excluded item is returned'
    return first


def _single_pair_rows(x, k, cosine, what, pairs=None):
    """``ihg_search_topk`` for every pair ALONE (the sources of the whole call where they lie, from the pair's entry on) under the mask of that pair."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    c = x.case
    n_bytes = int(lib.ihg_search_topk_workspace_bytes(1, c.n_items, c.dim, k))
    ws = Workspace(n_bytes, 0xFF)
    pairs = range(c.n_pairs) if pairs is None else pairs
    scores, items = Guarded(len(pairs) * k), GuardedInts(len(pairs) * k)
    by_row = x.ext is not None
    allowed = c.allowed()
    words = [Source(torch.from_numpy(S.pack_mask(allowed[p]).view(np.int32).copy())) for p in pairs]
    for j, p in enumerate(pairs):
        rc = lib.ihg_search_topk(ops._ptr(x.features.view), int(x.features.view.stride(0)), c.dim, c.query_row0, c.item_row0, c.n_items, ops._ptr(x.bias.t),
                                 ops._ptr(x.users.t[p:]), None if by_row else ops._ptr(x.queries.t[p:]), ops._ptr(x.ext.view[p:]) if by_row else None,
                                 int(x.ext.view.stride(0)) if by_row else 0, c.q_dim if by_row else 0, ops._ptr(words[j].t), c.lam, 1, k, ops._ptr(scores.view[j * k:]),
                                 ops._ptr(items.view[j * k:]), ops._ptr(ws.view), n_bytes, int(cosine), None, ops._stream())
        assert rc == _lib.OK, f'{what}: pair {p} alone: returned {rc}: {_lib.last_error()}'
    torch.cuda.synchronize()
    for t in (scores, items, ws):
        t.assert_guards(what)
    return scores.view.view(len(pairs), k).clone(), items.view.view(len(pairs), k).clone()


def _check(case, k, cosine, geometry='b', key=None, mask_words=None, pairs=None):
    """Every verdict of the module docstring on one case; returns the call's output."""
    what = f'{case.name} k={k} cosine={cosine}'
    x = ExcludeOperands(case, geometry, mask_words)
    got = _excluding(x, k, cosine, what)
    if case.exact:
        R.ensure_exact(case, cosine)
        E.assert_exact(got[0], got[1], case, k, cosine, what)
    else:
        key = key or f'float designs, cosine={cosine}'
        WORST[key] = max(WORST.get(key, 0.0), E.float_verdict(got[0], got[1], case, k, cosine, what))
    alone = _single_pair_rows(x, k, cosine, what, pairs)
    rows = slice(None) if pairs is None else list(pairs)
    differ = ((got[0][rows].view(torch.int32) != alone[0].view(torch.int32)) | (got[1][rows] != alone[1])).any(1).nonzero().flatten().tolist()
    assert not differ, f'{what}: rows {differ} differ from ihg_search_topk for the pair alone under its own mask'
    return got


# (pairs, items): every pair count (the PB = 2 block edge at 64 / 65, the repeated last pair) and every item count of the issue; k cycles with the shape
SHAPES = ((1, 1), (31, 31), (32, 33), (33, 2100), (64, 33), (65, 2100), (1, 2100), (33, 31), (65, 1), (64, 31))


@pytest.mark.parametrize('cosine', HEADS)
def test_every_kind_of_list_in_one_tile_of_pairs(cosine):
    """Float designs at width 32 (``PB = 2``): in every shape the pairs' runs go through all kinds in turn - lengths from 0 to ``n_items`` side by side in one 32-pair
    tile - and the single-id and all-but-one runs walk through ``positions``."""
    for j, (n_pairs, n_items) in enumerate(SHAPES):
        base = R.float_case('randn', n_pairs, n_items, 32, R.LAMS_FLOAT[1 + j % 2] if j % 3 else 0.5)
        k = KS[j % 4]
        runs = lists_by_kind(S.SearchCase(base), k, cosine, KINDS[j % len(KINDS):] + KINDS[:j % len(KINDS)], seed=j)
        _check(E.ExcludeCase(base, runs), k, cosine, 'bc'[j % 2])


@pytest.mark.parametrize('cosine', HEADS)
@pytest.mark.parametrize('k', KS)
def test_every_depth_at_two_item_slices(k, cosine):
    """2,100 items (two item slices, runs of about four tiles), 33 pairs, every ``k``: the runs that remove exactly the top-k, the top-1 and more than ``k`` ids move
    every pass boundary of the deep merge."""
    base = R.float_case('randn', 33, 2100, 32, 0.3, seed=k)
    _check(E.ExcludeCase(base, lists_by_kind(S.SearchCase(base), k, cosine, seed=k)), k, cosine)


@pytest.mark.parametrize('cosine', HEADS)
def test_each_position_alone(cosine):
    """Pair j leaves out ``positions[j]`` only, and pair ``P + j`` everything BUT it (its one rank is that item): a cursor that is positioned one entry off, steps over
    an id of the other lane half wrongly or is spent one tile early shows in exactly that pair."""
    for n_items, k in ((33, 11), (2100, 10)):
        pos = positions(2 * 41, n_items, 32)
        base = R.float_case('randn', 2 * len(pos), n_items, 32, 0.3)
        everything = set(range(n_items))
        runs = [[p] for p in pos] + [sorted(everything - {p}) for p in pos]
        case = E.ExcludeCase(base, runs)
        assert pos == positions(case.n_pairs, n_items, 32)                 # (the runs of tiles are those of this call's pair count)
        got = _check(case, k, cosine)
        assert got[1][len(pos):, 0].tolist() == pos and bool((got[1][len(pos):, 1:] == -1).all())


@pytest.mark.parametrize('design', ['random', 'all_equal', 'tied_across', 'tie_at_boundary', 'one_list_dec', 'ascending'])
def test_exact_designs_equal_the_reference(design):
    """Integer-valued operands (dot product): items and scores EQUAL the stable ranking of what each pair may rank - ties on both sides of an excluded id, of a tile
    edge and of a pass boundary come back in ascending item id."""
    for j, (n_pairs, n_items) in enumerate(((5, 33), (33, 2100), (65, 300))):
        base = R.exact_case(design, n_pairs, n_items, 64, False, R.LAMS_EXACT[j % 2])
        k = (11, 128, 10)[j]
        case = E.ExcludeCase(base, lists_by_kind(S.SearchCase(base), k, False, seed=j))
        assert case.exact
        _check(case, k, False, 'bc'[j % 2], pairs=range(0, n_pairs, 4) if j else None)


@pytest.mark.parametrize('design', ['all_equal', 'tied_across', 'row_scales'])
def test_exact_designs_under_the_cosine_head(design):
    base = R.exact_case(design, 33, 2100, 64, True, 0.5)
    _check(E.ExcludeCase(base, lists_by_kind(S.SearchCase(base), 11, True)), 11, True, pairs=range(0, 33, 4))


@pytest.mark.parametrize('cosine', HEADS)
def test_width_640_takes_the_single_pair_tile_kernel(cosine):
    """Width 640 does not fit two pair tiles in LDS (``PB = 1``): 33 pairs are two workgroups per item slice, the second with one pair and 31 repeats of it."""
    assert R.eval_pair_tiles(640) == 1 and R.eval_pair_tiles(32) == 2
    base = R.float_case('randn', 33, 2100, 640, 0.3)
    _check(E.ExcludeCase(base, lists_by_kind(S.SearchCase(base), 11, cosine)), 11, cosine, 'c', pairs=range(0, 33, 3))


@pytest.mark.parametrize('cosine', HEADS)
def test_lists_together_with_a_mask(cosine):
    """An excluded id outside the mask is not subtracted twice from the pair's target; an excluded id that is the only candidate leaves target 0 (no pass finds the
    pair incomplete); garbage mask bits at or past ``n_items`` reach nothing."""
    for j, (n_pairs, n_items, k) in enumerate(((33, 33, 11), (65, 2100, 10), (5, 31, 128))):
        base = R.float_case('randn', n_pairs, n_items, 32, 0.3, seed=j)
        mask = S.mask_pattern('every_other', n_items)                      # the even ids
        free = S.SearchCase(base, mask=mask)
        runs = lists_by_kind(free, k, cosine, seed=j)
        runs[0] = [1, 3, (n_items - 2) | 1]                                  # only ids outside the mask: the target is the mask's
        runs[1] = [0, 1, 2, 3]                                             # two inside, two outside
        case = E.ExcludeCase(base, runs, mask=mask)
        assert case.targets(k)[0] == free.target(k) and case.allowed()[1].sum() == mask.sum() - 2
        got = _check(case, k, cosine, 'bc'[j % 2])
        if n_items % 32:
            again = _excluding(ExcludeOperands(case, 'bc'[j % 2], S.pack_mask(mask, garbage=True)), k, cosine, case.name + ' (garbage past n_items)')
            assert _same(got, again), f'{case.name}: mask bits at or past n_items reach the result'
        only = S.mask_pattern('last', n_items)                             # one candidate: pair 0 excludes it, pair 1 excludes its neighbour, pair 2 nothing
        lone = E.ExcludeCase(base, [[n_items - 1], [max(n_items - 2, 0)], []] + [[]] * (n_pairs - 3), mask=only)
        assert lone.targets(k).tolist()[:3] == [0, 1, 1]
        got = _check(lone, k, cosine, mask_words=S.pack_mask(only, garbage=True))
        assert int(got[2][0]) == 0 and got[1][:3, 0].tolist() == [-1, n_items - 1, n_items - 1]


@pytest.mark.parametrize('cosine', HEADS)
def test_row_indirection_shares_runs_between_pairs(cosine):
    """``excl_row``: several pairs on one run, ``-1`` for none, runs that no pair uses - each row equals the call that gives every pair its own copy of its run
    (null ``excl_row``); one case with external query rows and pairs without a user."""
    for j, (n_pairs, n_items, k) in enumerate(((33, 2100, 11), (65, 33, 10), (2, 31, 1))):
        base = R.float_case('randn', n_pairs, n_items, 32, 0.3, seed=j)
        ext = _ext_rows(n_pairs, 16, j) if j == 0 else None
        anon = np.arange(n_pairs) % 3 == 1 if j == 0 else None
        free = S.SearchCase(base, ext=ext, anon=anon)
        shared = lists_by_kind(free, k, cosine, seed=j)[:7] if n_pairs > 7 else [[0, 5], [30]]
        rows = np.arange(n_pairs) % (len(shared) + 1) - 1                  # -1, 0, 1, ...: every run has several pairs where there are enough
        rows[-1] = rows[0] = len(shared) - 1 if n_pairs > 2 else 0         # the first and the last pair on the same run
        by_row = E.ExcludeCase(base, shared, rows=rows, ext=ext, anon=anon)
        got = _check(by_row, k, cosine, 'bc'[j % 2], pairs=None if j else range(0, n_pairs, 2))
        copied = E.ExcludeCase(base, [by_row.run_of(c) for c in range(n_pairs)], ext=ext, anon=anon)
        what = f'{copied.name} k={k} cosine={cosine}'
        assert _same(got, _excluding(ExcludeOperands(copied, 'bc'[j % 2]), k, cosine, what)), f'{what}: a shared run and its copies differ'


@pytest.mark.parametrize('cosine', HEADS)
def test_empty_lists_return_the_bits_of_search_topk(cosine):
    """Every run empty, ``excl_row`` all ``-1``, and a null ``excl_ptr``: scores, items and ``passes`` of ``ihg_search_topk`` on the same sources."""
    for j, (n_pairs, n_items, dim) in enumerate(((1, 1, 32), (33, 33, 32), (65, 2100, 32), (33, 2100, 640), (64, 31, 32))):
        base = R.float_case('randn', n_pairs, n_items, dim, 0.3, seed=j)
        mask = S.mask_pattern('random10', n_items, seed=j) if j % 2 else None
        anon = np.arange(n_pairs) % 4 == 0
        k = KS[j % 4]
        what = f'{base.name} k={k} cosine={cosine}'
        want = _search_launch(SearchOperands(S.SearchCase(base, anon=anon, mask=mask)), k, cosine, 0xFF, what + ' (ihg_search_topk)')
        empty = ExcludeOperands(E.ExcludeCase(base, [[]] * n_pairs, anon=anon, mask=mask))
        assert _same(_excluding(empty, k, cosine, what + ' empty runs'), want), f'{what}: empty runs differ from ihg_search_topk'
        none = ExcludeOperands(E.ExcludeCase(base, [[3 % n_items]], rows=np.full(n_pairs, -1), anon=anon, mask=mask))
        assert _same(_excluding(none, k, cosine, what + ' rows -1'), want), f'{what}: excl_row = -1 everywhere differs from ihg_search_topk'
        assert _same(_launch(empty, k, cosine, 0xFF, what + ' null lists', lists=False), want), f'{what}: a null excl_ptr differs from ihg_search_topk'
