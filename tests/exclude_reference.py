"""Reference for ``ihg_search_topk_excluding`` (``csrc/eval.hip``): ``ihg_search_topk`` with a list of items per pair that are never ranked for it - for
``tests/test_exclude_host.py`` (CPU), ``tests/test_exclude_kernels.py`` and ``tests/test_exclude_model.py`` (GPU).  Not a test module; numpy and torch on the CPU
only.  Built on ``search_reference`` / ``ranking_reference`` by import: an ``ExcludeCase`` IS a ``SearchCase`` with ``lists`` (one run of item ids per row) and
``row_of`` (the run of every pair: ``-1`` none, ``None``: run ``c``).  With ``allowed[c] = candidates & ~run of pair c`` ("the mask of pair c"):

    expected        the stable ranking of pair c's float64 scores over ``allowed[c]``; pair c holds ``target_c = min(k, |allowed[c]|)`` ranks, then the
                    ``(-FLT_MAX, -1)`` tail.  An excluded id outside the mask is in ``~mask`` already: it is not subtracted twice
    scores          exclusion changes no score: an allowed item's score has the bound of the call without lists, ``ranking_reference.score_bound`` unchanged.  No
                    tolerance is introduced here
    verdicts        ``filtered_prefix`` and ``float_verdict`` are ``search_reference``'s with "the mask" read as "the mask of pair c"
    one pair        ``single(c)`` is the ``SearchCase`` of pair c alone under the mask ``allowed[c]``: what ``ihg_search_topk`` must return for it BITWISE is row c
"""
import numpy as np
import torch

import ranking_reference as R
import search_reference as S
import topk_reference as tref

FLT_MAX = R.FLT_MAX


class ExcludeCase(S.SearchCase):
    """``base`` with ``SearchCase``'s ``ext`` / ``anon`` / ``mask``, ``lists`` (a sequence of ``R`` runs of item ids; stored strictly ascending, as the entry point
    takes them) and ``rows`` (kept as ``row_of``: int ``[C]``, ``-1``: no run; ``None``: pair ``c`` has run ``c`` and ``R = C``)."""

    def __init__(self, base, lists, rows=None, ext=None, anon=None, mask=None):
        super().__init__(base, ext=ext, anon=anon, mask=mask)
        self.lists = [np.unique(np.asarray(run, np.int64)).astype(np.int32) for run in lists]
        assert all(run.size == 0 or (run[0] >= 0 and run[-1] < self.n_items) for run in self.lists)
        self.row_of = None if rows is None else np.asarray(rows, np.int64)       # (``rows()`` is ``SearchCase``'s)
        assert (len(self.lists) == self.n_pairs) if rows is None else (self.row_of.shape == (self.n_pairs,) and self.row_of.max(initial=-1) < len(self.lists) >= 1)
        self.name += f' excl={sum(len(r) for r in self.lists)} in {len(self.lists)} runs' + (' by row' if rows is not None else '')
        self._allowed = None

    def run_of(self, c):
        r = c if self.row_of is None else int(self.row_of[c])
        return np.zeros(0, np.int32) if r < 0 else self.lists[r]

    def csr(self):
        """``(ptr int64 [R + 1], items int32 [max(total, 1)])`` (an empty list keeps one unread entry: the entry point takes a null pointer for "no lists")."""
        ptr = np.zeros(len(self.lists) + 1, np.int64)
        np.cumsum([len(r) for r in self.lists], out=ptr[1:])
        flat = np.concatenate(self.lists).astype(np.int32) if ptr[-1] else np.zeros(1, np.int32)
        return ptr, flat

    def allowed(self):
        """bool ``[C, I]``: the mask of pair c."""
        if self._allowed is None:
            a = np.broadcast_to(np.ones(self.n_items, bool) if self.mask is None else self.mask, (self.n_pairs, self.n_items)).copy()
            for c in range(self.n_pairs):
                a[c, self.run_of(c)] = False
            self._allowed = a
        return self._allowed

    def targets(self, k):
        """int ``[C]``: ``target_c``."""
        return np.minimum(k, self.allowed().sum(1))

    def single(self, c):
        """Pair ``c`` alone as a ``SearchCase`` whose mask is ``allowed[c]``."""
        b = object.__new__(R.RankCase)
        b.__dict__.update(self.base.__dict__)
        b.users, b.queries, b.n_pairs, b._scores = self.base.users[c:c + 1], self.base.queries[c:c + 1], 1, {}
        if getattr(self.base, 'pair_exp', None) is not None:
            b.pair_exp = self.base.pair_exp[c:c + 1]
        b.name = f'{self.base.name} pair {c}'
        return S.SearchCase(b, ext=None if self.ext is None else self.ext[c:c + 1].numpy(), anon=self.anon[c:c + 1], mask=self.allowed()[c])


def expected(case, k, cosine):
    """``(top_scores [C, k] float32, top_items [C, k] int32)``: per pair the stable ranking of the float64 scores of ``allowed[c]``, the tail past ``target_c``
    ``(-FLT_MAX, -1)`` (``search_reference.expected`` under the mask of pair c)."""
    s = case.scores64(cosine)
    scores = torch.full((case.n_pairs, k), -FLT_MAX, dtype=torch.float32)
    items = torch.full((case.n_pairs, k), -1, dtype=torch.int32)
    for c, n in enumerate(case.targets(k).tolist()):
        if n:
            cand = torch.from_numpy(np.flatnonzero(case.allowed()[c]))
            sub = s[c, cand]
            order = tref.ranking(sub, n)                                   # (the ids ascend, so a stable sort of the subset keeps ties in ascending item id)
            scores[c, :n], items[c, :n] = sub[order].float(), cand[order].int()
    return scores, items


def assert_exact(got_scores, got_items, case, k, cosine, what):
    want_scores, want_items = expected(case, k, cosine)
    got_scores, got_items = got_scores.cpu(), got_items.cpu()
    if not torch.equal(got_items, want_items):
        bad = (got_items != want_items).nonzero()[0].tolist()
        raise AssertionError(f'{what}: items differ from the stable ranking of what pair {bad[0]} may rank, first at (pair, rank) {bad}: got {int(got_items[tuple(bad)])}, '
                             f'want {int(want_items[tuple(bad)])}')
    assert torch.equal(got_scores, want_scores), f'{what}: scores differ from float32(float64 scores)'


def filtered_prefix(full_scores, full_items, case, k):
    """``search_reference.filtered_prefix`` with the mask of pair c: from a ranking of ALL items per pair (no mask, no lists) the rows the excluding call must return
    bitwise."""
    scores = torch.full((case.n_pairs, k), -FLT_MAX, dtype=torch.float32)
    items = torch.full((case.n_pairs, k), -1, dtype=torch.int32)
    for c in range(case.n_pairs):
        scores[c:c + 1], items[c:c + 1] = S.filtered_prefix(full_scores[c:c + 1], full_items[c:c + 1], case.allowed()[c], k)
    return scores, items


def float_verdict(got_scores, got_items, case, k, cosine, what):
    """``search_reference.masked_float_verdict`` with the mask of pair c; returns the worst ``|s - s64| / bound``."""
    s64, bound = case.scores64(cosine).numpy(), R.score_bound(case, cosine)
    gs_all, gi_all = got_scores.cpu().numpy().astype(np.float64), got_items.cpu().numpy().astype(np.int64)
    assert gs_all.shape == gi_all.shape == (case.n_pairs, k), f'{what}: shape'
    allowed, worst = case.allowed(), 0.0
    for c, n in enumerate(case.targets(k).tolist()):
        gs, gi, ok = gs_all[c], gi_all[c], allowed[c]
        assert np.all(gi[n:] == -1) and np.all(gs[n:] == -FLT_MAX), f'{what}: pair {c}: the tail past min(k, what it may rank) = {n} is not (-FLT_MAX, -1)'
        if n == 0:
            continue
        gs, gi = gs[:n], gi[:n]
        assert np.all(np.isfinite(gs)), f'{what}: pair {c}: a score is not finite'
        assert np.all((gi >= 0) & (gi < case.n_items)), f'{what}: pair {c}: an item id is out of range'
        assert np.all(ok[gi]), f'{what}: pair {c}: an item outside the mask of pair {c} is returned: {gi[~ok[gi]].tolist()}'
        assert len(set(gi.tolist())) == n, f'{what}: pair {c}: an item is returned twice'
        assert np.all(gs[1:] <= gs[:-1]), f'{what}: pair {c}: the scores increase somewhere'
        assert np.all((gs[1:] < gs[:-1]) | (gi[1:] > gi[:-1])), f'{what}: pair {c}: equal scores are not in ascending id'
        ratio = np.abs(gs - s64[c, gi]) / bound[c, gi]
        assert ratio.max() <= 1.0, f'{what}: pair {c}: |s - s64| / bound = {ratio.max():.3g} at rank {int(ratio.argmax())}'
        worst = max(worst, float(ratio.max()))
        omitted = ok.copy()
        omitted[gi] = False
        beats = omitted & (s64[c] - bound[c] > s64[c, gi[-1]] + bound[c, gi[-1]])
        assert not beats.any(), f'{what}: pair {c}: an omitted item of its mask beats the last returned one beyond both bounds: item {int(np.flatnonzero(beats)[0])}'
    return worst
