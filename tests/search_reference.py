"""Reference for the three additions of ``ihg_search_topk`` (``csrc/eval.hip``) over ``ihg_score_topk_deep`` - a query row given from outside the feature matrix, a
pair without a user, a candidate mask - for ``tests/test_search_host.py`` (CPU), ``tests/test_search_kernels.py`` and ``tests/test_search_model.py`` (GPU).  Not a test
module; numpy and torch on the CPU only.  Everything is built on ``ranking_reference`` / ``topk_reference`` by import: a ``SearchCase`` IS a ``RankCase`` whose
``rows()`` / ``scores64()`` state the additions, so ``score_bound``, ``ensure_exact``, ``expected`` and ``float_verdict`` of ``ranking_reference`` apply as they are.

    external row   the query row of pair c is ``ext[c]`` in columns ``0 .. q_dim`` and zero in ``q_dim .. dim`` - the row of an isolated query node appended to the
                   feature matrix (``appended_case`` builds exactly that matrix; ``test_search_host.py`` holds the two references equal)
    no user        ``m = q`` (``Models/PredictionLayers.py:34-37``), not ``lam q``; the cosine head's norm is that of ``q``
    mask           a bool [I]: the ranking is the stable ranking of the candidates' scores; a pair holds ``min(k, candidates)`` ranks, then the ``(-FLT_MAX, -1)`` tail

The per-score bound is ``ranking_reference``'s, unchanged, with ``T`` over the magnitudes actually mixed:

    pair with a user    T = sum_c |a_c| (lam |q_c| + (1 - lam) |u_c|), as there; for an external row q_c = 0 for c >= q_dim, so the query part of the sum runs over
                        q_dim columns - the kernel multiplies lam by a literal 0 there: the addend lam * 0 is exact and the bound's term for it is 0
    pair without one    T = sum_c |a_c| |q_c|.  The kernel copies q: none of the mix's C_MIX = 3 roundings happens.  The bound keeps C_MIX = 3 (a bound with 0 in its
                        place would hold as well; 3 of 48 ksteps + 6 units is no slack worth a second formula).  ``rows()`` states such a pair as u := q, for which
                        ``lam |q| + (1 - lam) |u| = |q|`` is the T above and, in ``score_bound``'s cosine branch, ``lam q + (1 - lam) u = q`` up to 2^-53 of a norm
                        that only scales a term of the bound; ``scores64`` itself takes ``m = q`` exactly
    mask                changes no score: a candidate's score has the bound of the unmasked call.  ``masked_float_verdict`` is ``float_verdict`` with "every item"
                        read as "every candidate": no returned item outside the mask, and no omitted CANDIDATE beats the last returned one beyond both bounds
"""
import numpy as np
import torch

import ranking_reference as R
import topk_reference as tref

FLT_MAX = R.FLT_MAX


class SearchCase(R.RankCase):
    """``base`` (a ``RankCase``) with ``ext`` (float32 ``[C, q_dim]`` external query rows, or None), ``anon`` (bool ``[C]``: the pairs without a user, or None) and
    ``mask`` (bool ``[I]``, or None).  ``users`` holds -1 for the pairs without a user, as the entry point takes them."""

    def __init__(self, base, ext=None, anon=None, mask=None):
        self.__dict__.update(base.__dict__)
        self._scores = {}
        self.base = base
        self.ext = None if ext is None else torch.as_tensor(np.asarray(ext, np.float32))
        self.q_dim = None if ext is None else int(self.ext.shape[1])
        assert ext is None or (tuple(self.ext.shape) == (self.n_pairs, self.q_dim) and 1 <= self.q_dim <= self.dim)
        self.anon = np.zeros(self.n_pairs, bool) if anon is None else np.asarray(anon, bool)
        self.users = torch.where(torch.from_numpy(self.anon), torch.full_like(base.users, -1), base.users)
        self.mask = None if mask is None else np.asarray(mask, bool)
        assert self.mask is None or self.mask.shape == (self.n_items,)
        self.name = base.name + (f' ext q={self.q_dim}' if ext is not None else '') + (f' anon={int(self.anon.sum())}' if self.anon.any() else '') + \
            (f' mask={int(self.mask.sum())}' if self.mask is not None else '')

    def query_rows64(self):
        """float64 ``[C, dim]``: the pairs' query rows, an external row padded with zeros."""
        f = self.features.double().numpy()
        if self.ext is None:
            return f[self.queries.numpy() + self.query_row0]
        q = np.zeros((self.n_pairs, self.dim))
        q[:, :self.q_dim] = self.ext.double().numpy()
        return q

    def rows(self):
        """``(u, q, a)`` as ``RankCase.rows``; a pair without a user has u := q (module docstring)."""
        f = self.features.double().numpy()
        q = self.query_rows64()
        u = f[np.where(self.anon, 0, self.base.users.numpy())].copy()
        u[self.anon] = q[self.anon]
        return u, q, f[self.item_row0:]

    def mixed64(self):
        u, q, _ = self.rows()
        return np.where(self.anon[:, None], q, self.lam * q + (1 - self.lam) * u)

    def scores64(self, cosine):
        """[C, I] float64 scores of EVERY item (the mask is applied to the ranking, not to the scores)."""
        if cosine not in self._scores:
            m = torch.from_numpy(self.mixed64())
            items = self.features.double()[self.item_row0:]
            if cosine:
                m = m / m.norm(dim=1, keepdim=True).clamp_min(tref.EPS)
                items = items / items.norm(dim=1, keepdim=True).clamp_min(tref.EPS)
            self._scores[cosine] = m @ items.t() + self.bias.double()
        return self._scores[cosine]

    def candidates(self):
        return np.arange(self.n_items) if self.mask is None else np.flatnonzero(self.mask)

    def target(self, k):
        return min(k, len(self.candidates()))


def case_from_features(name, features, users, queries, query_row0, item_row0, bias, lam):
    """A float ``RankCase`` over a feature matrix that exists already (a model's ``[N, D]`` propagation output): users / queries int64 ``[C]``, every row from
    ``item_row0`` on an item."""
    out = object.__new__(R.RankCase)
    f = torch.as_tensor(features).detach().float().cpu().contiguous()
    out.name, out.dim, out.n_items, out.lam, out.exact = name, int(f.shape[1]), int(f.shape[0]) - int(item_row0), float(np.float32(lam)), False
    out.users, out.queries = (torch.as_tensor(np.asarray(v)).long().reshape(-1) for v in (users, queries))
    out.n_pairs, out.query_row0, out.item_row0 = int(out.users.shape[0]), int(query_row0), int(item_row0)
    out.features, out.bias, out._scores = f, torch.as_tensor(bias).detach().float().cpu(), {}
    return out


def appended_case(case):
    """The ``RankCase`` that states an external-row case inside ``ranking_reference``'s own terms: the feature matrix with the external rows appended BEHIND the item
    rows (zero above ``q_dim``) and ``queries`` pointing at them (``query_row0 + queries[c]`` = the appended row of pair ``c``; the call names ``n_items`` itself, so
    the rows behind the items are no items).  Users as in the base case (a pair without a user keeps its base user: ask ``case.anon``)."""
    assert case.ext is not None
    base = case.base
    out = object.__new__(R.RankCase)
    out.__dict__.update(base.__dict__)
    extra = torch.zeros(case.n_pairs, case.dim)
    extra[:, :case.q_dim] = case.ext
    out.features = torch.cat([base.features, extra])
    first = base.item_row0 + base.n_items
    out.queries = torch.arange(first, first + case.n_pairs, dtype=torch.int64) - base.query_row0
    out._scores = {}
    out.name = base.name + ' (rows appended)'
    return out


def expected(case, k, cosine):
    """``(top_scores [C, k] float32, top_items [C, k] int32)``: the stable ranking of the candidates' float64 scores, the tail past ``min(k, candidates)``
    ``(-FLT_MAX, -1)`` (``ranking_reference.expected`` under a mask)."""
    s = case.scores64(cosine)
    cand = torch.from_numpy(case.candidates())
    n = case.target(k)
    scores = torch.full((case.n_pairs, k), -FLT_MAX, dtype=torch.float32)
    items = torch.full((case.n_pairs, k), -1, dtype=torch.int32)
    if n:
        sub = s[:, cand]
        order = tref.ranking(sub, n)                                       # (the candidates ascend, so a stable sort of the subset keeps ties in ascending item id)
        scores[:, :n], items[:, :n] = torch.gather(sub, 1, order).float(), cand[order].int()
    return scores, items


def assert_exact(got_scores, got_items, case, k, cosine, what):
    want_scores, want_items = expected(case, k, cosine)
    got_scores, got_items = got_scores.cpu(), got_items.cpu()
    assert torch.equal(got_items, want_items), f'{what}: items differ from the stable ranking of the candidates: got {got_items.tolist()[:2]}, want {want_items.tolist()[:2]}'
    assert torch.equal(got_scores, want_scores), f'{what}: scores differ from float32(float64 scores)'


def filtered_prefix(full_scores, full_items, mask, k):
    """From an unmasked ranking of ALL items (``[C, I']`` with ``I' >= I``: every item ranked, a ``-1`` tail allowed) the rows a masked call must return bitwise: the
    non-candidates removed, the first ``k`` kept, then the ``(-FLT_MAX, -1)`` tail."""
    fs, fi = full_scores.cpu(), full_items.cpu()
    keep_of = torch.from_numpy(np.asarray(mask, bool))
    scores = torch.full((fs.shape[0], k), -FLT_MAX, dtype=torch.float32)
    items = torch.full((fs.shape[0], k), -1, dtype=torch.int32)
    for c in range(fs.shape[0]):
        real = fi[c] >= 0
        keep = real.clone()
        keep[real] = keep_of[fi[c][real].long()]
        n = min(k, int(keep.sum()))
        scores[c, :n], items[c, :n] = fs[c][keep][:n], fi[c][keep][:n]
    return scores, items


def masked_float_verdict(got_scores, got_items, case, k, cosine, what):
    """``ranking_reference.float_verdict`` with the mask (module docstring); returns the worst ``|s - s64| / bound``.  Without a mask it IS ``float_verdict``."""
    if case.mask is None:
        return R.float_verdict(got_scores, got_items, case, k, cosine, what)
    s64, bound = case.scores64(cosine).numpy(), R.score_bound(case, cosine)
    gs, gi = got_scores.cpu().numpy().astype(np.float64), got_items.cpu().numpy().astype(np.int64)
    n = case.target(k)
    assert gs.shape == gi.shape == (case.n_pairs, k), f'{what}: shape'
    assert np.all(gi[:, n:] == -1) and np.all(gs[:, n:] == -FLT_MAX), f'{what}: the tail past min(k, candidates) is not (-FLT_MAX, -1)'
    if n == 0:
        return 0.0
    gs, gi = gs[:, :n], gi[:, :n]
    assert np.all(np.isfinite(gs)), f'{what}: a score is not finite'
    assert np.all((gi >= 0) & (gi < case.n_items)), f'{what}: an item id is out of range'
    assert np.all(case.mask[gi]), f'{what}: an item outside the mask is returned'
    assert all(len(set(row)) == n for row in gi.tolist()), f'{what}: an item is returned twice'
    assert np.all(gs[:, 1:] <= gs[:, :-1]), f'{what}: the scores increase somewhere'
    assert np.all((gs[:, 1:] < gs[:, :-1]) | (gi[:, 1:] > gi[:, :-1])), f'{what}: equal scores are not in ascending id'
    rows = np.arange(case.n_pairs)[:, None]
    ratio = np.abs(gs - s64[rows, gi]) / bound[rows, gi]
    worst = float(ratio.max())
    assert worst <= 1.0, f'{what}: |s - s64| / bound = {worst:.3g} at (pair, rank) {np.unravel_index(int(ratio.argmax()), ratio.shape)}'
    omitted = np.broadcast_to(case.mask[None, :], s64.shape).copy()
    omitted[rows, gi] = False
    floor = s64[rows, gi[:, -1:]] + bound[rows, gi[:, -1:]]
    beats = omitted & (s64 - bound > floor)
    assert not beats.any(), f'{what}: an omitted candidate beats the last returned one beyond both bounds, (pair, item) {np.argwhere(beats)[0].tolist()}'
    return worst


def pack_mask(mask, garbage=False):
    """numpy uint32 ``[ceil(I / 32)]``: bit ``i % 32`` of word ``i // 32`` = ``mask[i]``; ``garbage``: the bits at and past ``I`` of the last word set."""
    mask = np.asarray(mask, bool)
    n = mask.shape[0]
    padded = np.zeros((n + 31) // 32 * 32, bool)
    padded[:n] = mask
    if garbage:
        padded[n:] = True
    return np.packbits(padded, bitorder='little').view(np.uint32).copy()


MASK_PATTERNS = ('all', 'none', 'first', 'last', 'last_of_word', 'every_other', 'last_partial_word', 'random10')


def mask_pattern(name, n_items, seed=0):
    m = np.zeros(n_items, bool)
    if name == 'all':
        m[:] = True
    elif name == 'first':
        m[0] = True
    elif name == 'last':
        m[-1] = True
    elif name == 'last_of_word':                                           # bit 31 of the last FULL word (n < 32: there is none - the last item)
        m[(n_items // 32) * 32 - 1 if n_items >= 32 else n_items - 1] = True
    elif name == 'every_other':
        m[::2] = True
    elif name == 'last_partial_word':                                      # the items of the last word only (a multiple of 32: that word is full)
        m[(n_items - 1) // 32 * 32:] = True
    elif name == 'random10':
        m = np.random.default_rng([seed, n_items]).random(n_items) < 0.1
    elif name != 'none':
        raise KeyError(name)
    return m
