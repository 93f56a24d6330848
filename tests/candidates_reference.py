"""Reference for ``ihg_search_candidates`` (``csrc/candidates.hip``): a search ranks only the items of ITS run of a candidate CSR - for ``tests/test_candidates_host.py``
(CPU), ``tests/test_candidates_kernels.py`` and ``tests/test_candidates_model.py`` (GPU).  Not a test module; numpy and torch on the CPU only.  A ``CandidateCase`` IS an
``ExcludeCase`` (external rows, pairs without a user, the one-for-all mask, the exclusion runs) with candidate runs and ``cand_row_of``:

    allowed[c]      in the run of search c, in the mask, not in c's exclusion run
    targets(k)      ``min(k, |allowed[c]|)``: where the ``(-FLT_MAX, -1)`` tail of search c begins
    expected        the stable ranking of search c's float64 scores over ``allowed[c]`` (``exclude_reference.expected``, which reads ``allowed``)
    emulation       the kernels' own summation scheme in float32 (``emu_run_scores``) and the whole call (``emulate``), with ``mutation`` naming ONE way of being wrong
    bound           ``score_bound``, derived below; ``float_verdict`` is ``exclude_reference.float_verdict`` with it

The scheme (``csrc/candidates.hip``).  ``m_c = fma(lam, q_c, fl(fl(1 - lam) u_c))`` (q alone without a user; zero past ``q_dim`` for an external row).  With
``segs = ceil(d / 4)`` four-column segments and ``G = group_width(d) = min(16, 2^ceil(log2 segs))`` lanes per candidate, lane g runs ONE fma chain over the segments
``g, g + G, ...`` (four fmas each, columns ascending), a shuffle tree of ``log2 G`` levels adds the G partial sums, and ``s = fl(dot + bias)``.

The bound (u = 2^-24, first order, ``T = sum_c |a_c| (lam |q_c| + (1 - lam) |u_c|)``: the UNMIXED magnitudes, because the mix can cancel):

    |s - s64| <= gamma u T + u |s64|        gamma = C_MIX + CHAIN + TREE + 1

    C_MIX = 3   the roundings an addend of the mix passes through: ``1 - lam``, its product with the user row, the fma
    CHAIN       ``4 ceil(segs / G)``: the fmas of the longest lane chain - its first product passes through every one of them
    TREE        ``log2 G`` additions
    + 1         the final addition of the bias rounds relative to ``|s| <= |s64| + (the error so far)``: ``u |s64|`` is the bound's second term, and one unit of ``u T``
                stands for ``u`` times the error so far and for the second-order remainder of the product of ``(1 + u)`` factors, which is below
                ``gamma u / 2 < 2^-16`` of the first-order term at the widest row (gamma = 136 at d = 2048) where one unit is 1 / 136 of it

The cosine head divides the dot product by ``fl(na nm)`` with ``na = max(sqrt(sum a^2), 1e-8)`` and ``nm`` likewise, both sums in the chain-and-tree order above.  A sum
of squares has only positive terms, so its relative error is at most ``(CHAIN + TREE) u``; the square root halves that and rounds once: ``C_NORM = (CHAIN + TREE) / 2 + 1``
per norm; the product of the two norms and the division round once each; the mixed row under the norm carries the mix's roundings relative to the unmixed magnitudes
``mm``.  With the float64 norms clamped at the float64 1e-8 (the kernel clamps at the float32 ``1e-8f``, 0.1 u below it: a clamped norm has no sum and no root behind it, so
its ``C_NORM u``, which stays in the bound, covers that):

    |s - s64| <= gamma u T / (na nm) + |s64 - bias| (2 C_NORM u + 2 u + C_MIX u |mm|_2 / nm) + u |s64|

Nothing here is fitted to what the kernels return; ``tests/test_candidates_kernels.py`` prints the measured worst ``error / bound``.
"""
import numpy as np
import torch

import exclude_reference as E
import ranking_reference as R
import search_reference as S
from contraction_reference import U

FLT_MAX = R.FLT_MAX
TOP = 10                                 # kCandTop
CH = 256                                 # kCandChunk
MAX_DIM = 2048                           # kCandMaxDim
ROWS_IN_FLIGHT = 4                       # kCandRows
C_MIX = 3
EPS = 1e-8
NEG_INF = np.float32(-np.inf)


def group_width(dim):
    segs = (dim + 3) // 4
    g = 1
    while g < segs and g < 16:
        g *= 2
    return g


def chain_length(dim):
    segs = (dim + 3) // 4
    return 4 * ((segs + group_width(dim) - 1) // group_width(dim))


def tree_levels(dim):
    return int(np.log2(group_width(dim)))


def gamma(dim):
    return C_MIX + chain_length(dim) + tree_levels(dim) + 1


def workspace_bytes(n_pairs, total):
    return (4 * total + 15) // 16 * 16 + (8 * (n_pairs + 1) + 15) // 16 * 16 + 16 * n_pairs


class CandidateCase(E.ExcludeCase):
    """``base`` with ``cand`` (a sequence of ``R`` runs of item ids; stored strictly ascending, as the entry point takes them), ``cand_rows`` (kept as ``cand_row_of``:
    int ``[C]``, negative or ``>= R``: no run; ``None``: search ``c`` has run ``c`` and ``R = C``) and ``ExcludeCase``'s ``lists`` / ``rows`` (``lists=None``: the call
    passes no exclusion lists at all), ``ext``, ``anon``, ``mask``."""

    def __init__(self, base, cand, cand_rows=None, lists=None, rows=None, ext=None, anon=None, mask=None):
        self.has_lists = lists is not None
        super().__init__(base, [[]] * base.n_pairs if lists is None else lists, rows=rows if lists is not None else None, ext=ext, anon=anon, mask=mask)
        self.cand = [np.unique(np.asarray(run, np.int64)).astype(np.int32) for run in cand]
        assert all(run.size == 0 or (run[0] >= 0 and run[-1] < self.n_items) for run in self.cand)
        self.cand_row_of = None if cand_rows is None else np.asarray(cand_rows, np.int64)
        assert (len(self.cand) == self.n_pairs) if cand_rows is None else (self.cand_row_of.shape == (self.n_pairs,) and len(self.cand) >= 1)
        self.name += f' cand={sum(len(r) for r in self.cand)} in {len(self.cand)} runs' + (' by row' if cand_rows is not None else '')

    def cand_index(self, c):
        """The run of search ``c`` (an index into ``cand``), ``-1``: none."""
        r = c if self.cand_row_of is None else int(self.cand_row_of[c])
        return r if 0 <= r < len(self.cand) else -1

    def cand_of(self, c):
        r = self.cand_index(c)
        return np.zeros(0, np.int32) if r < 0 else self.cand[r]

    def cand_csr(self):
        """``(ptr int64 [R + 1], items int32 [max(total, 1)], total)``."""
        ptr = np.zeros(len(self.cand) + 1, np.int64)
        np.cumsum([len(r) for r in self.cand], out=ptr[1:])
        total = int(ptr[-1])
        flat = np.concatenate(self.cand).astype(np.int32) if total else np.zeros(1, np.int32)
        return ptr, flat, total

    def owner_of_run(self):
        """int ``[R]``: the lowest-numbered search that names each run, ``-1``: none (``all_scores`` holds that search's scores, or ``-inf``)."""
        owner = np.full(len(self.cand), -1, np.int64)
        for c in range(self.n_pairs - 1, -1, -1):
            r = self.cand_index(c)
            if r >= 0:
                owner[r] = c
        return owner

    def gate(self):
        """bool ``[C, I]``: in the mask and not in the exclusion run of search c (``ExcludeCase.allowed``)."""
        g = np.broadcast_to(np.ones(self.n_items, bool) if self.mask is None else self.mask, (self.n_pairs, self.n_items)).copy()
        for c in range(self.n_pairs):
            g[c, self.run_of(c)] = False
        return g

    def allowed(self):
        if self._allowed is None:
            gate = self.gate()
            a = np.zeros_like(gate)
            for c in range(self.n_pairs):
                run = self.cand_of(c)
                a[c, run] = gate[c, run]
            self._allowed = a
        return self._allowed

    def single(self, c):
        """Search ``c`` alone as an ``ExcludeCase``-free ``SearchCase`` whose mask is ``allowed[c]`` (what the whole-catalogue entry points rank for it)."""
        b = object.__new__(R.RankCase)
        b.__dict__.update(self.base.__dict__)
        b.users, b.queries, b.n_pairs, b._scores = self.base.users[c:c + 1], self.base.queries[c:c + 1], 1, {}
        if getattr(self.base, 'pair_exp', None) is not None:
            b.pair_exp = self.base.pair_exp[c:c + 1]
        b.name = f'{self.base.name} search {c}'
        return S.SearchCase(b, ext=None if self.ext is None else self.ext[c:c + 1].numpy(), anon=self.anon[c:c + 1], mask=self.allowed()[c])


expected = E.expected
assert_exact = E.assert_exact


def score_bound(case, cosine):
    """float64 ``[C, I]``: the bound of the module docstring on ``|s - s64|`` of every (search, item)."""
    u, q, a = case.rows()
    mm, t = case.magnitudes()
    s64 = case.scores64(cosine).numpy()
    dot = gamma(case.dim) * U * t
    if not cosine:
        return dot + U * np.abs(s64)
    m = case.mixed64()
    na, nm = np.maximum(np.linalg.norm(a, axis=1), EPS), np.maximum(np.linalg.norm(m, axis=1), EPS)
    c_norm = (chain_length(case.dim) + tree_levels(case.dim)) / 2 + 1
    cos = np.abs(s64 - case.bias.double().numpy()[None, :])
    rel = 2 * c_norm * U + 2 * U + (C_MIX * U * np.linalg.norm(mm, axis=1) / nm)[:, None]
    return dot / (na[None, :] * nm[:, None]) + cos * rel + U * np.abs(s64)


def _ratio(err, bound):
    """``err / bound``; a zero bound (an exact zero score of zero operands) admits a zero error only."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


def float_verdict(got_scores, got_items, case, k, cosine, what):
    """``exclude_reference.float_verdict`` under ``score_bound`` of this module, nothing left out: the tail where it belongs; the returned scores finite, non-increasing,
    ties in ascending id; the items distinct, in range and allowed; every score within its bound; no omitted allowed item beats the last returned one beyond both
    bounds.  Returns the worst ``|s - s64| / bound``."""
    s64, bound = case.scores64(cosine).numpy(), score_bound(case, cosine)
    gs_all, gi_all = torch.as_tensor(got_scores).cpu().numpy().astype(np.float64), torch.as_tensor(got_items).cpu().numpy().astype(np.int64)
    assert gs_all.shape == gi_all.shape == (case.n_pairs, k), f'{what}: shape'
    allowed, worst = case.allowed(), 0.0
    for c, n in enumerate(case.targets(k).tolist()):
        gs, gi, ok = gs_all[c], gi_all[c], allowed[c]
        assert np.all(gi[n:] == -1) and np.all(gs[n:] == -FLT_MAX), f'{what}: search {c}: the tail past min(k, what it may rank) = {n} is not (-FLT_MAX, -1)'
        if n == 0:
            continue
        gs, gi = gs[:n], gi[:n]
        assert np.all(np.isfinite(gs)), f'{what}: search {c}: a score is not finite'
        assert np.all((gi >= 0) & (gi < case.n_items)), f'{what}: search {c}: an item id is out of range'
        assert np.all(ok[gi]), f'{what}: search {c}: an item it may not rank is returned: {gi[~ok[gi]].tolist()}'
        assert len(set(gi.tolist())) == n, f'{what}: search {c}: an item is returned twice'
        assert np.all(gs[1:] <= gs[:-1]), f'{what}: search {c}: the scores increase somewhere'
        assert np.all((gs[1:] < gs[:-1]) | (gi[1:] > gi[:-1])), f'{what}: search {c}: equal scores are not in ascending id'
        ratio = _ratio(np.abs(gs - s64[c, gi]), bound[c, gi])
        assert ratio.max() <= 1.0, f'{what}: search {c}: |s - s64| / bound = {ratio.max():.3g} at rank {int(ratio.argmax())}'
        worst = max(worst, float(ratio.max()))
        omitted = ok.copy()
        omitted[gi] = False
        beats = omitted & (s64[c] - bound[c] > s64[c, gi[-1]] + bound[c, gi[-1]])
        assert not beats.any(), f'{what}: search {c}: an omitted item of its list beats the last returned one beyond both bounds: item {int(np.flatnonzero(beats)[0])}'
    return worst


def all_scores_verdict(flat, case, cosine, what):
    """The flat ``[total]`` scores: ``-inf`` exactly on the gated entries (and on runs nobody names), every other slot within its bound of the float64 score of the
    run's owner.  Returns the worst ratio."""
    flat = torch.as_tensor(flat).cpu().numpy()
    ptr, ids, total = case.cand_csr()
    assert flat.shape == (total,), f'{what}: all_scores has {flat.shape}, the lists hold {total}'
    s64, bound, gate, worst = case.scores64(cosine).numpy(), score_bound(case, cosine), case.gate(), 0.0
    for r, c in enumerate(case.owner_of_run().tolist()):
        got, run = flat[ptr[r]:ptr[r + 1]], case.cand[r]
        if c < 0:
            assert np.all(np.isneginf(got)), f'{what}: run {r} that no search names is not -inf'
            continue
        on = gate[c, run]
        assert np.all(np.isneginf(got[~on])), f'{what}: run {r}: a gated entry is not -inf'
        assert np.all(np.isfinite(got[on])), f'{what}: run {r}: an admitted entry is not finite'
        if on.any():
            ratio = _ratio(np.abs(got[on].astype(np.float64) - s64[c, run[on]]), bound[c, run[on]])
            assert ratio.max() <= 1.0, f'{what}: run {r} (search {c}): |s - s64| / bound = {ratio.max():.3g}'
            worst = max(worst, float(ratio.max()))
    return worst


def ranking_of_floats(flat, case, k):
    """``(top_scores, top_items)`` float32 / int32 ``[C, k]``: the stable ranking of these very floats (``all_scores``) per search, ``-inf`` entries left out - what the
    call's top-k must equal BITWISE where every search owns its run."""
    flat = torch.as_tensor(flat).cpu().numpy()
    ptr, _, _ = case.cand_csr()
    out_s = np.full((case.n_pairs, k), -FLT_MAX, np.float32)
    out_i = np.full((case.n_pairs, k), -1, np.int32)
    for c in range(case.n_pairs):
        r = case.cand_index(c)
        if r < 0:
            continue
        s, ids = flat[ptr[r]:ptr[r + 1]], case.cand[r]
        keep = s > NEG_INF
        s, ids = s[keep], ids[keep]
        order = np.lexsort((ids, -s.astype(np.float64)))[:k]
        out_s[c, :len(order)], out_i[c, :len(order)] = s[order], ids[order]
    return torch.from_numpy(out_s), torch.from_numpy(out_i)


# =============================================================================================
# emulation
# =============================================================================================
MUTATIONS = ('stale_mixed_row', 'drop_last_partial_chunk', 'ties_by_higher_id', 'boundary_not_advanced', 'excluded_still_ranked', 'mask_bit_of_next_item', 'cand_row_ignored',
             'tail_at_min_k_len')


def _f32(x):
    return np.asarray(x, np.float32)


def _fma(a, b, c):
    return _f32(np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64))


def emu_mixed(case):
    """float32 ``[C, dim]``: the mixed rows as the kernel forms them."""
    f = case.features.numpy()
    lam = np.float32(case.lam)
    if case.ext is None:
        q = f[case.queries.numpy() + case.query_row0]
    else:
        q = np.zeros((case.n_pairs, case.dim), np.float32)
        q[:, :case.q_dim] = case.ext.numpy()
    u = f[np.where(case.anon, 0, case.base.users.numpy())]
    m = _fma(lam, q, _f32(_f32(np.float32(1) - lam) * u))
    return np.where(case.anon[:, None], q, m)


def _chain_tree(x, y, dim):
    """float32 ``[n]``: ``sum_c x[:, c] y[:, c]`` in the kernel's order - per lane one fma chain over its segments, then the shuffle tree.  ``x`` ``[n, dim]``, ``y``
    ``[dim]`` or ``[n, dim]``."""
    g, segs = group_width(dim), (dim + 3) // 4
    steps = (segs + g - 1) // g
    width = steps * g * 4
    xp = np.zeros((x.shape[0], width), np.float32)
    xp[:, :dim] = x
    y = np.broadcast_to(_f32(y), x.shape)
    yp = np.zeros((x.shape[0], width), np.float32)
    yp[:, :dim] = y
    xp, yp = xp.reshape(-1, steps, g, 4), yp.reshape(-1, steps, g, 4)
    acc = np.zeros((x.shape[0], g), np.float32)
    for j in range(steps):
        for t in range(4):
            acc = _fma(xp[:, j, :, t], yp[:, j, :, t], acc)
    lanes = np.arange(g)
    off = g >> 1
    while off >= 1:
        acc = _f32(acc + acc[:, lanes ^ off])
        off >>= 1
    return acc[:, 0]


def emu_run_scores(case, c, cosine, m_row):
    """float32 ``[L]``: the scores of every entry of search c's run under the mixed row ``m_row`` (no gate)."""
    run = case.cand_of(c)
    a = case.features.numpy()[case.item_row0 + run.astype(np.int64)]
    bias = case.bias.numpy()[run]
    if len(run) == 0:
        return np.zeros(0, np.float32)
    dot = _chain_tree(a, m_row, case.dim)
    if not cosine:
        return _f32(dot + bias)
    na = np.maximum(np.sqrt(_chain_tree(a, a, case.dim)), np.float32(EPS))
    nm = np.maximum(np.sqrt(_chain_tree(m_row[None, :], m_row[None, :], case.dim)), np.float32(EPS))[0]
    return _f32(_f32(dot / _f32(na * nm)) + bias)


def emulate(case, k, cosine=False, mutation=None):
    """The whole call: ``(top_scores [C, k] float32, top_items [C, k] int32, passes [C] int32, all_scores [total] float32)``; ``all_scores`` as the entry point
    fills it (a run's slots by its lowest-numbered search)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    mixed = emu_mixed(case)
    ptr, _, total = case.cand_csr()
    flat = np.full(total, NEG_INF, np.float32)
    owner = case.owner_of_run()
    gate = case.gate()
    if mutation == 'excluded_still_ranked':
        gate = np.broadcast_to(np.ones(case.n_items, bool) if case.mask is None else case.mask, gate.shape)
    if mutation == 'mask_bit_of_next_item' and case.mask is not None:
        nxt = np.append(case.mask[1:], False)                              # item i is admitted by the bit of item i + 1
        gate = _not_excluded(case) & nxt[None, :]
    out_s = np.full((case.n_pairs, k), -FLT_MAX, np.float32)
    out_i = np.full((case.n_pairs, k), -1, np.int32)
    passes = np.zeros(case.n_pairs, np.int32)
    for c in range(case.n_pairs):
        r = case.cand_index(c)
        if mutation == 'cand_row_ignored':
            r = c if c < len(case.cand) else -1
        if r < 0:
            continue
        run = case.cand[r]
        if len(run) == 0:
            continue
        probe = case if mutation != 'cand_row_ignored' else _with_rows(case, None)
        s = emu_run_scores(probe, c, cosine, mixed[c])
        if mutation == 'stale_mixed_row' and c > 0:                         # the first chunk of a new run still sees the previous search's row
            s[:CH] = emu_run_scores(probe, c, cosine, mixed[c - 1])[:CH]
        s = np.where(gate[c, run], s, NEG_INF)
        if mutation == 'drop_last_partial_chunk' and len(run) % CH:
            s[len(run) // CH * CH:] = NEG_INF
        if mutation == 'cand_row_ignored' or owner[r] == c:
            flat[ptr[r]:ptr[r + 1]] = s
        keep = s > NEG_INF
        ids, sv = run[keep], s[keep]
        order = np.lexsort((-ids if mutation == 'ties_by_higher_id' else ids, -sv.astype(np.float64)))
        target = min(k, len(order))
        count, boundary = 0, 0                                              # `boundary`: the ranks at or before it are emitted
        while count < target:
            emit = order[boundary:boundary + min(TOP, target - count)]
            out_s[c, count:count + len(emit)], out_i[c, count:count + len(emit)] = sv[emit], ids[emit]
            count += len(emit)
            if mutation != 'boundary_not_advanced':
                boundary += len(emit)
            passes[c] += 1
        if mutation == 'tail_at_min_k_len':                                 # the gated entries fill the row up to min(k, L), as a kernel that counts the run would
            gated = run[~keep][:min(k, len(run)) - target]
            out_s[c, target:target + len(gated)], out_i[c, target:target + len(gated)] = NEG_INF, gated
    return torch.from_numpy(out_s), torch.from_numpy(out_i), torch.from_numpy(passes), torch.from_numpy(flat)


def _not_excluded(case):
    a = np.ones((case.n_pairs, case.n_items), bool)
    for c in range(case.n_pairs):
        a[c, case.run_of(c)] = False
    return a


def _with_rows(case, cand_rows):
    out = object.__new__(CandidateCase)
    out.__dict__.update(case.__dict__)
    out.cand_row_of, out._allowed = cand_rows, None
    return out


# =============================================================================================
# the cases of tests/test_candidates_kernels.py (the host module runs the emulation over the same ones)
# =============================================================================================
N_PAIRS = 70
DIMS = (1, 3, 4, 30, 64, 100, 384, 1280)
KS = (1, 10, 11, 128)


def run_lengths(k, n_items):
    """The lengths a search's run takes in turn (the issue's ladder), cut at the catalogue."""
    return [min(n, n_items) for n in (0, 1, 2, k - 1, k, k + 1, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 1, n_items)]


def runs_by_length(n_pairs, n_items, k, seed=0):
    """One run per search, the ladder of ``run_lengths`` in turn; every other non-empty run holds id 0 or id ``n_items - 1`` (first / last id at the catalogue's edge)."""
    rng = np.random.default_rng([seed, n_pairs, n_items, k])
    lengths = run_lengths(k, n_items)
    runs = []
    for c in range(n_pairs):
        n = max(lengths[c % len(lengths)], 0)
        run = rng.choice(n_items, size=n, replace=False)
        if n and c % 2 == 0:
            edge = 0 if c % 4 == 0 else n_items - 1
            if edge not in run:
                run[0] = edge
        runs.append(np.sort(run))
    return runs


def excl_runs(case_runs, n_items, seed=0):
    """Exclusion runs beside candidate runs: in turn nothing, the run's first id, its last, every other entry, ids that are in no run's neighbourhood, the whole run."""
    rng = np.random.default_rng([seed, len(case_runs), n_items])
    out = []
    for c, run in enumerate(case_runs):
        kind = c % 6
        if kind == 0 or len(run) == 0:
            ex = rng.choice(n_items, size=min(3, n_items), replace=False) if kind == 4 else []
        elif kind == 1:
            ex = run[:1]
        elif kind == 2:
            ex = run[-1:]
        elif kind == 3:
            ex = run[::2]
        elif kind == 4:
            ex = rng.choice(n_items, size=min(7, n_items), replace=False)
        else:
            ex = run
        out.append(np.asarray(ex, np.int64))
    return out


def ext_rows(n_pairs, q_dim, seed):
    ext = np.random.default_rng([seed, n_pairs, q_dim]).standard_normal((n_pairs, q_dim)).astype(np.float32)
    if n_pairs > 1:
        ext[-1] = 0
    return ext


def float_cases(cosine):
    """``(case, k, geometry)`` of the float designs: every width of the issue, every k, 300 items (2,100 at widths 4 and 64, where the ladder reaches 2 CH + 1 and every
    item), plain / excluded / masked / external-row and anonymous in turn."""
    out = []
    for j, dim in enumerate(DIMS):
        design = R.FLOAT_DESIGNS[j % 3]
        n_items = 2100 if dim in (4, 64) else 300
        k = KS[j % 4]
        base = R.float_case(design, N_PAIRS, n_items, dim, R.LAMS_FLOAT[j % 3] if j % 2 else 0.3, seed=j)
        runs = runs_by_length(N_PAIRS, n_items, k, seed=j)
        lists = excl_runs(runs, n_items, seed=j) if j % 2 == 0 else None
        mask = S.mask_pattern('every_other', n_items) if j % 3 == 1 else None
        ext = ext_rows(N_PAIRS, max(1, dim // 2), j) if j % 4 == 2 else None
        anon = np.arange(N_PAIRS) % 3 == 1 if j % 4 >= 2 else None
        out.append((CandidateCase(base, runs, lists=lists, ext=ext, anon=anon, mask=mask), k, 'bcd'[j % 3]))
    return out


EXACT_DOT = ('random', 'all_equal', 'tied_across', 'tie_at_boundary', 'one_list_dec', 'ascending')
EXACT_COSINE = ('all_equal', 'tied_across', 'row_scales')


def exact_cases(cosine):
    """``(case, k, geometry)`` of the exact designs (integer-valued operands, ``LAMS_EXACT``): width 64, 300 items, and one of 2,100."""
    out = []
    for j, design in enumerate(EXACT_COSINE if cosine else EXACT_DOT):
        n_items = 2100 if j == 1 else 300
        k = KS[(j + 1) % 4]
        base = R.exact_case(design, N_PAIRS, n_items, 64, cosine, R.LAMS_EXACT[j % 2])
        runs = runs_by_length(N_PAIRS, n_items, k, seed=100 + j)
        lists = excl_runs(runs, n_items, seed=j) if j % 2 else None
        out.append((CandidateCase(base, runs, lists=lists), k, 'bc'[j % 2]))
    return out


def one_long_run_case(cosine):
    """One run of all 2,100 ids beside 69 empty ones (nine scoring units of one search)."""
    base = R.float_case('randn', N_PAIRS, 2100, 32, 0.3, seed=7)
    runs = [[] for _ in range(N_PAIRS)]
    runs[33] = np.arange(2100)
    return CandidateCase(base, runs), 128, 'b'


def shared_runs_case(cosine, seed=0):
    """Runs shared through ``cand_row``: several searches (of different users) on one run, ``-1`` and an out-of-range row for none, runs that no search names."""
    n_items, k = 300, 11
    base = R.float_case('randn', N_PAIRS, n_items, 100, 0.3, seed=seed)
    shared = runs_by_length(9, n_items, k, seed=seed)[1:] + [np.arange(n_items)]
    rows = np.arange(N_PAIRS) % (len(shared) + 1) - 1                      # -1, 0, 1, ...
    rows[5] = len(shared) + 3                                              # out of range: an empty run
    rows[rows == 2] = 3                                                    # run 2 is named by nobody
    anon = np.arange(N_PAIRS) % 5 == 2
    return CandidateCase(base, shared, cand_rows=rows, anon=anon, lists=excl_runs([shared[r] if 0 <= r < len(shared) else [] for r in rows], n_items, seed)), k, 'c'


def copied(case):
    """The case whose every search has its own copy of its run (null ``cand_row``)."""
    out = CandidateCase(case.base, [case.cand_of(c) for c in range(case.n_pairs)], lists=case.lists if case.has_lists else None, rows=case.row_of,
                        ext=None if case.ext is None else case.ext.numpy(), anon=case.anon, mask=case.mask)
    return out


def all_cases(cosine):
    return float_cases(cosine) + exact_cases(cosine) + [one_long_run_case(cosine), shared_runs_case(cosine)]
