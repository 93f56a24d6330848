#!/usr/bin/env python3
"""What per-search exclusion lists cost (``ihg_search_topk_excluding``, ``ops.search_topk(exclude=)``), from one run on one GPU, at ``tools/search_bench.py``'s shape:
config C3's catalogue (120,000 items, D = 384) and a batch of 4,096 searches by query index, at k = 10 and k = 100:

    search, no lists           ``ops.search_topk`` as before (``ihg_search_topk``)
    exclude 0 / 16 / 500 ids   ``ops.search_topk(exclude=(ptr, items))`` with that many random ids per search, normalised once outside the timed region
                               (0: every run empty - the cost of the cursor's one comparison per group of four items and of the per-pair target)
    exclude 500 ids, shared    the same ids as 64 runs shared by all searches through ``exclude_rows=`` (the ``exclude_seen`` route: one CSR, no copy per search)
    normalise 500 ids          ``ops.exclusion_lists`` alone on the raw 4,096 x 500 ids (what a caller with raw lists pays besides)
    dense alternative          what one did without the entry point: the ``[C, I]`` scores (``RawGnn.score_all_items``'s ``addmm``), ``masked_fill`` with a ``[C, I]``
                               bool matrix of the 500-id lists (built outside the timed region) and ``torch.topk`` - 1.9 GB of scores and 0.5 GB of mask

No graph and no model are built (a random feature matrix stands in, as in ``tools/search_bench.py``).  Every case is warmed up, then the cases are timed in interleaved
rounds (each round runs every case ``reps`` times between two HIP events); the table gives the median and the min - max over the rounds, in ms.  Nothing is asserted
on these figures.

    python tools/exclude_bench.py [--rounds 5] [--reps 5] [--pairs 4096]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.cosine_bench import show, timed_rounds  # noqa: E402

EMB, LAYERS = 128, 3
SHARED_RUNS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--pairs', type=int, default=4096)
    args = ap.parse_args()
    from ihgnn_amd import _lib, ops, synth
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS['C3']
    n_items, dim, Uc, Qc, pairs, lam = cfg['item_count'], EMB * LAYERS, 5000, 2000, args.pairs, 0.5
    gen = torch.Generator().manual_seed(1)
    feats = (torch.randn(Uc + Qc + n_items, dim, generator=gen) / dim ** 0.5).to(dev)
    bias = (0.1 * torch.randn(n_items, generator=gen)).to(dev)
    users = torch.randint(0, Uc, (pairs,), generator=gen).to(dev)
    queries = torch.randint(0, Qc, (pairs,), generator=gen).to(dev)
    print(f'library: {_lib.LIB_PATH}')

    def lists(rows, per_row):
        """``rows`` runs of ``per_row`` random ids: the raw ``(offsets, ids)`` and their normal form, on the device."""
        ids = torch.randint(0, n_items, (rows * per_row,), generator=gen).to(dev)      # (drawn with repeats: a run of 500 keeps about 499 distinct ids)
        offsets = torch.arange(rows + 1, dtype=torch.int64, device=dev) * per_row
        return (offsets, ids), ops.exclusion_lists(offsets, ids, n_items)

    per_pair = {n: lists(pairs, n) for n in (0, 16, 500)}
    shared = lists(SHARED_RUNS, 500)[1]
    shared_rows = torch.randint(0, SHARED_RUNS, (pairs,), generator=gen).to(dev)
    raw_offsets, raw_ids = per_pair[500][0]
    excluded = torch.zeros(pairs, n_items, dtype=torch.bool, device=dev)
    excluded[torch.arange(pairs, device=dev).repeat_interleave(500), raw_ids] = True
    items_t = feats[Uc + Qc:].t().contiguous()

    def dense(k):
        mixed = lam * feats[queries + Uc] + (1 - lam) * feats[users]
        scores = torch.addmm(bias.unsqueeze(0), mixed, items_t)
        return torch.topk(scores.masked_fill_(excluded, float('-inf')), k, dim=1)

    for k in (10, 100):
        search = lambda **kw: ops.search_topk(feats, users, Uc, Uc + Qc, bias, lam, k, queries=queries, **kw)
        cases = {'search, no lists': search}
        for n, (_, normal) in per_pair.items():
            cases[f'exclude {n} ids per search'] = (lambda e: lambda: search(exclude=e))(normal)
        cases['exclude 500 ids, 64 shared runs'] = lambda: search(exclude=shared, exclude_rows=shared_rows)
        cases[f'normalise {pairs:,} x 500 raw ids'] = lambda: ops.exclusion_lists(raw_offsets, raw_ids, n_items)
        cases['dense: addmm + masked_fill + topk'] = lambda: dense(k)
        with torch.no_grad():
            times = timed_rounds(cases, args.rounds, args.reps)
        print(f'{pairs} searches x {n_items:,} items, D = {dim}, k = {k}; ms, median [min - max] over {args.rounds} rounds of {args.reps}')
        show(times)


if __name__ == '__main__':
    main()
