#!/usr/bin/env python3
"""What ranking deeper than ten costs (``ihg_score_topk_deep``, ``RawGnn.top_items(u, q, k)`` with k > 10, ``--cutoffs``), from one run on one GPU:

  (1) at config C3's catalogue (120,000 items, D = 384, 4,096 pairs): ``ihg_score_topk`` at k = 10; the deep call on random features at k = 10, 20, 50, 100 and
      128; the deep call at k = 128 on its worst case (zero user and query rows, bias descending in item id: every pass finds its winners in the first lists);
      and the torch route that served k > 10 before - the dense scores of ``RawGnn.score_all_items`` in chunks of pairs + ``torch.topk`` - restated here so that
      both sides run on one build.  The deep call is reported as a ratio to the k = 10 call of the same run, with the passes it took;
  (2) an evaluation pass (``TrainTestHelper._evaluate_batched``: ranking, one copy to the host, the metrics in Python) over 200 logs x 120,000 items with and
      without ``--cutoffs 100``, on a stand-in model that ranks a random feature matrix (no graph is built: the pass does not touch one).

    python tools/topk_bench.py [--rounds 5] [--reps 5] [--logs 200] [--base-only [--tree DIR]]

``--base-only``: the k = 10 call alone - run it alternately for two builds to see whether the k = 10 call moved.  ``--tree DIR`` imports ``ihgnn_amd`` (and its
built library) from another checkout: a library from before ``ihg_score_topk_deep`` lacks symbols this package binds, so ``IHGNN_HIP_LIBRARY`` alone cannot load it.

Every case is warmed up, then the cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives the
median and the min - max over the rounds, in ms.
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.cosine_bench import show, timed_rounds  # noqa: E402

if '--tree' in sys.argv[1:-1]:                                             # in front of this checkout, before anything imports ihgnn_amd
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index('--tree') + 1]))

DEPTHS = (10, 20, 50, 100, 128)


def catalogue(dev):
    from ihgnn_amd import synth
    cfg = synth.CONFIGS['C3']
    n_items, dim, pairs, Uc, Qc = cfg['item_count'], 384, 4096, 5000, 2000
    gen = torch.Generator().manual_seed(1)
    feats = (torch.randn(Uc + Qc + n_items, dim, generator=gen) / dim ** 0.5).to(dev)
    bias = (0.1 * torch.randn(n_items, generator=gen)).to(dev)
    users, queries = torch.randint(0, Uc, (pairs,), generator=gen).to(dev), torch.randint(0, Qc, (pairs,), generator=gen).to(dev)
    return feats, bias, users, queries, Uc, Qc, n_items, dim, pairs


def launches(rounds, reps, base_only):
    from ihgnn_amd import _lib, ops
    dev = torch.device('cuda:0')
    feats, bias, users, queries, Uc, Qc, n_items, dim, pairs = catalogue(dev)
    base = 'score_topk k = 10'
    cases = {base: lambda: ops.score_topk(feats, users, queries, Uc, Uc + Qc, bias, 0.5, 10)}
    print(f'library: {_lib.LIB_PATH}')
    if base_only:
        times = timed_rounds(cases, rounds, reps)
        print(f'(1) {pairs} pairs x {n_items:,} items, D = {dim}; ms, median [min - max] over {rounds} rounds of {reps}')
        show(times)
        return
    worst_feats = feats.clone()
    worst_feats[:Uc + Qc] = 0
    worst_bias = -torch.arange(n_items, dtype=torch.float32, device=dev)
    passes = {}

    def deep(name, f, b, k):
        def run():
            passes[name] = ops.score_topk_deep(f, users, queries, Uc, Uc + Qc, b, 0.5, k)[2]
        return run

    for k in DEPTHS:
        cases[f'score_topk_deep k = {k}'] = deep(f'score_topk_deep k = {k}', feats, bias, k)
    worst = 'score_topk_deep k = 128, sorted bias'
    cases[worst] = deep(worst, worst_feats, worst_bias, 128)

    def dense(k, chunk=1024):
        # RawGnn.score_all_items + torch.topk, a chunk of pairs at a time (the whole [C, I] matrix is 1.9 GB)
        def run():
            items = feats[Uc + Qc:]
            for lo in range(0, pairs, chunk):
                mixed = 0.5 * feats[queries[lo:lo + chunk] + Uc] + 0.5 * feats[users[lo:lo + chunk]]
                torch.topk(torch.addmm(bias.unsqueeze(0), mixed, items.t()), k, dim=1, largest=True, sorted=True)
        return run

    for k in (10, 128):
        cases[f'torch dense scores + topk, k = {k}'] = dense(k)
    times = timed_rounds(cases, rounds, reps)
    print(f'(1) {pairs} pairs x {n_items:,} items, D = {dim}; ms, median [min - max] over {rounds} rounds of {reps}')
    show(times)
    med = {name: statistics.median(v) for name, v in times.items()}
    for name in cases:
        if name in passes:
            p = passes[name]
            print(f'  {name:<40s} {med[name] / med[base]:6.2f} x the k = 10 call; passes per pair: max {int(p.max())}, mean {float(p.float().mean()):.2f}')
    print(f'  torch route / deep call at k = 128: {med["torch dense scores + topk, k = 128"] / med["score_topk_deep k = 128"]:.1f} x')


class RankedCatalogue:
    """What ``_evaluate_batched`` asks of a model: ``top_items`` over a cached feature matrix."""

    def __init__(self, feats, bias, query_row0, item_row0):
        self.feats, self.bias, self.query_row0, self.item_row0 = feats, bias, query_row0, item_row0

    def top_items(self, users, queries, k=10):
        from ihgnn_amd import ops
        return ops.score_topk(self.feats, users, queries, self.query_row0, self.item_row0, self.bias, 0.5, k)


def evaluation(rounds, n_logs):
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Helpers.TrainTestHelper import _evaluate_batched
    dev = torch.device('cuda:0')
    feats, bias, _, _, Uc, Qc, n_items, dim, _ = catalogue(dev)
    gen = torch.Generator().manual_seed(2)
    logs = [(int(torch.randint(0, Uc, (1,), generator=gen)), int(torch.randint(0, Qc, (1,), generator=gen)),
             torch.randint(0, n_items, (5,), generator=gen).tolist(), None, True) for _ in range(n_logs)]
    model = RankedCatalogue(feats, bias, Uc, Uc + Qc)
    old = Gs.Evaluation.extra_cutoffs

    def run(cutoffs):
        def go():
            Gs.Evaluation.extra_cutoffs = cutoffs
            _evaluate_batched(model, logs, n_items, dev, list(range(n_logs)))
        return go

    try:
        times = timed_rounds({'evaluation pass, @10 only': run(()), 'evaluation pass, --cutoffs 100': run((100,))}, rounds, 1)
    finally:
        Gs.Evaluation.extra_cutoffs = old
    print(f'(2) evaluation pass over {n_logs} logs x {n_items:,} items, D = {dim} (features cached); ms, median [min - max] over {rounds} rounds of 1')
    show(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--logs', type=int, default=200, help='logs of the evaluation pass in (2)')
    ap.add_argument('--base-only', action='store_true', help='the k = 10 call alone (for a comparison of two builds)')
    ap.add_argument('--tree', default='', help='with --base-only: the checkout to import ihgnn_amd from (default: this one)')
    args = ap.parse_args()
    if args.tree and not args.base_only:
        ap.error('--tree goes with --base-only')
    launches(args.rounds, args.reps, args.base_only)
    if not args.base_only:
        evaluation(args.rounds, args.logs)


if __name__ == '__main__':
    main()
