#!/usr/bin/env python3
"""What re-ranking a shortlist per search costs (``ihg_search_candidates``, ``RawGnn.search(candidate_lists=)``, ``--eval_candidates``), from one run on one GPU:

  (1) at config C3's catalogue (120,000 items, D = 384) with 4,096 searches and lists of 100 / 1,000 / 10,000 ids each (uniform draws, prepared once by
      ``ops.candidate_lists``, which is timed on its own): ``ops.search_candidates`` at k = 10 against
        (a) ``ops.search_topk`` over the whole catalogue for the same searches (what a caller without per-search lists would launch once per distinct list, so (a) is
            the cost of ONE such call, a lower bound of that route), and
        (b) the flattened route: ``RawGnn.forward(u, q, i)`` over every (search, candidate) triple, restated in torch on the cached features (a gather of the three
            rows per triple and a row-wise dot product), followed by a segmented top-k (the lists have one length here: ``torch.topk`` over ``[C, L]``), in chunks of
            searches that keep the gathered rows under 1 GB;
  (2) one evaluation pass (``TrainTestHelper._evaluate_batched``) over ``--logs`` logs with ``--eval_candidates 99`` against the plain pass over the whole catalogue,
      on a stand-in model that ranks a random feature matrix (no graph is built: the pass does not touch one); the sets are built before the clock starts, as the
      driver builds them once per run.

    python tools/candidates_bench.py [--rounds 5] [--reps 3] [--logs 2000]

Every case is warmed up, then the cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives the
median and the min - max over the rounds, in ms.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.cosine_bench import show, timed_rounds  # noqa: E402
from tools.topk_bench import catalogue  # noqa: E402

LENGTHS = (100, 1000, 10000)


def launches(rounds, reps):
    from ihgnn_amd import _lib, ops
    dev = torch.device('cuda:0')
    feats, bias, users, queries, Uc, Qc, n_items, dim, pairs = catalogue(dev)
    print(f'library: {_lib.LIB_PATH}')
    gen = torch.Generator().manual_seed(3)
    cases, prep = {}, {}
    cases['(a) search_topk, whole catalogue'] = lambda: ops.search_topk(feats, users, Uc, Uc + Qc, bias, 0.5, 10, queries=queries)
    for length in LENGTHS:
        raw = torch.randint(0, n_items, (pairs, length), generator=gen).to(dev)
        offsets = torch.arange(pairs + 1, dtype=torch.int64, device=dev) * length
        lists = ops.candidate_lists(offsets, raw.reshape(-1), n_items)
        prep[f'candidate_lists of {pairs} x {length:,} raw ids'] = (lambda o=offsets, r=raw: ops.candidate_lists(o, r.reshape(-1), n_items))
        cases[f'search_candidates, {length:,} ids per search'] = (lambda l=lists: ops.search_candidates(feats, users, Uc, Uc + Qc, bias, 0.5, 10, lists=l, queries=queries))
        chunk = max(1, min(pairs, (1 << 28) // (length * dim)))

        def flattened(r=raw, chunk=chunk, length=length):
            for lo in range(0, pairs, chunk):
                ids = r[lo:lo + chunk]
                mixed = 0.5 * feats[queries[lo:lo + chunk] + Uc] + 0.5 * feats[users[lo:lo + chunk]]
                scores = (feats[ids.reshape(-1) + Uc + Qc].view(ids.shape[0], length, dim) * mixed.unsqueeze(1)).sum(2) + bias[ids]
                torch.topk(scores, 10, dim=1, largest=True, sorted=True)

        cases[f'(b) flattened forward + top-k, {length:,} ids'] = flattened
    times = timed_rounds(cases, rounds, reps)
    print(f'(1) {pairs} searches, {n_items:,} items, D = {dim}, k = 10; ms, median [min - max] over {rounds} rounds of {reps}')
    show(times)
    med = {name: statistics.median(v) for name, v in times.items()}
    base = med['(a) search_topk, whole catalogue']
    for length in LENGTHS:
        mine = med[f'search_candidates, {length:,} ids per search']
        gb = pairs * length * dim * 4 / 1e9
        print(f'  {length:>6,} ids: {mine / base:6.3f} x (a), (b) is {med[f"(b) flattened forward + top-k, {length:,} ids"] / mine:5.1f} x the list call; '
              f'{gb / (mine * 1e-3):7.0f} GB/s of gathered item rows')
    show(timed_rounds(prep, rounds, reps))


class RankedCatalogue:
    """What ``_evaluate_batched`` asks of a model: ``top_items`` over a cached feature matrix."""

    def __init__(self, feats, bias, query_row0, item_row0):
        self.feats, self.bias, self.query_row0, self.item_row0 = feats, bias, query_row0, item_row0

    def top_items(self, users, queries, k=10, exclude=None, candidate_lists=None):
        from ihgnn_amd import ops
        if candidate_lists is not None:
            return ops.search_candidates(self.feats, users, self.query_row0, self.item_row0, self.bias, 0.5, k, lists=candidate_lists, queries=queries)[:2]
        return ops.score_topk(self.feats, users, queries, self.query_row0, self.item_row0, self.bias, 0.5, k)


def evaluation(rounds, n_logs):
    from ihgnn_amd.Helpers.TrainTestHelper import SampledCandidates, _evaluate_batched
    dev = torch.device('cuda:0')
    feats, bias, _, _, Uc, Qc, n_items, dim, _ = catalogue(dev)
    rng = np.random.default_rng(2)
    logs = [(int(rng.integers(0, Uc)), int(rng.integers(0, Qc)), rng.integers(0, n_items, 5).tolist(), None, True) for _ in range(n_logs)]
    model = RankedCatalogue(feats, bias, Uc, Uc + Qc)
    indices = list(range(n_logs))
    sampled = SampledCandidates(logs, indices, n_items, 99, 0)
    times = timed_rounds({'evaluation pass, whole catalogue': lambda: _evaluate_batched(model, logs, n_items, dev, indices),
                          'evaluation pass, --eval_candidates 99': lambda: _evaluate_batched(model, logs, n_items, dev, indices, None, sampled)}, rounds, 1)
    print(f'(2) evaluation pass over {n_logs} logs, {n_items:,} items, D = {dim} (features cached, sets built beforehand); ms, median [min - max] over {rounds} rounds of 1')
    show(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--logs', type=int, default=2000, help='logs of the evaluation pass in (2)')
    args = ap.parse_args()
    launches(args.rounds, args.reps)
    evaluation(args.rounds, args.logs)


if __name__ == '__main__':
    main()
