#!/usr/bin/env python3
"""What answering a search costs (``ihg_search_topk``, ``ops.search_topk``, the bag path of ``RawGnn.search``), from one run on one GPU, at config C3's catalogue
(120,000 items, D = 384 = a 128-wide embedding and three layers; a 30,000-word table) for batches of 1, 64 and 4,096 searches at k = 10:

    top_items by index       ``ops.score_topk`` (``ihg_score_topk``): what ``RawGnn.top_items`` launches for the same pairs
    search by index          ``ops.search_topk(queries=)``: the deep kernels at k = 10 plus the target launch
    search by bag            what ``RawGnn.search(words=, offsets=)`` does per call behind its checks: the ad-hoc ``ops.BagLayout`` (built on the HOST: numpy and two
                             small copies), the bag mean launch, ``ops.search_topk(query_rows=)``
    bag layout / bag mean / bag mean + transform     its parts, one at a time (the transform: ``ihg_rows_linear_act_fwd`` at d = 128)
    search on rows           ``ops.search_topk(query_rows=)`` alone
    anonymous                the same with every user -1
    mask 100 % / 10 % / 1 %  ``candidates=`` a bool [I] tensor on the device (packed by torch ops inside the call) with that share of the items set

No graph and no model are built: the scoring does not touch one (a random feature matrix stands in, as in ``tools/topk_bench.py``).  Every case is warmed up, then the
cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives the median and the min - max over the
rounds, in ms.  Nothing is asserted on these figures.

    python tools/search_bench.py [--rounds 5] [--reps 5] [--batches 1,64,4096]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.cosine_bench import show, timed_rounds  # noqa: E402

EMB, LAYERS, K = 128, 3, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batches', default='1,64,4096')
    args = ap.parse_args()
    from ihgnn_amd import _lib, ops, synth
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS['C3']
    n_items, vocab, dim, Uc, Qc = cfg['item_count'], cfg['vocab_size'], EMB * LAYERS, 5000, 2000
    gen = torch.Generator().manual_seed(1)
    feats = (torch.randn(Uc + Qc + n_items, dim, generator=gen) / dim ** 0.5).to(dev)
    bias = (0.1 * torch.randn(n_items, generator=gen)).to(dev)
    table = (torch.randn(vocab + 1, EMB, generator=gen) / EMB ** 0.5).to(dev)
    wq, bq = (torch.randn(EMB, EMB, generator=gen) / EMB ** 0.5).to(dev), (0.1 * torch.randn(EMB, generator=gen)).to(dev)
    masks = {share: (torch.rand(n_items, generator=gen) < share).to(dev) if share < 1 else torch.ones(n_items, dtype=torch.bool, device=dev) for share in (1.0, 0.1, 0.01)}
    print(f'library: {_lib.LIB_PATH}')
    rng = np.random.default_rng(2)
    for pairs in (int(b) for b in args.batches.split(',')):
        users = torch.randint(0, Uc, (pairs,), generator=gen).to(dev)
        queries = torch.randint(0, Qc, (pairs,), generator=gen).to(dev)
        nobody = torch.full_like(users, -1)
        lens = rng.integers(1, 6, pairs)
        words = rng.integers(1, vocab + 1, int(lens.sum())).astype(np.int64)                       # (stored ids: row 0 of the table is padding)
        offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        bag = ops.BagLayout(words, offsets, vocab + 1, dev)
        with torch.no_grad():
            rows = ops.bag_mean(table, bag)
        search = lambda **kw: ops.search_topk(feats, kw.pop('users', users), Uc, Uc + Qc, bias, 0.5, K, **kw)

        def by_bag():
            layout = ops.BagLayout(words, offsets, vocab + 1, dev)
            search(query_rows=ops.bag_mean(table, layout))

        cases = {
            'top_items by index (ihg_score_topk)': lambda: ops.score_topk(feats, users, queries, Uc, Uc + Qc, bias, 0.5, K),
            'search by index': lambda: search(queries=queries),
            'search by bag (layout + mean + search)': by_bag,
            '  bag layout (host)': lambda: ops.BagLayout(words, offsets, vocab + 1, dev),
            '  bag mean': lambda: ops.bag_mean(table, bag),
            '  bag mean + transform': lambda: ops.bag_mean(table, bag, wq, bq, 'relu'),
            '  search on rows': lambda: search(query_rows=rows),
            'search on rows, anonymous': lambda: search(query_rows=rows, users=nobody),
        }
        for share, mask in masks.items():
            cases[f'search on rows, mask {share:.0%}'] = (lambda m: lambda: search(query_rows=rows, candidates=m))(mask)
        with torch.no_grad():
            times = timed_rounds(cases, args.rounds, args.reps)
        print(f'{pairs} searches x {n_items:,} items, D = {dim} (q_dim = {EMB}), k = {K}; ms, median [min - max] over {args.rounds} rounds of {args.reps}')
        show(times)


if __name__ == '__main__':
    main()
