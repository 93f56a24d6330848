#!/usr/bin/env python3
"""What hard negatives (``--hard_negatives M``) cost against the plain step, from one run on one GPU:

  (1) the two new launches alone at the working point, P = 100 positives, k = 10 kept, M in {20, 50, 100}: ``ihg_sample_pool`` against ``ihg_sample_negatives`` (k = 10),
      and ``ihg_hard_negative_loss`` (three kinds) against ``ihg_bce_with_logits`` / ``ihg_ranking_loss`` on the P (1 + k) scores of a plain batch;
  (2) one full eager training step of config C3 (d = 128, 3 layers, order 3; forward + backward + Adam) under ``--loss bpr`` with the pool at M in {20, 50, 100}
      (``RawGnn.hard_negative_loss``), against the plain step with k = 10 uniform negatives (``RawGnn.ranking_loss``: the code path as it was before hard negatives), in
      the same process.

    python tools/hard_negatives_bench.py [--rounds 5] [--reps 200] [--step-reps 5] [--no-steps]

Every case is warmed up, then the cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives the
median and the min - max over the rounds.  Nothing is asserted and there is no threshold: the comparison is a record.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from loss_bench import show, timed_rounds, verdict                        # noqa: E402  (the timing scheme of tools/loss_bench.py)

POOLS = (20, 50, 100)
P, KEEP = 100, 10


def launches(rounds, reps):
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device('cuda:0')
    n_items = 100000
    drawn = {m: torch.empty(P, m, dtype=torch.int64, device=dev) for m in POOLS + (KEEP,)}

    def negatives():
        _lib.check(lib.ihg_sample_negatives(1, 2, P, n_items, KEEP, ops._ptr(drawn[KEEP]), ops._stream()), 'ihg_sample_negatives')

    def pool(m):
        def run():
            _lib.check(lib.ihg_sample_pool(1, 2, P, n_items, m, ops._ptr(drawn[m]), ops._stream()), 'ihg_sample_pool')
        return run

    cases = {f'ihg_sample_negatives k = {KEEP}': negatives}
    cases.update({f'ihg_sample_pool M = {m}': pool(m) for m in POOLS})
    times = timed_rounds(cases, rounds, reps)
    print(f'(1a) negatives of {P} positives from {n_items} items; microseconds per call (back-to-back launches on one stream), median [min - max] over {rounds} rounds of {reps}')
    show(times, 1e3, 'us')

    gen = torch.Generator().manual_seed(0)
    plain = torch.randn(P * (1 + KEEP), generator=gen).to(dev)
    labels = torch.cat([torch.ones(P), torch.zeros(P * KEEP)]).to(dev)
    loss, selected = torch.empty((), device=dev), torch.empty(P, KEEP, dtype=torch.int32, device=dev)
    wide = {m: torch.randn(P * (1 + m), generator=gen).to(dev) for m in POOLS}
    dscores = torch.empty(P * (1 + max(POOLS)), device=dev)

    def bce():
        _lib.check(lib.ihg_bce_with_logits(ops._ptr(plain), ops._ptr(labels), plain.numel(), ops._ptr(loss), ops._ptr(dscores), ops._stream()), 'ihg_bce_with_logits')

    def ranking(code):
        def run():
            _lib.check(lib.ihg_ranking_loss(ops._ptr(plain), P, KEEP, code, ops._ptr(loss), ops._ptr(dscores), ops._stream()), 'ihg_ranking_loss')
        return run

    def hard(code, m):
        def run():
            _lib.check(lib.ihg_hard_negative_loss(ops._ptr(wide[m]), P, m, KEEP, code, ops._ptr(loss), ops._ptr(dscores), ops._ptr(selected), ops._stream()), 'ihg_hard_negative_loss')
        return run

    cases = {'ihg_bce_with_logits': bce, 'ihg_ranking_loss bpr': ranking(1), 'ihg_ranking_loss softmax': ranking(2)}
    for kind, code in _lib.HARD_NEGATIVE_KINDS.items():
        cases.update({f'ihg_hard_negative_loss {kind} M = {m}': hard(code, m) for m in POOLS})
    times = timed_rounds(cases, rounds, reps)
    print(f'(1b) loss + d loss / d scores, P = {P}, k = {KEEP}; microseconds per call, median [min - max] over {rounds} rounds of {reps}')
    show(times, 1e3, 'us')
    for m in POOLS:
        verdict(times, 'ihg_ranking_loss bpr', f'ihg_hard_negative_loss bpr M = {m}')


def steps(rounds, reps):
    from ihgnn_amd import ops, synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    from ihgnn_amd.optim import Adam
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS['C3']
    w = synth.draw_config('C3')
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, graph_type=PpsHyperGraph, device=dev)
    torch.manual_seed(0)
    model = RawGnn(dev, ds, cfg['dim'], IHGNNLayer, cfg['layers'], 3, False, HemPredictionLayer, 0.5).to(dev)
    opt = Adam(model.parameters(), 1e-3, weight_decay=0)
    pos = torch.from_numpy(ds.pos_triples[torch.randint(0, len(ds), (P,), generator=torch.Generator().manual_seed(1)).numpy()]).to(dev)

    def batch(per_positive):
        items = ops.sample_pool(3, per_positive, P, ds.item_count, per_positive, device=dev)
        return (torch.cat([pos[:, 0], pos[:, 0].repeat_interleave(per_positive)]), torch.cat([pos[:, 1], pos[:, 1].repeat_interleave(per_positive)]),
                torch.cat([pos[:, 2], items.reshape(-1)]))

    batches = {m: batch(m) for m in POOLS + (KEEP,)}

    def plain():
        loss = model.ranking_loss(*batches[KEEP], P, 'bpr')
        loss.backward(); opt.step(); opt.zero_grad()

    def hard(m):
        def run():
            loss = model.hard_negative_loss(*batches[m], P, KEEP, 'bpr')
            loss.backward(); opt.step(); opt.zero_grad()
        return run

    base = f'plain step, k = {KEEP} uniform negatives'
    cases = {base: plain}
    cases.update({f'hard negatives, best {KEEP} of M = {m}': hard(m) for m in POOLS})
    times = timed_rounds(cases, rounds, reps)
    print(f'(2) C3 full eager training step --loss bpr (d = {cfg["dim"]}, {cfg["layers"]} layers, {P} positives); ms, median [min - max] over {rounds} rounds of {reps}')
    show(times)
    for m in POOLS:
        verdict(times, base, f'hard negatives, best {KEEP} of M = {m}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200, help='calls per round of the launches')
    ap.add_argument('--step-reps', type=int, default=5, help='steps per round of the full training step')
    ap.add_argument('--no-steps', action='store_true', help='the launches only')
    args = ap.parse_args()
    launches(args.rounds, args.reps)
    if not args.no_steps:
        steps(args.rounds, args.step_reps)


if __name__ == '__main__':
    main()
