#!/usr/bin/env python3
"""What the ranking losses (``--loss bpr | softmax``) cost against the BCE, from one run on one GPU:

  (1) the loss launch alone at the working point, P = 100 positives with k = 10 (1,100 scores) and k = 15 (1,600 scores): ``ihg_ranking_loss`` (both kinds)
      against ``ihg_bce_with_logits`` on the same scores, and against a torch composition of the same formulas (forward + backward to ``d loss / d scores``);
  (2) one full eager training step of config C3 (d = 128, 3 layers, order 3; forward + backward + Adam) with ``--loss bce | bpr | softmax``, in the same process.

    python tools/loss_bench.py [--rounds 5] [--reps 200] [--step-reps 5] [--no-steps]

Every case is warmed up, then the cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives the
median and the min - max over the rounds.  Nothing is asserted and there is no threshold: the comparison is a record.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_rounds(cases, rounds, reps):
    for run in cases.values():
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for k, run in cases.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                run()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) / reps)
    return times


def show(times, scale=1.0, unit='ms'):
    for k, v in times.items():
        print(f'  {k:<44s} {statistics.median(v) * scale:10.3f}  [{min(v) * scale:.3f} - {max(v) * scale:.3f}] {unit}')


def verdict(times, base, other):
    """Where ``other``'s median sits against ``base``'s min - max spread."""
    lo, hi, med = min(times[base]), max(times[base]), statistics.median(times[other])
    where = 'inside' if lo <= med <= hi else (f'{(med / hi - 1) * 100:.1f} % above' if med > hi else f'{(1 - med / lo) * 100:.1f} % below')
    print(f'  {other}: median is {where} the spread of {base}; ratio of medians {med / statistics.median(times[base]):.3f}')


def composition(kind, scores, positives):
    """The formulas as torch ops in float32 (what a user without the launch would write)."""
    sp, neg = scores[:positives], scores[positives:].view(positives, -1)
    if kind == 'bpr':
        return torch.nn.functional.softplus(neg - sp[:, None]).mean()
    return (torch.logsumexp(torch.cat([sp[:, None], neg], 1), 1) - sp).mean()


def launches(rounds, reps):
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device('cuda:0')
    P = 100
    for k in (10, 15):
        n = P * (1 + k)
        gen = torch.Generator().manual_seed(k)
        scores = torch.randn(n, generator=gen).to(dev)
        labels = torch.cat([torch.ones(P), torch.zeros(P * k)]).to(dev)
        loss, dscores = torch.empty((), device=dev), torch.empty(n, device=dev)
        leaf = scores.clone().requires_grad_(True)

        def bce():
            _lib.check(lib.ihg_bce_with_logits(ops._ptr(scores), ops._ptr(labels), n, ops._ptr(loss), ops._ptr(dscores), ops._stream()), 'ihg_bce_with_logits')

        def ranking(code):
            def run():
                _lib.check(lib.ihg_ranking_loss(ops._ptr(scores), P, k, code, ops._ptr(loss), ops._ptr(dscores), ops._stream()), 'ihg_ranking_loss')
            return run

        def composed(kind):
            def run():
                leaf.grad = None
                composition(kind, leaf, P).backward()
            return run

        def bce_composed():
            leaf.grad = None
            torch.nn.functional.binary_cross_entropy_with_logits(leaf, labels).backward()

        cases = {'ihg_bce_with_logits': bce, 'ihg_ranking_loss bpr': ranking(_lib.LOSS_KINDS['bpr']), 'ihg_ranking_loss softmax': ranking(_lib.LOSS_KINDS['softmax']),
                 'torch composition bce': bce_composed, 'torch composition bpr': composed('bpr'), 'torch composition softmax': composed('softmax')}
        times = timed_rounds(cases, rounds, reps)
        print(f'(1) loss + d loss / d scores, P = {P}, k = {k} ({n} scores); microseconds per call (back-to-back launches on one stream), median [min - max] over {rounds} rounds of {reps}')
        show(times, 1e3, 'us')
        verdict(times, 'ihg_bce_with_logits', 'ihg_ranking_loss bpr')
        verdict(times, 'ihg_bce_with_logits', 'ihg_ranking_loss softmax')


def steps(rounds, reps):
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    from ihgnn_amd.optim import Adam
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS['C3']
    w = synth.draw_config('C3')
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, graph_type=PpsHyperGraph, device=dev)
    u, q, i, y = next(iter(ds.sample_batches(Gs.batch_size, 1, seed=1)))
    torch.manual_seed(0)
    model = RawGnn(dev, ds, cfg['dim'], IHGNNLayer, cfg['layers'], 3, False, HemPredictionLayer, 0.5).to(dev)
    opt = Adam(model.parameters(), 1e-3, weight_decay=0)

    def step(kind):
        def run():
            loss = model.bce_loss(u, q, i, y) if kind == 'bce' else model.ranking_loss(u, q, i, Gs.batch_size, kind)
            loss.backward(); opt.step(); opt.zero_grad()
        return run

    times = timed_rounds({f'step --loss {kind}': step(kind) for kind in ('bce', 'bpr', 'softmax')}, rounds, reps)
    print(f'(2) C3 full eager training step (d = {cfg["dim"]}, {cfg["layers"]} layers, {u.shape[0]} batch rows); ms, median [min - max] over {rounds} rounds of {reps}')
    show(times)
    verdict(times, 'step --loss bce', 'step --loss bpr')
    verdict(times, 'step --loss bce', 'step --loss softmax')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200, help='calls per round of the loss launches')
    ap.add_argument('--step-reps', type=int, default=5, help='steps per round of the full training step')
    ap.add_argument('--no-steps', action='store_true', help='the launches only')
    args = ap.parse_args()
    launches(args.rounds, args.reps)
    if not args.no_steps:
        steps(args.rounds, args.step_reps)


if __name__ == '__main__':
    main()
