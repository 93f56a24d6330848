#!/usr/bin/env python3
"""What popularity-weighted negatives (``--popularity_negatives``, exponent 0.75) cost against the uniform draws, from one run on one GPU:

  (1) the new launch alone at the working point, P = 100 positives of config C3, m in {10, 20, 50, 100}: ``ihg_sample_pool_weighted`` without lists against
      ``ihg_sample_pool``, and with the users' real training lists against ``ihg_sample_pool_excluding`` - the binary search over ``cum`` is the difference in both pairs;
  (2) one full eager training step of config C3 (d = 128, 3 layers, order 3; the device loader's batch + forward + backward + Adam) with and without the flag, under the
      plain loss (BCE, k = 10 negatives) and under ``--hard_negatives 50 --loss bpr`` (the best 10 of a pool of 50), in the same process.  A step draws its own batch
      from ``GraphDataset.device_batches``, so the sampling launch and the torch launches around it are inside the timed region.

    python tools/popularity_negatives_bench.py [--rounds 5] [--reps 200] [--step-reps 5] [--no-steps]

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

DRAWS = (10, 20, 50, 100)
P, KEEP, POOL, ALPHA = 100, 10, 50, 0.75


def c3_dataset():
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    w = synth.draw_config('C3')
    return GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, graph_type=PpsHyperGraph,
                                    device=torch.device('cuda:0'), popularity_power=ALPHA)


def launches(ds, rounds, reps):
    from ihgnn_amd import Main, _lib, ops
    lib = _lib.load()
    dev = torch.device('cuda:0')
    n_items = ds.item_count
    pick = torch.randint(0, len(ds), (P,), generator=torch.Generator().manual_seed(1)).numpy()
    users = torch.from_numpy(ds.pos_triples[pick, 0].copy()).to(dev)
    ptr, items = ds.user_item_lists_on(dev)
    cum, total = ds.item_sampling_table_on(dev)
    longest = ds.max_user_items
    shares = Main.popularity_shares(ds)
    print(f'C3 weights (exponent {ALPHA}): {n_items} items, table of {cum.numel() * 8} bytes, sum {total}; {100 * shares["head_share"]:.2f} % of draws on the '
          f'{shares["head_items"]} most popular items; {100 * shares["own_item_share"]:.4f} % of weighted draws would be an item of their own user '
          f'(uniform: {100 * Main.own_item_share(ds):.4f} %); longest user list {longest} items')
    for filtered in (False, True):
        ds.filter_negatives = filtered
        for m in DRAWS:
            try:
                Main.check_popularity_negatives(ds, m)
            except ValueError as refused:
                print(f'(the driver\'s mass policy would refuse m = {m}{" with the lists" if filtered else ""}: {refused})')
    ds.filter_negatives = False
    drawn = {m: torch.empty(P, m, dtype=torch.int64, device=dev) for m in DRAWS}

    def pool(m):
        def run():
            _lib.check(lib.ihg_sample_pool(1, 2, P, n_items, m, ops._ptr(drawn[m]), ops._stream()), 'ihg_sample_pool')
        return run

    def excluding(m):
        def run():
            _lib.check(lib.ihg_sample_pool_excluding(1, 2, P, n_items, m, ops._ptr(users), ds.user_count, ops._ptr(ptr), ops._ptr(items), longest, ops._ptr(drawn[m]),
                                                     ops._stream()), 'ihg_sample_pool_excluding')
        return run

    def weighted(m, lists):
        def run():
            _lib.check(lib.ihg_sample_pool_weighted(1, 2, P, n_items, m, ops._ptr(cum), total, ops._ptr(users) if lists else None, ds.user_count if lists else 0,
                                                    ops._ptr(ptr) if lists else None, ops._ptr(items) if lists else None, longest if lists else 0, ops._ptr(drawn[m]),
                                                    ops._stream()), 'ihg_sample_pool_weighted')
        return run

    cases = {f'ihg_sample_pool m = {m}': pool(m) for m in DRAWS}
    cases.update({f'ihg_sample_pool_weighted m = {m}, no lists': weighted(m, False) for m in DRAWS})
    cases.update({f'ihg_sample_pool_excluding m = {m}': excluding(m) for m in DRAWS})
    cases.update({f'ihg_sample_pool_weighted m = {m}, user lists': weighted(m, True) for m in DRAWS})
    times = timed_rounds(cases, rounds, reps)
    print(f'(1) negatives of {P} positives from {n_items} items; microseconds per call (back-to-back launches on one stream), median [min - max] over {rounds} rounds of {reps}')
    show(times, 1e3, 'us')
    for m in DRAWS:
        verdict(times, f'ihg_sample_pool m = {m}', f'ihg_sample_pool_weighted m = {m}, no lists')
        verdict(times, f'ihg_sample_pool_excluding m = {m}', f'ihg_sample_pool_weighted m = {m}, user lists')


def steps(ds, rounds, reps):
    from ihgnn_amd import synth
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    from ihgnn_amd.optim import Adam
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS['C3']
    torch.manual_seed(0)
    model = RawGnn(dev, ds, cfg['dim'], IHGNNLayer, cfg['layers'], 3, False, HemPredictionLayer, 0.5).to(dev)
    opt = Adam(model.parameters(), 1e-3, weight_decay=0)
    ds.item_sampling_table_on(dev)                                          # (built at the exponent above; the unflagged loaders below never look at it)

    def loader(per_positive, power):
        """One epoch of the device loader's batches under these settings (the generator reads them when it starts: its first batch is drawn here)."""
        ds.rand_neg_sample_size, ds.popularity_power = per_positive, power
        batches = ds.device_batches(P, epoch=0, seed=3)
        next(batches)
        return batches

    def step(batches, hard):
        def run():
            p_u, p_q, p_i, p_f, n_u, n_q, n_i, n_f = next(batches)
            users, queries, items = torch.cat([p_u, n_u]), torch.cat([p_q, n_q]), torch.cat([p_i, n_i])
            if hard:
                loss = model.hard_negative_loss(users, queries, items, P, KEEP, 'bpr')
            else:
                loss = model.bce_loss(users, queries, items, torch.cat([p_f, n_f]).float())
            loss.backward(); opt.step(); opt.zero_grad()
        return run

    names = {(False, False): f'plain loss, k = {KEEP} uniform negatives', (False, True): f'plain loss, k = {KEEP} weighted negatives',
             (True, False): f'hard negatives bpr, best {KEEP} of {POOL} uniform', (True, True): f'hard negatives bpr, best {KEEP} of {POOL} weighted'}
    cases = {name: step(loader(POOL if hard else KEEP, ALPHA if weighted else 0.0), hard) for (hard, weighted), name in names.items()}
    ds.rand_neg_sample_size, ds.popularity_power = KEEP, ALPHA
    times = timed_rounds(cases, rounds, reps)
    print(f'(2) C3 full eager training step, batch drawn by the device loader (d = {cfg["dim"]}, {cfg["layers"]} layers, {P} positives); ms, median [min - max] over '
          f'{rounds} rounds of {reps}')
    show(times)
    for hard in (False, True):
        verdict(times, names[(hard, False)], names[(hard, True)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200, help='calls per round of the launches')
    ap.add_argument('--step-reps', type=int, default=5, help='steps per round of the full training step')
    ap.add_argument('--no-steps', action='store_true', help='the launches only')
    args = ap.parse_args()
    ds = c3_dataset()
    launches(ds, args.rounds, args.reps)
    if not args.no_steps:
        steps(ds, args.rounds, args.step_reps)


if __name__ == '__main__':
    main()
