#!/usr/bin/env python3
"""What a device-drawn training batch costs with logged negatives (``--device_sampling --logged_negatives N``), from one run on one GPU: one epoch of batches from
``DeviceBatchLoader``, nothing else on the device,

  (a) 10 random negatives per positive: the path without logged negatives - index, gather, ``ihg_sample_negatives`` and the torch launches that lay the tuple out;
  (b) 5 random + 5 logged negatives per positive: one ``ihg_device_batch`` launch per batch into one fresh tensor;

at B = 100 and B = 4,096 positives per batch (the same rows per batch in both), on a synthetic corpus of 200,000 positives in which every (user, query) pair has 5 to 8
logged negatives.  Only the batches are produced: no model runs, so this is the cost a step pays for its batch when the batch source is not hidden behind the step.

    python tools/sampling_bench.py [--rounds 5] [--edges 200000]

Every case is warmed up (one epoch), then the cases are timed in interleaved rounds, one epoch between two HIP events with the device drained on both sides; the table
gives the median and the min - max over the rounds, per batch, in microseconds: the device span between the events, and the time the host's loop took to ISSUE the
epoch, taken when the loop returns and before the device is waited for.  A host loop about as long as the device span means the device kept up and the host's launches
are the bound; a host loop shorter than the span means the device is still working off its queue when the loop ends, and the kernels are the bound.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def corpus(edges, rand, nonrand, dev):
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    w = synth.draw(20_000, 2_000, 50_000, 300, edges, seed=0)
    rng = np.random.default_rng(1)
    pairs = np.unique(w.triples[:, :2], axis=0)
    uq = np.repeat(pairs, rng.integers(5, 9, len(pairs)), axis=0)
    neg = np.concatenate([uq, rng.integers(0, w.item_count, (len(uq), 1))], 1)[rng.permutation(len(uq))]
    return GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, random_negative_sample_size=rand,
                                    non_random_negative_sample_size=nonrand, device=dev, neg_triples=neg)


def epoch(loader, number):
    loader.set_epoch(number)
    rows = 0
    for batch in loader:
        rows += batch[0].shape[0] + batch[4].shape[0]
    return rows


def main():
    from ihgnn_amd.Dataset import DeviceBatchLoader
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--edges', type=int, default=200_000)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    sets = {'10 random (as before)': corpus(args.edges, 10, 0, dev), '5 random + 5 logged (one launch)': corpus(args.edges, 5, 5, dev)}
    for batch_size in (100, 4096):
        loaders = {name: DeviceBatchLoader(ds, batch_size) for name, ds in sets.items()}
        for loader in loaders.values():
            assert epoch(loader, 0) == args.edges * 11
        torch.cuda.synchronize()
        device_us, host_us = {k: [] for k in loaders}, {k: [] for k in loaders}
        for r in range(args.rounds):
            for name, loader in loaders.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                h0 = time.perf_counter()
                t0.record()
                epoch(loader, 1 + r)
                h1 = time.perf_counter()                                 # the loop has issued everything; the device may still be behind
                t1.record()
                torch.cuda.synchronize()
                host_us[name].append((h1 - h0) * 1e6 / len(loader))
                device_us[name].append(t0.elapsed_time(t1) * 1e3 / len(loader))
        n_batches = -(-args.edges // batch_size)
        assert all(len(loader) == n_batches for loader in loaders.values())
        print(f'B = {batch_size}: {n_batches} batches of {batch_size * 11} rows per epoch; microseconds per batch, median [min - max] over {args.rounds} epochs')
        for name in loaders:
            d, h = device_us[name], host_us[name]
            print(f'  {name:<34s} device span {statistics.median(d):8.1f}  [{min(d):.1f} - {max(d):.1f}]   host loop {statistics.median(h):8.1f}  [{min(h):.1f} - {max(h):.1f}]')


if __name__ == '__main__':
    main()
