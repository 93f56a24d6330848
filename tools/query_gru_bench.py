#!/usr/bin/env python3
"""What the GRU query encoder (``Gs.Query.transform == 'gru'``) costs, from one run on one GPU: forward + backward of the query rows of X0 at the query bags of
BASELINE configs C1 (500 queries, d = 64), C2 (989, d = 64) and C3 (26 k, d = 128) - the synthetic stand-ins' own bags, words in order -

  (1) ``ops.bag_mean`` with the GRU description: ``ihg_gru_fwd`` (one launch) and ``ihg_gru_bwd`` (the time loop backwards, the weight-gradient slabs, their
      fixed-order sum, the segment sum over every word's positions); the forward alone, outside autograd, is what search and the evaluation cache run;
  (2) against the ``activation`` transform on the same bags (``ihg_bag_mean_fwd`` + ``ihg_rows_linear_act_fwd`` and their backwards);
  (3) against a torch composition on the same GPU: ``nn.GRU`` over ``pack_padded_sequence`` of the gathered word rows (non-empty bags only; empty bags are zero rows),
      autograd's backward down to the word table.

    python tools/query_gru_bench.py [--configs C1,C2,C3] [--rounds 5] [--reps 10] [--only gru]

Every case is warmed up, then the cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives the
median and the min - max over the rounds, in ms.  ``--only gru`` runs case (1) alone, a few times: the run to put under ``rocprofv3 --kernel-trace --stats`` for the
launch count and the per-launch times.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = ('C1', 'C2', 'C3')


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


def query_rows(name, rounds, reps, only):
    from ihgnn_amd import _lib, ops, synth
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS[name]
    w = synth.draw_config(name)
    d, q, rows = cfg['dim'], w.query_count, w.vocab_size + 1
    bag = ops.BagLayout(w.bag_words + 1, w.bag_offsets, rows, dev)
    lens = np.diff(np.append(w.bag_offsets, len(w.bag_words)))
    torch.manual_seed(0)
    table = (torch.randn(rows, d, device=dev) * 0.5).requires_grad_(True)
    gru = torch.nn.GRU(d, d, batch_first=True).to(dev)
    params = (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
    qt = ops.QueryTransform('gru', params)
    wq = (torch.randn(d, d, device=dev) / d ** 0.5).requires_grad_(True)
    bq = (torch.randn(d, device=dev) * 0.2).requires_grad_(True)
    cot = torch.randn(q, d, device=dev)

    def clear():
        for t in (table, wq, bq) + params:
            t.grad = None

    def gru_fwd_bwd():
        clear()
        ops.bag_mean(table, bag, transform=qt).backward(cot)

    def gru_fwd():
        with torch.no_grad():
            ops.bag_mean(table, bag, transform=qt)

    def act_fwd_bwd():
        clear()
        ops.bag_mean(table, bag, wq, bq, 'relu').backward(cot)

    # the torch composition: rows of the non-empty bags, padded to the longest, packed (lengths on the host, as pack_padded_sequence takes them: no synchronisation)
    full = np.nonzero(lens > 0)[0]
    longest = int(lens.max()) if len(lens) else 0
    ids = np.zeros((len(full), longest), np.int64)
    for r, b in enumerate(full):
        ids[r, :lens[b]] = w.bag_words[w.bag_offsets[b]:w.bag_offsets[b] + lens[b]] + 1
    ids_dev, full_dev, lens_host = torch.from_numpy(ids).to(dev), torch.from_numpy(full).to(dev), torch.from_numpy(lens[full])

    def torch_fwd_bwd():
        clear()
        packed = torch.nn.utils.rnn.pack_padded_sequence(table[ids_dev], lens_host, batch_first=True, enforce_sorted=False)
        h = gru(packed)[1][0]
        torch.zeros(q, d, device=dev).index_copy(0, full_dev, h).backward(cot)

    print(f'{name}: {q:,} queries, {int(lens.sum()):,} word occurrences (bags of {int(lens.min())} .. {longest} words), d = {d}; saved state '
          f'{int(_lib.load().ihg_gru_saved_bytes(int(lens.sum()), d)) / 1e6:.2f} MB, backward workspace {int(_lib.load().ihg_gru_workspace_bytes(q, int(lens.sum()), d)) / 1e6:.2f} MB')
    if only == 'gru':
        for _ in range(5):
            gru_fwd_bwd()
        torch.cuda.synchronize()
        return
    with torch.no_grad():
        packed = torch.nn.utils.rnn.pack_padded_sequence(table[ids_dev], lens_host, batch_first=True, enforce_sorted=False)
        theirs = torch.zeros(q, d, device=dev).index_copy(0, full_dev, gru(packed)[1][0])
        ours = ops.bag_mean(table, bag, transform=qt)
    print(f'  rows against torch nn.GRU on the same GPU: largest difference {float((ours - theirs).abs().max()):.2e} of {float(theirs.abs().max()):.2e}')
    cases = {'gru fwd + bwd (1)': gru_fwd_bwd, 'gru fwd, no autograd (1)': gru_fwd, 'activation transform fwd + bwd (2)': act_fwd_bwd,
             'torch nn.GRU packed fwd + bwd (3)': torch_fwd_bwd}
    times = timed_rounds(cases, rounds, reps)
    print(f'  ms per call, median [min - max] over {rounds} rounds of {reps}')
    for k, v in times.items():
        print(f'  {k:<38s} {statistics.median(v):9.4f}  [{min(v):.4f} - {max(v):.4f}]')
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f'  gru / activation {med["gru fwd + bwd (1)"] / med["activation transform fwd + bwd (2)"]:.2f} x, gru / torch {med["gru fwd + bwd (1)"] / med["torch nn.GRU packed fwd + bwd (3)"]:.2f} x')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default=','.join(CONFIGS))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--only', default=None, choices=('gru',), help='the GRU forward + backward alone, five times (for a kernel trace)')
    args = ap.parse_args()
    for name in args.configs.split(','):
        query_rows(name, args.rounds, args.reps, args.only)


if __name__ == '__main__':
    main()
