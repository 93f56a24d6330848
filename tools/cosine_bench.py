#!/usr/bin/env python3
"""What the cosine-similarity HEM head (``Gs.Prediction.use_cosine_similarity``, ``--cosine``) costs, from one run on one GPU:

  (1) the batch tail, forward + backward (``ops.hem_bce_loss`` + ``backward`` over plain matrices, no holder), dot product against cosine, at config C3's batch:
      1,100 rows (100 positives + 1,000 negatives), D = 384 (three blocks of d = 128), N = C3's node count;
  (2) the same tail as the torch composition that ran for this setting before the head had kernels: ``torch.cat([x[rows] for x in layers], 1)``,
      ``torch.cosine_similarity``, ``BCEWithLogitsLoss``, autograd's backward (dense ``[N, d]`` gradients per layer through ``index_put_``);
  (3) ``ops.score_topk`` dot product against cosine at C3's catalogue (120,000 items, D = 384, 4,096 pairs);
  (4) a full C3 training step (the model ``bench.py`` builds: d = 128, 3 layers) and an evaluation pass over its test logs with the setting on: the fused path against
      the path that ran before - ``loss_function(head(picked rows))`` with torch's cosine for the step, one log at a time over all items with a full sort for the
      evaluation - restated here from the layers' outputs, so that both run in one process on one build (``--no-steps`` leaves (4) out).

    python tools/cosine_bench.py [--rounds 5] [--reps 10] [--no-steps] [--logs 200]

Every case is warmed up, then the cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives the
median and the min - max over the rounds, in ms.  The spread of the dot-product case between rounds is the margin every comparison with it carries.
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


def show(times):
    for k, v in times.items():
        print(f'  {k:<40s} {statistics.median(v):9.4f}  [{min(v):.4f} - {max(v):.4f}]')


def verdict(times, base, other):
    """Where ``other``'s median sits against ``base``'s min - max spread."""
    lo, hi, med = min(times[base]), max(times[base]), statistics.median(times[other])
    where = 'inside' if lo <= med <= hi else (f'{(med / hi - 1) * 100:.1f} % above' if med > hi else f'{(1 - med / lo) * 100:.1f} % below')
    print(f'  {other} median {med:.4f} ms is {where} the spread of {base} [{lo:.4f} - {hi:.4f}]; ratio of medians {med / statistics.median(times[base]):.3f}')


def tail(rounds, reps):
    from ihgnn_amd import ops, synth
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS['C3']
    U, Q, I = cfg['user_count'], cfg['query_count'], cfg['item_count']
    n, d, n_layers, pos, neg = U + Q + I, 128, 3, 100, 1000
    gen = torch.Generator().manual_seed(0)
    layers = [(torch.randn(n, d, generator=gen) / d ** 0.5).to(dev).requires_grad_(True) for _ in range(n_layers)]
    bias = torch.randn(I, generator=gen).to(dev).requires_grad_(True)
    # a batch as the loader draws it: every positive's user and query repeated with its negatives
    pu, pq = torch.randint(0, U, (pos,), generator=gen), torch.randint(0, Q, (pos,), generator=gen)
    u, q = torch.cat([pu, pu.repeat_interleave(neg // pos)]).to(dev), torch.cat([pq, pq.repeat_interleave(neg // pos)]).to(dev)
    i = torch.randint(0, I, (pos + neg,), generator=gen).to(dev)
    y = torch.cat([torch.ones(pos), torch.zeros(neg)]).to(dev)
    rows = torch.cat([u, q + U, i + U + Q])
    lossf = torch.nn.BCEWithLogitsLoss()

    def clear():
        for x in layers:
            x.grad = None
        bias.grad = None

    def fused(cosine):
        def run():
            clear()
            ops.hem_bce_loss(layers, rows, i, y, bias, 0.5, U + Q, cosine=cosine).backward()
        return run

    def composed(cosine):
        def run():
            clear()
            picked = torch.cat([x[rows] for x in layers], 1)
            b = u.shape[0]
            m = 0.5 * picked[b:2 * b] + 0.5 * picked[:b]
            s = (torch.cosine_similarity(picked[2 * b:], m) if cosine else (picked[2 * b:] * m).sum(1)) + bias[i]
            lossf(s, y).backward()
        return run

    cases = {'tail dot product (fused)': fused(False), 'tail cosine (fused)': fused(True), 'tail cosine (torch composition)': composed(True),
             'tail dot product (torch composition)': composed(False)}
    times = timed_rounds(cases, rounds, reps)
    print(f'(1, 2) batch tail forward + backward: {pos + neg} rows, D = {n_layers * d}, N = {n:,}; ms, median [min - max] over {rounds} rounds of {reps}')
    show(times)
    verdict(times, 'tail dot product (fused)', 'tail cosine (fused)')
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f'  fused cosine tail against the torch composition: {med["tail cosine (torch composition)"] / med["tail cosine (fused)"]:.1f} x faster')
    del layers
    torch.cuda.empty_cache()


def topk(rounds, reps):
    from ihgnn_amd import ops, synth
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS['C3']
    n_items, dim, pairs, Uc, Qc = cfg['item_count'], 384, 4096, 5000, 2000
    gen = torch.Generator().manual_seed(1)
    feats = (torch.randn(Uc + Qc + n_items, dim, generator=gen) / dim ** 0.5).to(dev)
    bias = (0.1 * torch.randn(n_items, generator=gen)).to(dev)
    users, queries = torch.randint(0, Uc, (pairs,), generator=gen).to(dev), torch.randint(0, Qc, (pairs,), generator=gen).to(dev)
    cases = {f'score_topk {name}': (lambda cosine=cosine: ops.score_topk(feats, users, queries, Uc, Uc + Qc, bias, 0.5, 10, cosine=cosine))
             for name, cosine in (('dot product', False), ('cosine', True))}
    times = timed_rounds(cases, rounds, reps)
    print(f'(3) score_topk: {pairs} pairs x {n_items:,} items, D = {dim}; ms, median [min - max] over {rounds} rounds of {reps}')
    show(times)
    verdict(times, 'score_topk dot product', 'score_topk cosine')
    del feats
    torch.cuda.empty_cache()


def steps(rounds, reps, n_logs):
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    from ihgnn_amd.Helpers.Metrics import Metrics
    from ihgnn_amd.Helpers.TrainTestHelper import _evaluate_batched
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    from ihgnn_amd.optim import Adam
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS['C3']
    w = synth.draw_config('C3', eval_logs=n_logs)
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, graph_type=PpsHyperGraph, device=dev)
    u, q, i, y = next(iter(ds.sample_batches(Gs.batch_size, 1, seed=1)))
    torch.manual_seed(0)
    model = RawGnn(dev, ds, cfg['dim'], IHGNNLayer, cfg['layers'], 3, False, HemPredictionLayer, 0.5).to(dev)
    opt = Adam(model.parameters(), 1e-3, weight_decay=0)
    lossf = torch.nn.BCEWithLogitsLoss()
    old = Gs.Prediction.use_cosine_similarity

    def fused_step(cosine):
        def run():
            Gs.Prediction.use_cosine_similarity = cosine
            loss = model.bce_loss(u, q, i, y)
            loss.backward(); opt.step(); opt.zero_grad()
        return run

    def composed_step():
        # RawGnn.forward's torch branch as it ran for this setting before: rows picked from every layer's output, the torch head, autograd
        Gs.Prediction.use_cosine_similarity = True
        rows = torch.cat([u, q + ds.query_start_index_in_graph, i + ds.item_start_index_in_graph])
        picked = torch.cat([x[rows] for x in model.propagate_layers()], 1)
        b = u.shape[0]
        loss = lossf(model.prediction_layer(picked[:b], picked[b:2 * b], picked[2 * b:], i), y)
        loss.backward(); opt.step(); opt.zero_grad()

    try:
        times = timed_rounds({'step, dot product (fused)': fused_step(False), 'step, cosine (fused)': fused_step(True), 'step, cosine (torch head, as before)': composed_step},
                             rounds, max(reps // 2, 1))
        print(f'(4) C3 full training step (d = {cfg["dim"]}, {cfg["layers"]} layers), ms, median [min - max] over {rounds} rounds of {max(reps // 2, 1)}')
        show(times)
        verdict(times, 'step, dot product (fused)', 'step, cosine (fused)')
        logs = [(lu, lq, items, None, True) for lu, lq, items in w.test_logs]
        Gs.Prediction.use_cosine_similarity = True

        def batched():
            _evaluate_batched(model, logs, ds.item_count, dev, list(range(len(logs))))

        def per_log():
            for lu, lq, items, flags, all1 in logs:
                users = torch.tensor([lu], device=dev).expand(ds.item_count)
                queries = torch.tensor([lq], device=dev).expand(ds.item_count)
                Metrics.calculate_on_all_items(model(users, queries, None), items, flags, all1)

        with torch.no_grad():
            model.save_features_for_test()
            times = timed_rounds({'evaluation, cosine (score_topk_cosine)': batched, 'evaluation, cosine (per log, as before)': per_log}, rounds, 1)
            model.clear_saved_feature()
        print(f'(4) C3 evaluation pass over {len(logs)} test logs x {ds.item_count:,} items (features cached), ms, median [min - max] over {rounds} rounds of 1')
        show(times)
    finally:
        Gs.Prediction.use_cosine_similarity = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--logs', type=int, default=200, help='test logs of the evaluation pass in (4)')
    ap.add_argument('--no-steps', action='store_true', help='the launches only, no full training step / evaluation pass')
    args = ap.parse_args()
    tail(args.rounds, args.reps)
    topk(args.rounds, args.reps)
    if not args.no_steps:
        steps(args.rounds, args.reps, args.logs)


if __name__ == '__main__':
    main()
