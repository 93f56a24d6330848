#!/usr/bin/env python3
"""What the Srrl baseline (``--model Srrl``) costs on the HIP block kernels, from one run on one GPU, against a torch composition of the same math restated here
(``F.normalize(torch.cat(...))`` -> ``F.linear`` -> ``F.leaky_relu`` per module, embedding lookups by indexing, ``F.logsigmoid`` / ``BCEWithLogitsLoss``, autograd's
backward, ``torch.optim.Adam``) on the same parameters, in the same process:

  (1) a PS step at the reference's default batch (100 positives + 1,000 negatives), forward + backward + Adam;
  (2) a KG step of each mode (100 positives x 10 negatives), forward + backward + Adam;
  (3) an evaluation pass over ``--logs`` (200) test logs x config C3's 120,000 items: ``Srrl.top_items`` against one log at a time over all items with ``torch.topk``;

at d = 32 (the reference's default) and d = 64, on config C3's corpus.  ``--config C1 --no-eval`` times the same steps over C1's small tables (1,000 users and items):
what a step costs beyond that at C3 is what scales with the tables - their dense gradients (zero-filled per indexed source, added by autograd) and Adam over them.

    python tools/srrl_bench.py [--rounds 5] [--reps 10] [--logs 200] [--dims 32 64] [--config C3] [--no-eval]

Every case is warmed up, then the cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives the
median and the min - max over the rounds, in ms.  Nothing is asserted: the comparison is a record.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ('tail-company-batch', 'head-company-batch', 'query-company-batch')


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
        print(f'  {k:<44s} {statistics.median(v):10.4f}  [{min(v):.4f} - {max(v):.4f}]')
    names = list(times)
    for hip, composed in zip(names[0::2], names[1::2]):
        print(f'  {composed} / {hip}: {statistics.median(times[composed]) / statistics.median(times[hip]):.2f} x')


class Composition:
    """The same model as a torch composition over the SAME parameter tensors."""

    def __init__(self, model, ds):
        self.p = dict(model.named_parameters())
        self.bag_input, self.bag_offsets = ds.queries_for_embeddingbag, ds.queries_offset_for_embeddingbag

    def aggregation(self, name, x):
        return F.leaky_relu(F.linear(F.normalize(x, dim=-1), self.p[name + '.aggregation.0.weight'], self.p[name + '.aggregation.0.bias']))

    def mlp(self, name, x):
        hidden = F.leaky_relu(F.linear(F.normalize(x, dim=-1), self.p[name + '.mlp.0.weight'], self.p[name + '.mlp.0.bias']))
        return F.linear(hidden, self.p[name + '.mlp.2.weight'], self.p[name + '.mlp.2.bias'])

    def queries(self):
        return F.embedding_bag(self.bag_input, self.p['KG.embedding_bag_vocabulary.weight'], self.bag_offsets, mode='mean')

    def ps_scores(self, users, queries, items, q_all=None):
        q_all = self.queries() if q_all is None else q_all
        rows = lambda key, idx: self.p[key][1:][idx]
        u = self.aggregation('g_u', torch.cat([rows('PS.embedding_user.weight', users), rows('KG.embedding_user.weight', users).detach()], -1))
        i = self.aggregation('g_i', torch.cat([rows('PS.embedding_item.weight', items), rows('KG.embedding_item.weight', items).detach()], -1))
        uq = self.mlp('ps_mlp_uq', torch.cat([u, q_all[queries]], -1))
        ui = self.mlp('ps_mlp_ui', torch.cat([u, i], -1))
        return self.mlp('ps_mlp_pred', torch.cat([uq, ui], -1)).squeeze(-1)

    def kg_scores(self, positive, scored_ids, items2, users2, queries2, mode, positive_mode):
        U_, I_, Q_ = self.p['KG.embedding_user.weight'][1:], self.p['KG.embedding_item.weight'][1:], self.queries()
        u, q, i = U_[positive[:, 0]].unsqueeze(1), Q_[positive[:, 1]].unsqueeze(1), I_[positive[:, 2]].unsqueeze(1)
        scored = I_[scored_ids]
        k = scored.shape[1]
        if mode == MODES[0]:
            other = I_[items2[:, 0]].unsqueeze(1) if positive_mode else i.expand(-1, k, -1)
            scored = self.aggregation('kg_aggre_tail', torch.cat([scored, other], -1))
            context = self.mlp('kg_mlp_pre', torch.cat([u, q], -1))
        elif mode == MODES[1]:
            context = self.mlp('kg_mlp_pre', torch.cat([self.aggregation('kg_aggre_head', torch.cat([u, U_[users2[:, 0]].unsqueeze(1)], -1)), q], -1))
        else:
            context = self.mlp('kg_mlp_pre', torch.cat([u, self.aggregation('kg_aggre_query', torch.cat([q, Q_[queries2[:, 0]].unsqueeze(1)], -1))], -1))
        return (scored * context).sum(2)

    def kg_loss(self, batch):
        positive, negative, weight, mode, tails, heads, queries = batch
        neg = F.logsigmoid(-self.kg_scores(positive, negative, tails, heads, queries, mode, False)).mean(dim=1)
        pos = F.logsigmoid(self.kg_scores(positive, positive[:, 2:3], tails, heads, queries, mode, True)).squeeze(1)
        return (-(weight * pos).sum() / weight.sum() - (weight * neg).sum() / weight.sum()) / 2


def bench(dim, w, rounds, reps, n_logs, evaluate=True):
    from torch.utils.data import DataLoader
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Helpers.TrainTestHelper import _evaluate_batched, srrl_kg_step, srrl_ps_step
    from ihgnn_amd.Models import Srrl
    from ihgnn_amd.SrrlDataset import MetaPaths, SrrlDatasetKG
    from ihgnn_amd.optim import Adam
    dev = torch.device('cuda:0')
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev)
    torch.manual_seed(0)
    model = Srrl(ds, dim, None, 0.5).to(dev)
    composed = Composition(model, ds)
    opt, opt_torch = Adam(model.parameters(), 1e-3, weight_decay=0), torch.optim.Adam(model.parameters(), 1e-3, weight_decay=0)
    gen = torch.Generator().manual_seed(1)
    pos, neg = Gs.batch_size, Gs.batch_size * Gs.negative_sample_size
    pu, pq = torch.randint(0, ds.user_count, (pos,), generator=gen), torch.randint(0, ds.query_count, (pos,), generator=gen)
    ps_batch = (pu, pq, torch.randint(0, ds.item_count, (pos,), generator=gen), torch.ones(pos), pu.repeat_interleave(neg // pos), pq.repeat_interleave(neg // pos),
                torch.randint(0, ds.item_count, (neg,), generator=gen), torch.zeros(neg))
    ps_batch = tuple(t.to(dev) for t in ps_batch)
    users, queries, items = (torch.cat(pair) for pair in ((ps_batch[0], ps_batch[4]), (ps_batch[1], ps_batch[5]), (ps_batch[2], ps_batch[6])))
    labels = torch.cat([ps_batch[3], ps_batch[7]])
    lossf = torch.nn.BCEWithLogitsLoss()

    def composed_ps():
        opt_torch.zero_grad()
        lossf(composed.ps_scores(users, queries, items), labels).backward()
        opt_torch.step()

    cases = {f'PS step d={dim} (HIP)': lambda: srrl_ps_step(model, opt, ps_batch, dev), f'PS step d={dim} (torch composition)': composed_ps}
    meta = MetaPaths(ds)
    for mode in MODES:
        batch = next(iter(DataLoader(SrrlDatasetKG(meta, Gs.negative_sample_size, mode), Gs.batch_size, True, collate_fn=SrrlDatasetKG.collate_fn)))
        batch = tuple(t.to(dev) if torch.is_tensor(t) else t for t in batch)

        def composed_kg(batch=batch):
            opt_torch.zero_grad()
            composed.kg_loss(batch).backward()
            opt_torch.step()

        cases[f'KG step {mode[:5]} d={dim} (HIP)'] = lambda batch=batch: srrl_kg_step(model, opt, batch, dev)
        cases[f'KG step {mode[:5]} d={dim} (torch composition)'] = composed_kg
    times = timed_rounds(cases, rounds, reps)
    print(f'(1, 2) training steps, d = {dim}: {pos} positives + {neg} negatives (PS), {pos} x {Gs.negative_sample_size} negatives (KG); ms, median [min - max] over {rounds} rounds of {reps}')
    show(times)

    if not evaluate:
        return
    logs = [(lu, lq, its, None, True) for lu, lq, its in w.test_logs[:n_logs]]
    every_item = torch.arange(ds.item_count, device=dev)

    def hip_eval():
        _evaluate_batched(model, logs, ds.item_count, dev, list(range(len(logs))))

    def composed_eval():
        q_all = composed.queries()
        for lu, lq, _, _, _ in logs:
            composed.ps_scores(torch.full((ds.item_count,), lu, device=dev), torch.full((ds.item_count,), lq, device=dev), every_item, q_all).topk(10).indices.tolist()

    with torch.no_grad():
        model.save_features_for_test()
        times = timed_rounds({f'evaluation d={dim} (HIP top_items)': hip_eval, f'evaluation d={dim} (torch, per log)': composed_eval}, rounds, 1)
        model.clear_saved_feature()
    print(f'(3) evaluation pass, d = {dim}: {len(logs)} logs x {ds.item_count:,} items; ms, median [min - max] over {rounds} rounds of 1')
    show(times)
    del model, composed
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--logs', type=int, default=200, help='test logs of the evaluation pass')
    ap.add_argument('--dims', type=int, nargs='+', default=[32, 64])
    ap.add_argument('--config', default='C3', help='the synthetic corpus (ihgnn_amd.synth.CONFIGS)')
    ap.add_argument('--no-eval', action='store_true', help='the training steps only')
    args = ap.parse_args()
    from ihgnn_amd import synth
    w = synth.draw_config(args.config, eval_logs=args.logs)
    print(f'corpus {args.config}: {w.user_count:,} users, {w.query_count:,} queries, {w.item_count:,} items')
    for dim in args.dims:
        bench(dim, w, args.rounds, args.reps, args.logs, evaluate=not args.no_eval)


if __name__ == '__main__':
    main()
