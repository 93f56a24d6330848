#!/usr/bin/env python3
"""What gradient clipping (``--clip_grad_norm X``, ``optim.Adam(max_grad_norm=X)``) costs, from one run on one GPU:

  (1) at config C3's parameter set (shapes of the model's parameters, random gradients): the plain update ``ihg_adam_step``; the norm and record launches alone
      (``ihg_grad_sqnorm`` + ``ihg_clip_record``); the clipped update ``ihg_adam_step_clipped`` alone; the three together (a clipped ``step()``); and
      ``torch.nn.utils.clip_grad_norm_`` on the same gradients (which also rewrites them) alone.  The expectation to check: the norm pass costs about one read
      of the gradients - 1 of the 7 four-byte passes per parameter the update makes;
  (2) one full eager training step of C3 (d = 128, 3 layers, order 3; forward + backward + Adam) with clipping on against off, in the same process.

    python tools/clip_bench.py [--rounds 5] [--reps 50] [--step-reps 5] [--no-steps]

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


def c3_model():
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS['C3']
    w = synth.draw_config('C3')
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, graph_type=PpsHyperGraph, device=dev)
    torch.manual_seed(0)
    return ds, cfg, RawGnn(dev, ds, cfg['dim'], IHGNNLayer, cfg['layers'], 3, False, HemPredictionLayer, 0.5).to(dev)


def launches(model, rounds, reps):
    import ctypes
    from ihgnn_amd import _lib, ops
    from ihgnn_amd.optim import Adam
    lib = _lib.load()
    gen = torch.Generator(device='cuda:0').manual_seed(0)
    params = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=p.device) * 1e-3
    floats = sum(p.numel() for p in params)
    plain = Adam(params, 1e-3)
    clipped = Adam(params, 1e-3, max_grad_norm=1e-3)
    plain.step(); clipped.step()                             # state and clip buffers exist
    items = [(p, p.grad, clipped.state[p]) for p in params]
    stream = ops._stream()

    def norm_and_record():
        clipped._launch_clip_record(lib, items, stream)

    from ihgnn_amd.optim import _table
    table = _table(items)
    record = ctypes.c_void_p(clipped.grad_norm.data_ptr())

    def clipped_update():
        _lib.check(lib.ihg_adam_step_clipped(ctypes.cast(table, ctypes.c_void_p), len(items), 1e-3, 0.9, 0.999, 1e-8, 0.0, 5, record, stream), 'ihg_adam_step_clipped')

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(params, 1e3)          # (a bound above the norm: the gradients are multiplied by 1 and keep their values over the repetitions)

    cases = {'ihg_adam_step (plain update)': plain.step, 'ihg_grad_sqnorm + ihg_clip_record': norm_and_record, 'ihg_adam_step_clipped alone': clipped_update,
             'clipped step() (norm + record + update)': clipped.step, 'torch.nn.utils.clip_grad_norm_ alone': torch_clip}
    times = timed_rounds(cases, rounds, reps)
    print(f'(1) C3 parameter set: {len(params)} tensors, {floats} floats ({floats * 4 / 1e6:.1f} MB of gradients); microseconds per call, median [min - max] over {rounds} rounds of {reps}')
    show(times, 1e3, 'us')
    import statistics
    med = {k: statistics.median(v) for k, v in times.items()}
    base = med['ihg_adam_step (plain update)']
    print(f'  norm + record / plain update = {med["ihg_grad_sqnorm + ihg_clip_record"] / base:.3f} (one read of seven passes would be {1 / 7:.3f}); '
          f'gradient read rate of the norm pass {floats * 4 / med["ihg_grad_sqnorm + ihg_clip_record"] / 1e9:.2f} TB/s; update {7 * floats * 4 / base / 1e9:.2f} TB/s')
    verdict(times, 'ihg_adam_step (plain update)', 'ihg_adam_step_clipped alone')


def steps(ds, cfg, model, rounds, reps):
    from ihgnn_amd.optim import Adam
    off = Adam(model.parameters(), 1e-3, weight_decay=0)
    on = Adam(model.parameters(), 1e-3, weight_decay=0, max_grad_norm=1.0)
    u, q, i, y = next(iter(ds.sample_batches(100, 1, seed=1)))

    def step(opt):
        def run():
            loss = model.bce_loss(u, q, i, y)
            loss.backward(); opt.step(); opt.zero_grad()
        return run

    cases = {'clipping off': step(off), 'clipping on (max_grad_norm 1.0)': step(on)}
    times = timed_rounds(cases, rounds, reps)
    print(f'(2) C3 full eager training step (d = {cfg["dim"]}, {cfg["layers"]} layers, {u.shape[0]} batch rows); ms, median [min - max] over {rounds} rounds of {reps}')
    show(times)
    verdict(times, 'clipping off', 'clipping on (max_grad_norm 1.0)')
    print(f'  clip statistics of the run: {on.clip_statistics()}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50, help='calls per round of the launches')
    ap.add_argument('--step-reps', type=int, default=5, help='steps per round of the full training step')
    ap.add_argument('--no-steps', action='store_true', help='the launches only')
    args = ap.parse_args()
    ds, cfg, model = c3_model()
    launches(model, args.rounds, args.reps)
    if not args.no_steps:
        steps(ds, cfg, model, args.rounds, args.step_reps)


if __name__ == '__main__':
    main()
