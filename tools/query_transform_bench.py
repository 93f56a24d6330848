#!/usr/bin/env python3
"""What the query transform (``Gs.Query.transform == 'activation'``: ``act(mean W^T + b)`` on the queries' bag means) costs, from one run on one GPU:

  (1) its forward and backward launches at the query shapes of BASELINE configs C3 (26 k x 128) and C5 (1 M x 256) - ``ihg_rows_linear_act_fwd`` / ``_bwd`` -
      beside the plain ``ops.rows_linear`` forward / backward on the same rows (no activation: what the node-level transforms of the layers launch).  By bytes the
      forward equals the plain launch (the epilogue adds no traffic); the backward reads y on top - 20 d B per row where the input gradient is fused into the
      weight-gradient kernel (d = 64), 24 d B elsewhere (the dm row GEMM and the weight-gradient kernel each read dy and y) against the plain backward's 16 d B;
  (2) the same block as a torch composition (``torch.nn.functional.linear`` + ``relu`` / ``tanh``, autograd's backward) on the same GPU;
  (3) a full training step of C3 and of C5 with the transform on against off (``--no-steps`` leaves it out; C5 takes minutes to build: ``--configs C3``).

    python tools/query_transform_bench.py [--configs C3,C5] [--rounds 5] [--reps 10] [--no-steps] [--activation relu]

Every case is warmed up, then the cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives the
median and the min - max over the rounds, in ms.  The spread of the plain launch between rounds is the margin every comparison with it carries.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {'C3': (26_000, 128), 'C5': (1_000_000, 256)}


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
        print(f'  {k:<34s} {statistics.median(v):9.4f}  [{min(v):.4f} - {max(v):.4f}]')


def launches(name, act, rounds, reps):
    from ihgnn_amd import _lib, ops
    dev = torch.device('cuda:0')
    rows, d = SHAPES[name]
    lib = _lib.load()
    torch.manual_seed(0)
    m = torch.randn(rows, d, device=dev) * 0.5
    w = torch.randn(d, d, device=dev) / d ** 0.5
    b = torch.randn(d, device=dev) * 0.2
    dy = torch.randn(rows, d, device=dev)
    y, dm, dw, db = torch.empty_like(m), torch.empty_like(m), torch.empty_like(w), torch.empty_like(b)
    ws = ops._workspace(int(lib.ihg_node_linear_workspace_bytes(d)), dev)
    code = ops.QUERY_ACTIVATIONS[act]
    tb = ops._plain_type_begin(rows)

    def act_fwd():
        _lib.check(lib.ihg_rows_linear_act_fwd(ops._ptr(m), d, ops._ptr(w), d, ops._ptr(b), code, ops._ptr(y), d, rows, ops._ptr(ws), ws.numel() * 4, d, ops._stream()), 'fwd')

    def act_bwd():
        _lib.check(lib.ihg_rows_linear_act_bwd(ops._ptr(dy), d, ops._ptr(y), d, ops._ptr(m), d, ops._ptr(w), d, code, ops._ptr(dw), d, ops._ptr(db), ops._ptr(dm), d, rows,
                                               ops._ptr(ws), ws.numel() * 4, d, ops._stream()), 'bwd')

    def plain_fwd():
        _lib.check(lib.ihg_node_linear_fwd(ops._ptr(m), d, ops._ptr(w), d, 0, ops._ptr(b), 0b111, 0, tb, ops._ptr(y), d, ops._ptr(ws), ws.numel() * 4, d, ops._stream()), 'plain fwd')

    def plain_bwd():
        _lib.check(lib.ihg_node_linear_bwd_weight(ops._ptr(dy), d, ops._ptr(m), d, tb, ops._ptr(dw), d, 0, ops._ptr(db), 0b111, 0, ops._ptr(w), d, ops._ptr(dm), d, 0,
                                                  ops._ptr(ws), ws.numel() * 4, d, ops._stream()), 'plain bwd')

    mt, wt, bt = m.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    fn = torch.relu if act == 'relu' else torch.tanh

    def torch_fwd():
        with torch.no_grad():
            fn(torch.nn.functional.linear(mt, wt, bt))

    def torch_fwd_bwd():
        mt.grad = wt.grad = bt.grad = None
        fn(torch.nn.functional.linear(mt, wt, bt)).backward(dy)

    act_fwd()                                                              # (y holds real activations for the backward cases)
    cases = {'transform fwd': act_fwd, 'plain rows_linear fwd': plain_fwd, 'transform bwd': act_bwd, 'plain rows_linear bwd': plain_bwd,
             'torch linear + act fwd (2)': torch_fwd, 'torch linear + act fwd + bwd (2)': torch_fwd_bwd}
    times = timed_rounds(cases, rounds, reps)
    fwd_bytes, bwd_plain, bwd_act = 8 * d * rows, 16 * d * rows, (20 if d == 64 else 24) * d * rows      # compulsory bytes (DESIGN section 4's table)
    print(f'{name}: {rows:,} rows x {d}, {act}; ms per launch set, median [min - max] over {rounds} rounds of {reps}')
    show(times)
    print(f'  by bytes: fwd {fwd_bytes / 1e6:.1f} MB either way; bwd {bwd_plain / 1e6:.1f} MB plain, {bwd_act / 1e6:.1f} MB with y ({bwd_act / bwd_plain:.2f} x)')
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f'  measured: fwd {med["transform fwd"] / med["plain rows_linear fwd"]:.2f} x the plain launch, bwd {med["transform bwd"] / med["plain rows_linear bwd"]:.2f} x')


def steps(name, act, rounds, reps):
    import torch.nn as nn
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    from ihgnn_amd.optim import Adam
    dev = torch.device('cuda:0')
    cfg = synth.CONFIGS[name]
    w = synth.draw_config(name)
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, graph_type=PpsHyperGraph, device=dev)
    batch = next(iter(ds.sample_batches(Gs.batch_size, 1, seed=1)))
    cases = {}
    for label, transform in (('step, transform off', Gsv.mean), (f'step, transform on ({act})', Gsv.activation)):
        Gs.Query.transform, Gs.Query.transform_activation = transform, {'relu': nn.ReLU, 'tanh': nn.Tanh}[act]
        torch.manual_seed(0)
        model = RawGnn(dev, ds, cfg['dim'], IHGNNLayer, cfg.get('layers', 2), cfg.get('order', 3), False, HemPredictionLayer, 0.5).to(dev)
        opt = Adam(model.parameters(), 1e-3, weight_decay=0)

        def run(model=model, opt=opt):
            loss = model.bce_loss(*batch)
            loss.backward(); opt.step(); opt.zero_grad()
        cases[label] = run
    Gs.Query.transform = Gsv.mean
    times = timed_rounds(cases, rounds, reps)
    print(f'{name}: full training step (d = {cfg["dim"]}), ms, median [min - max] over {rounds} rounds of {reps}')
    show(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C3,C5')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-steps', action='store_true', help='the launches only, no full training steps')
    ap.add_argument('--activation', default='relu', choices=('relu', 'tanh'))
    args = ap.parse_args()
    for name in args.configs.split(','):
        launches(name, args.activation, args.rounds, args.reps)
    if not args.no_steps:
        for name in args.configs.split(','):
            steps(name, args.activation, args.rounds, max(args.reps // 2, 1))
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
