#!/usr/bin/env python3
"""Forward + backward timings of the GAT layer against the GCN layer and a torch composition of the reference's GAT forward, on the uqi pair graph of a
BASELINE config (C2: d = 64, C3: d = 128), plus one 2-layer RawGnn GAT training step.

    python tools/gat_bench.py [--configs C2,C3] [--rounds 5] [--reps 10]

Every case is warmed up, then the cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives
the median and the min - max over the rounds, in ms per forward + backward.  The torch composition gathers ``[nnz, 2, d]`` rows, takes the softmax with
``scatter_reduce`` and sums with ``index_add_`` (GnnLayers.py:98-115 with DGL's two ops written in torch) - what the reference computes, on the same GPU.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_gat(x, W, b, w, c, src, dst, n):
    """The reference's forward in torch ops (concatenation head, LeakyReLU)."""
    h = torch.nn.functional.linear(x, W, b)
    pair = h[torch.stack([src, dst], 1)]                                   # [nnz, 2, d]
    s = torch.nn.functional.leaky_relu(pair.reshape(pair.shape[0], -1) @ w + c, 0.01)
    top = torch.full((n,), -float('inf'), device=x.device).scatter_reduce(0, dst, s, 'amax', include_self=True)
    e = torch.exp(s - top[dst])
    den = torch.zeros(n, device=x.device).index_add_(0, dst, e)
    a = e / den[dst]
    return torch.zeros_like(h).index_add_(0, dst, h[src] * a[:, None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
    from ihgnn_amd.Helpers.Graph import Pps2DGraph
    from ihgnn_amd.Models import GATLayer, GCNLayer, HemPredictionLayer, RawGnn
    from ihgnn_amd.optim import Adam
    dev = torch.device('cuda:0')
    for name in args.configs.split(','):
        d = synth.CONFIGS[name]['dim']
        w = synth.draw_config(name)
        ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, graph_type=Pps2DGraph,
                                      device=dev)
        lay = ds.graph2d.layout
        n, nnz = lay.node_count, lay.csr.nnz
        torch.manual_seed(0)
        x = (torch.randn(n, d, device=dev) * 0.5).requires_grad_(True)
        cot = torch.randn(n, d, device=dev)
        layers = {}
        for head in (Gsv.concat, Gsv.product):
            Gs.Gnn.gat_head = head
            layers[f"GAT {'concat' if head == Gsv.concat else 'product'}"] = GATLayer(dev, ds, d, d).to(dev)
        Gs.Gnn.gat_head = Gsv.concat
        layers['GCN'] = GCNLayer(dev, ds, d, d).to(dev)
        ref = layers['GAT concat']
        W, b = ref.feature_transform.weight, ref.feature_transform.bias
        wv, c = ref.feature_aggregate[0].weight.reshape(-1), ref.feature_aggregate[0].bias
        ptr = lay.csr.ptr.long()
        dst = torch.repeat_interleave(torch.arange(n, device=dev), ptr[1:] - ptr[:-1])
        src = lay.csr.ids.long()
        model = RawGnn(dev, ds, d, GATLayer, 2, 1, False, HemPredictionLayer, 0.5).to(dev)
        opt = Adam(model.parameters(), 1e-3, weight_decay=0)
        batch = next(iter(ds.sample_batches(100, 1, seed=1)))

        def step():
            loss = model.bce_loss(*batch)
            loss.backward()
            opt.step()
            opt.zero_grad()

        def layer_case(layer):
            def run():
                layer(x).backward(cot)
            return run

        cases = {k: layer_case(v) for k, v in layers.items()}
        cases['torch reference'] = lambda: torch_gat(x, W, b, wv, c, src, dst, n).backward(cot)
        cases['RawGnn 2xGAT step'] = step
        for run in cases.values():                                         # warm-up
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, run in cases.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.reps):
                    run()
                t1.record()
                torch.cuda.synchronize()
                times[k].append(t0.elapsed_time(t1) / args.reps)
        print(f'{name}: N = {n:,}, nnz = {nnz:,}, d = {d}, split rows {lay.csr.n_heavy} ({lay.csr.n_segments} segments); ms per forward + backward, '
              f'median [min - max] over {args.rounds} rounds of {args.reps}')
        for k, v in times.items():
            print(f'  {k:<20s} {statistics.median(v):8.3f}  [{min(v):.3f} - {max(v):.3f}]')
        x.grad = None
        del model, opt, layers, cases
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
