#!/usr/bin/env python3
"""Forward + backward timings of one order-3 IHGNN layer with phase-2 attention on a BASELINE config (C2: d = 64, C3: d = 128), against two yardsticks
measured on the same GPU in the same run:

  (a) the same layer with the attention off (``Y = Dv^-1 H Interact(h)``: the node-level form, no ``[E, d]`` rows);
  (b) a torch composition of the phase-2 block on the same ``h`` and ``Ef`` (one Linear on both row sets, ``index_select`` of ``[3 E, d]`` rows,
      ``scatter_reduce`` for the row maxima, ``index_add_`` for the sums) - what the reference computes after its interactor, in torch ops - next to the
      library's block on the same operands (``ops.rows_linear`` x 2 + ``ops.hyper_attention``).

    python tools/phase2_bench.py [--configs C2,C3] [--rounds 5] [--reps 10] [--only NAME]

Every case is warmed up, then the cases are timed in interleaved rounds (each round runs every case ``reps`` times between two HIP events); the table gives
the median and the min - max over the rounds, in ms per forward + backward.  ``--only NAME`` runs one case (three warm-up passes, then ``reps`` passes) and
prints nothing but its time: what a kernel trace of one step is taken from.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_block(h, ef, W, b, w, c, src, dst, n):
    """The phase-2 block in torch ops (concatenation head, LeakyReLU): GATLayer.forward over the graph whose edges run hyperedge ``src`` -> node ``dst``."""
    d = h.shape[1]
    h2 = torch.nn.functional.linear(h, W, b)
    ef2 = torch.nn.functional.linear(ef, W, b)
    rows = ef2.index_select(0, src)                                         # [3 E, d]
    s = torch.nn.functional.leaky_relu(rows @ w[:d] + (h2 @ w[d:]).index_select(0, dst) + c, 0.01)
    top = torch.full((n,), -float('inf'), device=h.device).scatter_reduce(0, dst, s, 'amax', include_self=True)
    e = torch.exp(s - top[dst])
    den = torch.zeros(n, device=h.device).index_add_(0, dst, e)
    a = e / den[dst]
    return torch.zeros_like(h2).index_add_(0, dst, rows * a[:, None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    from ihgnn_amd import ops, synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    from ihgnn_amd.Models import IHGNNLayer
    dev = torch.device('cuda:0')
    for name in args.configs.split(','):
        d = synth.CONFIGS[name]['dim']
        w = synth.draw_config(name)
        ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, graph_type=PpsHyperGraph,
                                      device=dev)
        lay = ds.hypergraph.layout
        n, e = lay.node_count, lay.edge_count
        torch.manual_seed(0)
        x = (torch.randn(n, d, device=dev) * 0.5).requires_grad_(True)
        cot = torch.randn(n, d, device=dev)
        layers = {}
        for head in (Gsv.concat, Gsv.product):
            Gs.Gnn.gat_head = head
            layers[f"attention {'concat' if head == Gsv.concat else 'product'}"] = IHGNNLayer(dev, ds, d, d, 3, True).to(dev)
        Gs.Gnn.gat_head = Gsv.concat
        layers['attention off (a)'] = IHGNNLayer(dev, ds, d, d, 3, False).to(dev)
        ref = layers['attention concat'].fake_gat
        W, b = ref.feature_transform.weight, ref.feature_transform.bias
        wv, c = ref.feature_aggregate[0].weight.reshape(-1), ref.feature_aggregate[0].bias
        ptr = lay.node_csr.ptr.long()
        dst = torch.repeat_interleave(torch.arange(n, device=dev), ptr[1:] - ptr[:-1])
        src = lay.node_csr.ids.long()
        h = (torch.randn(n, d, device=dev) * 0.5).requires_grad_(True)
        ef = (torch.randn(e, d, device=dev) * 0.5).requires_grad_(True)

        def layer_case(layer):
            def run():
                layer(x).backward(cot)
            return run

        cases = {k: layer_case(v) for k, v in layers.items()}
        cases['block, library'] = lambda: ops.hyper_attention(ops.node_linear(h, W, b, lay), ops.rows_linear(ef, W, b), lay, wv, c, 'concatenation',
                                                              'leaky_relu').backward(cot)
        cases['block, torch (b)'] = lambda: torch_block(h, ef, W, b, wv, c, src, dst, n).backward(cot)
        if args.only:
            run = cases[args.only]
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.reps):
                run()
            t1.record()
            torch.cuda.synchronize()
            print(f'{name} {args.only}: {t0.elapsed_time(t1) / args.reps:.3f} ms')
            continue
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
        csr = lay.node_csr
        print(f'{name}: N = {n:,}, E = {e:,}, d = {d}, split rows {csr.n_heavy} ({csr.n_segments} segments); order-3 layer, ms per forward + backward, '
              f'median [min - max] over {args.rounds} rounds of {args.reps}')
        for k, v in times.items():
            print(f'  {k:<20s} {statistics.median(v):8.3f}  [{min(v):.3f} - {max(v):.3f}]')
        x.grad = h.grad = ef.grad = None
        del layers, cases
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
