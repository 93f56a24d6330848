#!/usr/bin/env python3
"""Benchmark of the hypergraph message-passing hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config C3] [--dump-outputs DIR] [--full [--no-cpu-baseline] [--no-extras] [--no-kernel-events]]

A plain run sets up, warms up, times the K steps and prints the headline line (metric, value, unit, ms_per_step, dtype, config, final loss;
gradient_exchange when N > 1).  Everything else below (roofline and per-kernel figures, the untimed extra passes, the CPU baseline) is measured
only with --full; there the --no-* switches leave parts of it out.  --dump-outputs DIR writes what the last timed step computed as .npy files
(dump_outputs below).

Metric (BASELINE.json / SURVEY.md §8 d1): hyperedges aggregated per second = E * L * steps / wall time, where one
"hyperedge aggregated" is one hyperedge taken through one layer's node->hyperedge and hyperedge->node phases.
A step is one FULL training step of RawGnn (full-graph propagation forward over every row of every layer, BCE loss on a
1100-row batch, backward, gradient all-reduce when N > 1, Adam) - nothing is skipped inside the timed region.  Inputs
(graph layout, weights, pre-drawn batches) are resident in HBM before the clock starts.  With N > 1 every rank holds a
full replica and its own batches (weak scaling) and the value is the aggregate over ranks.

Workload: the largest BASELINE config that fits one GPU's step budget, C3 (CIKM-Cup-2016 stand-in: d = 128, 3 layers; C4
(Amazon full catalog stand-in, same model shape, E = 3.3 M) is the per-GPU replica of the 8-GPU config).  --config C1 / C2 / C4 / C5 select the others (C5 on one GPU: 0.43 s per step; one warm-up step is enough - Adam's state is created before it).

`--gpus N` without a torchrun environment launches itself: the parent starts N child processes (one per GPU) BEFORE it
touches the GPU and forwards rank 0's JSON line; under `python -m torch.distributed.run` it uses the ranks it was given.

One JSON line is printed by rank 0.  It carries
  roofline                    the aggregation kernel the step is dominated by, against the HBM roofline: K5 (node->hyperedge gather-sum)
                              where the step launches it, else the interactive layer's gather launch - the pair sums of its node-level form
                              (ihg_node_pair_sums: per node the sums over its hyperedges' other two members; the default at d = 64 / 128 / 256), or K7's
                              hyperedge->node launch of its hyperedge form (IHG_NODE_LEVEL_FORWARD=0).  `achieved` / `frac` = COMPULSORY HBM bytes per launch (every
                              source row once + stores + ids) / the kernel's average duration measured with HIP events on the launch
                              stream inside the timed region; `frac_algorithmic` / `algorithmic_gbs` = the SURVEY §8 d3 byte model (every gathered
                              row counted); `traffic` = PMC-measured bytes per launch from the newest committed profile of this exact workload
                              (profiles/r*/pmc_traffic_<config>.json; NOT measured in this run: the object names the file and its commit and
                              carries the number only when that profile's kernel time is within 10 % of this run's, `traffic_refused` otherwise);
  roofline_node_to_hyperedge  K5 at this workload, launched on its own after the timed region (same fields);
  roofline_hyperedge_to_node  one object per K7 launch role (edge features -> nodes, member gradients -> nodes, two-hop ...), each with
                              its own byte counts;
  roofline_interaction        the interactive layer's contractions (node-level form: contraction per node, member gradients per hyperedge, weight
                              gradients per node; flops = the multiply-adds of the algorithm in use) against the matrix-core peak of the arithmetic
                              they run in (fp32 MFMA, or for d = 64 / 128 / 256 the 16-bit peak / 3 - two fp16 terms per operand: node-level contraction, member gradients - or / 6 -
                              three bf16 terms: the hyperedge form's kernels), with the clocks and matrix-pipe occupancy of
                              the newest committed counter pass (`profiled_clock`);
  gradient_exchange           (N > 1) mode, backend, gradient bytes per rank, every rank's ms per step and the time its stream spent in the exchange;
  recorded_step_ms_per_step   the same step replayed from one recorded hipGraph (ihgnn_amd/captured_step.py); NOT the headline;
  cpu_baseline                the CPU oracle (= the reference's PyTorch-CPU op sequence) timed on this box's host cores on a stated
                              sub-sample of the same config; cpu_baseline_c1_full_size: the oracle on BASELINE configs[0] at FULL size, with the
                              HIP path timed on the identical input.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

WORKLOAD_NOTES = {
    'C1': 'C1 = BASELINE configs[0]: synthetic 1k-user / 1k-item / 500-query hypergraph (the reference\'s CPU-runnable case);',
    'C2': 'C2: size-matched synthetic stand-in for BASELINE configs[1] (Amazon-Electronics subset; the corpus is not in the image);',
    'C3': 'C3: size-matched synthetic stand-in for BASELINE configs[2] (CIKM-Cup-2016 Track 2, dim 128, 3 layers; the corpus is not in the image; '
          'the same model shape as configs[3], whose own stand-in is --config C4);',
    'C4': 'C4: size-matched synthetic stand-in for BASELINE configs[3] (Amazon full catalog = the five Amazon 5-core corpora of the reference\'s Main.py:35-39 '
          'as one graph: 317,713 users / 148,456 items / 3.15 M reviews -> 3.3 M training hyperedges; dim 128, 3 layers; one replica per GPU; the corpus is not in the image);',
    'C5': 'C5 = BASELINE configs[4]: synthetic power-law 10M-node / 50M-hyperedge hypergraph;',
}
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md); a float4 streaming copy reaches ~6290
MFMA_F32_PEAK_TF = 157.3       # dense fp32 MFMA peak (v_mfma_f32_32x32x2_f32)
MFMA_BF16_PEAK_TF = 2500.0     # dense bf16 / fp16 MFMA peak (MI355X_MICROARCH.md); the split arithmetic spends three fp16 or six bf16 products per fp32 multiply


def split_arithmetic(dim, order, direction='any'):
    """True when the library runs this shape's contractions through exactly split fp32 operands on the 16-bit matrix pipe (csrc/split_arith.hip): orders 2 and 3 at
    d = 64 / 128 / 256."""
    return order in (2, 3) and os.environ.get('IHG_INTERACT_ARITH') != 'f32' and dim in (64, 128, 256)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--config', default='C3', help='synth.CONFIGS key (C1 | C2 | C3 | C4 | C5)')
    ap.add_argument('--order', type=int, default=3)
    ap.add_argument('--dim', type=int, default=0, help='embedding width instead of the config\'s (the reference\'s default is --emb 32, Helpers/GlobalSettings.py:30)')
    ap.add_argument('--layer', default='ihgnn', choices=['ihgnn', 'hgcn'])
    ap.add_argument('--full', action='store_true', help='measure more than the headline: roofline and per-kernel figures (HIP events around the roofline kernel inside '
                                                        'the timed region), the untimed extra passes and the CPU baseline (each can be left out with its --no-* switch)')
    ap.add_argument('--dump-outputs', metavar='DIR', help='after the timed steps, write the loss and the parameters the last timed step left as DIR/<name>.npy (float32; '
                                                          'tables above 1 MiB as a fixed sample of their rows, under 64 MB in all)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--cpu-scale', type=float, default=0.125, help='fraction of the workload the CPU baseline runs on (C3: ~3 s per oracle step on 32 threads; 7 steps)')
    ap.add_argument('--no-kernel-events', action='store_true', help='do not bracket kernels with HIP events')
    ap.add_argument('--no-extras', action='store_true', help='skip the untimed extra passes (per-kernel table, restricted last layer, forward only)')
    ap.add_argument('--scale', type=float, default=1.0, help='shrink every count of the workload (exploratory runs of the big configs)')
    ap.add_argument('--union-of-ranks', type=int, default=1, help='NOT the headline: batches of 1,100 x K rows on ONE GPU - what a rank\'s step costs under the cotangent exchange '
                                                                  'at K ranks, whose backward runs on the union of the ranks\' batch rows (DESIGN.md section 7); prints union_of_ranks in config')
    ap.add_argument('--backend', default='nccl', help='torch.distributed backend for --gpus > 1 (nccl = RCCL; gloo only for smoke tests)')
    ap.add_argument('--device', type=int, default=-1, help='force every rank onto this GPU ordinal (single-GPU smoke test of the N-rank path)')
    ap.add_argument('--sync', default='auto', choices=['auto', 'cotangent', 'flat', 'bucketed', 'sharded'],
                    help='gradient exchange for --gpus > 1: auto (ihgnn_amd.distributed.choose_gradient_sync: cotangent wherever the fused batch tail runs) | cotangent: all-gather of '
                         'the batch rows\' cotangents, propagation backward on the union, no dense exchange | one flat all-reduce | per-bucket all-reduces from a side stream | '
                         'reduce-scatter + sharded Adam + all-gather')
    args = ap.parse_args()
    if not args.full:
        # a plain run does only what the headline needs: no HIP events in the timed region, no extra passes after it, no CPU baseline
        args.no_cpu_baseline = args.no_extras = args.no_kernel_events = True
    return args


DUMP_LIMIT_BYTES = 56 << 20        # --dump-outputs: the arrays of all files together (under 64 MB with the .npy headers)
DUMP_WHOLE_BYTES = 1 << 20         # a parameter up to this size is written whole, a larger one as a sample of its rows


def dump_outputs(out_dir, loss, model):
    """--dump-outputs: what a caller of the timed step holds after the last timed step - its loss and every parameter as Adam left it - as float32
    DIR/loss.npy and DIR/param.<name>.npy.  The parameters above DUMP_WHOLE_BYTES share what is left of DUMP_LIMIT_BYTES equally, each written as the rows
    a generator of fixed seed picks (sorted): the same rows in every run and every build at the same shapes."""
    import numpy as np
    import torch
    params = [(name, p.detach()) for name, p in model.named_parameters()]
    whole = [(name, p) for name, p in params if 4 * p.numel() <= DUMP_WHOLE_BYTES]
    sampled = [(name, p) for name, p in params if 4 * p.numel() > DUMP_WHOLE_BYTES]
    share = (DUMP_LIMIT_BYTES - 4 - sum(4 * p.numel() for _, p in whole)) // max(len(sampled), 1)
    arrays = {'loss': loss.detach().reshape(1)}
    arrays.update((f'param.{name}', p) for name, p in whole)
    for name, p in sampled:
        rows = p.shape[0]
        keep = min(rows, share // (4 * max(p[0].numel(), 1)))
        pick = np.sort(np.random.default_rng(0).choice(rows, keep, replace=False))
        arrays[f'param.{name}'] = p[torch.from_numpy(pick).to(p.device)]
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        a = t.float().cpu().numpy()
        total += a.nbytes
        np.save(os.path.join(out_dir, name + '.npy'), a)
    assert total <= DUMP_LIMIT_BYTES, total


def launch_ranks(args) -> int:
    """Parent of a self-launched N-rank run.  Nothing here initialises the GPU: the children do."""
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    children = []
    for rank in range(args.gpus):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        children.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                         stdout=None if rank == 0 else subprocess.DEVNULL))
    codes = []
    deadline = None
    while children:
        for c in list(children):
            rc = c.poll()
            if rc is None:
                continue
            children.remove(c)
            codes.append(rc)
            if rc != 0 and deadline is None:
                deadline = time.time() + 30          # a rank died: give the others a moment, then stop them (they would wait forever)
        if deadline is not None and time.time() > deadline:
            for c in children:
                c.kill()
        time.sleep(0.05)
    return max(abs(c) for c in codes) if codes else 1


def build_model(ds, dev, layer, layers, order, dim):
    import torch
    from ihgnn_amd.Models import HGCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn
    torch.manual_seed(0)
    layer_t = IHGNNLayer if layer == 'ihgnn' else HGCNLayer
    return RawGnn(dev, ds, dim, layer_t, layers, order, False, HemPredictionLayer, 0.5).to(dev)


CPU_BASELINE_THREADS = 32     # torch threads of the CPU leg: min(this, host cores).  FIXED per host (rounds 4 / 5 chose it with a one-step probe and printed 3.05e5 on 32 threads,
                              # then 2.58e5 on 8: the probe's noise moved the stated baseline by 15 %); PyTorch-CPU does not scale past a few dozen threads on this op mix


def cpu_baseline(config, layer, layers, order, dim, scale, runs=3, steps_per_run=2):
    """Time the oracle's full training step on the host cores, on a `scale` sub-sample of the SAME config (every count scaled): one warm-up step, then `runs` timed runs
    of `steps_per_run` steps each; `value` is the MEDIAN run, the spread (slowest / fastest run) is printed beside it.  The thread count is a function of the host's core
    count alone (min(cores, CPU_BASELINE_THREADS))."""
    import numpy as np
    import torch
    from ihgnn_amd import synth
    from oracle import ihgnn_ref as ref
    host = os.cpu_count() or 1
    cores = min(host, CPU_BASELINE_THREADS)
    rng = np.random.default_rng(1)
    w = synth.draw_config(config, scale=scale)
    g = ref.HyperGraph(w.triples, w.user_count, w.query_count, w.item_count)
    torch.manual_seed(0)
    m = ref.OracleRawGnn(g, torch.from_numpy(w.bag_words + 1), torch.from_numpy(w.bag_offsets), w.vocab_size, dim, layer, layers, order)
    with torch.no_grad():
        for p in m.parameters():
            p.uniform_(-0.1, 0.1)
    opt = torch.optim.Adam(m.parameters(), 1e-3)
    lossf = torch.nn.BCEWithLogitsLoss()

    def step():
        u = torch.from_numpy(rng.integers(0, w.user_count, 1100)); q = torch.from_numpy(rng.integers(0, w.query_count, 1100))
        i = torch.from_numpy(rng.integers(0, w.item_count, 1100))
        y = torch.cat([torch.ones(100), torch.zeros(1000)])
        loss = lossf(m(u, q, i), y)
        loss.backward(); opt.step(); opt.zero_grad()

    before = torch.get_num_threads()
    torch.set_num_threads(cores)
    step()                                   # warm-up
    rates, total_s = [], 0.0
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(steps_per_run):
            step()
        dt = time.perf_counter() - t0
        total_s += dt
        rates.append(w.edge_count * layers * steps_per_run / dt)
    torch.set_num_threads(before)
    rates.sort()
    median = rates[len(rates) // 2]
    n = runs * steps_per_run
    return dict(value=median, unit='hyperedges/s', cores=cores, kind='port',
                sample=f'{n} full training steps of the PyTorch-CPU oracle (reference op sequence) on a {scale:g}x sub-sample of '
                       f'{config} (every count scaled: E={w.edge_count}, N={w.node_count}, d={dim}, {layers} layers), after one warm-up step; value = median of {runs} runs of '
                       f'{steps_per_run} steps; {cores} threads = min(host cores, {CPU_BASELINE_THREADS}) on a {host}-core host, torch {torch.__version__}',
                runs=[round(r, 1) for r in rates], spread=round(rates[-1] / rates[0], 3), ms_per_step=1e3 * total_s / n, cpu_seconds=round(total_s, 1))


def mfma_pass_clocks(config):
    """Clock and matrix-pipe occupancy of the interact kernels from the newest committed MFMA counter pass (profiles/r*/..._pmc_mfma.json;
    rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE over tools/kbench.py at C3) - NOT measured in this run."""
    import glob
    files = sorted(glob.glob(os.path.join(REPO, 'profiles', 'r*', '*_pmc_mfma.json')), key=lambda f: (int(os.path.basename(os.path.dirname(f))[1:]), os.path.basename(f)))
    docs = [(f, json.load(open(f))) for f in files]
    docs = [(f, d) for f, d in docs if f'--config {config} ' in d.get('command', '') + ' ']      # the pass over THIS workload
    if not docs:
        return None
    files, doc = [docs[-1][0]], docs[-1][1]
    return dict(source=os.path.relpath(files[-1], REPO), commit=doc.get('commit', 'unrecorded'),
                kernels={k: dict(clock_ghz=v.get('clock_ghz'), mfma_busy_fraction=v.get('mfma_busy_fraction'), avg_us_under_pmc=v.get('avg_us_under_pmc'))
                         for k, v in doc.get('kernels', {}).items()})


def k7_roles(table, E, N, dim, layout, table_steps):
    """One roofline object per K7 launch role.  Bytes per launch:
         algorithmic  = every gathered row counted (12 d + 12 per incidence triple + (N/E)(4 d + 8) per output row)
         compulsory   = every source row once + the ids + the output rows (what must cross the HBM pins at least once).
    E here = the ROWS the launches walk: the layout's distinct hyperedges (layout.edge_count; = the workload's E unless the layout carries multiplicities)."""
    row = 4 * dim
    from ihgnn_amd import ops as _ops
    weighted = layout.edge_weight is not None
    # the first-order layers' launches walk the MERGED two-hop list (layout.two_hop_merged: one weighted entry per distinct (destination, source) pair,
    # 4 B id + 4 B weight) where the layout says so (>= 25 % repeats; ops.two_hop_merged_for): fewer gathers than the 6 E of the plain list
    merged = _ops.two_hop_merged_for(layout)
    hop = layout.two_hop_merged()[0].nnz if merged else 6 * E
    hop_ids = 8 * hop if merged else 24 * E
    # member-gradient buffers beyond ops.MEMBER_BUFFER_LIMIT_BYTES are produced and scattered in hyperedge chunks (config C5): a launch walks 1 / chunks of the rows
    c3 = max(1, -(-(3 * E * row) // _ops.MEMBER_BUFFER_LIMIT_BYTES))
    c2 = max(1, -(-(2 * E * row) // _ops.MEMBER_BUFFER_LIMIT_BYTES))
    w4 = 4 if weighted else 0                                 # a multiplicity per hyperedge row / per pair
    roles = {
        # name: (source rows, gathers, id bytes, what)
        'k7.edges_to_nodes': (E, 3 * E, 12 * E + w4 * E, 'forward of the interactive layer: [E,d] hyperedge features -> [N,d] (x Dv^-1)'),
        'k7.first_order_gradient': (E, 3 * E, 12 * E, 'backward: [E,d] cotangent -> d P0 [N,d]'),
        'k7.member_gradients': (3 * E // c3, 3 * E // c3, 12 * E // c3, 'backward: [E,3,d] member gradients -> d H [N,d] (every row read exactly once'
                                + (f'; {c3} hyperedge chunks, bytes per launch' if c3 > 1 else '') + ')'),
        'k7.member_gradients_rows': (2 * E // c2, 2 * E // c2, 8 * E // c2, 'backward: [E,2,d] query / item member gradients -> d H rows of queries and items (the user slot '
                                                          'was summed on chip by the member-gradient kernel); every row read exactly once'
                                     + (f'; {c2} hyperedge chunks, bytes per launch' if c2 > 1 else '')),
        'k7.two_hop': (N, hop + N, hop_ids, 'first-order layer forward: node table -> node table over the ' + ('MERGED (weighted) ' if merged else '') + 'two-hop list (no [E,d] intermediate)'),
        'k7.two_hop_bwd': (N, hop + N, hop_ids, 'first-order layer backward (same operator, scalings swapped)'),
        'k7.two_hop_bwd_masked': (N, hop + N, hop_ids, 'backward of the LAST first-order layer: its cotangent is zero outside the 3B batch rows (the output feeds the batch '
                                                          'tail only), the pull skips the gathers of the zero rows - same gradient; bytes as for the dense pull (an upper bound)'),
        'k7.edges_to_nodes_bwd_of_k5': (E, 3 * E, 12 * E, 'backward of a K5 launch'),
        'k7.two_hop_first_order_gradient': (N, hop + N, hop_ids, 'backward of the interactive layer, first-order part: the two-hop operator on the node-level cotangent ([E, d] tables beyond ops.FIRST_ORDER_TWO_HOP_BYTES: config C5)'),
        'node_pair_sums': (N, 6 * E, 24 * E + 3 * w4 * E, 'interactive layer forward, node-level form: node table -> [N,3d] pair sums over hop2_csr (the output row is 3 d wide'
                                                            + ('; one weighted pair per DISTINCT hyperedge of a node' if weighted else '') + ')', 3),
    }
    out = {}
    for name, (src_rows, gathers, id_bytes, what, *rest) in roles.items():
        if name not in table:
            continue
        out_row = (rest[0] if rest else 1) * row
        t = table[name]['avg_us'] * 1e-6
        algorithmic = gathers * row + id_bytes + N * (out_row + 8)
        compulsory = src_rows * row + id_bytes + N * (out_row + 8)
        out[name] = dict(what=what, avg_us=round(table[name]['avg_us'], 2), launches_per_step=table[name]['launches'] / table_steps,
                         compulsory_bytes=compulsory, achieved=round(compulsory / t / 1e9, 1), frac=round(compulsory / t / 1e9 / HBM_PEAK_GBS, 4),
                         algorithmic_bytes=algorithmic, algorithmic_gbs=round(algorithmic / t / 1e9, 1))
    return out


def gather_stress(dev, dim=64, rounds=6):
    """K5 where every row gather really is an HBM access: uniform members over a node table far larger than the Infinity Cache
    (1.07 GB: 4.2 M nodes at d = 64, 2.1 M at d = 128, 1.05 M at d = 256; one hyperedge per node-table row, about).  Here the SURVEY §8 d3 byte model
    (16 d + 12 B per hyperedge) is also (almost) the compulsory traffic, so algorithmic rate = HBM rate; the microarch guide's figure for random whole rows
    (>= 1 KiB: d = 256) gathered into registers from a buffer far larger than the Infinity Cache is 5.5-5.8 TB/s."""
    import numpy as np
    import torch
    from ihgnn_amd import ops
    n_nodes, n_edges = 4_200_000 * 64 // dim, 4_000_000 * 64 // dim
    rng = np.random.default_rng(77)
    i3 = torch.from_numpy(rng.integers(0, n_nodes, (n_edges, 3), dtype=np.int64).astype(np.int32)).to(dev)
    x = torch.randn(n_nodes, dim, device=dev)
    out = torch.empty(n_edges, dim, device=dev)
    flush = torch.empty(96 << 20, device=dev)                   # 384 MB written between launches: nothing of x survives in the caches
    times = []
    for r in range(rounds + 1):
        flush.fill_(float(r))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.edge_gather_sum_raw(x, i3, out=out)
        b.record()
        torch.cuda.synchronize()
        if r:
            times.append(a.elapsed_time(b) * 1e-3)
    t = sum(times) / len(times)
    touched = int(torch.unique(i3.reshape(-1)).numel())
    algorithmic = n_edges * (16 * dim + 12)
    compulsory = touched * 4 * dim + n_edges * 4 * dim + 12 * n_edges
    return dict(bound='hbm', kernel='edge_gather_sum (K5) on an HBM-resident table', workload=f'uniform members, N={n_nodes} (table {n_nodes * dim * 4 / 1e9:.2f} GB), E={n_edges}, d={dim}',
                avg_us=round(t * 1e6, 1), launches=len(times), algorithmic_bytes_per_launch=algorithmic, achieved=round(algorithmic / t / 1e9, 1),
                peak=HBM_PEAK_GBS, unit='GB/s', frac=round(algorithmic / t / 1e9 / HBM_PEAK_GBS, 4), compulsory_bytes_per_launch=compulsory,
                compulsory_gbs=round(compulsory / t / 1e9, 1), frac_compulsory=round(compulsory / t / 1e9 / HBM_PEAK_GBS, 4), hyperedges_per_s=round(n_edges / t, 1),
                target=0.40, target_met=bool(algorithmic / t / 1e9 / HBM_PEAK_GBS >= 0.40),
                target_definition='north_star: >= 40 % of the HBM roofline on the node -> hyperedge gather-reduce, priced as SURVEY §8 d3 prices it: ALGORITHMIC bytes '
                                  '(16 d + 12 B per hyperedge) / time >= 3.2 TB/s.  On this table the algorithmic bytes ARE HBM traffic (no cache residency), so frac is a true roofline fraction',
                note=f'every gathered row is counted: with 3 uniform draws per hyperedge from {n_nodes / 1e6:.2f} M rows a row is re-read 2.9 times on average, at random '
                     'distances in a 1.07 GB table (Infinity Cache 256 MB): the algorithmic rate is an HBM + cache-hit mix, the compulsory rate the floor')


def main():
    args = parse()
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        raise SystemExit(launch_ranks(args))

    import numpy as np
    import torch
    import torch.distributed as dist
    from ihgnn_amd import distributed as ihg_dist, ops as ihg_ops, profiler, synth
    from ihgnn_amd.Dataset import GraphDataset

    rank, local_rank, world = ihg_dist.init_from_env(args.backend if args.gpus > 1 else None)
    if world != args.gpus:
        raise SystemExit(f'--gpus {args.gpus} but WORLD_SIZE={world}')
    dev = torch.device(f'cuda:{args.device if args.device >= 0 else local_rank}')
    torch.cuda.set_device(dev)

    cfg = synth.CONFIGS[args.config]
    dim, layers = args.dim or cfg['dim'], cfg['layers']
    w = synth.draw_config(args.config, scale=args.scale)
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets,
                                  w.triples, device=dev)
    model = build_model(ds, dev, args.layer, layers, args.order, dim)
    layout = ds.hypergraph.layout
    from ihgnn_amd.optim import Adam
    lossf = torch.nn.BCEWithLogitsLoss()
    sync = None
    sync_mode = args.sync
    if world > 1 or ihg_dist.force_collectives():            # (IHG_FORCE_COLLECTIVES=1: a one-rank process group that really issues the collectives)
        if sync_mode == 'auto':                              # by the gradient bytes and the loss path: cotangent for every BASELINE config (fused batch tail); C5's 9.4 GB
            sync_mode = ihg_dist.choose_gradient_sync(4 * sum(p.numel() for p in model.parameters()), world, model.supports_fused_loss(lossf),
                                                      ihg_dist.cotangent_bytes_per_rank(1100, model.compute_width * (layers + 1)))      # of gradients otherwise: sharded
        sync = ihg_dist.make_gradient_sync(model, sync_mode)
        sync.broadcast_parameters(0)
        if sync_mode == 'cotangent':
            sync.equal_batches, sync.time_exchanges = True, True      # (every rank draws batches of 1,100 rows)
    opt = sync.optimizer(1e-3) if (sync is not None and sync.owns_optimizer) else Adam(model.parameters(), 1e-3, weight_decay=0)
    if hasattr(opt, 'ensure_state'):
        # Adam's moment buffers exist BEFORE the first step: otherwise they are created at the end of step 1, step 2 meets a different memory pattern and the caching
        # allocator grows its pool again (C5: two more device allocations, 47 GB, and a second step of 1.6 s instead of 0.43 s) - with them in place ONE warm-up step is enough
        opt.ensure_state()
    batches = list(ds.sample_batches(100 * max(args.union_of_ranks, 1), args.steps + args.warmup, seed=1000 + rank))
    fused_loss = model.supports_fused_loss(lossf)
    # headline = the step with every layer evaluated over ALL rows (each hyperedge through both phases of each layer)
    model.batch_rows_only_last_layer = False

    exchange_events = []                                     # (before, after) the gradient exchange on the step's stream, timed region only
    cotangent = sync is not None and getattr(sync, 'mode', None) == 'cotangent'
    if cotangent and not fused_loss:
        raise SystemExit('--sync cotangent needs the fused batch tail (IHGNN / HGCN layers, BCEWithLogitsLoss)')

    def step(k, timed=False):
        u, q, i, y = batches[k]
        if cotangent:
            if timed:
                sync.exchange_events = []
            loss = model.bce_loss(u, q, i, y, cotangent_sync=sync)      # (the exchange - two all-gathers - happens inside: before the forward and in the tail's backward)
        else:
            loss = model.bce_loss(u, q, i, y) if fused_loss else lossf(model(u, q, i), y)       # what train_and_get_avg_loss does
        ihg_ops.backward(loss)                               # loss.backward() with a cached root gradient
        if sync is not None:
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            sync.average_gradients()
            if timed:
                e1.record()
                exchange_events.append((e0, e1))
                if cotangent:
                    exchange_events.extend(sync.exchange_events)
        opt.step()
        if sync is not None:
            sync.zero_grad()
        else:
            opt.zero_grad()
        return loss

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    for k in range(args.warmup):
        step(k)
    # Inside the timed region only the roofline kernel (K5 where the step launches it, else the interactive layer's gather launch - the pair sums of its node-level
    # form, or K7's hyperedge -> node launch of its hyperedge form) is bracketed by HIP events: a pair of timing events costs a few
    # microseconds of stream time, and bracketing all launches of a step would inflate it.
    if not args.no_kernel_events:
        profiler.start(only={'edge_gather_sum', 'k7.edges_to_nodes', 'node_pair_sums'} | ({'k7.two_hop'} if args.layer == 'hgcn' else set()))
    fence()
    t0 = time.perf_counter()
    for k in range(args.warmup, args.warmup + args.steps):
        last = step(k, timed=True)
    fence()
    my_elapsed = time.perf_counter() - t0
    elapsed = max_over_ranks(my_elapsed)
    # per-rank breakdown for the scaling run: every rank's own step time and the time its stream sat in the gradient exchange (events on the
    # step's stream around average_gradients(): what of the exchange is NOT hidden behind the backward)
    exchange = None
    if sync is not None:
        exposed = sum(a.elapsed_time(b) for a, b in exchange_events) / max(args.steps, 1)
        mine = torch.tensor([1e3 * my_elapsed / args.steps, exposed], dtype=torch.float64, device=dev)
        table_ranks = [torch.zeros_like(mine) for _ in range(world)]
        if dist.is_initialized():
            dist.all_gather(table_ranks, mine)
        else:
            table_ranks = [mine]
        flat = getattr(sync, '_grads_padded', None) if getattr(sync, '_grads_padded', None) is not None else sync.flat
        dense_bytes = int(sum(p.numel() * p.element_size() for p in model.parameters() if p.requires_grad))
        exchange = dict(mode=sync_mode, requested=args.sync, backend=dist.get_backend() if dist.is_initialized() else None, ranks=world,
                        gradient_bytes_per_rank=dense_bytes,
                        # what this rank hands to the collective(s) of one step and what it receives from the other ranks
                        bytes_sent_per_rank=int(sync.sent_bytes) if cotangent else int(flat.numel() * flat.element_size()),
                        bytes_received_per_rank=int(sync.exchanged_bytes) if cotangent else int(2 * (world - 1) / max(world, 1) * flat.numel() * flat.element_size()),
                        bytes_note=('cotangent: two all-gathers per step - the batch node rows (3 B int64) before the forward, the batch rows\' cotangents (3 B x (D + 4) f32) in the '
                                    'tail\'s backward; received = (W - 1) x sent; the dense gradients (gradient_bytes_per_rank) never cross' if cotangent else
                                    'dense gradients through a ring all-reduce / reduce-scatter + all-gather: 2 (W - 1) / W x the buffer in and out per rank'),
                        per_rank=[dict(rank=r, ms_per_step=round(float(t[0]), 4), exposed_exchange_ms_per_step=round(float(t[1]), 4)) for r, t in enumerate(table_ranks)],
                        exposed_exchange_ms_per_step_max=round(max(float(t[1]) for t in table_ranks), 4),
                        note='exposed = HIP events on the step\'s stream around average_gradients() (cotangent: around its two all-gathers): the part of the exchange the stream '
                             'waits for (bucketed: the dense bucket overlaps the backward, the embedding tables\' buckets are produced by its last kernels)')
    profiler.stop()
    kernels = profiler.summary() if not args.no_kernel_events else {}
    final_loss = float(last.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last, model)         # before the extra passes below step the model again

    table, table_steps, restricted_elapsed, fwd_elapsed, stress, eval_stats, f32_elapsed, k5_alone = {}, min(args.steps, 5), None, None, None, None, None, None
    dense_cot_elapsed = None
    recorded_elapsed = None
    N_nodes = w.node_count
    if not args.no_extras:
        # per-kernel table (K7 roles, MFMA kernels): a second, untimed pass over the same batches with every launch bracketed
        if not args.no_kernel_events:
            profiler.start()
            for k in range(args.warmup, args.warmup + table_steps):
                step(k)
            fence()
            profiler.stop()
            table = profiler.summary()
        # the same step with the d = 128 contractions on the fp32-MFMA kernels (the library reads the switch at every call)
        if split_arithmetic(dim, args.order):
            os.environ['IHG_INTERACT_ARITH'] = 'f32'
            for k in range(2):
                step(k)
            fence()
            t3 = time.perf_counter()
            n_3 = min(args.steps, 10)
            for k in range(args.warmup, args.warmup + n_3):
                step(k)
            fence()
            f32_elapsed = max_over_ranks((time.perf_counter() - t3) / n_3)
            del os.environ['IHG_INTERACT_ARITH']
        # the same step with the last layer's backward pulling every row of its (zero outside the batch rows) cotangent
        from ihgnn_amd import ops as _ops
        if _ops.SPARSE_LAST_COTANGENT:
            _ops.SPARSE_LAST_COTANGENT = False
            for k in range(2):
                step(k)
            fence()
            t4 = time.perf_counter()
            n_4 = min(args.steps, 10)
            for k in range(args.warmup, args.warmup + n_4):
                step(k)
            fence()
            dense_cot_elapsed = max_over_ranks((time.perf_counter() - t4) / n_4)
            _ops.SPARSE_LAST_COTANGENT = True
        # the same step with the last layer's hyperedge -> node pass evaluated only at the rows the loss reads (split rows + the 3B
        # batch rows): identical loss and gradients, what the training loop runs by default; reported beside the headline
        model.batch_rows_only_last_layer = True
        for k in range(2):
            step(k)
        fence()
        t2 = time.perf_counter()
        n_r = min(args.steps, 10)
        for k in range(args.warmup, args.warmup + n_r):
            step(k)
        fence()
        restricted_elapsed = max_over_ranks((time.perf_counter() - t2) / n_r)
        model.batch_rows_only_last_layer = False
        # forward-only propagation (the save_features_for_test path)
        with torch.no_grad():
            model.propagate(); torch.cuda.synchronize()
            t1 = time.perf_counter()
            n_f = max(min(args.steps, 10), 3)
            for _ in range(n_f):
                model.propagate()
            torch.cuda.synchronize()
            fwd_elapsed = (time.perf_counter() - t1) / n_f
        # the same step replayed from a recording (forward + backward + Adam as one hipGraph): reported beside the headline; at C3 the GPU is
        # the bound (the kernels of a step add up to its wall time), so this shows what the host's launch path costs - nothing, there
        if world == 1 and fused_loss:
            try:
                from ihgnn_amd.captured_step import CapturedTrainingStep
                recorded_step = CapturedTrainingStep(model, opt, int(batches[0][0].shape[0]), warmup_batch=batches[0])
                for k in range(2):
                    recorded_step.step(*batches[k])
                fence()
                t6 = time.perf_counter()
                n_6 = min(args.steps, 10)
                for k in range(args.warmup, args.warmup + n_6):
                    recorded_step.step(*batches[k])
                fence()
                recorded_elapsed = (time.perf_counter() - t6) / n_6
                del recorded_step
                opt.zero_grad(set_to_none=True)
            except Exception as exc:                         # a recording is an extra: report why it is missing, keep the bench line
                recorded_elapsed = f'{type(exc).__name__}: {exc}'
        stress = {f'd{d_}': gather_stress(dev, d_) for d_ in (64, 128, 256)} if rank == 0 else None      # (rows of 256 B / 512 B / 1 KiB)
        # K5 at this workload, launched on its own (it is not part of a step whose layer-0 backward forms the hyperedges' cotangents in the
        # member-gradient kernel): the node -> hyperedge gather-sum of a [N, d] table with the layer's Dv^-1 scaling
        if rank == 0 and not args.no_kernel_events:
            from ihgnn_amd import ops
            xk = torch.randn(N_nodes, dim, device=dev)
            for _ in range(2):
                ops.edge_gather_sum_raw(xk, layout.i3, layout.inv_deg)
            profiler.start(only={'edge_gather_sum'})
            for _ in range(6):
                ops.edge_gather_sum_raw(xk, layout.i3, layout.inv_deg)
            profiler.stop()
            k5_alone = profiler.summary().get('edge_gather_sum')
            del xk
        # evaluation: cached propagation + fused scoring / running top-10 of 4,096 (user, query) pairs against every item
        eval_stats = None
        if rank == 0:
            with torch.no_grad():
                model.save_features_for_test()
                rng = np.random.default_rng(3)
                eu = torch.from_numpy(rng.integers(0, w.user_count, 4096)).to(dev)
                eq = torch.from_numpy(rng.integers(0, w.query_count, 4096)).to(dev)
                model.top_items(eu, eq)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                for _ in range(3):
                    model.top_items(eu, eq)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t3) / 3
                model.clear_saved_feature()
            flops = 2.0 * 4096 * dim * (layers + 1) * w.item_count
            eval_stats = dict(pairs=4096, items=w.item_count, width=dim * (layers + 1), ms=round(1e3 * dt, 3), logs_per_s=round(4096 / dt, 1),
                              tflops=round(flops / dt / 1e12, 1), frac_of_f32_mfma_peak=round(flops / dt / 1e12 / MFMA_F32_PEAK_TF, 4),
                              peak=round(MFMA_BF16_PEAK_TF / 3, 1), frac=round(flops / dt / 1e12 / (MFMA_BF16_PEAK_TF / 3), 4),
                              kernel='ihg_score_topk: HEM scores of every (pair, item) through two fp16 terms per operand (three v_mfma_f32_32x32x16_f16 products per multiply, '
                                     'fp32 accumulation; peak = dense fp16 MFMA peak / 3, flops counted as fp32 multiply-adds) + running top-10 per pair, no [pairs, items] matrix')

    if rank != 0:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    E, N = w.edge_count, w.node_count
    value = world * E * layers * args.steps / elapsed      # the metric counts the reference's hyperedges: one per interaction, duplicates included (Helpers/Graph.py:107-118)
    Er = layout.edge_count                                  # rows the kernels walk: the layout's DISTINCT hyperedges (= E unless it carries multiplicities, C5)
    N_public, N = N, layout.node_count                      # node rows the kernels walk: the layout's nodes (= the graph's unless it leaves the isolated ones out, C5)
    row = 4 * dim
    touched = int((layout.degree > 0.5).sum().item())
    k5_compulsory = touched * row + Er * row + 12 * Er        # every touched node row once + the [E,d] store + the ids
    k5_algorithmic = Er * (16 * dim + 12)                      # 3 ids + 3 row reads + 1 row write per hyperedge (row of the launch)
    pmc = None                                                 # HBM bytes per launch from the committed PMC passes (profiles/), newest round first
    pmc_files = []                                             # (--full only: the roofline objects and step_bytes quote them)
    if args.full:
        rounds = sorted((d for d in os.listdir(os.path.join(REPO, 'profiles')) if d.startswith('r') and d[1:].isdigit()), key=lambda d: -int(d[1:]))
        pmc_files = [os.path.join(REPO, 'profiles', r, f'pmc_traffic_{args.config}.json') for r in rounds] + [os.path.join(REPO, 'profiles', 'r1', 'pmc_traffic.json')]
    for pmc_file in pmc_files:
        if os.path.exists(pmc_file):
            cand = json.load(open(pmc_file))
            if (cand.get('workload'), cand.get('dim'), cand.get('edges')) == (args.config, dim, E) and cand.get('rows', E) == Er:
                pmc, pmc_name = cand, os.path.relpath(pmc_file, REPO)
                break

    def hbm_roofline(kernel, what, rec, compulsory, algorithmic, bytes_note, algorithmic_note, pmc_key, measured):
        t = rec['avg_us'] * 1e-6
        achieved = compulsory / t / 1e9
        # PMC traffic is NOT measured in this run: it comes from a committed rocprofv3 pass over the same kernel at the same shapes.  It is only
        # carried when that pass's kernel duration agrees with this run's within 10 % (another box, another clock, another kernel version: refused)
        traffic = traffic_refused = None
        if pmc is not None and pmc_key in pmc:
            prof_us = pmc[pmc_key].get('avg_us_under_pmc')
            if prof_us and abs(prof_us - rec['avg_us']) <= 0.10 * rec['avg_us']:
                traffic = pmc[pmc_key]['hbm_bytes_per_launch']
            else:
                traffic_refused = f'committed profile {pmc_name} times this kernel at {prof_us} us, this run at {rec["avg_us"]:.1f} us (> 10 % apart): not carried'
        return dict(bound='hbm', kernel=f'{kernel} ({what})', achieved=round(achieved, 1), peak=HBM_PEAK_GBS, unit='GB/s', frac=round(achieved / HBM_PEAK_GBS, 4),
                    frac_note='frac = COMPULSORY bytes / time / peak (every source row once + stores + ids): what must cross the HBM pins; frac_algorithmic uses SURVEY §8 d3\'s byte model',
                    # (a gather-sum over a cache-resident node table - K5 at d = 64 - re-reads rows out of L2 / the Infinity Cache: its algorithmic rate is
                    #  not an HBM rate and can exceed the peak; no fraction is quoted then)
                    frac_algorithmic=round(algorithmic / t / 1e9 / HBM_PEAK_GBS, 4) if algorithmic / t / 1e9 <= HBM_PEAK_GBS else None,
                    bytes=bytes_note, bytes_per_launch=compulsory, algorithmic_bytes_per_launch=algorithmic, algorithmic_gbs=round(algorithmic / t / 1e9, 1),
                    algorithmic_note=algorithmic_note, traffic=traffic, traffic_gbs=round(traffic / t / 1e9, 1) if traffic else None,
                    traffic_frac=round(traffic / t / 1e9 / HBM_PEAK_GBS, 4) if traffic else None,
                    traffic_source=(f'NOT measured in this run: from the committed profile {pmc_name} (commit {pmc.get("commit", "unrecorded")}; rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, '
                                    f'separate passes, FETCH_SIZE doubled per the gfx950 correction; {pmc[pmc_key].get("source", "in-situ pass")}; kernel time in that pass '
                                    f'{pmc[pmc_key].get("avg_us_under_pmc")} us)') if traffic else None,
                    traffic_refused=traffic_refused,
                    traffic_note='FETCH_SIZE / WRITE_SIZE count at the L2 <-> fabric boundary: L2-miss bytes, Infinity-Cache hits included - an upper '
                                 'bound of the HBM bytes; traffic above the compulsory bytes = rows re-fetched after leaving L2' if traffic else None,
                    avg_us=round(rec['avg_us'], 2), launches=rec['launches'], hyperedges_per_s=round(E / t, 1), rows_per_launch=Er, measured=measured)

    k5_args = ('edge_gather_sum', 'K5 node->hyperedge gather-sum; first-order hyperedge features and the backward of K7', None, k5_compulsory, k5_algorithmic,
               'compulsory HBM bytes per launch: touched node rows once + [E,d] store + ids',
               '16 d + 12 B per hyperedge (SURVEY §8 d3) counts three row gathers per hyperedge; repeats are served by L2 / Infinity Cache, so this rate '
               'is not an HBM rate and may exceed the peak', 'edge_gather_sum')
    roofline = k5_outside = None
    if 'edge_gather_sum' in kernels:                           # the step launches K5: it is the bracketed kernel
        roofline = hbm_roofline(*k5_args[:2], kernels['edge_gather_sum'], *k5_args[3:], 'HIP events on the launch stream, inside the timed region')
    elif 'k7.edges_to_nodes' in kernels:
        # no K5 launch in this step (the layer-0 backward forms the hyperedges' cotangents inside the member-gradient kernel): the bracketed
        # kernel is the hyperedge -> node launch of the interactive layer, the largest of the seven K7 launches that own 40 % of the step
        k7_compulsory = Er * row + 12 * Er + N * (row + 8)     # every hyperedge row once + the member lists + the [N,d] store and its row pointers
        k7_algorithmic = 3 * Er * row + 12 * Er + N * (row + 8)  # every (node, hyperedge) incidence reads its row
        roofline = hbm_roofline('node_segment_sum, role k7.edges_to_nodes', 'K7 hyperedge->node: [E,d] hyperedge features -> [N,d] x Dv^-1, the forward of the interactive layer',
                                kernels['k7.edges_to_nodes'], k7_compulsory, k7_algorithmic,
                                'compulsory HBM bytes per launch: every hyperedge row once + member lists + [N,d] store',
                                '12 d + 12 B per hyperedge + (4 d + 8) B per node (SURVEY §8 d3): every incidence reads its 4 d-byte row; a row is read by its three '
                                'members at unrelated times out of a table (E x 4 d B) far larger than L2 + Infinity Cache, so most of these ARE fabric reads',
                                'k7.edges_to_nodes', 'HIP events on the launch stream, inside the timed region')
    elif 'node_pair_sums' in kernels:
        # the interactive layer runs in its node-level form (no [E, d] tensor, no hyperedge -> node launch): its gather is the pair-sum launch - per node
        # the sums of h[a], h[b], h[a] h[b] over the other two members of its hyperedges - the largest gather launch of the step
        pw = 12 * Er if layout.edge_weight is not None else 0  # a weight per pair where the layout carries multiplicities
        ps_compulsory = N * row + 24 * Er + pw + N * (3 * row + 8)  # every node row once + the pair lists + the [N, 3 d] store and its row pointers
        ps_algorithmic = 6 * Er * row + 24 * Er + pw + N * (3 * row + 8)   # every incidence (of a distinct hyperedge) reads its two other members' rows
        roofline = hbm_roofline('node_pair_sums', 'pair sums of the interactive layer\'s node-level form: [N,d] node table -> [N,3d] (sum h[a] | sum h[b] | sum h[a] h[b] over each '
                                'node\'s hyperedges) - the hyperedge aggregation of the layer\'s forward', kernels['node_pair_sums'], ps_compulsory, ps_algorithmic,
                                'compulsory HBM bytes per launch: every node row once + pair lists (2 ids per incidence) + [N,3d] store',
                                '2 x 4 d B per incidence (3 E incidences) + 24 B of ids per hyperedge + (12 d + 8) B per node: the two other members\' rows of every incidence; '
                                'the node table (N x 4 d B) fits the Infinity Cache at C3, so most of these are cache reads - this rate is not an HBM rate and may exceed the peak',
                                'node_pair_sums', 'HIP events on the launch stream, inside the timed region')
    if args.layer == 'hgcn' and 'k7.two_hop' in kernels:
        # HGCNLayer (GnnLayers.py:142-153) is the pure aggregation layer: Dv^-1/2 H De^-1 H^T Dv^-1/2 (X W + b) - node -> hyperedge scatter-reduce and hyperedge -> node
        # reduce with no per-hyperedge dense work.  The build applies H De^-1 H^T in ONE launch over the two-hop list (no [E, d] round trip), so that launch IS the
        # layer's node -> hyperedge + hyperedge -> node aggregation and it is the bracketed kernel
        hop_merged = ihg_ops.two_hop_merged_for(layout)
        hop_entries = layout.two_hop_merged()[0].nnz if hop_merged else 6 * Er
        th_compulsory = N * row + (8 if hop_merged else 4) * hop_entries + N * (row + 8)      # every node row once + the two-hop list (id, and weight when merged) + the [N, d] store and its row pointers
        th_algorithmic = E * (16 * dim + 12) + E * (12 * dim + 12) + N * (row + 8)    # K5 (16 d + 12) + K7 (12 d + 12 + (N / E)(4 d + 8)) per hyperedge of the reference's formulation
        roofline = hbm_roofline('node_segment_sum, role k7.two_hop', 'HGCN layer: node -> hyperedge -> node aggregation H De^-1 H^T in one pass over the two-hop list', kernels['k7.two_hop'],
                                th_compulsory, th_algorithmic, 'compulsory HBM bytes per launch: every node row once + two-hop lists (2 ids per incidence) + [N,d] store',
                                'SURVEY §8 d3 for the two phases it replaces: K5 16 d + 12 B and K7 12 d + 12 B per hyperedge + (4 d + 8) B per node; the launch gathers 6 E + N rows '
                                'of a node table that fits the Infinity Cache at C2-C4, so this rate is not an HBM rate there and may exceed the peak', 'k7.two_hop',
                                'HIP events on the launch stream, inside the timed region')
    if k5_alone is not None:
        k5_outside = hbm_roofline(*k5_args[:2], k5_alone, *k5_args[3:], 'HIP events on the launch stream; six launches of their own after the timed region (no step launches K5)')
    mfma_roof = None
    if args.layer == 'ihgnn' and args.order in (2, 3) and 'interact_bwd' in table and ('interact_fwd' in table or 'node_interact_fwd' in table):
        # the order-2/3 contraction of layer 0 is the only MFMA-bound piece: 2 m d^2 flop per hyperedge forward
        # (m product blocks after hoisting), twice that backward (member gradients + weight gradients), against fp32 MFMA
        m_blocks = 4 if args.order == 3 else 3
        node_level = 'node_interact_fwd' in table
        # node-level form: the forward contracts 3 + m blocks per NODE (first-order blocks included), the product blocks' weight gradients m blocks per node;
        # the member gradients stay per hyperedge.  Hyperedge form: m blocks per hyperedge forward, 2 m backward (members + weights).
        flops_fwd = 2.0 * (3 + m_blocks) * dim * dim * N if node_level else 2.0 * m_blocks * dim * dim * Er
        f, bw = table['node_interact_fwd' if node_level else 'interact_fwd'], table['interact_bwd']
        bwd_us = bw['avg_us'] * bw['launches'] / table_steps        # the backward may run in several hyperedge chunks
        flops_bwd = 2 * 2.0 * m_blocks * dim * dim * Er
        if 'node_interact_bwd_weight' in table:
            nw = table['node_interact_bwd_weight']
            bwd_us += nw['avg_us'] * nw['launches'] / table_steps
            flops_bwd = 2.0 * m_blocks * dim * dim * Er + 2.0 * m_blocks * dim * dim * N
        dtype_by_products = {
            3: ('f32 operands scaled by a power of two and taken apart into two fp16 terms (22 significand bits), three v_mfma_f32_16x16x32_f16 products per multiply '
                '(hi lo + lo hi + hi hi), f32 accumulate: peak = dense 16-bit MFMA peak / 3, flops counted as fp32 multiply-adds'),
            6: ('f32 operands taken apart exactly into three bf16 terms, six v_mfma_f32_16x16x32_bf16 products per multiply, f32 accumulate: '
                'peak = dense bf16 MFMA peak / 6, flops counted as fp32 multiply-adds'),
            4.5: 'member gradients through two fp16 terms (3 products), weight gradients through three bf16 terms (6 products), equal flops: peak = dense 16-bit MFMA peak / 4.5',
            0: 'f32 in / f32 accumulate (v_mfma_f32_16x16x4_f32 / 32x32x2_f32)'}

        def direction(name, pieces, extra):
            """pieces: (kernel, flops, us, MFMA products per multiply in the split arithmetic); the direction's peak is the flop-weighted harmonic mean of its kernels' peaks."""
            split = split_arithmetic(dim, args.order, name)
            rows, flops_all, us_all, floor_s = [], 0.0, 0.0, 0.0
            for kernel, flops, us, products in pieces:
                products = products if split else 0
                peak = MFMA_BF16_PEAK_TF / products if products else MFMA_F32_PEAK_TF
                rows.append(dict(kernel=kernel, achieved=round(flops / (us * 1e-6) / 1e12, 1), peak=round(peak, 1), frac=round(flops / (us * 1e-6) / (peak * 1e12), 4),
                                 us=round(us, 2), flops=flops, dtype=dtype_by_products[products]))
                flops_all, us_all, floor_s = flops_all + flops, us_all + us, floor_s + flops / (peak * 1e12)
            peak = flops_all / floor_s / 1e12
            return dict(achieved=round(flops_all / (us_all * 1e-6) / 1e12, 1), peak=round(peak, 1), frac=round(flops_all / (us_all * 1e-6) / (peak * 1e12), 4),
                        dtype=rows[0]['dtype'] if len(rows) == 1 else 'per kernel: see `kernels`', kernels=rows,
                        vs_f32_mfma_peak=round(flops_all / (us_all * 1e-6) / (MFMA_F32_PEAK_TF * 1e12), 3), **extra)

        fwd_pieces = [('node_interact_fwd' if node_level else 'interact_fwd', flops_fwd, f['avg_us'], 3 if node_level else 6)]
        bwd_pieces = [('interact_bwd (member gradients)', 2.0 * m_blocks * dim * dim * Er, bw['avg_us'] * bw['launches'] / table_steps, 3)]
        if 'node_interact_bwd_weight' in table:
            bwd_pieces.append(('node_interact_bwd_weight', 2.0 * m_blocks * dim * dim * N, nw['avg_us'] * nw['launches'] / table_steps, 3))
        else:
            bwd_pieces[0] = ('interact_bwd (member + weight gradients, hyperedge form)', flops_bwd, bwd_us, 4.5)
        mfma_roof = dict(bound='mfma', kernel=('node_interact_fwd (node-level contraction, %d blocks per node) + interact_bwd (member gradients, per hyperedge) + node_interact_bwd_weight (per node)' % (3 + m_blocks)
                                               if node_level else 'interact_fwd + interact_bwd (order-%d product blocks of layer 0)' % args.order), unit='TFLOP/s',
                         note='flops are the multiply-adds the algorithm in use performs (the node-level form does E / N times fewer than the hyperedge form for the same result), '
                              'not the hyperedge form\'s count' if node_level else None,
                         f32_mfma_peak=MFMA_F32_PEAK_TF, two_fp16_terms_peak=round(MFMA_BF16_PEAK_TF / 3, 1), three_bf16_terms_peak=round(MFMA_BF16_PEAK_TF / 6, 1),
                         forward=direction('forward', fwd_pieces, dict(flops_per_launch=flops_fwd, avg_us=round(f['avg_us'], 2))),
                         backward=direction('backward', bwd_pieces, dict(flops_per_step=flops_bwd, us_per_step=round(bwd_us, 2))),
                         share_of_step=round((f['avg_us'] + bwd_us) * 1e-3 / (1e3 * elapsed / args.steps), 3),
                         measured='instrumented pass after the timed region (every launch bracketed)',
                         profiled_clock=mfma_pass_clocks(args.config))
    out = {
        'metric': 'hyperedges_aggregated_per_sec', 'value': round(value, 1), 'unit': 'hyperedges/s',
        'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(1e3 * elapsed / args.steps, 4),
        'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': ('f32 (contraction operands 2xfp16, 22-bit; f32 accumulate)' if split_arithmetic(dim, args.order) and args.layer == 'ihgnn' else 'f32'), 'data': 'synthetic',
        'config': {'workload': WORKLOAD_NOTES.get(args.config, args.config) + (f' SCALED x{args.scale:g};' if args.scale != 1.0 else '') +
                               (f' WIDTH OVERRIDE --dim {dim};' if args.dim else '') +
                               f' U={w.user_count} Q={w.query_count} I={w.item_count} E={E}, {cfg["distribution"]} members, '
                               f'dim={dim}, {layers}x{args.layer} layers, interaction order {args.order}, batch 100 pos + 1000 neg' +
                               (f' x {args.union_of_ranks} (--union-of-ranks: the per-rank cost of a {args.union_of_ranks}-rank cotangent-exchange step, NOT the headline)' if args.union_of_ranks > 1 else ''),
                   'step': 'full training step: propagate fwd (every layer over all rows) + BCE + bwd (the last layer\'s backward pulls the 3B non-zero rows of its cotangent) + Adam' +
                           (f' + RCCL gradient exchange ({sync_mode})' if world > 1 else ''),
                   'edges': E, 'nodes': N_public, 'dim': dim, 'layers': layers, 'parallelism': f'dp{world}',
                   # share of the two-hop list's 6 E entries that repeat a (destination, source) pair of their row: merged into weighted entries for the first-order launches
                   'two_hop_duplicates': round(layout.two_hop_duplicate_share, 4), 'two_hop_merged': bool(ihg_ops.two_hop_merged_for(layout)),
                   # interactions that repeat an earlier (user, query, item) triple; where the layout collapses them (>= 25 %: layout.MULTIPLICITY_MIN_SHARE) the kernels walk
                   # distinct_hyperedges rows with a multiplicity each - the metric, the degrees and PpsHyperGraph keep counting every copy (Helpers/Graph.py:107-118)
                   'duplicate_hyperedges': round(layout.duplicate_share, 4), 'hyperedge_multiplicities': layout.edge_weight is not None, 'distinct_hyperedges': Er,
                   # nodes that are in no hyperedge (every layer output exactly zero): where they are >= 25 % the layout leaves them out of its own numbering and the
                   # per-node kernels run on nodes_in_hyperedges rows (layout.COMPACT_MIN_SHARE; RawGnn translates at its edges)
                   'isolated_nodes': round(1.0 - int((layout.public_degree() > 0.5).sum().item()) / max(N_public, 1), 4), 'compact_nodes': bool(layout.compact),
                   'nodes_in_hyperedges': N,
                   'arithmetic': ('f32 results; f32 accumulation everywhere.  Row contractions (node-level contraction and member gradients at d = 64 / 128 / 256, node-level linear '
                                  'maps and their input gradients at d = 128 / 256): operands scaled by a power of two and taken apart into two fp16 terms, three fp16 MFMA products '
                                  'per multiply (error <= 3 x 2^-22 per product) - also the node-level weight gradients of the product blocks (a row\'s two operands scaled against each other); '
                                  'and of the node-level linear maps; the hyperedge form\'s weight gradients (IHG_NODE_LEVEL_WEIGHT=0): three exact bf16 terms, six bf16 MFMA products; '
                                  'both within the fp32-MFMA kernels\' error against float64 (tests/test_gpu_parity.py); IHG_INTERACT_ARITH=f32 selects the fp32-MFMA kernels')
                                 if split_arithmetic(dim, args.order) else 'f32 (fp32 MFMA / VALU)'},
        'final_loss': round(final_loss, 6),
        'gradient_exchange': exchange,
        'roofline': roofline,
        'roofline_hyperedge_to_node': k7_roles(table, Er, N, dim, layout, table_steps) or None,
        'roofline_interaction': mfma_roof,
    }
    if restricted_elapsed is not None:
        out['batch_rows_last_layer_ms_per_step'] = round(1e3 * restricted_elapsed, 4)
        out['batch_rows_last_layer_value'] = round(world * E * layers / restricted_elapsed, 1)
        out['batch_rows_last_layer_note'] = ('same step with the last layer\'s hyperedge->node pass evaluated only at the rows the loss reads '
                                             '(identical loss and gradients; the training loop\'s default); NOT the headline')
    if dense_cot_elapsed is not None:
        out['dense_last_cotangent_ms_per_step'] = round(1e3 * dense_cot_elapsed, 4)
        out['dense_last_cotangent_note'] = ('same full step with the last layer\'s backward pulling all N rows of its cotangent (zero outside the 3B batch rows: '
                                            'the layer\'s output feeds the batch tail only) instead of the 3B rows; identical loss and gradients (IHG_SPARSE_LAST_COTANGENT=0); NOT the headline')
    if isinstance(recorded_elapsed, float):
        out['recorded_step_ms_per_step'] = round(1e3 * recorded_elapsed, 4)
        out['recorded_step_note'] = ('same full step replayed from ONE recorded hipGraph (ihgnn_amd/captured_step.py: forward + backward + Adam, Adam scalars from device '
                                     'memory); identical results; NOT the headline (the headline issues every launch from Python)')
    elif recorded_elapsed is not None:
        out['recorded_step_error'] = recorded_elapsed
    if f32_elapsed is not None:
        out['fp32_mfma_kernels_ms_per_step'] = round(1e3 * f32_elapsed, 4)
        out['fp32_mfma_kernels_note'] = 'same full step with IHG_INTERACT_ARITH=f32 (fp32-MFMA contractions instead of the split-arithmetic ones: two fp16 terms on the default path, three bf16 terms in the forward / weight kernels of the hyperedge form); NOT the headline'
    if fwd_elapsed is not None:
        out['fwd_only_hyperedges_per_s'] = round(E * layers / fwd_elapsed, 1)
        out['fwd_only_ms'] = round(1e3 * fwd_elapsed, 4)
    if k5_outside is not None:
        # north_star: ">= 40 % of the MI355X HBM roofline on the node -> hyperedge scatter-reduce at 1 GPU" - judged on the COMPULSORY bytes (frac); the SURVEY §8 d3
        # byte model counts every gathered row, which at these node-table sizes is a cache rate and can exceed the HBM peak
        k5_outside['target'] = 0.40
        k5_outside['target_met'] = bool(k5_outside['frac'] >= 0.40)
        k5_outside['target_met_algorithmic'] = bool(k5_outside['algorithmic_gbs'] >= 0.40 * HBM_PEAK_GBS)
        k5_outside['target_definition'] = ('north_star: >= 40 % of the HBM roofline on the node -> hyperedge gather-reduce.  SURVEY §8 d3 prices it on ALGORITHMIC bytes '
                                           '(16 d + 12 B per hyperedge, >= 3.2 TB/s): target_met_algorithmic.  At this workload the node table fits the Infinity Cache, so that rate '
                                           'is a cache rate (it may exceed the HBM peak; frac_algorithmic is null then): target_met is the STRICTER reading - compulsory bytes '
                                           '(every row once) / time >= 0.40 of 8 TB/s.  The HBM-resident reading of the same kernel is roofline_gather_stress')
        out['roofline_node_to_hyperedge'] = k5_outside
    if args.full:
        # SURVEY §8 d3's byte model against what the step really moves: the model prices the reference's two-phase formulation (K5 + K7 per layer, training ~ 3 x forward);
        # the build's re-associations (two-hop fusion, node-level form of the interactive layer) move fewer bytes for the same result, so model / time can exceed the HBM peak
        d3_fwd = (16 * dim + 12 + 12 * dim + 12) * E * layers + (4 * dim + 8) * N_public * layers      # (the reference formulation: every interaction a hyperedge, every node a row)
        step_s = elapsed / args.steps
        measured = measured_src = None
        if pmc is not None and pmc.get('step_l2_miss_bytes'):
            measured = int(pmc['step_l2_miss_bytes'])
            measured_src = f'NOT measured in this run: every kernel of one training step of the committed in-situ counter pass {pmc_name} (commit {pmc.get("commit", "unrecorded")})'
        out['step_bytes'] = dict(model_d3_forward=d3_fwd, model_d3_training=3 * d3_fwd, model_d3_gbs=round(3 * d3_fwd / step_s / 1e9, 1),
                                 model_d3_frac_of_hbm_peak=round(3 * d3_fwd / step_s / 1e9 / HBM_PEAK_GBS, 3), measured_l2_miss=measured,
                                 measured_l2_miss_gbs=round(measured / step_s / 1e9, 1) if measured else None, measured_source=measured_src, ms=round(1e3 * step_s, 4),
                                 note='model_d3 = SURVEY §8 d3 algorithmic bytes of the REFERENCE formulation ((16 d + 12) + (12 d + 12) per hyperedge-layer + (4 d + 8) per node-layer forward, '
                                      'training = 3 x); a model rate above the HBM peak is not skipped work: the step computes the same function with fewer bytes (DESIGN.md section 4); '
                                      'measured_l2_miss = FETCH_SIZE (doubled) + WRITE_SIZE at the L2 <-> fabric boundary, Infinity-Cache hits included')
    if stress is not None:
        out['roofline_gather_stress'] = stress
    if eval_stats is not None:
        out['evaluation_top10'] = eval_stats
    if table:
        out['kernels_us'] = {name: {'avg_us': round(v['avg_us'], 2), 'launches_per_step': v['launches'] / table_steps} for name, v in table.items()}
        out['kernels_us_note'] = f'HIP events around every launch, {table_steps} untimed steps after the timed region; the timed region brackets the `roofline` kernel only'
    if world == 1 and not args.no_cpu_baseline:
        out['cpu_baseline'] = cpu_baseline(args.config, args.layer, layers, args.order, dim, args.cpu_scale)
        if args.config != 'C1':
            # the reference's own CPU-runnable config at FULL size (BASELINE configs[0]), the SAME input on both sides
            c1 = synth.CONFIGS['C1']
            w1 = synth.draw_config('C1')
            ds1 = GraphDataset.from_arrays(w1.user_count, w1.query_count, w1.item_count, w1.vocab_size, w1.bag_words, w1.bag_offsets, w1.triples, device=dev)
            m1 = build_model(ds1, dev, args.layer, c1['layers'], args.order, c1['dim'])
            o1 = Adam(m1.parameters(), 1e-3, weight_decay=0)
            b1 = list(ds1.sample_batches(100, 60, seed=7))
            m1.batch_rows_only_last_layer = False
            for k in range(10):
                m1.bce_loss(*b1[k]).backward(); o1.step(); o1.zero_grad()
            torch.cuda.synchronize()
            t5 = time.perf_counter()
            for k in range(10, 60):
                m1.bce_loss(*b1[k]).backward(); o1.step(); o1.zero_grad()
            torch.cuda.synchronize()
            gpu_ms = 1e3 * (time.perf_counter() - t5) / 50
            rec_ms = None
            try:
                from ihgnn_amd.captured_step import CapturedTrainingStep
                rs = CapturedTrainingStep(m1, o1, int(b1[0][0].shape[0]), warmup_batch=b1[0])
                for k in range(5):
                    rs.step(*b1[k])
                torch.cuda.synchronize()
                t7 = time.perf_counter()
                for k in range(10, 60):
                    rs.step(*b1[k])
                torch.cuda.synchronize()
                rec_ms = 1e3 * (time.perf_counter() - t7) / 50
            except Exception:
                rec_ms = None
            leg = cpu_baseline('C1', args.layer, c1['layers'], args.order, c1['dim'], 1.0, runs=3, steps_per_run=8)
            leg['gpu_same_input'] = dict(ms_per_step=round(gpu_ms, 4), value=round(w1.edge_count * c1['layers'] / (gpu_ms * 1e-3), 1), unit='hyperedges/s',
                                         recorded_step_ms_per_step=round(rec_ms, 4) if rec_ms else None,
                                         recorded_step_value=round(w1.edge_count * c1['layers'] / (rec_ms * 1e-3), 1) if rec_ms else None,
                                         note='the HIP path on the identical C1 workload (E = 20,000: ~85 launches of a few microseconds each, so the eager step is bound by '
                                              'the host\'s launch rate; replayed from one recorded hipGraph it is not)')
            out['cpu_baseline_c1_full_size'] = leg
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
