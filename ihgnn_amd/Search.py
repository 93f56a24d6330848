"""Answer searches with a trained model: ``python -m ihgnn_amd.Search --ds <dataset> --cp <checkpoint | latest> [--k K] [--candidates FILE] [--exclude_seen] [--shortlists] < searches``.

The model is described by the driver's own flags (``--ds --gnn --gnns --fo --emb --cosine --query_transform --query_activation --device``, ``Helpers/ArgsParser.py``)
and built as ``Main.py`` builds it; ``--cp`` is a checkpoint file (a path, or a name inside the run's result directory) or ``latest``.  Every line of the standard
input is one search, ``user<TAB>w1 w2 ...``: the user's index (``-1``: nobody is logged in) and the query's 0-based word ids as ``queries_multihot.txt`` holds them -
the query need not be one the model was trained on (``RawGnn.search``).  ``--candidates FILE`` (one item id per line) restricts every search to these items;
``--exclude_seen`` answers every search of a logged-in user without the items that user interacted with in training.  ``--shortlists``: every line is
``user<TAB>w1 w2 ...<TAB>i1 i2 ...`` and the search is ranked over those item ids only (``RawGnn.search(candidate_lists=)``: the shortlist of a first retrieval
stage; an empty third field gives an empty output line); both other flags compose with it.
Output: one line per search, ``item:score`` pairs, best first.  One process; the features are propagated once and the searches are answered in batches.
"""
import os
import sys
from typing import Optional, Sequence

import numpy as np
import torch

from .Dataset import GraphDataset
from .Helpers.ArgsParser import ConsoleArgs, build_parser
from .Helpers.GlobalSettings import Gs
from .Helpers.Graph import Pps2DGraph, PpsHyperGraph
from .Helpers.IOHelper import IOHelper
from .Main import DEFAULT_DATASET, apply_prediction_settings, apply_query_settings, result_directory
from .Models import GATLayer, GCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn, parse_gnn_layer

BATCH = 4096                                                                # searches per launch


def parse_search_line(line: str):
    """``'user<TAB>w1 w2 ...'`` -> ``(user, [word ids])``; the words may be missing (an empty bag)."""
    head, _, tail = line.rstrip('\n').partition('\t')
    return int(head), [int(w) for w in tail.split()]


def parse_shortlist_line(line: str):
    """``'user<TAB>w1 w2 ...<TAB>i1 i2 ...'`` -> ``(user, [word ids], [item ids])`` (``--shortlists``); the words and the items may be missing (an empty bag, an
    empty shortlist: nothing to rank)."""
    fields = line.rstrip('\n').split('\t')
    if len(fields) > 3:
        raise ValueError(f'a shortlist line is user<TAB>words<TAB>items, got {len(fields)} fields')
    fields += [''] * (3 - len(fields))
    return int(fields[0]), [int(w) for w in fields[1].split()], [int(i) for i in fields[2].split()]


def format_answer(items, scores) -> str:
    return ' '.join(f'{int(i)}:{float(s):.6g}' for i, s in zip(items, scores) if int(i) >= 0)


def build_model(args, device):
    """Dataset and model as ``Main.main`` builds them, the checkpoint's weights loaded."""
    Gs.graph_completeness = args.completeness
    Gs.embedding_size = args.embedding_size or Gs.embedding_size
    layer_type = parse_gnn_layer[args.gnn] or IHGNNLayer
    layer_count, order = args.gnns or 2, args.feature_order or 3
    apply_query_settings(args)
    apply_prediction_settings(args)
    dataset_name = args.dataset or DEFAULT_DATASET
    root = IOHelper.GetFirstLineContent('./dataset_dir.txt') if os.path.exists('./dataset_dir.txt') else './Data/'
    data_dir = os.path.join(root, dataset_name)
    IOHelper.quiet = True
    dataset = GraphDataset(fn_graph_info=os.path.join(data_dir, 'graph_info.txt'), fn_queries_multihot=os.path.join(data_dir, 'queries_multihot.txt'),
                           fn_train_data=os.path.join(data_dir, 'train_data.csv'), graph_type=Pps2DGraph if layer_type in (GCNLayer, GATLayer) else PpsHyperGraph,
                           random_negative_sample_size=Gs.random_negative_sample_size, non_random_negative_sample_size=Gs.non_random_negative_sample_size, device=device)
    model = RawGnn(device=device, dataset=dataset, embedding_size=Gs.embedding_size, gnn_layer_type=layer_type, gnn_layer_count=layer_count, predictions=HemPredictionLayer,
                   lambda_muq=Gs.lambda_muq_for_hem, feature_interaction_order=order, phase2_attention=bool(args.phase2)).to(device)
    if not args.checkpoint:
        raise SystemExit('ihgnn_amd.Search: --cp names the checkpoint to answer with (a file, or "latest")')
    result_dir = result_directory(dataset_name, layer_count, layer_type, order, Gs.embedding_size)
    name = args.checkpoint
    if name == 'latest':
        found = sorted(fn for fn in os.listdir(result_dir) if fn.startswith('checkpoint_') and os.path.isfile(os.path.join(result_dir, fn)))
        if not found:
            raise FileNotFoundError(f'no checkpoint_* file in {result_dir}')
        name = os.path.join(result_dir, found[-1])
    elif not os.path.isfile(name):
        name = os.path.join(result_dir, name)
    model.load_state_dict(torch.load(name, map_location=device)['model'])
    model.eval()
    return model


def main(argv: Optional[Sequence[str]] = None, lines=None, out=None) -> int:
    parser = build_parser()
    parser.description = 'answer searches with a trained IHGNN model'
    parser.add_argument('--k', dest='k', type=int, default=10, help='items returned per search (1..128)')
    parser.add_argument('--candidates', dest='candidates', type=str, default='', help='a file of item ids, one per line: only these items are ranked')
    parser.add_argument('--exclude_seen', dest='exclude_seen', action='store_true', default=False,
                        help='leave out, for every search of a logged-in user, the items that user interacted with in training')
    parser.add_argument('--shortlists', dest='shortlists', action='store_true', default=False,
                        help='every input line carries a third field, the item ids to rank for that search (user<TAB>words<TAB>i1 i2 ...): re-rank a shortlist')
    ns = parser.parse_args(argv)
    args = ConsoleArgs(ns)
    if args.device == 'cpu':
        raise RuntimeError('ihgnn_amd has no CPU path: the scoring kernels are HIP-only')
    device = torch.device(f'cuda:{args.device}' if args.device else 'cuda:0')
    torch.cuda.set_device(device)
    model = build_model(args, device)
    candidates = None
    if ns.candidates:
        with open(ns.candidates, encoding='utf-8') as f:
            candidates = torch.from_numpy(np.asarray([int(t) for t in f.read().split()], np.int64))
    lines = sys.stdin if lines is None else lines
    out = sys.stdout if out is None else out
    with torch.no_grad():
        model.save_features_for_test()
        batch = []

        def answer():
            users = torch.tensor([b[0] for b in batch], dtype=torch.int64)
            offsets = np.cumsum([0] + [len(b[1]) for b in batch[:-1]]).astype(np.int64)
            words = np.asarray([w for b in batch for w in b[1]], np.int64)
            shortlists = None
            if ns.shortlists:
                shortlists = (np.cumsum([0] + [len(b[2]) for b in batch]).astype(np.int64), np.asarray([i for b in batch for i in b[2]], np.int64))
            items, scores = model.search(users, words=words, offsets=offsets, k=ns.k, candidates=candidates, exclude_seen=ns.exclude_seen, candidate_lists=shortlists)
            for row_i, row_s in zip(items.cpu().tolist(), scores.cpu().tolist()):
                out.write(format_answer(row_i, row_s) + '\n')
            batch.clear()

        for line in lines:
            if not line.strip():
                continue
            batch.append(parse_shortlist_line(line) if ns.shortlists else parse_search_line(line))
            if len(batch) == BATCH:
                answer()
        if batch:
            answer()
    out.flush()
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
