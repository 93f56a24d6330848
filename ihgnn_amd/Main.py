"""Training / evaluation driver: ``python -m ihgnn_amd.Main --ds <dataset> [...]``.

Same flags, defaults, call sequence, result-directory naming, checkpoint and metrics files as the reference's
``Main.py`` (lines 20-325): the RawGnn model with its GNN layers and the Srrl baseline (``--model Srrl``), written as a function
so tests can drive it.  Launched under ``torchrun`` it trains data-parallel (one process per GPU, RCCL).
"""
import os
import sys
import time
from typing import Optional, Sequence

import torch
import torch.nn as nn
from torch.utils.data import DataLoader

from . import distributed as ihg_dist
from .Dataset import GraphDataset, TestSearchLogDataLoader
from .Helpers.ArgsParser import parse_args
from .Helpers.GlobalSettings import Gs, Gsv
from .Helpers.Graph import Pps2DGraph, PpsHyperGraph
from .Helpers.IOHelper import IOHelper
from .Helpers.Metrics import Metrics, MetricsCollection
from .Helpers.ProcessController import ProcessController
from .Helpers.TrainTestHelper import print_network_parameters, test_and_get_avg_metrics, train_and_get_avg_loss
from .Models import GATLayer, GCNLayer, HGCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn, Srrl, parse_gnn_layer, parse_model_type

DEFAULT_DATASET = 'AlibabaAir/Complete5Core/'


def result_directory(dataset_name: str, layers: int, layer_type: type, order: int, emb: int, model_type: type = RawGnn) -> str:
    if model_type is Srrl:                                   # (Main.py:80-86: no layer part for a model without layers)
        return os.path.join('Results', '-'.join(dataset_name.strip('/').split('/') + ['Srrl', f'emb{emb}']))
    parts = dataset_name.strip('/').split('/') + ['RawGnn', f'{layers}{layer_type.__name__}']
    if layer_type is IHGNNLayer:
        parts.append(f'O{order}')
    parts.append(f'emb{emb}')
    return os.path.join('Results', '-'.join(parts))


def apply_query_settings(args) -> None:
    """``--query_transform`` / ``--query_activation`` -> ``Gs.Query`` (not in the reference's command line: one edits ``Helpers/GlobalSettings.py:68-76`` there)."""
    Gs.Query.transform = getattr(args, 'query_transform', Gsv.mean) or Gsv.mean
    Gs.Query.transform_activation = {'relu': nn.ReLU, 'tanh': nn.Tanh}[getattr(args, 'query_activation', 'relu') or 'relu']


def apply_prediction_settings(args) -> None:
    """``--cosine`` -> ``Gs.Prediction.use_cosine_similarity``, assigned both ways: a run without the flag scores with the dot product whatever an earlier ``main()`` of
    this process set (not in the reference's command line: one edits ``Helpers/GlobalSettings.py`` there)."""
    Gs.Prediction.use_cosine_similarity = bool(getattr(args, 'cosine', False))


def apply_evaluation_settings(args) -> None:
    """``--cutoffs`` -> ``Gs.Evaluation.extra_cutoffs``, ``--filter_seen`` -> ``Gs.Evaluation.filter_seen`` and ``--eval_candidates N`` ->
    ``Gs.Evaluation.sampled_candidates``, assigned both ways like the head above (not in the
    reference, which reports @10 only, over the whole catalogue)."""
    Gs.Evaluation.extra_cutoffs = tuple(getattr(args, 'cutoffs', ()) or ())
    Gs.Evaluation.filter_seen = bool(getattr(args, 'filter_seen', False))
    from .Helpers.ArgsParser import checked_candidate_count
    Gs.Evaluation.sampled_candidates = checked_candidate_count(getattr(args, 'eval_candidates', 0) or 0)      # (a caller that builds its own args: the parser's check)


def apply_training_settings(args) -> None:
    """``--loss`` -> ``Gs.Training.loss``, ``--hard_negatives M`` -> ``Gs.Training.negative_pool``, ``--clip_grad_norm X`` -> ``Gs.Training.clip_grad_norm`` and
    ``--filter_negatives`` -> ``Gs.Training.filter_negatives`` and ``--popularity_negatives [A]`` -> ``Gs.Training.popularity_power``, assigned both ways like the head above (not in the reference, which
    trains on ``nn.BCEWithLogitsLoss`` over uniform negatives only).  A pool needs ``Gs.random_negative_sample_size < M <= 256`` and no logged negatives (the pool is
    random-only), and so do filtered negatives (the filter is on the random draws; on both loaders, so that they agree) and popularity-weighted ones (the random part of
    a batch with logged negatives is not weighted); called after ``apply_sampling_settings``."""
    from . import _lib
    from .Helpers.ArgsParser import LOSSES, checked_clip_norm, checked_popularity_power
    loss = getattr(args, 'loss', 'bce') or 'bce'
    if loss not in LOSSES:
        raise ValueError(f'--loss: one of {", ".join(LOSSES)}, got {loss!r}')
    pool = int(getattr(args, 'hard_negatives', 0) or 0)
    if pool < 0:
        raise ValueError(f'--hard_negatives takes a pool size >= 0 (0 = off), got {pool}')
    if pool:
        if not Gs.random_negative_sample_size < pool <= _lib.POOL_MAX:
            raise ValueError(f'--hard_negatives {pool}: the pool must be larger than the {Gs.random_negative_sample_size} negatives kept of it '
                             f'(Gs.random_negative_sample_size) and at most {_lib.POOL_MAX}')
        if int(getattr(args, 'logged_negatives', 0) or 0) > 0 or Gs.non_random_negative_sample_size > 0:
            raise ValueError('--hard_negatives draws its pool from the catalogue only: it does not go with --logged_negatives (Gs.non_random_negative_sample_size > 0)')
    filtered = bool(getattr(args, 'filter_negatives', False))
    if filtered and (int(getattr(args, 'logged_negatives', 0) or 0) > 0 or Gs.non_random_negative_sample_size > 0):
        raise ValueError('--filter_negatives filters the random draws only: it does not go with --logged_negatives (Gs.non_random_negative_sample_size > 0) yet, '
                         'with or without --device_sampling')
    power = checked_popularity_power(getattr(args, 'popularity_negatives', 0.0) or 0.0)      # (a caller that builds its own args: the parser's check)
    if power and (int(getattr(args, 'logged_negatives', 0) or 0) > 0 or Gs.non_random_negative_sample_size > 0):
        raise ValueError('--popularity_negatives weights the draws of the pool kernels only: it does not go with --logged_negatives (Gs.non_random_negative_sample_size > 0), '
                         'whose random part is uniform, with or without --device_sampling')
    clip = checked_clip_norm(getattr(args, 'clip_grad_norm', 0.0) or 0.0)      # (a caller that builds its own args: the parser's check)
    Gs.Training.loss = loss
    Gs.Training.negative_pool = pool
    Gs.Training.filter_negatives = filtered
    Gs.Training.popularity_power = power
    Gs.Training.clip_grad_norm = clip


def own_item_share(dataset) -> float:
    """The share of uniform draws that would have been an item of their own user: ``sum_u deg_u |seen_u| / (E I)`` with ``deg_u`` the positives of user ``u``, ``seen_u``
    its run of ``user_item_lists``, ``E`` the positives and ``I`` the catalogue - what ``--filter_negatives`` removes.  Host arithmetic on ``pos_triples`` and the CSR."""
    import numpy as np
    ptr, _ = dataset.user_item_lists
    degree = np.bincount(dataset.pos_triples[:, 0], minlength=dataset.user_count)[:dataset.user_count]
    positives = max(len(dataset), 1)
    return float((degree * np.diff(ptr)).sum()) / (positives * max(dataset.item_count, 1))


def check_filtered_negatives(dataset, per_positive: int) -> None:
    """``--filter_negatives`` on this dataset: the driver's policy is that the negatives of a positive and the longest user history together stay within half the catalogue,
    so that a draw costs at most two attempts per item on average (the entry point itself only needs a solution to exist)."""
    if per_positive + dataset.max_user_items > dataset.item_count // 2:
        raise ValueError(f'--filter_negatives: {per_positive} negatives per positive + {dataset.max_user_items} items of the user with the longest history exceed half the '
                         f'catalogue ({dataset.item_count} items): the filtered draw would spend most of its attempts on rejections; train without the flag')


def popularity_shares(dataset) -> dict:
    """What the popularity-weighted draw does on this dataset, for the startup log: ``head_share`` = the share of weighted draws that fall on the most popular 1 % of items
    (at least one item; a uniform draw: ``uniform_head_share``), ``own_item_share`` = the share of weighted draws that would be an item of their own user, ``sum_u deg_u
    w(seen_u) / (E total)`` - the weighted counterpart of ``own_item_share``, what ``--filter_negatives`` removes.  Host arithmetic on the weights and the CSR."""
    import numpy as np
    weights = dataset.item_sampling_weights
    total = float(weights.sum())
    head = max(1, dataset.item_count // 100)
    ptr, items = dataset.user_item_lists
    degree = np.bincount(dataset.pos_triples[:, 0], minlength=dataset.user_count)[:dataset.user_count]
    return dict(head_items=head, head_share=float(np.sort(weights)[-head:].sum()) / total, uniform_head_share=head / dataset.item_count,
                own_item_share=float((degree * _list_masses(weights, ptr, items)).sum()) / (max(len(dataset), 1) * total))


def _list_masses(weights, ptr, items):
    """float64 ``[U]``: the sum of ``weights`` over every run of the CSR ``(ptr, items)``, 0 for an empty run (``np.add.reduceat`` over the non-empty ones)."""
    import numpy as np
    masses = np.zeros(len(ptr) - 1, np.float64)
    filled = np.flatnonzero(np.diff(ptr) > 0)
    if len(filled):
        masses[filled] = np.add.reduceat(weights[items].astype(np.float64), ptr[filled])
    return masses


def check_popularity_negatives(dataset, per_positive: int) -> None:
    """``--popularity_negatives`` on this dataset: the driver's policy is that the mass a row can reject stays within half of the weights' sum, so that a draw costs at most
    two attempts per item on average (the entry point itself only needs ``m + max_list_len <= n_items``).  That mass is the sum of the ``per_positive`` heaviest weights -
    the most a row's own accepted values can hold - plus, under ``filter_negatives``, the largest sum of weights over any one user's list."""
    import numpy as np
    weights = dataset.item_sampling_weights
    total = int(weights.sum())
    mass = int(np.sort(weights)[-min(int(per_positive), len(weights)):].sum())
    told = f'the {per_positive} heaviest items'
    if dataset.filter_negatives:
        mass += int(_list_masses(weights, *dataset.user_item_lists).max(initial=0.0))
        told += ' + the heaviest user history'
    if 2 * mass > total:
        raise ValueError(f'--popularity_negatives: {told} weigh {mass}, more than half of all weights ({total}, {dataset.item_count} items): the weighted draw would spend most '
                         'of its attempts on rejections; use a smaller exponent, fewer negatives per positive, or train without the flag')


def apply_sampling_settings(args) -> None:
    """``--logged_negatives N`` -> ``Gs.non_random_negative_sample_size`` (0: the setting stays as it is) and the sum ``Gs.negative_sample_size``, which the class
    body evaluates once and which would go stale (not in the reference's command line: one edits ``Helpers/GlobalSettings.py`` there)."""
    wanted = int(getattr(args, 'logged_negatives', 0) or 0)
    if wanted < 0:
        raise ValueError(f'--logged_negatives takes a count >= 0, got {wanted}')
    if wanted:
        Gs.non_random_negative_sample_size = wanted
    Gs.negative_sample_size = Gs.random_negative_sample_size + Gs.non_random_negative_sample_size


def check_srrl_settings(args, world: int) -> None:
    """``--model Srrl``: what cannot apply is refused before anything is built."""
    from . import ops
    if world > 1:
        raise NotImplementedError('--model Srrl trains in a single process: the gradient exchanges of ihgnn_amd.distributed have not been run with it')
    if getattr(args, 'record_step', 'auto') in (True, 'on', '1', 'yes'):
        raise NotImplementedError('--model Srrl trains eagerly: --record_step on records the RawGnn step (auto stays eager)')
    if getattr(args, 'device_sampling', False):
        raise NotImplementedError('--model Srrl draws its batches on the host (SrrlDatasetKG): --device_sampling does not apply')
    if getattr(args, 'phase2', False):
        raise ValueError('--phase2 is the IHGNN layer\'s phase-2 attention; --model Srrl has no layers')
    if (getattr(args, 'loss', 'bce') or 'bce') != 'bce':
        raise NotImplementedError('--model Srrl trains its PS half on the BCE, as the reference does: --loss bpr / softmax have not been built for it')
    if int(getattr(args, 'hard_negatives', 0) or 0) > 0:
        raise NotImplementedError('--model Srrl trains on uniform negatives, as the reference does: --hard_negatives has not been built for it')
    if getattr(args, 'filter_negatives', False):
        raise NotImplementedError('--model Srrl trains on uniform negatives, as the reference does: --filter_negatives has not been built for it')
    if float(getattr(args, 'popularity_negatives', 0.0) or 0.0) > 0:
        raise NotImplementedError('--model Srrl trains on uniform negatives, as the reference does: --popularity_negatives has not been built for it')
    if getattr(args, 'filter_seen', False):
        raise NotImplementedError('--model Srrl ranks the whole catalogue: --filter_seen has not been built for its scoring kernels')
    if int(getattr(args, 'eval_candidates', 0) or 0) > 0:
        raise NotImplementedError('--model Srrl ranks the whole catalogue: --eval_candidates has not been built for its scoring kernels')
    if getattr(args, 'query_transform', Gsv.mean) == Gsv.gru:
        raise NotImplementedError('--model Srrl embeds its queries by the bag mean or the activation transform: --query_transform gru has not been built for it')
    widest = ops.cat_linear_max_width()
    if 2 * Gs.embedding_size > widest:
        # every block of the model concatenates two rows of the embedding width: said here, not by the first forward's launch
        raise ValueError(f'--model Srrl: --emb {Gs.embedding_size} makes concatenated rows of {2 * Gs.embedding_size} floats, beyond the {widest} the block kernels take '
                         f'(ihg_cat_linear_max_width()); use --emb {widest // 2} or less')
    batch_rows = Gs.batch_size * (1 + Gs.negative_sample_size)
    if batch_rows > ops.SCATTER_CHUNK_ROWS:
        # the row gradients of a batch reach the embedding tables through ihg_batch_combine, whose launch takes ihg_batch_scatter_max_rows() rows: said here, not
        # in the middle of the first backward
        raise ValueError(f'--model Srrl: a batch of {Gs.batch_size} x (1 + {Gs.negative_sample_size}) = {batch_rows} rows is beyond the {ops.SCATTER_CHUNK_ROWS} rows of one '
                         'deterministic scatter launch; use a smaller batch')


def build_srrl(dataset_train, device):
    """The Srrl model with its three KG loaders and the KG steps per epoch (Main.py:169-187)."""
    from .SrrlDataset import MODES, MetaPaths, OneShotIterator, SrrlDatasetKG
    meta_paths = MetaPaths(dataset_train)
    loaders = [DataLoader(SrrlDatasetKG(meta_paths, Gs.negative_sample_size, mode), Gs.batch_size, True, collate_fn=SrrlDatasetKG.collate_fn) for mode in MODES]
    model = Srrl(dataset=dataset_train, embedding_size=Gs.embedding_size, prediction_layer_type=None, lambda_muq=Gs.lambda_muq_for_hem).to(device)
    model.srrl_steps = -(-len(meta_paths.positive_interactions) // Gs.batch_size)
    model.train_iterator_KG = OneShotIterator(*loaders)
    return model


def main(argv: Optional[Sequence[str]] = None) -> MetricsCollection:
    args = parse_args(argv)
    rank, local_rank, world = ihg_dist.init_from_env()
    chief = rank == 0

    if getattr(args, 'seed', -1) is not None and int(getattr(args, 'seed', -1)) >= 0:
        # not in the reference (which seeds nothing): reproducible runs - the initial weights, the loader's shuffles and the sampled negatives follow from --seed
        import random
        import numpy
        random.seed(int(args.seed)); numpy.random.seed(int(args.seed)); torch.manual_seed(int(args.seed))
    Gs.graph_completeness = args.completeness
    Gs.long_tail_stat_fn = args.long_tail_filename or None
    Gs.embedding_size = args.embedding_size or Gs.embedding_size
    epoch_count = args.epoch_count or 110
    start_test = args.epoch_start_test or 10
    test_every = args.epoch_test_frequency or start_test
    dataset_name = args.dataset or DEFAULT_DATASET
    model_type = parse_model_type[args.model] or RawGnn
    layer_type = parse_gnn_layer[args.gnn] or IHGNNLayer
    if layer_type not in (IHGNNLayer, HGCNLayer, GCNLayer, GATLayer):
        raise NotImplementedError(f'{layer_type.__name__} is outside the MI355X hypergraph path')
    phase2 = bool(getattr(args, 'phase2', False))
    if phase2 and layer_type is not IHGNNLayer:
        raise ValueError(f'--phase2 is the IHGNN layer\'s phase-2 attention; --gnn {args.gnn} has none')
    if phase2 and world > 1:
        raise NotImplementedError('--phase2 runs in a single process: the gradient exchanges of ihgnn_amd.distributed have not been run with the attention on')
    layer_count = args.gnns or 2
    order = args.feature_order or 3
    apply_query_settings(args)
    apply_prediction_settings(args)
    apply_evaluation_settings(args)
    apply_sampling_settings(args)
    apply_training_settings(args)
    if model_type is Srrl:
        check_srrl_settings(args, world)
    if args.device == 'cpu':
        raise RuntimeError('ihgnn_amd has no CPU path: the hypergraph kernels are HIP-only')
    device = torch.device(f'cuda:{args.device}' if args.device else f'cuda:{local_rank}')
    torch.cuda.set_device(device)

    root = IOHelper.GetFirstLineContent('./dataset_dir.txt') if os.path.exists('./dataset_dir.txt') else './Data/'
    data_dir = os.path.join(root, dataset_name)
    result_dir = result_directory(dataset_name, layer_count, layer_type, order, Gs.embedding_size, model_type)
    os.makedirs(result_dir, exist_ok=True)
    stamp = time.strftime('%y%m%d-%H%M%S', time.localtime())
    fn_metrics = os.path.join(result_dir, f'{stamp}_metrics.txt')
    if chief:
        IOHelper.StartLogging(os.path.join(result_dir, f'{stamp}_train_log.txt' if args.storemetrics else 'train_log.txt'))
    else:
        IOHelper.StartLogging(None)
        IOHelper.quiet = True
    say = IOHelper.LogPrint if chief else (lambda *a, **k: None)

    pool = Gs.Training.negative_pool
    per_positive = pool or Gs.random_negative_sample_size + Gs.non_random_negative_sample_size      # negative rows a batch carries per positive
    say(f'device {device} | ranks {world} | batch {Gs.batch_size} | lr {Gs.learning_rate} | emb {Gs.embedding_size} | '
        f'L2 {Gs.weight_decay} | negatives {Gs.random_negative_sample_size}/{Gs.non_random_negative_sample_size}' +
        (f' | hard negatives: the best {Gs.random_negative_sample_size} of a pool of {pool}' if pool else '') +
        (f' | clip grad norm {Gs.Training.clip_grad_norm:g}' if Gs.Training.clip_grad_norm else '') +
        (' | negatives filtered: outside the user\'s training items' if Gs.Training.filter_negatives else '') +
        (f' | negatives weighted: item frequency ^ {Gs.Training.popularity_power:g}' if Gs.Training.popularity_power else ''))
    if pool:
        from . import ops
        if 3 * Gs.batch_size * (1 + pool) > ops.SCATTER_CHUNK_ROWS:
            say(f'a batch of {Gs.batch_size} x (1 + {pool}) rows has {3 * Gs.batch_size * (1 + pool)} row gradients, beyond the {ops.SCATTER_CHUNK_ROWS} of one combine launch: '
                'the step runs on the chunked scatter paths')
    say((f'model Srrl | dataset {dataset_name} | KG loss {Gs.Srrl.KG_loss} | uniform KG weights {Gs.Srrl.uni_weight} | ' if model_type is Srrl else
         f'model RawGnn | dataset {dataset_name} | {layer_count} x {layer_type.__name__} | order {order}{" + phase-2 attention" if phase2 else ""} | ') +
        f'query transform {Gs.Query.transform}{" (" + Gs.Query.transform_activation.__name__ + ")" if Gs.Query.transform == Gsv.activation else ""} | '
        f'head {"cosine similarity" if Gs.Prediction.use_cosine_similarity else "dot product"} | loss {Gs.Training.loss} | validation {Gs.use_valid_dataset}' +
        (' | evaluation filtered: without the user\'s training items' if Gs.Evaluation.filter_seen else '') +
        (f' | evaluation sampled: each log among its own items and {Gs.Evaluation.sampled_candidates} drawn ones (not comparable with whole-catalogue metrics)'
         if Gs.Evaluation.sampled_candidates else ''))
    say(f'store metrics {args.storemetrics} | store checkpoint {args.storecheckpoint} | load {args.checkpoint or False}\n')

    dataset_train = GraphDataset(
        fn_graph_info=os.path.join(data_dir, 'graph_info.txt'),
        fn_queries_multihot=os.path.join(data_dir, 'queries_multihot.txt'),
        fn_train_data=os.path.join(data_dir, 'train_data.csv'),
        graph_type=Pps2DGraph if layer_type in (GCNLayer, GATLayer) else PpsHyperGraph,
        random_negative_sample_size=pool or Gs.random_negative_sample_size,      # (a pool: the loaders draw M candidates per positive, the step keeps the best of them)
        non_random_negative_sample_size=Gs.non_random_negative_sample_size,
        device=device, filter_negatives=Gs.Training.filter_negatives, popularity_power=Gs.Training.popularity_power)
    if Gs.Training.filter_negatives:
        check_filtered_negatives(dataset_train, per_positive)
        say(f'filtered negatives: drawn outside the user\'s training items (longest history {dataset_train.max_user_items} items; '
            f'{100 * own_item_share(dataset_train):.4f} % of uniform draws would have been an item of their own user)')
    if Gs.Training.popularity_power:
        check_popularity_negatives(dataset_train, per_positive)
        shares = popularity_shares(dataset_train)
        uniform_own = own_item_share(dataset_train)
        say(f'popularity-weighted negatives: item frequency ^ {Gs.Training.popularity_power:g}, no logQ correction; {100 * shares["head_share"]:.2f} % of draws fall on the '
            f'{shares["head_items"]} most popular items (1 % of the catalogue; uniform: {100 * shares["uniform_head_share"]:.2f} %); '
            f'{100 * shares["own_item_share"]:.4f} % of weighted draws would be an item of their own user (uniform: {100 * uniform_own:.4f} %)' +
            (': removed by --filter_negatives' if Gs.Training.filter_negatives else
             ' - add --filter_negatives to draw outside the user\'s items' if shares['own_item_share'] > uniform_own else ''))
    if args.device_sampling:
        from .Dataset import DeviceBatchLoader
        dataloader_train = DeviceBatchLoader(dataset_train, Gs.batch_size, rank, world)
    elif world > 1:
        # data parallel: the ranks split every epoch's permutation between them (same number of steps on every rank, each row once
        # per epoch) and draw their negatives from differently seeded generators; global batch = batch_size x ranks
        import random
        random.seed(0x5eed + 7919 * rank)
        sampler = ihg_dist.ShardedBatchSampler(len(dataset_train), Gs.batch_size, rank, world, shuffle=True, seed=0)
        dataloader_train = DataLoader(dataset_train, batch_sampler=sampler, collate_fn=GraphDataset.collate_fn)
    else:
        dataloader_train = DataLoader(dataset_train, Gs.batch_size, shuffle=True, collate_fn=GraphDataset.collate_fn)
    if Gs.Evaluation.sampled_candidates:
        from .Helpers.ArgsParser import checked_candidate_count
        checked_candidate_count(Gs.Evaluation.sampled_candidates, dataset_train.item_count)      # (N >= I is refused here, where the catalogue is known)
    dataloader_valid = TestSearchLogDataLoader(os.path.join(data_dir, 'valid_data.csv'), dataset_train, device)
    dataloader_test = TestSearchLogDataLoader(os.path.join(data_dir, 'test_data.csv'), dataset_train, device)

    if model_type is Srrl:
        model = build_srrl(dataset_train, device)
    else:
        model = RawGnn(device=device, dataset=dataset_train, embedding_size=Gs.embedding_size, gnn_layer_type=layer_type,
                       gnn_layer_count=layer_count, predictions=HemPredictionLayer, lambda_muq=Gs.lambda_muq_for_hem,
                       feature_interaction_order=order, phase2_attention=phase2).to(device)
    loss_function = nn.BCEWithLogitsLoss().to(device)
    from .optim import Adam
    grad_sync = None
    if world > 1:
        # one exchange step per training step: the batch rows' cotangents (no dense exchange: the default where the fused batch tail runs) | flat
        # all-reduce | per-bucket all-reduces overlapped with the backward | reduce-scatter + Adam on this rank's shard + all-gather.  Built BEFORE the optimizer: the
        # sharded exchange owns it.
        mode = args.grad_sync
        if mode in ('auto', '', None):
            batch_rows = Gs.batch_size * (1 + per_positive)
            mode = ihg_dist.choose_gradient_sync(4 * sum(p.numel() for p in model.parameters()), world, model.supports_fused_loss(loss_function),
                                                 ihg_dist.cotangent_bytes_per_rank(batch_rows, model.compute_width * (layer_count + 1)))
            say(f'gradient exchange: {mode}')
        grad_sync = ihg_dist.make_gradient_sync(model, mode)
        grad_sync.broadcast_parameters(0)
    max_grad_norm = Gs.Training.clip_grad_norm or None       # (0 = off: the optimizer then launches what it launches without the keyword)
    if grad_sync is not None and grad_sync.owns_optimizer:
        optimizer = grad_sync.optimizer(Gs.learning_rate, Gs.weight_decay, max_grad_norm=max_grad_norm)
    else:
        optimizer = Adam(model.parameters(), Gs.learning_rate, weight_decay=Gs.weight_decay, max_grad_norm=max_grad_norm)      # torch.optim.Adam's rule (Main.py:192), one launch

    epoch_start = 1
    if args.checkpoint:
        name = args.checkpoint
        if name == 'latest':
            found = sorted(fn for fn in os.listdir(result_dir)
                           if fn.startswith('checkpoint_') and os.path.isfile(os.path.join(result_dir, fn)))
            if not found:
                raise FileNotFoundError(f'no checkpoint_* file in {result_dir}')
            name = found[-1]
        state = torch.load(os.path.join(result_dir, name), map_location=device)
        model.load_state_dict(state['model'])
        optimizer.load_state_dict(state['optimizer'])
        epoch_start = int(state['epoch_count']) + 1
        say(f'resumed from {name} ({epoch_start - 1} epochs done)')

    if grad_sync is not None and args.checkpoint:
        grad_sync.broadcast_parameters(0)                    # (the loaded weights, identical on every rank anyway)

    store_from, store_every = (epoch_count, 1000000) if args.storecheckpoint else (None, None)
    if chief:
        say(f'\nmodel parameters ({len(list(model.parameters()))}):')
        print_network_parameters(model)
    pc = ProcessController(epoch_count, epoch_start, start_test, test_every, store_from, store_every)
    say(f'\nepochs {pc.EpochCount} | first test {start_test} | test every {test_every} | '
        f'first checkpoint {store_from} | checkpoint every {store_every}\n')

    history = MetricsCollection(Gs.use_valid_dataset)
    for _ in pc:
        avg_loss, train_seconds = train_and_get_avg_loss(model, optimizer, loss_function, dataset_train, dataloader_train,
                                                         pc, device, grad_sync=grad_sync, record_step=getattr(args, 'record_step', 'auto') if world == 1 else 'off')
        pc.AddTrainTime(train_seconds)
        if pc.ShouldStore():
            # every rank builds the state (a sharded optimizer gathers its Adam shards with a collective), the chief writes it
            state = ihg_dist.checkpoint_state(pc.CurrentEpoch, model, optimizer)
            if chief:
                fn = os.path.join(result_dir, time.strftime(f'checkpoint_%y%m%d-%H%M%S_epoch{pc.CurrentEpoch}', time.localtime()))
                say(f'\ncheckpoint -> {fn}')
                torch.save(state, fn)
            del state
        if pc.ShouldTest():
            say('\nevaluating on the TEST set ...')
            per_user, m_test, t_test = test_and_get_avg_metrics(model, dataset_train, dataloader_test, bool(Gs.long_tail_stat_fn))
            if chief and Gs.long_tail_stat_fn:
                with open(os.path.join(result_dir, Gs.long_tail_stat_fn), 'w', encoding='utf-8') as f:
                    for user, m in enumerate(per_user):
                        seen = int((dataset_train.pos_triples[:, 0] == user).sum())
                        tail = ',,,' if m is None else ',' + ','.join(m.to_string(no_title=True).split(' '))
                        f.write(f'{user},{seen}{tail}\n')
            if Gs.use_valid_dataset:
                say('evaluating on the VALIDATION set ...')
                _, m_valid, t_valid = test_and_get_avg_metrics(model, dataset_train, dataloader_valid)
                history.add(pc.CurrentEpoch, m_test, m_valid)
                pc.AddTestTime(t_test + t_valid)
            else:
                history.add(pc.CurrentEpoch, m_test)
                pc.AddTestTime(t_test)
            if chief and args.storemetrics:
                with open(fn_metrics, 'a', encoding='utf-8') as f:
                    f.write(f'Epoch {pc.CurrentEpoch} Avg loss {avg_loss:.4f}\n{m_test.to_string()}\n')

    if chief and len(list(history.iter_epoch_test())):
        by_ndcg = lambda m: m.NDCG_at10
        if Gs.use_valid_dataset:
            best_epoch, best_test, best_valid = history.get_valid_best(key=by_ndcg)
            say(f'best validation metrics at epoch \033[0;44m{best_epoch}\033[0m:')
            say(best_valid.to_string(highlight=True), put_time_in_single_line=True)
            say('test metrics at that epoch:')
        else:
            best_epoch, best_test = history.get_test_best(key=by_ndcg)
            best_valid = None
            say(f'best test metrics at epoch \033[0;44m{best_epoch}\033[0m:')
        say(best_test.to_string(highlight=True), put_time_in_single_line=True)
        if args.storemetrics:
            with open(fn_metrics, 'a', encoding='utf-8') as f:
                if best_valid is not None:
                    f.write(f'\n\nBest valid metrics at epoch {best_epoch}:\n{best_valid.to_string()}\nCorresponding test metrics:\n')
                else:
                    f.write('\nBest test metrics:\n')
                f.write(best_test.to_string() + '\n\n\nAll TEST metrics:\n' + f'Epoch {Metrics.title}\n')
                f.writelines(f'{e} {m.to_string(no_title=True)}\n' for e, m in history.iter_epoch_test())
                if Gs.use_valid_dataset:
                    f.write(f'\n\nAll VALID metrics:\nEpoch {Metrics.title}\n')
                    f.writelines(f'{e} {m.to_string(no_title=True)}\n' for e, _, m in history.iter_epoch_test_valid())
    # what the training loop decided about the step (TrainTestHelper.train_and_get_avg_loss, --record_step auto | on | off)
    history.training_step_recorded = bool(getattr(model, '_record_decision', False))
    history.eager_step_ms = getattr(model, '_auto_step_ms', None)
    if chief:
        IOHelper.EndLogging()
    return history


if __name__ == '__main__':
    main(sys.argv[1:])
