"""Command line of the driver: the reference's flags, aliases and defaults (``Helpers/ArgsParser.py:49-96``)."""
import argparse
import math
from typing import Optional, Sequence

from .GlobalSettings import Gsv

MIN_EXTRA_CUTOFF, MAX_EXTRA_CUTOFF = 11, 128               # above the reference's ten, up to the deepest ranking the scoring kernel returns


def cutoff_list(text: str):
    """``'20,50,100'`` -> ``(20, 50, 100)`` (sorted, duplicates dropped; ``''`` -> ``()``); every value an integer in 11..128."""
    out = set()
    for part in (text or '').split(','):
        if not part.strip():
            continue
        try:
            value = int(part)
        except ValueError:
            raise argparse.ArgumentTypeError(f'--cutoffs takes integers separated by commas, got {part.strip()!r}')
        if not MIN_EXTRA_CUTOFF <= value <= MAX_EXTRA_CUTOFF:
            raise argparse.ArgumentTypeError(f'--cutoffs: every cutoff must be in {MIN_EXTRA_CUTOFF}..{MAX_EXTRA_CUTOFF} (@10 is always reported), got {value}')
        out.add(value)
    return tuple(sorted(out))


def checked_clip_norm(value) -> float:
    """The bound of ``--clip_grad_norm`` / ``Gs.Training.clip_grad_norm``: a finite float >= 0 (0 = off), or a ``ValueError`` - the one check the parser and the
    driver's settings share."""
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f'--clip_grad_norm takes a number, got {value!r}')
    if not math.isfinite(value) or value < 0:
        raise ValueError(f'--clip_grad_norm takes a finite bound >= 0 (0 = off), got {value}')
    return value


def clip_norm(text: str) -> float:
    """``checked_clip_norm`` as an argparse type."""
    try:
        return checked_clip_norm(text)
    except ValueError as refused:
        raise argparse.ArgumentTypeError(str(refused))


POPULARITY_POWER_DEFAULT = 0.75                          # a bare --popularity_negatives: the exponent of word2vec's and HEM's noise distribution


def checked_popularity_power(value) -> float:
    """The exponent of ``--popularity_negatives`` / ``Gs.Training.popularity_power``: 0 (off: uniform negatives) or a float in (0, 1], or a ``ValueError`` - the one check
    the parser and the driver's settings share."""
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f'--popularity_negatives takes a number, got {value!r}')
    if not 0.0 <= value <= 1.0:                             # (also refuses a NaN)
        raise ValueError(f'--popularity_negatives takes an exponent in (0, 1] (0 = off: uniform negatives; a bare flag = {POPULARITY_POWER_DEFAULT}), got {value}')
    return value


def popularity_power(text: str) -> float:
    """``checked_popularity_power`` as an argparse type."""
    try:
        return checked_popularity_power(text)
    except ValueError as refused:
        raise argparse.ArgumentTypeError(str(refused))


def checked_candidate_count(value, item_count=None) -> int:
    """The N of ``--eval_candidates`` / ``Gs.Evaluation.sampled_candidates``: an integer >= 0 (0 = off) and, once the catalogue is known, below its size - or a
    ``ValueError``; the one check the parser and the driver share."""
    try:
        number = int(value)
    except (TypeError, ValueError):
        raise ValueError(f'--eval_candidates takes an integer, got {value!r}')
    if number < 0:
        raise ValueError(f'--eval_candidates takes a count >= 0 (0 = off), got {number}')
    if item_count is not None and number >= int(item_count):
        raise ValueError(f'--eval_candidates {number}: the catalogue has {int(item_count)} items - draw fewer than that (0 ranks the whole catalogue)')
    return number


def candidate_count(text: str) -> int:
    """``checked_candidate_count`` as an argparse type."""
    try:
        return checked_candidate_count(text)
    except ValueError as refused:
        raise argparse.ArgumentTypeError(str(refused))


# (dest, flags, kind, default, help); kind is a type, 'flag', 'optional' (auto | on | off) or ('optional', type, the bare flag's value)
_FLAGS = (
    ('checkpoint', ('--checkpoint', '--cp'), str, '', 'checkpoint file inside the result dir, or "latest"; empty = fresh start'),
    ('storecheckpoint', ('--storecheckpoint', '--scp', '-c'), 'flag', False, 'write a checkpoint when the schedule says so'),
    ('storemetrics', ('--storemetrics', '--sm', '-m'), 'flag', False, 'append test metrics to <time>_metrics.txt'),
    ('epoch_count', ('--epoch_count', '--ec'), int, 0, 'epochs to run (0 = driver default 110)'),
    ('epoch_start_test', ('--epoch_start_test', '--est'), int, 0, 'first epoch to test at (0 = driver default 10)'),
    ('epoch_test_frequency', ('--epoch_test_frequency', '--etf'), int, 0, 'test every this many epochs'),
    ('dataset', ('--dataset', '--ds'), str, '', 'dataset sub-directory under the data root'),
    ('model', ('--model',), str, '', 'model type (RawGnn | Srrl)'),
    ('gnn', ('--gnn',), str, '', 'GNN layer type: IHGNN | HGCN | GCN | GAT'),
    ('gnns', ('--gnns',), int, 0, 'number of GNN layers (0 = driver default 2)'),
    ('feature_order', ('--feature_order', '--fo'), int, 0, 'interaction order 1 | 2 | 3 (0 = driver default 3)'),
    ('completeness', ('--completeness',), str, Gsv.graph_uqi, 'pairwise-graph completeness (GCN / GAT)'),
    ('longtail', ('--longtail',), str, '', 'per-user long-tail statistics file name'),
    ('device', ('--device', '-d'), str, '', 'GPU ordinal ("0" = cuda:0)'),
    ('embedding_size', ('--embedding_size', '--emb'), int, 0, 'embedding width (0 = Gs.embedding_size)'),
    # not in the reference: batches (positive permutation + negative sampling) produced on the GPU instead of by DataLoader + random.sample
    ('device_sampling', ('--device_sampling',), 'flag', False, 'draw training batches on the device (same distribution, different random stream)'),
    # not in the reference's command line: there one edits non_random_negative_sample_size in Helpers/GlobalSettings.py
    ('logged_negatives', ('--logged_negatives',), int, 0, 'logged negatives per positive: items the same (user, query) pair was shown and did not click, beside the random ones '
                                                          '(Gs.non_random_negative_sample_size; 0 = leave the setting alone); with or without --device_sampling'),
    # not in the reference's command line: its driver hard-codes phase2_attention=False (Main.py:57)
    ('phase2', ('--phase2',), 'flag', False, 'IHGNN layers with phase-2 attention: attention weights over a node\'s hyperedges instead of their mean (Gs.Gnn.gat_head / gat_activation)'),
    # not in the reference's command line: there one edits Gs.Query in Helpers/GlobalSettings.py:68-76
    ('query_transform', ('--query_transform',), str, Gsv.mean, 'query transform: mean | activation (nn.Linear + --query_activation on the bag mean) | gru (nn.GRU over the words in order, its last state; Gs.Query.transform)'),
    ('query_activation', ('--query_activation',), str, 'relu', 'activation of --query_transform activation: relu | tanh (Gs.Query.transform_activation)'),
    # not in the reference's command line: there one edits Gs.Prediction in Helpers/GlobalSettings.py
    ('cosine', ('--cosine',), 'flag', False, 'score with the cosine-similarity HEM head (Gs.Prediction.use_cosine_similarity) instead of the dot product'),
    # not in the reference, which reports @10 only (Metrics.py:60-63)
    ('cutoffs', ('--cutoffs',), cutoff_list, '', 'further metric cutoffs, e.g. 20,50,100 (each in 11..128): HR / NDCG / MAP @K beside the @10 triple, from one ranking at the largest (Gs.Evaluation.extra_cutoffs)'),
    # not in the reference, which ranks every item of the catalogue for every test log
    ('filter_seen', ('--filter_seen',), 'flag', False, 'evaluate under the "filter seen" protocol: rank each test log without the items its user interacted with in training '
                                                       '(the log\'s own positives stay rankable; Gs.Evaluation.filter_seen)'),
    # not in the reference: the sampled-metrics protocol much of the literature reports (the positive ranked among 99 or 999 drawn items)
    ('eval_candidates', ('--eval_candidates',), candidate_count, 0, 'evaluate on sampled candidates: rank each test log among its own logged items plus N items drawn uniformly without '
                                                                   'replacement from the rest of the catalogue (Gs.Evaluation.sampled_candidates; 0 = off: the whole catalogue). '
                                                                   'Sampled metrics are not comparable with whole-catalogue ones'),
    # not in the reference, which trains on nn.BCEWithLogitsLoss only (Main.py:191)
    ('loss', ('--loss',), str, 'bce', 'training objective: bce (the reference\'s point-wise loss) | bpr (pairwise: every positive against each of its negatives) | '
                                      'softmax (the positive against its own negatives; Gs.Training.loss)'),
    # not in the reference, whose negatives are uniform draws (and a pair's logged ones): dynamic negative sampling
    ('hard_negatives', ('--hard_negatives',), int, 0, 'hard negatives: draw a pool of M random candidates per positive and train on the Gs.random_negative_sample_size of them that the '
                                                      'current model scores highest (Gs.Training.negative_pool; 0 = off; needs random_negative_sample_size < M <= 256, no --logged_negatives)'),
    # not in the reference, whose negatives may be items the same user bought under another query, or the positive itself
    ('filter_negatives', ('--filter_negatives',), 'flag', False, 'filtered negatives: draw every random negative outside the items the positive\'s user interacted with in training '
                                                                 '(Gs.Training.filter_negatives; with or without --device_sampling and --hard_negatives; no --logged_negatives, '
                                                                 'and negatives per positive + the longest user history must stay within half the catalogue)'),
    # not in the reference, whose negatives are uniform over the catalogue (HEM itself, like word2vec, draws its noise from the item frequency raised to 3/4)
    ('popularity_negatives', ('--popularity_negatives',), ('optional', popularity_power, POPULARITY_POWER_DEFAULT), 0.0,
     'popularity-weighted negatives: draw every random negative in proportion to its item\'s training frequency raised to A (Gs.Training.popularity_power; A in (0, 1], a bare '
     'flag = 0.75, 0 = off: uniform; with or without --device_sampling, --hard_negatives and --filter_negatives; no --logged_negatives, no --model Srrl; no logQ correction)'),
    # not in the reference, whose step has no gradient clipping
    ('clip_grad_norm', ('--clip_grad_norm',), clip_norm, 0.0, 'clip every step\'s gradient to this global L2 norm, as torch.nn.utils.clip_grad_norm_ before Adam (Gs.Training.clip_grad_norm; '
                                                             '0 = off); the epoch log then shows the largest norm and the number of clipped steps'),
    ('grad_sync', ('--grad_sync',), str, 'auto', 'gradient exchange under torchrun: auto | cotangent (batch-row cotangents: no dense exchange) | flat | bucketed | sharded (ihgnn_amd.distributed)'),
    ('seed', ('--seed',), int, -1, 'seed torch / random / numpy before the model is built (the reference seeds nothing, Main.py: -1 leaves the generators alone)'),
    ('record_step', ('--record_step',), 'optional', 'auto', 'replay the training step as one recorded hipGraph (single process): auto (default: when an eager step measures launch-bound, '
                                                             '< 1.5 ms) | on (also a bare --record_step) | off'),
)


LOSSES = ('bce', 'bpr', 'softmax')
_CHOICES = {'query_transform': (Gsv.mean, Gsv.activation, Gsv.gru), 'query_activation': ('relu', 'tanh'), 'loss': LOSSES}


class ConsoleArgs:
    def __init__(self, ns: argparse.Namespace):
        for dest, *_ in _FLAGS:
            setattr(self, dest, getattr(ns, dest))
        self.long_tail_filename = ns.longtail


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description='IHGNN on MI355X')
    for dest, flags, kind, default, text in _FLAGS:
        if kind == 'flag':
            parser.add_argument(*flags, dest=dest, action='store_true', default=default, help=text)
        elif isinstance(kind, tuple):                        # ('optional', type, value of the bare flag)
            parser.add_argument(*flags, dest=dest, nargs='?', type=kind[1], const=kind[2], default=default, metavar='A', help=text)
        elif kind == 'optional':
            parser.add_argument(*flags, dest=dest, nargs='?', const='on', default=default, choices=('auto', 'on', 'off'), help=text)
        elif dest in _CHOICES:
            parser.add_argument(*flags, dest=dest, type=kind, default=default, choices=_CHOICES[dest], help=text)
        else:
            parser.add_argument(*flags, dest=dest, type=kind, default=default, help=text)
    return parser


def parse_args(argv: Optional[Sequence[str]] = None) -> ConsoleArgs:
    return ConsoleArgs(build_parser().parse_args(argv))
