"""HR@10 / NDCG@10 / MAP@10 of one search scored over all items, and the per-epoch collection that picks the
best epoch by validation NDCG@10 (reference ``Helpers/Metrics.py:8-162``).

Top-10 selection uses ``torch.topk`` on the score vector's own device (one small D2H copy of ten indices per
search instead of a full sort + copy, reference ``Metrics.py:60-61``); ties inside the top ten may order
differently from the reference's unstable ``torch.sort``.

Not in the reference, which hard-codes ten: the same three metrics at further cutoffs K (``--cutoffs``, ``Gs.Evaluation.extra_cutoffs``) - its formulas
(``Metrics.py:60-109``) with every 10 read as K.  A ``Metrics`` object keeps them in ``extra`` beside the @10 triple, which stays what it was.
"""
import math
from io import UnsupportedOperation
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

TOP_K = 10
MAX_CUTOFF = 128                                                            # the deepest ranking the scoring kernel returns (ihg_score_topk_max_k)
_LOG2_OF = [0.0, 0.0] + [math.log(2, r) for r in range(2, MAX_CUTOFF + 2)]  # log_r(2), r = rank + 2


class Metrics:
    title = 'HitRatio@10 NDCG@10 MAP@10'

    def __init__(self, hit_ratio: float = 0.0, ndcg: float = 0.0, mean_ap: float = 0.0, extra: Optional[Dict[int, Tuple[float, float, float]]] = None):
        self.HitRatio_at10 = hit_ratio
        self.NDCG_at10 = ndcg
        self.MAP_at10 = mean_ap
        self.extra: Dict[int, Tuple[float, float, float]] = dict(extra) if extra else {}      # {K: (HR@K, NDCG@K, MAP@K)} of the extra cutoffs

    # accumulation ---------------------------------------------------------------------------
    def add_to_self(self, other: 'Metrics') -> None:
        self.HitRatio_at10 += other.HitRatio_at10
        self.NDCG_at10 += other.NDCG_at10
        self.MAP_at10 += other.MAP_at10
        for cutoff, triple in other.extra.items():
            mine = self.extra.get(cutoff, (0.0, 0.0, 0.0))
            self.extra[cutoff] = tuple(a + b for a, b in zip(mine, triple))

    def divide_and_get_new(self, count) -> 'Metrics':
        return Metrics(self.HitRatio_at10 / count, self.NDCG_at10 / count, self.MAP_at10 / count,
                       {cutoff: tuple(v / count for v in triple) for cutoff, triple in self.extra.items()})

    # formatting -----------------------------------------------------------------------------
    def to_string(self, highlight: bool = False, no_title: bool = False) -> str:
        """The reference's two lines (``no_title``: the three @10 numbers alone, the form the per-epoch and per-user tables are made of); every extra cutoff adds
        a title line and a row of its own below them."""
        if no_title:
            return f'{self.HitRatio_at10:.4f} {self.NDCG_at10:.4f} {self.MAP_at10:.4f}'
        row = f'{self.HitRatio_at10:<11.4f} {self.NDCG_at10:<7.4f} {self.MAP_at10:<6.4f}'
        if highlight:
            row = f'\033[0;41m{row}\033[0m'
        return self.title + '\n' + row + self.extra_to_string()

    def extra_to_string(self) -> str:
        """``''`` without extra cutoffs; else one ``HitRatio@K NDCG@K MAP@K`` title line and one row per cutoff, each preceded by a newline."""
        out = ''
        for cutoff in sorted(self.extra):
            hr, ndcg, mean_ap = self.extra[cutoff]
            names = [f'HitRatio@{cutoff}', f'NDCG@{cutoff}', f'MAP@{cutoff}']
            out += '\n' + ' '.join(names) + f'\n{hr:<{len(names[0])}.4f} {ndcg:<{len(names[1])}.4f} {mean_ap:<{len(names[2])}.4f}'
        return out

    def to_highlight_string(self) -> str:
        return self.to_string(highlight=True)

    __str__ = __repr__ = lambda self: self.to_string()

    # the metric itself ----------------------------------------------------------------------
    @staticmethod
    def from_top_indices(top: Sequence[int], interacted_items: Sequence[int], flags: Optional[Sequence[int]],
                         flags_are_all_1: bool, cutoff: int = TOP_K) -> 'Metrics':
        """Metrics from the best item indices (best first), of which the first ``cutoff`` count (default: the reference's ten): HR / NDCG / MAP @cutoff in the
        object's three attributes.  ``cutoff`` <= ``MAX_CUTOFF``."""
        if not 1 <= cutoff <= MAX_CUTOFF:
            raise ValueError(f'cutoff must be in 1..{MAX_CUTOFF}, got {cutoff}')
        rank_of = {item: rank for rank, item in enumerate(top[:cutoff])}
        cap = min(len(interacted_items), cutoff)
        if flags_are_all_1:
            hits = [rank_of[item] for item in interacted_items if item in rank_of]
            dcg = sum(_LOG2_OF[r + 2] for r in hits)
            idcg = Metrics._get_idcg_for_all1(cap)
        else:
            pairs = [(rank_of[item], f) for item, f in zip(interacted_items, flags) if item in rank_of]
            hits = [r for r, _ in pairs]
            dcg = Metrics._get_dcg(hits, [f for _, f in pairs])
            idcg = Metrics._get_idcg(sorted((f for _, f in pairs), reverse=True))
        return Metrics(len(hits) / cap, dcg / idcg, Metrics._get_map_for_all1(hits))

    @staticmethod
    def at_cutoffs(top: Sequence[int], interacted_items: Sequence[int], flags: Optional[Sequence[int]], flags_are_all_1: bool,
                   extra_cutoffs: Sequence[int] = ()) -> 'Metrics':
        """The @10 metrics of a ranked list and, in ``extra``, those at every further cutoff - each read from a prefix of the one list."""
        m = Metrics.from_top_indices(top, interacted_items, flags, flags_are_all_1)
        for cutoff in extra_cutoffs:
            at = Metrics.from_top_indices(top, interacted_items, flags, flags_are_all_1, cutoff)
            m.extra[int(cutoff)] = (at.HitRatio_at10, at.NDCG_at10, at.MAP_at10)
        return m

    @staticmethod
    def calculate_on_all_items(model_outputs: Tensor, interacted_items: List[int], flags: List[int],
                               flags_are_all_1: bool) -> 'Metrics':
        k = min(TOP_K, model_outputs.shape[0])
        top = torch.topk(model_outputs, k, largest=True, sorted=True).indices.tolist()
        return Metrics.from_top_indices(top, interacted_items, flags, flags_are_all_1)

    @staticmethod
    def _get_dcg(indices_hit, flags_hit) -> float:
        return sum(math.log(2, i + 2) * (2 ** r - 1) for i, r in zip(indices_hit, flags_hit))

    @staticmethod
    def _get_dcg_for_all1(indices_hit) -> float:
        return sum(math.log(2, i + 2) for i in indices_hit)

    @staticmethod
    def _get_idcg(flags_descending) -> float:
        return sum(math.log(2, i + 2) * (2 ** r - 1) for i, r in enumerate(flags_descending))

    @staticmethod
    def _get_idcg_for_all1(truth_count: int) -> float:
        return sum(math.log(2, r) for r in range(2, 2 + truth_count))

    @staticmethod
    def _get_map_for_all1(indices_hit) -> float:
        if not indices_hit:
            return 0
        return sum(j / (i + 1) for j, i in enumerate(indices_hit, start=1)) / len(indices_hit)


class MetricsCollection:
    """(epoch, test metrics[, valid metrics]) history."""

    def __init__(self, has_valid: bool = False):
        self._has_valid = has_valid
        self._epochs: List[int] = []
        self._tests: List[Metrics] = []
        self._valids: List[Metrics] = []

    @property
    def has_valid(self) -> bool:
        return self._has_valid

    def add(self, epoch: int, m_test: Metrics, m_valid: Optional[Metrics] = None) -> None:
        if self._has_valid != (m_valid is not None):
            raise ValueError(f'has_valid is {self._has_valid}.')
        if m_valid is not None:
            self._valids.append(m_valid)
        self._epochs.append(epoch)
        self._tests.append(m_test)

    def _best(self, pool: List[Metrics], key: Callable[[Metrics], Any], max_is_best: bool) -> int:
        scores = [key(m) for m in pool]
        return scores.index(max(scores) if max_is_best else min(scores))    # first best, like list.index(max(...))

    def get_valid_best(self, key, max_is_best: bool = True) -> Tuple[int, Metrics, Metrics]:
        if not self._has_valid:
            raise UnsupportedOperation('has_valid is False.')
        i = self._best(self._valids, key, max_is_best)
        return self._epochs[i], self._tests[i], self._valids[i]

    def get_test_best(self, key, max_is_best: bool = True):
        i = self._best(self._tests, key, max_is_best)
        if self._has_valid:
            return self._epochs[i], self._tests[i], self._valids[i]
        return self._epochs[i], self._tests[i]

    def iter_epoch_test_valid(self) -> Iterable[Tuple[int, Metrics, Metrics]]:
        if not self._has_valid:
            raise UnsupportedOperation('has_valid is False.')
        return zip(self._epochs, self._tests, self._valids)

    def iter_epoch_test(self) -> Iterable[Tuple[int, Metrics]]:
        return zip(self._epochs, self._tests)
