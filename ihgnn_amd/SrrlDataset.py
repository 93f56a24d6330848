"""Knowledge-graph batches of the Srrl baseline (reference ``SrrlDataset.py``): host code, as in the reference.

``MetaPaths`` indexes the training interactions three ways - the tails (items) of a (user, query), the heads (users) of a (query, item), the queries of a
(user, item) - for the positives and for the logged negatives.  ``SrrlDatasetKG`` serves one positive per index with ``negative_sample_size`` random items,
its subsampling weight and one random true "company" of each kind; ``OneShotIterator`` cycles three loaders, one per mode.
"""
import random
from typing import Dict, List, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

Pair = Tuple[int, int]

MODES = ('tail-company-batch', 'head-company-batch', 'query-company-batch')


def _index_triples(triples) -> Tuple[Dict[Pair, List[int]], Dict[Pair, List[int]], Dict[Pair, List[int]]]:
    """-> (heads of (q, i), queries of (u, i), tails of (u, q)), every list without duplicates (``list(set(...))``, the reference's order)."""
    heads: Dict[Pair, List[int]] = {}
    queries: Dict[Pair, List[int]] = {}
    tails: Dict[Pair, List[int]] = {}
    for u, q, i in triples:
        tails.setdefault((u, q), []).append(i)
        heads.setdefault((q, i), []).append(u)
        queries.setdefault((u, i), []).append(q)
    for table in (heads, queries, tails):
        for key, members in table.items():
            table[key] = list(set(members))
    return heads, queries, tails


class MetaPaths:
    def __init__(self, graph_dataset) -> None:
        self.graph_dataset = graph_dataset
        self.positive_interactions: List[Tuple[int, int, int]] = [(int(u), int(q), int(i)) for u, q, i in graph_dataset.pos_triples.tolist()]
        self.positive_heads, self.positive_queries, self.positive_tails = _index_triples(self.positive_interactions)
        self.negative_heads, self.negative_queries, self.negative_tails = _index_triples(graph_dataset.neg_interactions)


class SrrlDatasetKG(Dataset):
    def __init__(self, meta_paths: MetaPaths, negative_sample_size: int, mode: str = 'tail_batch', only_use_random_negative_sample: bool = True) -> None:
        super().__init__()
        if not only_use_random_negative_sample:
            raise NotImplementedError('SrrlDatasetKG: only random negatives (the branch the driver uses, Main.py:172-174) are part of this build')
        self.meta_paths = meta_paths
        self.negative_sample_size = negative_sample_size
        self.mode = mode
        self.only_random_sample = True
        # 4 on first sight, + 1 for every further positive of the same (user, query)
        self.head_query_frequency: Dict[Pair, int] = {}
        for u, q, _ in meta_paths.positive_interactions:
            self.head_query_frequency[(u, q)] = self.head_query_frequency.get((u, q), 3) + 1

    def __len__(self) -> int:
        return len(self.meta_paths.positive_interactions)

    def subsampling_weight(self, idx: int) -> torch.Tensor:
        head, query, _ = self.meta_paths.positive_interactions[idx]
        return torch.sqrt(1 / torch.Tensor([self.head_query_frequency[(head, query)]]))

    def __getitem__(self, idx: int):
        paths = self.meta_paths
        head, query, tail = paths.positive_interactions[idx]
        weight = self.subsampling_weight(idx)
        negatives = np.random.randint(paths.graph_dataset.item_count, size=self.negative_sample_size)
        # the draws come in the reference's order: tail, head, query
        true_tail = torch.LongTensor([random.choice(paths.positive_tails[(head, query)])])
        true_head = torch.LongTensor([random.choice(paths.positive_heads[(query, tail)])])
        true_query = torch.LongTensor([random.choice(paths.positive_queries[(head, tail)])])
        return torch.LongTensor([head, query, tail]), torch.LongTensor(negatives), weight, self.mode, true_tail, true_head, true_query

    @staticmethod
    def collate_fn(data):
        """-> (positives [B, 3], negatives [B, k], weights [B], mode, true tails [B, 1], true heads [B, 1], true queries [B, 1])"""
        stack = lambda field: torch.stack([row[field] for row in data], dim=0)
        return stack(0), stack(1), torch.cat([row[2] for row in data], dim=0), data[0][3], stack(4), stack(5), stack(6)


class OneShotIterator:
    """Endless batches, one loader after the other: step s comes from loader s mod 3."""

    def __init__(self, dataloader_tail_company, dataloader_head_company, dataloader_query_company):
        self.step = 0
        self.iterators = [self._forever(loader) for loader in (dataloader_tail_company, dataloader_head_company, dataloader_query_company)]

    def next(self):
        batch = next(self.iterators[self.step % 3])
        self.step += 1
        return batch

    @staticmethod
    def _forever(dataloader):
        while True:
            for batch in dataloader:
                yield batch
