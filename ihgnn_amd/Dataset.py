"""Training / evaluation data feeding the hypergraph path (reference ``Dataset.py``).

``GraphDataset`` keeps the reference's constructor, attributes, ``__getitem__`` / ``collate_fn`` contract and
lazy graph properties (``Dataset.py:11-293``) and adds ``from_arrays`` for in-memory synthetic corpora.
Positive interactions are held as one ``[E,3]`` int64 array (file order = hyperedge order); the reference's
list-of-namedtuples view is built only if somebody asks for ``pos_interactions``.
"""
from __future__ import annotations

import bisect
import os
import random
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor
from torch.utils.data import Dataset

from .Helpers.Graph import Pps2DGraph, PpsGraph, PpsHyperGraph, PpsLogHyperGraph
from .Helpers.IOHelper import IOHelper
from .Helpers.SearchLog import PosInteraction, SearchLog
from .Helpers.SearchLogCollection import SearchLogCollection

Sample = Tuple[Tuple[int, int, int, int], List[int]]


def parse_search_logs(filename: str, with_rows: bool = False):
    """Native two-pass parse of a search-log CSV -> (row count, positive ``[P,3]``, negative ``[M,3]`` (user, query, item));
    ``with_rows`` appends the 0-based row of every positive (``[P]`` int64: positives of one search log share it)."""
    import ctypes
    from . import _lib
    lib = _lib.load()
    path = os.fsencode(filename)
    n_logs, n_pos, n_neg = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.ihg_parse_search_logs(path, ctypes.byref(n_logs), ctypes.byref(n_pos), ctypes.byref(n_neg), None, 0, None, 0, None),
               'ihg_parse_search_logs')
    pos = np.empty((max(n_pos.value, 1), 3), np.int64)
    neg = np.empty((max(n_neg.value, 1), 3), np.int64)
    rows = np.empty(max(n_pos.value, 1), np.int64)
    as_ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    _lib.check(lib.ihg_parse_search_logs(path, ctypes.byref(n_logs), ctypes.byref(n_pos), ctypes.byref(n_neg),
                                         as_ptr(pos), n_pos.value, as_ptr(neg), n_neg.value, as_ptr(rows)), 'ihg_parse_search_logs')
    out = (int(n_logs.value), pos[:n_pos.value], neg[:n_neg.value])
    return out + (rows[:n_pos.value],) if with_rows else out


def read_graph_info(filename: str) -> List[int]:
    """``graph_info.txt`` -> ``[users, queries, items, vocabulary]`` (native reader; ``Dataset.py:143-147`` of the reference)."""
    import ctypes
    from . import _lib
    counts = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().ihg_read_graph_info(os.fsencode(filename), counts), 'ihg_read_graph_info')
    return [int(c) for c in counts]


def read_query_bags(filename: str) -> Tuple[np.ndarray, np.ndarray]:
    """``queries_multihot.txt`` -> (flat 0-based word ids, start offset of every query) (native two-pass reader;
    ``Dataset.py:165-176`` of the reference)."""
    import ctypes
    from . import _lib
    lib = _lib.load()
    path = os.fsencode(filename)
    n_q, n_w = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.ihg_read_query_bags(path, ctypes.byref(n_q), ctypes.byref(n_w), None, 0, None, 0), 'ihg_read_query_bags')
    offsets = np.empty(max(n_q.value, 1), np.int64)
    words = np.empty(max(n_w.value, 1), np.int64)
    as_ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    _lib.check(lib.ihg_read_query_bags(path, ctypes.byref(n_q), ctypes.byref(n_w), as_ptr(offsets), n_q.value, as_ptr(words), n_w.value),
               'ihg_read_query_bags')
    return words[:n_w.value], offsets[:n_q.value]


class GraphDataset(Dataset):
    device: torch.device = None        # class attribute, as in the reference (Dataset.py:135): collate_fn is static
    SAMPLE_MAX = 16                    # negatives per positive the device sampler draws at most (kSampleMax of csrc/tail.hip)

    def __init__(self, fn_graph_info: str, fn_queries_multihot: str, fn_train_data: str, graph_type: type,
                 random_negative_sample_size: int, non_random_negative_sample_size: int, device: torch.device, filter_negatives: bool = False,
                 popularity_power: float = 0.0):
        super().__init__()
        counts = read_graph_info(fn_graph_info)                      # the three input files go through the native readers
        bag_words, bag_offsets = read_query_bags(fn_queries_multihot)
        n_logs, triples, negatives, rows = parse_search_logs(fn_train_data, with_rows=True)
        self._setup(counts, bag_words, bag_offsets, triples, graph_type,
                    random_negative_sample_size, non_random_negative_sample_size, device, filter_negatives, popularity_power)
        self.pos_log = rows
        self._fn_train_data = fn_train_data
        self._search_logs = None
        self._neg_triples = negatives
        self._neg_interactions = None
        self._neg_of = None

        IOHelper.LogPrint(f'training set ready: {fn_train_data}')
        IOHelper.LogPrint(f'users {self.user_count} | queries {self.query_count} | items {self.item_count} | '
                          f'vocabulary {self.vocab_size} | logs {n_logs} | hyperedges {len(self)} | {graph_type.__name__}')
        if len(self):
            IOHelper.LogPrint(f'{len(negatives) / len(self):.4f} logged negatives per positive')

    @classmethod
    def from_arrays(cls, user_count: int, query_count: int, item_count: int, vocab_size: int,
                    bag_words: np.ndarray, bag_offsets: np.ndarray, triples: np.ndarray,
                    graph_type: type = PpsHyperGraph, random_negative_sample_size: int = 10,
                    non_random_negative_sample_size: int = 0, device: torch.device = torch.device('cuda:0'),
                    pos_log: Optional[np.ndarray] = None, neg_triples: Optional[np.ndarray] = None, filter_negatives: bool = False,
                    popularity_power: float = 0.0) -> 'GraphDataset':
        """In-memory construction (synthetic corpora): ``bag_words`` are 0-based word ids, ``triples`` 0-based per type;
        ``pos_log[e]`` = the search log hyperedge ``e`` came from (default: one log per positive); ``neg_triples`` ``[M, 3]`` = the logged
        negatives (user, query, item), array order standing for file order (default: none); ``filter_negatives``: random negatives are drawn outside what the
        positive's user interacted with in training (``user_item_lists``; default off: uniform over the catalogue); ``popularity_power`` alpha in (0, 1]: random negatives
        fall on an item in proportion to its training frequency raised to alpha (``item_sampling_weights``; default 0 = off: uniform)."""
        self = cls.__new__(cls)
        Dataset.__init__(self)
        self._setup([user_count, query_count, item_count, vocab_size], np.asarray(bag_words, np.int64),
                    np.asarray(bag_offsets, np.int64), np.asarray(triples, np.int64).reshape(-1, 3), graph_type,
                    random_negative_sample_size, non_random_negative_sample_size, device, filter_negatives, popularity_power)
        if pos_log is not None:
            self.pos_log = np.ascontiguousarray(pos_log, dtype=np.int64)
        self._fn_train_data = None
        self._search_logs = None
        self._neg_triples = np.zeros((0, 3), np.int64) if neg_triples is None else np.ascontiguousarray(neg_triples, dtype=np.int64).reshape(-1, 3)
        self._neg_interactions = None
        self._neg_of = None
        return self

    def _setup(self, counts: Sequence[int], bag_words: np.ndarray, bag_offsets: np.ndarray, triples: np.ndarray,
               graph_type: type, rand_neg: int, nonrand_neg: int, device: torch.device, filter_negatives: bool = False,
               popularity_power: float = 0.0) -> None:
        if graph_type not in (Pps2DGraph, PpsHyperGraph, PpsLogHyperGraph):
            raise AssertionError(f'unsupported graph type: {graph_type}')
        GraphDataset.device = device
        self.graph_type = graph_type
        self.rand_neg_sample_size = rand_neg
        self.nonrand_neg_sample_size = nonrand_neg
        self.neg_sample_size = rand_neg + nonrand_neg
        self.filter_negatives = bool(filter_negatives)
        if self.filter_negatives and nonrand_neg:
            raise ValueError('filter_negatives draws random negatives only: it does not go with logged negatives (non_random_negative_sample_size > 0)')
        self.popularity_power = float(popularity_power)
        if not 0.0 <= self.popularity_power <= 1.0:                             # (also refuses a NaN)
            raise ValueError(f'popularity_power must be in (0, 1], or 0 for uniform negatives, got {popularity_power}')
        if self.popularity_power and nonrand_neg:
            raise ValueError('popularity_power weights the random negatives of the pool draw only: it does not go with logged negatives '
                             '(non_random_negative_sample_size > 0), whose random part is uniform')

        self.user_count, self.query_count, self.item_count, self.vocab_size = (int(c) for c in counts)
        self.node_count = self.user_count + self.query_count + self.item_count
        self.query_start_index_in_graph = self.user_count
        self.item_start_index_in_graph = self.user_count + self.query_count
        if bag_offsets.shape[0] != self.query_count:
            raise ValueError(f'{bag_offsets.shape[0]} query bags for {self.query_count} queries')

        # ids are 0-based on disk; row 0 of every embedding table is padding, so stored id = index + 1
        self.users_onehot = torch.arange(1, 1 + self.user_count, device=device)
        self.items_onehot = torch.arange(1, 1 + self.item_count, device=device)
        self.vocabulary_onehot = torch.arange(1, 1 + self.vocab_size, device=device)
        self.bag_words_host = bag_words + 1
        self.bag_offsets_host = bag_offsets
        self.queries_for_embeddingbag = torch.from_numpy(self.bag_words_host).to(device)
        self.queries_offset_for_embeddingbag = torch.from_numpy(bag_offsets).to(device)

        self.pos_triples = np.ascontiguousarray(triples)
        self._pos_interactions: Optional[List[PosInteraction]] = None
        self._hgraph: Optional[PpsHyperGraph] = None
        self._hloggraph: Optional[PpsLogHyperGraph] = None
        self.pos_log = np.arange(self.pos_triples.shape[0], dtype=np.int64)      # search log (file row) of every positive; from_arrays: one each
        self._graph2d = None
        self._bag_layout = None
        self._queries_multihot = None

    # -- lazily built views -----------------------------------------------------------------------
    @property
    def search_logs(self) -> Optional[SearchLogCollection]:
        """The parsed rows as the reference keeps them (``Dataset.py:192``); only materialised if somebody asks."""
        if self._search_logs is None and self._fn_train_data is not None:
            self._search_logs = SearchLogCollection.read(self._fn_train_data)
        return self._search_logs

    @property
    def neg_interactions(self) -> List[Tuple[int, int, int]]:
        if self._neg_interactions is None:
            self._neg_interactions = [tuple(r) for r in self._neg_triples.tolist()]
        return self._neg_interactions

    @property
    def neg_items_for_user_query_pair(self) -> Dict[Tuple[int, int], List[int]]:
        """(user, query) -> logged negative items in file order; every logged pair has an entry (``Dataset.py:201-210``).  Without a
        file (``from_arrays``) the table is built from the ``neg_triples`` given there."""
        if self._neg_of is None:
            table: Dict[Tuple[int, int], List[int]] = {}
            if self.search_logs is not None:
                for log in self.search_logs:
                    bucket = table.setdefault((log.user, log.query), [])
                    bucket.extend(item for item, flag in zip(log.items, log.interactions) if flag <= 0)
            else:
                for u, q, item in self._neg_triples.tolist():
                    table.setdefault((u, q), []).append(item)
            self._neg_of = table
        return self._neg_of

    @property
    def logged_negative_lists(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The logged negatives as the device sampler reads them: ``(pair_of_edge [E] int32, neg_ptr [P + 1] int64, neg_items [M'] int32)``.
        ``pair_of_edge[e]`` is the (user, query) pair of positive ``e`` among the ``P`` pairs that have a positive, and
        ``neg_items[neg_ptr[p]:neg_ptr[p + 1]]`` is the list ``neg_items_for_user_query_pair`` holds for pair ``p``: file order, repeats
        kept, empty for a pair without logged negatives.  Logged negatives of a pair without a positive are dropped (nothing looks them up)."""
        if getattr(self, '_neg_lists', None) is None:
            pos, neg = self.pos_triples, self._neg_triples
            span = int(max(self.query_count, pos[:, 1].max(initial=-1) + 1, neg[:, 1].max(initial=-1) + 1))
            pairs, pair_of_edge = np.unique(pos[:, 0] * span + pos[:, 1], return_inverse=True)
            neg_key = neg[:, 0] * span + neg[:, 1]
            slot = np.minimum(np.searchsorted(pairs, neg_key), max(len(pairs) - 1, 0))
            kept = np.flatnonzero(pairs[slot] == neg_key) if len(pairs) else np.zeros(0, np.int64)
            by_pair = kept[np.argsort(slot[kept], kind='stable')]                    # stable: a pair's items stay in file order
            neg_ptr = np.zeros(len(pairs) + 1, np.int64)
            np.cumsum(np.bincount(slot[kept], minlength=len(pairs)), out=neg_ptr[1:])
            self._neg_lists = (np.ascontiguousarray(pair_of_edge.reshape(-1), np.int32), neg_ptr, np.ascontiguousarray(neg[by_pair, 2], np.int32))
        return self._neg_lists

    @property
    def user_item_lists(self) -> Tuple[np.ndarray, np.ndarray]:
        """What every user interacted with in training, as the search kernels read exclusion lists: ``(ptr [U + 1] int64, items int32)`` where
        ``items[ptr[u]:ptr[u + 1]]`` are user ``u``'s distinct items of ``pos_triples``, ascending; empty for a user without a positive.  Built once."""
        if getattr(self, '_user_items', None) is None:
            keys = np.unique(self.pos_triples[:, 0].astype(np.int64) * self.item_count + self.pos_triples[:, 2])
            ptr = np.searchsorted(keys, np.arange(self.user_count + 1, dtype=np.int64) * self.item_count).astype(np.int64)
            self._user_items = (ptr, np.ascontiguousarray(keys % self.item_count, np.int32))
        return self._user_items

    @property
    def max_user_items(self) -> int:
        """The longest run of ``user_item_lists``: the most distinct training items any one user has.  Computed once, on the host."""
        if getattr(self, '_max_user_items', None) is None:
            self._max_user_items = int(np.diff(self.user_item_lists[0]).max(initial=0))
        return self._max_user_items

    def user_item_set(self, user: int) -> frozenset:
        """User ``user``'s run of ``user_item_lists`` as a set, built when first asked for (the host sampler's rejection test under ``filter_negatives``)."""
        sets = self.__dict__.setdefault('_user_item_sets', {})
        seen = sets.get(user)
        if seen is None:
            ptr, items = self.user_item_lists
            seen = sets[user] = frozenset(items[ptr[user]:ptr[user + 1]].tolist()) if 0 <= user < self.user_count else frozenset()
        return seen

    @property
    def item_sampling_weights(self) -> np.ndarray:
        """The integer weights of the popularity-weighted draw, int64 ``[I]``: ``w_i = max(1, rint(2^32 ((c_i + 1) / (c_max + 1))^alpha))`` in float64, ``c_i`` the rows
        of ``pos_triples`` whose item is ``i`` and alpha ``popularity_power`` (which must be > 0).  The ``+ 1`` keeps a never-bought item drawable; the most frequent item
        has weight ``2^32``, so the sum is at most ``I 2^32``.  Built once, on the host."""
        if not self.popularity_power:
            raise ValueError('item_sampling_weights: the dataset was built with popularity_power = 0 (uniform negatives)')
        if getattr(self, '_item_weights', None) is None:
            counts = np.bincount(self.pos_triples[:, 2], minlength=self.item_count)[:self.item_count].astype(np.float64)
            share = (counts + 1.0) / (counts.max(initial=0.0) + 1.0)
            self._item_weights = np.maximum(1, np.rint(2.0 ** 32 * share ** self.popularity_power)).astype(np.int64)
        return self._item_weights

    @property
    def item_sampling_cum(self) -> Tuple[List[int], int]:
        """``(cum, total)`` on the host, ``cum`` a list of ``I + 1`` Python ints (what ``bisect`` reads on the ``DataLoader`` path): the running sum of
        ``item_sampling_weights``, ``cum[0] = 0``, ``cum[I] = total``."""
        if getattr(self, '_item_cum', None) is None:
            cum = [0] + np.cumsum(self.item_sampling_weights).tolist()
            self._item_cum = (cum, cum[-1])
        return self._item_cum

    def item_sampling_table_on(self, device) -> Tuple[Tensor, int]:
        """``ops.item_sampling_table(item_sampling_weights)`` on ``device``, built and copied there once."""
        from . import ops
        device = torch.device(device)
        cached = getattr(self, '_item_table_device', None)
        if cached is None or cached[0].device.type != device.type or (device.index is not None and cached[0].device.index != device.index):
            cached = self._item_table_device = ops.item_sampling_table(self.item_sampling_weights, device=device)
        return cached

    def user_item_lists_on(self, device) -> Tuple[Tensor, Tensor]:
        """``user_item_lists`` as tensors on ``device``, copied there once."""
        device = torch.device(device)
        cached = getattr(self, '_user_items_device', None)
        if cached is None or cached[0].device.type != device.type or (device.index is not None and cached[0].device.index != device.index):
            cached = self._user_items_device = tuple(torch.from_numpy(a).to(device) for a in self.user_item_lists)
        return cached

    @property
    def pos_interactions(self) -> List[PosInteraction]:
        if self._pos_interactions is None:
            if self.search_logs is not None:
                self._pos_interactions = [p for log in self.search_logs for p in PosInteraction.from_search_log(log, True)]
            else:
                self._pos_interactions = [PosInteraction(u, q, '', i, 1, 1, 1, '') for u, q, i in self.pos_triples.tolist()]
        return self._pos_interactions

    @property
    def queries_multihot(self) -> Tensor:
        """Sparse ``[Q x V]`` row-normalised bag-of-words matrix (``Dataset.py:178-183``); unused by the models."""
        if self._queries_multihot is None:
            ends = np.append(self.bag_offsets_host[1:], self.bag_words_host.shape[0])
            lens = ends - self.bag_offsets_host
            rows = np.repeat(np.arange(self.query_count), lens)
            vals = np.repeat(1.0 / np.maximum(lens, 1), lens).astype(np.float32)
            self._queries_multihot = torch.sparse_coo_tensor(
                np.stack([rows, self.bag_words_host - 1]), vals, (self.query_count, self.vocab_size)).coalesce().to(GraphDataset.device)
        return self._queries_multihot

    @property
    def bag_layout(self):
        """Device layout of the query bags for the HIP embedding-bag kernels."""
        if self._bag_layout is None:
            from .ops import BagLayout
            self._bag_layout = BagLayout(self.bag_words_host, self.bag_offsets_host, self.vocab_size + 1, GraphDataset.device)
        return self._bag_layout

    @property
    def hypergraph(self) -> PpsHyperGraph:
        if self._hgraph is None:
            self._hgraph = PpsHyperGraph.from_triples(self.pos_triples, self.node_count, self.user_count,
                                                      self.query_count, GraphDataset.device)
        return self._hgraph

    @property
    def graph2d(self) -> Pps2DGraph:
        if self._graph2d is None:
            self._graph2d = Pps2DGraph.from_triples(self.pos_triples, self.node_count, self.user_count, self.query_count,
                                                    False, GraphDataset.device)
        return self._graph2d

    @property
    def hypergraph_log(self) -> PpsLogHyperGraph:
        """One variable-arity hyperedge per search log with a positive (``Dataset.py:98-103``, ``Graph.py:138-189``)."""
        if self._hloggraph is None:
            self._hloggraph = PpsLogHyperGraph.from_positives(self.pos_triples, self.pos_log, self.node_count, self.user_count,
                                                              self.query_count, GraphDataset.device)
        return self._hloggraph

    @property
    def graph(self) -> PpsGraph:
        if self.graph_type == Pps2DGraph:
            return self.graph2d
        return self.hypergraph_log if self.graph_type == PpsLogHyperGraph else self.hypergraph

    # -- sampling ------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return int(self.pos_triples.shape[0])

    def __getitem__(self, index: int) -> Sample:
        """One positive and its sampled negative items (``Dataset.py:107-119``): ``random.sample`` draws distinct
        items per call and may hit the positive; logged negatives of the (user, query) pair come first if requested.  Under ``filter_negatives``
        (random negatives only) the items are ``random.randrange`` draws, kept while distinct and outside the user's training items."""
        u, q, i = (int(x) for x in self.pos_triples[index])
        if self.popularity_power:
            # a threshold below the sum of the weights, the item whose run of the running sum holds it: kept while distinct (and, filtered, outside the user's items)
            seen, k = (self.user_item_set(u) if self.filter_negatives else frozenset()), self.rand_neg_sample_size
            if k + len(seen) > self.item_count:
                raise ValueError(f'popularity_power: user {u} has {len(seen)} of {self.item_count} items, which leaves fewer than {k} to draw')
            cum, total = self.item_sampling_cum
            drawn: List[int] = []
            while len(drawn) < k:
                item = bisect.bisect_right(cum, random.randrange(total)) - 1
                if item not in seen and item not in drawn:
                    drawn.append(item)
            return (u, q, i, 1), drawn
        if self.filter_negatives:
            seen, k = self.user_item_set(u), self.rand_neg_sample_size
            if k + len(seen) > self.item_count:
                raise ValueError(f'filter_negatives: user {u} has {len(seen)} of {self.item_count} items, which leaves fewer than {k} to draw')
            drawn: List[int] = []
            while len(drawn) < k:
                item = random.randrange(self.item_count)
                if item not in seen and item not in drawn:
                    drawn.append(item)
            return (u, q, i, 1), drawn
        want_logged = self.nonrand_neg_sample_size
        if want_logged == 0:
            return (u, q, i, 1), random.sample(range(self.item_count), self.rand_neg_sample_size)
        logged = self.neg_items_for_user_query_pair.get((u, q), [])
        if len(logged) < want_logged:
            return (u, q, i, 1), random.sample(range(self.item_count), self.neg_sample_size - len(logged)) + logged
        chosen = random.sample(logged, want_logged)
        return (u, q, i, 1), chosen + random.sample(range(self.item_count), self.rand_neg_sample_size)

    @staticmethod
    def collate_fn(data: List[Sample]) -> Tuple[Tensor, ...]:
        """-> (users, queries, items, flags) of the positives then of the negatives, on ``GraphDataset.device``.

        Everything is packed into one host array and crosses PCIe once (the reference builds eight tensors from
        Python lists, one copy each, ``Dataset.py:282-291``)."""
        n_pos = len(data)
        n_neg = sum(len(negs) for _, negs in data)
        pack = np.zeros((4, n_pos + n_neg), dtype=np.int64)
        cursor = n_pos
        for k, ((u, q, item, flag), negs) in enumerate(data):
            pack[:, k] = (u, q, item, flag)
            stop = cursor + len(negs)
            pack[0, cursor:stop] = u
            pack[1, cursor:stop] = q
            pack[2, cursor:stop] = negs
            cursor = stop
        dev = _to_device_async(pack, GraphDataset.device)
        pos, neg = dev[:, :n_pos], dev[:, n_pos:]
        return pos[0], pos[1], pos[2], pos[3], neg[0], neg[1], neg[2], neg[3]

    def device_batches(self, batch_size: int, epoch: int = 0, seed: int = 0, rank: int = 0, world_size: int = 1):
        """One epoch of training batches produced ON THE DEVICE: the positives are a device-side permutation of the hyperedges
        (this rank's share of it when ``world_size`` > 1), the ``rand_neg_sample_size`` negatives of every positive come from
        ``ihg_sample_negatives`` (distinct within a sample, uniform over the catalogue, may hit the positive - the semantics of
        ``random.sample(range(I), k)``, ``Dataset.py:107-109``; more than ``SAMPLE_MAX`` of them - a pool of candidates for hard negatives - from
        ``ihg_sample_pool``, the same stream continued).  Yields the 8-tuple of ``collate_fn`` (positives then negatives;
        users, queries, items, flags) with no host -> device copy and no host-side sampling per step.  Under ``filter_negatives`` the negatives
        come from ``ihg_sample_pool_excluding`` for every count: the same stream under the same keys with the items of the positive's user
        (``user_item_lists_on``) deleted; permutation, positives and layout are the unflagged epoch's.  With ``popularity_power`` > 0 they come from
        ``ihg_sample_pool_weighted`` for every count, under the same keys again: every attempt falls on an item in proportion to ``item_sampling_weights``
        (``item_sampling_table_on``), with the user's items deleted when ``filter_negatives`` is on as well.

        With ``nonrand_neg_sample_size`` > 0 a batch is ONE launch, ``ihg_device_batch``: it gathers the positives, draws every
        positive's logged negatives from ``logged_negative_lists`` by the rule of ``__getitem__`` (``Dataset.py:110-119``) and its
        random ones from the stream of ``ihg_sample_negatives``, and writes the ``[4, n (1 + k)]`` array of ``collate_fn``, of which
        the 8-tuple is views."""
        import ctypes
        from . import _lib
        lib = _lib.load()
        dev = GraphDataset.device
        if getattr(self, '_pos_device', None) is None:
            self._pos_device = torch.from_numpy(self.pos_triples).to(dev)
        k = self.rand_neg_sample_size
        k_logged = self.nonrand_neg_sample_size
        if k_logged:
            if k + k_logged > self.SAMPLE_MAX:
                raise ValueError(f'device_batches draws at most {self.SAMPLE_MAX} negatives per positive, got {k} random + {k_logged} logged')
            if k + k_logged > self.item_count:
                raise ValueError(f'device_batches draws distinct items: at most item_count = {self.item_count} negatives per positive, '
                                 f'got {k} random + {k_logged} logged')
            if getattr(self, '_neg_device', None) is None:
                # (a corpus without logged negatives: one unread int32, since an empty tensor has no address to pass)
                self._neg_device = tuple(torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(dev) for a in self.logged_negative_lists)
            pair_of_edge, neg_ptr, neg_items = (ctypes.c_void_p(t.data_ptr()) for t in self._neg_device)
        filtered = self.filter_negatives
        if filtered:
            from . import ops
            if k + self.max_user_items > self.item_count:
                raise ValueError(f'filter_negatives: a user has {self.max_user_items} of {self.item_count} items, which leaves fewer than {k} negatives to draw')
            user_lists = self.user_item_lists_on(dev)
        weighted = bool(self.popularity_power)
        if weighted:
            from . import ops
            if k > self.item_count:
                raise ValueError(f'popularity_power: {k} distinct negatives per positive from a catalogue of {self.item_count} items')
            table = self.item_sampling_table_on(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed * 1_000_003 + epoch)
        order = torch.randperm(len(self), device=dev, generator=gen)[rank::world_size]
        if k_logged:
            order = order.contiguous()                                           # the launch reads a batch's edge ids where they lie
        n_batches = -(-(-(-len(self) // world_size)) // batch_size)
        mine = int(order.shape[0])
        if mine < n_batches:
            raise ValueError(f'rank {rank} holds {mine} positives for {n_batches} batches: batch_size {batch_size} is too small for {world_size} ranks '
                             '(an empty batch on one rank would leave the others waiting in the gradient exchange)')
        base, extra = divmod(mine, n_batches)
        lo = 0
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for b in range(n_batches):
            if world_size == 1:                                          # DataLoader's batching: full batches and a shorter last one
                hi = min(lo + batch_size, mine)
            else:                                                        # equal batch counts on every rank, sizes within one row of each other
                hi = lo + base + (1 if b < extra else 0)
            if k_logged:
                n = hi - lo
                pack = torch.empty(4, n * (1 + k + k_logged), dtype=torch.int64, device=dev)
                _lib.check(lib.ihg_device_batch(seed * 7919 + rank, (epoch << 32) + b, ctypes.c_void_p(self._pos_device.data_ptr()),
                                                ctypes.c_void_p(order.data_ptr() + 8 * lo), n, pair_of_edge, neg_ptr, neg_items, self.item_count, k, k_logged,
                                                ctypes.c_void_p(pack.data_ptr()), stream), 'ihg_device_batch')
                lo = hi
                pos, neg = pack[:, :n], pack[:, n:]
                yield pos[0], pos[1], pos[2], pos[3], neg[0], neg[1], neg[2], neg[3]
                continue
            pos = self._pos_device[order[lo:hi]]
            lo = hi
            n = int(pos.shape[0])
            if weighted:
                # the same keys, every attempt falling on an item in proportion to its weight; filtered as below when that is on too (ihg_sample_pool_weighted, every k)
                neg_items = ops.sample_pool_weighted(seed * 7919 + rank, (epoch << 32) + b, n, self.item_count, k, table, pos[:, 0] if filtered else None,
                                                     user_lists if filtered else None, self.max_user_items if filtered else 0, device=dev)
            elif filtered:
                # the same stream under the same keys, without what the positive's user has bought: one kernel for every k (ihg_sample_pool_excluding)
                neg_items = ops.sample_pool_excluding(seed * 7919 + rank, (epoch << 32) + b, n, self.item_count, k, pos[:, 0], user_lists, self.max_user_items, device=dev)
            else:
                neg_items = torch.empty(n, k, dtype=torch.int64, device=dev)
                # (beyond SAMPLE_MAX draws - a pool of candidates, --hard_negatives - the same stream from ihg_sample_pool; up to SAMPLE_MAX the launch batches always had)
                draw, name = (lib.ihg_sample_pool, 'ihg_sample_pool') if k > self.SAMPLE_MAX else (lib.ihg_sample_negatives, 'ihg_sample_negatives')
                _lib.check(draw(seed * 7919 + rank, (epoch << 32) + b, n, self.item_count, k, ctypes.c_void_p(neg_items.data_ptr()), stream), name)
            ones = torch.ones(n, dtype=torch.int64, device=dev)
            yield (pos[:, 0], pos[:, 1], pos[:, 2], ones, pos[:, 0].repeat_interleave(k), pos[:, 1].repeat_interleave(k),
                   neg_items.reshape(-1), torch.zeros(n * k, dtype=torch.int64, device=dev))

    def sample_batches(self, batch_size: int, steps: int, seed: int = 0) -> Iterator[Tuple[Tensor, Tensor, Tensor, Tensor]]:
        """Vectorised batch source for benchmarks: ``steps`` batches of ``batch_size`` positives (uniform with
        replacement) each followed by ``rand_neg_sample_size`` uniform negatives; yields device tensors
        ``(users, queries, items, labels)`` of ``batch_size * (1 + negatives)`` rows."""
        rng = np.random.default_rng(seed)
        k = self.rand_neg_sample_size
        for _ in range(steps):
            pick = rng.integers(0, len(self), batch_size)
            pos = self.pos_triples[pick]
            neg_items = rng.integers(0, self.item_count, batch_size * k)
            users = np.concatenate([pos[:, 0], np.repeat(pos[:, 0], k)])
            queries = np.concatenate([pos[:, 1], np.repeat(pos[:, 1], k)])
            items = np.concatenate([pos[:, 2], neg_items])
            labels = np.concatenate([np.ones(batch_size, np.float32), np.zeros(batch_size * k, np.float32)])
            dev = GraphDataset.device
            yield (torch.from_numpy(users).to(dev), torch.from_numpy(queries).to(dev),
                   torch.from_numpy(items).to(dev), torch.from_numpy(labels).to(dev))


class DeviceBatchLoader:
    """Training-batch source that never leaves the GPU (``GraphDataset.device_batches``): drop-in for the ``DataLoader`` of the
    training loop (iterating yields the ``collate_fn`` 8-tuple; ``batch_sampler.set_epoch`` selects the epoch's permutation)."""

    def __init__(self, dataset: GraphDataset, batch_size: int, rank: int = 0, world_size: int = 1, seed: int = 0):
        self.dataset, self.batch_size, self.rank, self.world_size, self.seed = dataset, batch_size, rank, world_size, seed
        self.epoch = 0
        self.batch_sampler = self

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        return -(-(-(-len(self.dataset) // self.world_size)) // self.batch_size)

    def __iter__(self):
        return self.dataset.device_batches(self.batch_size, self.epoch, self.seed, self.rank, self.world_size)


class _PinnedRing:
    """A few page-locked staging buffers reused round-robin: a pageable ``.to(device)`` blocks the host until every kernel
    queued before it has run, which serialises the training loop with the GPU once per step; a pinned, non-blocking copy does
    not.  A slot is reused only after the copy that last read it has executed (event per slot)."""

    SLOTS = 4

    def __init__(self):
        self.buffers = [None] * self.SLOTS
        self.events = [None] * self.SLOTS
        self.cursor = 0

    def stage(self, array: np.ndarray) -> Tensor:
        k = self.cursor
        self.cursor = (k + 1) % self.SLOTS
        if self.events[k] is not None:
            self.events[k].synchronize()
        n = array.size
        buf = self.buffers[k]
        if buf is None or buf.numel() < n or buf.dtype != torch.from_numpy(array).dtype:
            buf = self.buffers[k] = torch.empty(max(n, 4096), dtype=torch.from_numpy(array).dtype).pin_memory()
        view = buf[:n].view(array.shape)
        view.copy_(torch.from_numpy(array))
        return view

    def mark(self, k_stream_event) -> None:
        self.events[(self.cursor - 1) % self.SLOTS] = k_stream_event


_RING = None


def _to_device_async(array: np.ndarray, device: torch.device) -> Tensor:
    """Host array -> device tensor without stalling the host behind the GPU's queue (see ``_PinnedRing``)."""
    global _RING
    if device.type != 'cuda':
        return torch.from_numpy(array).to(device)
    if _RING is None:
        _RING = _PinnedRing()
    staged = _RING.stage(np.ascontiguousarray(array))
    out = staged.to(device, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    _RING.mark(ev)
    return out


class TestSearchLogDataLoader:
    """Evaluation logs: every search with >= 1 positive, as (user, query, de-duplicated positive items).

    Iteration yields the reference's 5-tuple (``Dataset.py:324-329``).  ``users`` / ``queries`` are length-``I``
    index vectors like the reference's ``u * ones(I)``, but as stride-0 expansions of a single element, so the
    model can tell "one (user, query) against every item" apart and score it as a matrix-vector product.
    """
    __test__ = False          # not a pytest class

    def __init__(self, fn_search_log: str, dataset_train: GraphDataset, device: torch.device):
        self.logs: List[Tuple[int, int, List[int], Optional[List[int]], bool]] = []
        rows = 0
        with open(fn_search_log, 'r', encoding='utf-8') as f:
            next(f, None)
            for line in f:
                if not line.strip():
                    continue
                rows += 1
                log = SearchLog.parse(line)
                if sum(log.interactions) > 0:
                    self.logs.append((log.user, log.query, log.get_interacted_items()[0], None, True))
        self.item_count = dataset_train.item_count
        self.device = device
        IOHelper.LogPrint(f'evaluation set ready: {fn_search_log} ({rows} rows, {len(self.logs)} usable logs)')

    def __len__(self) -> int:
        return len(self.logs)

    def __iter__(self):
        if not self.logs:
            return
        uq = torch.tensor([(u, q) for u, q, *_ in self.logs], dtype=torch.long, device=self.device)
        for k, (_, _, items, flags, all_1) in enumerate(self.logs):
            yield uq[k, 0:1].expand(self.item_count), uq[k, 1:2].expand(self.item_count), items, flags, all_1
