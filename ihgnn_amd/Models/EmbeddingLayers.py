"""Input node features (reference ``Models/EmbeddingLayers.py``).

Same parameters and state-dict keys as the reference (``embedding_user.weight [U+1,d]``,
``embedding_item.weight [I+1,d]``, ``embedding_bag_vocabulary.weight [V+1,d]``; row 0 of each is the
padding row, xavier-uniform initialised), but the full-graph lookup that every training step performs
(``EmbeddingLayer(None, None, None)``, ``RawGnn.py:112``) is not three gather kernels:

* users / items: ids are exactly ``1..U`` / ``1..I`` (``Dataset.py:153-154``), so the "lookup" is the view
  ``weight[1:]`` - no kernel, and its backward is a plain dense gradient;
* queries: the HIP embedding-bag mean kernel over the CSR of query words (``ihg_bag_mean_fwd/bwd``); with ``Gs.Query.transform == Gsv.activation`` the
  reference's ``query_transform = nn.Sequential(nn.Linear(d, d), Gs.Query.transform_activation())`` (``EmbeddingLayers.py:40-44``, applied at 83-84) on top of it:
  the module is built as in the reference (state-dict keys, shapes, default init, RNG consumption), its forward is the row GEMM with the activation in its
  epilogue (``ihg_rows_linear_act_fwd/bwd``) - ``nn.ReLU`` and ``nn.Tanh``.  ``Gsv.rnn`` raises, as in the reference;
* ``Gs.Query.transform == Gsv.gru`` (not in the reference, which names a recurrent query model and raises for it): ``query_transform = nn.GRU(d, d, batch_first=True)``
  - state-dict keys ``query_transform.weight_ih_l0 / weight_hh_l0 / bias_ih_l0 / bias_hh_l0``, torch's default init and RNG draws - whose module is never called: a
  query's row of X0 is the last hidden state of that GRU over the rows of its words in file order, from ``h_0 = 0`` (``ihg_gru_fwd/bwd``, fp32 MFMA; a query without
  words: the zero row).  The bag mean is not formed and ``--query_activation`` does not apply.
"""
from typing import Optional, Tuple

import torch.nn as nn
import torch.nn.init as init
from torch import Tensor

from .. import ops
from ..Helpers.GlobalSettings import Gs, Gsv


QUERY_ACTIVATION_NAMES = {nn.ReLU: 'relu', nn.Tanh: 'tanh'}     # Gs.Query.transform_activation -> ops.QUERY_ACTIVATIONS


class EmbeddingLayer(nn.Module):
    def __init__(self, dataset, embedding_size: int):
        super().__init__()
        if Gs.Query.transform not in (Gsv.mean, Gsv.activation, Gsv.gru):
            raise NotImplementedError(f'query transform {Gs.Query.transform!r}: mean, activation and gru are on the MI355X path (the reference itself raises for rnn, EmbeddingLayers.py:45-46)')
        self.dataset = dataset
        self.embedding_size = embedding_size
        self.embedding_user = EmbeddingLayer.create_embedding(dataset.user_count + 1, embedding_size, padding_idx=0)
        self.embedding_item = EmbeddingLayer.create_embedding(dataset.item_count + 1, embedding_size, padding_idx=0)
        self.embedding_bag_vocabulary = EmbeddingLayer.create_embedding_bag(dataset.vocab_size + 1, embedding_size)
        self.query_activation: Optional[str] = None           # the activation's name for the kernels ('relu' | 'tanh'); None: the plain bag mean
        if Gs.Query.transform == Gsv.activation:
            act = Gs.Query.transform_activation
            if act not in QUERY_ACTIVATION_NAMES:
                raise NotImplementedError(f'query transform activation {act!r}: nn.ReLU and nn.Tanh are on the MI355X path')
            self.query_activation = QUERY_ACTIVATION_NAMES[act]
            self.query_transform = nn.Sequential(nn.Linear(embedding_size, embedding_size), act())      # (EmbeddingLayers.py:40-44: same keys, init and RNG draws)
        elif Gs.Query.transform == Gsv.gru:
            self.query_transform = nn.GRU(embedding_size, embedding_size, batch_first=True)                # one layer, one direction; only its parameters are used

    def _transform(self) -> ops.QueryTransform:
        """The query transform as the ops take it: its kind and its parameter tensors."""
        if isinstance(getattr(self, 'query_transform', None), nn.GRU):
            gru = self.query_transform
            return ops.QueryTransform(ops.QueryTransform.GRU, (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0))
        if self.query_activation is None:
            return ops.QueryTransform()
        linear = self.query_transform[0]
        return ops.QueryTransform(ops.QueryTransform.ACTIVATION, (linear.weight, linear.bias), activation=self.query_activation)

    def forward(self, user_indices: Optional[Tensor] = None, query_indices: Optional[Tensor] = None,
                item_indices: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        return self.embed_user(user_indices), self.embed_query(query_indices), self.embed_item(item_indices)

    def all_nodes(self, out: Optional[Tensor] = None) -> Tensor:
        """``torch.cat(self(None, None, None))`` as one op (``RawGnn.py:112-113``): ``[U+Q+I, d]``.  ``out`` (inference only): write into
        this ``[N, d]`` destination (a column slice of the feature matrix)."""
        return ops.embed_all_nodes(self.embedding_user.weight, self.embedding_item.weight, self.embedding_bag_vocabulary.weight, self.dataset.bag_layout, out, transform=self._transform())

    def node_tables(self, holder):
        """The same features WITHOUT assembling them (``ops.NodeTables``): the first layer's node-level transform reads the tables in place and its backward writes
        their gradients in place; ``None`` where the library does not offer that (other widths, fp32-MFMA arithmetic)."""
        tables = (self.embedding_user.weight, self.embedding_item.weight, self.embedding_bag_vocabulary.weight)
        if not ops.NodeTables.supported(*tables):
            return None
        return ops.NodeTables(*tables, self.dataset.bag_layout, holder, transform=self._transform())

    def embed_user(self, user_indices: Optional[Tensor] = None) -> Tensor:
        w = self.embedding_user.weight
        return w[1:] if user_indices is None else w[user_indices + 1]

    def embed_item(self, item_indices: Optional[Tensor] = None) -> Tensor:
        w = self.embedding_item.weight
        return w[1:] if item_indices is None else w[item_indices + 1]

    def embed_query(self, query_indices: Optional[Tensor] = None) -> Tensor:
        queries = ops.bag_mean(self.embedding_bag_vocabulary.weight, self.dataset.bag_layout, transform=self._transform())
        return queries if query_indices is None else queries[query_indices]

    def embed_bags(self, words, offsets) -> Tensor:
        """``[C, d]``: the layer-0 rows of ``C`` queries given by their words - ``words`` flat 0-based word ids as ``GraphDataset`` reads them from
        ``queries_multihot.txt``, ``offsets`` the start of every bag (``nn.EmbeddingBag``'s input) - through the kernels of ``embed_query`` over an ad-hoc
        ``ops.BagLayout``: the bag mean, then the query transform where there is one, or the GRU over the words in order.  An empty bag gives a zero row, or ``act(b)`` under the activation transform, as in
        training; a bag that equals a training query's words gives that query's X0 row bit for bit."""
        import numpy as np
        words = np.asarray(words.cpu() if isinstance(words, Tensor) else words, dtype=np.int64).reshape(-1)
        offsets = np.asarray(offsets.cpu() if isinstance(offsets, Tensor) else offsets, dtype=np.int64).reshape(-1)
        table = self.embedding_bag_vocabulary.weight
        bag = ops.BagLayout(words + 1, offsets, int(table.shape[0]), table.device)      # (stored id = index + 1: row 0 is padding)
        return ops.bag_mean(table, bag, transform=self._transform())

    @staticmethod
    def create_embedding(num_embeddings: int, embedding_dimension: int, padding_idx: Optional[int] = None) -> nn.Embedding:
        table = nn.Embedding(num_embeddings, embedding_dimension, padding_idx=padding_idx)
        init.xavier_uniform_(table.weight)
        return table

    @staticmethod
    def create_embedding_bag(num_embeddings: int, embedding_dimension: int, mode: str = 'mean') -> nn.EmbeddingBag:
        table = nn.EmbeddingBag(num_embeddings, embedding_dimension, mode=mode)
        init.xavier_uniform_(table.weight)
        return table
