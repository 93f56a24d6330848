"""The Srrl baseline (reference ``Models/Srrl.py``): KG and PS embeddings, small MLPs, no graph propagation.

Same parameters, state-dict keys, initialisation and methods as the reference.  Every module of the model is the block ``F.normalize(cat(a, b), dim=-1)`` ->
``nn.Linear`` -> optional ``nn.LeakyReLU()``; here a block is one launch of ``ihg_cat_linear_fwd`` (``ops.cat_linear``) that reads its two operands where they are -
rows of an embedding table named by an index vector, or a ``[B, 1, .]`` operand repeated over the k negatives - instead of the reference's gather / expand / cat /
normalize / Linear / LeakyReLU sequence with a ``[rows, 2d]`` temporary each.  The KG scores are ``ops.rows_dot``; evaluation ranks with ``ihg_rows_topk``.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from .. import ops
from ..Helpers.GlobalSettings import Gs
from .CommonLayers import MLP, Aggregation
from .EmbeddingLayers import EmbeddingLayer
from .PredictionLayers import HemPredictionLayer

Source = Tuple[Tensor, Optional[Tensor]]      # (row table, index vector or None = all rows in order)

EVALUATION_TEMPORARY_BYTES = 1 << 30           # top_items sizes its chunks of (user, query) pairs to stay under this


class Srrl(nn.Module):
    def __init__(self, dataset, embedding_size: int, prediction_layer_type, lambda_muq: float):
        super().__init__()
        if prediction_layer_type is HemPredictionLayer:
            raise NotImplementedError('Srrl with the HEM head is not part of this build (the reference\'s driver never builds it, Main.py:179)')
        self.dataset = dataset
        self.embedding_size = embedding_size
        self.prediction_layer_type = prediction_layer_type
        self.lambda_muq = lambda_muq

        self.KG = EmbeddingLayer(dataset=dataset, embedding_size=embedding_size)
        self.PS = EmbeddingLayer(dataset=dataset, embedding_size=embedding_size)
        self.PS.embedding_bag_vocabulary = None          # the queries are the KG's (Srrl.py:37-42)
        for table in (self.KG.embedding_user, self.KG.embedding_item, self.KG.embedding_bag_vocabulary, self.PS.embedding_user, self.PS.embedding_item):
            self.init_embedding(table)

        d = embedding_size
        self.kg_aggre_head = Aggregation(2 * d, d)
        self.kg_aggre_query = Aggregation(2 * d, d)
        self.kg_aggre_tail = Aggregation(2 * d, d)
        self.kg_mlp_pre = MLP(2 * d, d)
        self.g_u = Aggregation(2 * d, d)
        self.g_i = Aggregation(2 * d, d)
        self.ps_mlp_uq = MLP(2 * d, d)
        self.ps_mlp_ui = MLP(2 * d, d)
        self.ps_mlp_pred = MLP(2 * d, 1)
        self.init_parameters()

        self.srrl_steps = 0
        self.train_iterator_KG = None
        self.clear_saved_feature()

    # ------------------------------------------------------------------ initialisation (Srrl.py:236-252)
    def init_embedding(self, emb) -> None:
        emb.weight.data = F.normalize(emb.weight.data, p=2, dim=1)

    def init_parameters(self, method: str = 'xavier', exclude: str = 'embedding') -> None:
        for name, w in self.named_parameters():
            if exclude in name:
                continue
            if 'weight' in name:
                {'xavier': nn.init.xavier_normal_, 'kaiming': nn.init.kaiming_normal_}.get(method, nn.init.normal_)(w)
            elif 'bias' in name:
                nn.init.constant_(w, 0)

    # ------------------------------------------------------------------ the knowledge graph
    def trainkg(self, sample, mode: str, positive_mode: bool) -> Tensor:
        """Scores of a KG batch (Srrl.py:72-98, 176-234): ``[B, 1]`` for the positives, ``[B, k]`` for the negatives.  ``sample`` = (positives ``[B, 3]``, (negatives
        ``[B, k]``,) true tails, true heads, true queries ``[B, 1]`` each)."""
        if positive_mode:
            positive, items2, users2, queries2 = sample
            item_ids, k = positive[:, 2], 1
        else:
            positive, negatives, items2, users2, queries2 = sample
            item_ids, k = negatives.long().reshape(-1), int(negatives.shape[1])
        users, items, queries = self.KG.embed_user(), self.KG.embed_item(), self.KG.embed_query()
        u, q, i = positive[:, 0], positive[:, 1], positive[:, 2]
        batch = int(positive.shape[0])
        if mode == 'tail-company-batch':
            if positive_mode:
                scored = self.kg_aggre_tail(items, items, idx_a=i, idx_b=items2[:, 0])
            else:
                scored = self.kg_aggre_tail(items, items, idx_a=item_ids, idx_b=i, rep_b=k)       # the positive's item beside each of its negatives
            context = self.kg_mlp_pre(users, queries, idx_a=u, idx_b=q)
        elif mode == 'head-company-batch':
            scored = ops.gather_rows(items, item_ids)
            context = self.kg_mlp_pre(self.kg_aggre_head(users, users, idx_a=u, idx_b=users2[:, 0]), queries, idx_b=q)
        elif mode == 'query-company-batch':
            scored = ops.gather_rows(items, item_ids)
            context = self.kg_mlp_pre(users, self.kg_aggre_query(queries, queries, idx_a=q, idx_b=queries2[:, 0]), idx_a=u)
        else:
            raise ValueError(f'KG batch mode {mode!r}')
        return ops.rows_dot(scored, context, rep=k).view(batch, k)

    # ------------------------------------------------------------------ personalised search
    def _latents(self, uids: Tensor, items: Optional[Tensor]):
        """-> (user source, item source, query table): the operands of the three PS MLPs, from the saved features under evaluation."""
        saved = self._saved_q_kg is not None
        ps_u = self._saved_u_ps if saved else self.PS.embed_user()
        ps_i = self._saved_i_ps if saved else self.PS.embed_item()
        q_all = self._saved_q_kg if saved else self.KG.embed_query()
        if not Gs.Srrl.KG_loss:
            return (ps_u, uids), (ps_i, items), q_all
        kg_u = self._saved_u_kg if saved else self.KG.embed_user().detach()      # the KG rows are constants of the PS step (Srrl.py:115-116)
        kg_i = self._saved_i_kg if saved else self.KG.embed_item().detach()
        u_latent = self.g_u(ps_u, kg_u, idx_a=uids, idx_b=uids)
        if saved and items is None and self._saved_i_latent is not None:
            i_latent = self._saved_i_latent
        else:
            i_latent = self.g_i(ps_i, kg_i, idx_a=items, idx_b=items)
        return (u_latent, None), (i_latent, None), q_all

    def forward(self, uids: Tensor, queries: Tensor, items: Optional[Tensor] = None) -> Tensor:
        """Scores of a batch of triples (Srrl.py:101-159); ``items=None``: row r pairs (uids[r], queries[r]) with item r, over all items."""
        (u, u_idx), (i, i_idx), q_all = self._latents(uids, items)
        uq = self.ps_mlp_uq(u, q_all, idx_a=u_idx, idx_b=queries)
        ui = self.ps_mlp_ui(u, i, idx_a=u_idx, idx_b=i_idx)
        return self.ps_mlp_pred(uq, ui).squeeze(-1)

    def bce_loss(self, uids: Tensor, queries: Tensor, items: Tensor, labels: Tensor) -> Tensor:
        """``nn.BCEWithLogitsLoss()(self(uids, queries, items), labels)`` with the loss and its gradient from one launch."""
        return ops.bce_with_logits(self(uids, queries, items), labels)

    def training_loss(self, uids: Tensor, queries: Tensor, items: Tensor, objective, labels: Optional[Tensor] = None, cotangent_sync=None) -> Tensor:
        """``RawGnn.training_loss``'s signature; the baseline trains on the BCE over ``labels`` alone, in one process (``Main.check_srrl_settings`` refuses the rest)."""
        if objective.grouped or cotangent_sync is not None:
            raise NotImplementedError('the Srrl baseline trains on the BCE in one process: no --loss bpr | softmax, no --hard_negatives, no gradient exchange')
        return self.bce_loss(uids, queries, items, labels)

    def save_features_for_test(self) -> None:
        """Evaluation (no gradient): keeps the tables, and what does not depend on the (user, query) pair - ``g_i`` over all items."""
        self._saved_u_ps, self._saved_i_ps = self.PS.embed_user(), self.PS.embed_item()
        self._saved_q_kg = self.KG.embed_query()
        if Gs.Srrl.KG_loss:
            self._saved_u_kg, self._saved_i_kg = self.KG.embed_user(), self.KG.embed_item()
            self._saved_i_latent = self.g_i(self._saved_i_ps, self._saved_i_kg)

    def clear_saved_feature(self) -> None:
        self._saved_u_kg = self._saved_q_kg = self._saved_i_kg = None
        self._saved_u_ps = self._saved_i_ps = None
        self._saved_i_latent = None
        self._tiled_items = None

    def evaluation_chunk_pairs(self, item_count: int) -> int:
        """(user, query) pairs per chunk of ``top_items``: per scored row the hidden and output rows of ``ps_mlp_ui`` and ``ps_mlp_pred``, the inverse norm each of
        the two normalising blocks stores, and the item index."""
        d = self.embedding_size
        row_bytes = 4 * (2 * d + d + 2 * d + 1) + 2 * 4 + 8
        return max(1, EVALUATION_TEMPORARY_BYTES // (row_bytes * max(item_count, 1)))

    def top_items(self, users: Tensor, queries: Tensor, k: int = 10):
        """The ``k`` best items of every (user, query) pair over ALL items: ``(items [C, k] int64, scores [C, k])``, best first, equal scores in ascending item id.
        Chunks of pairs x all items go through the block kernels (the pair's rows by the repeat factor), then ``ihg_rows_topk``; needs ``save_features_for_test``."""
        if self._saved_q_kg is None:
            raise RuntimeError('Srrl.top_items: call save_features_for_test() first')
        n_items = int(self._saved_i_ps.shape[0])
        chunk = self.evaluation_chunk_pairs(n_items)
        top_i, top_s = [], []
        with torch.no_grad():
            for lo in range(0, int(users.shape[0]), chunk):
                u, q = users[lo:lo + chunk], queries[lo:lo + chunk]
                c = int(u.shape[0])
                if self._tiled_items is None or self._tiled_items.shape[0] < c * n_items:
                    self._tiled_items = torch.arange(n_items, device=u.device).repeat(c)
                every_item = self._tiled_items[:c * n_items]
                (u_rows, u_idx), (i_rows, _), q_all = self._latents(u, None)
                uq = self.ps_mlp_uq(u_rows, q_all, idx_a=u_idx, idx_b=q)                                   # [C, d]: once per pair
                ui = self.ps_mlp_ui(u_rows, i_rows, idx_a=u_idx, rep_a=n_items, idx_b=every_item)          # [C I, d]
                scores = self.ps_mlp_pred(uq, ui, rep_a=n_items).view(c, n_items)
                items, best = ops.rows_topk(scores, k)
                top_i.append(items)
                top_s.append(best)
        return torch.cat(top_i), torch.cat(top_s)
