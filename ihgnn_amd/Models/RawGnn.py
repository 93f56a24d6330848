"""The model (reference ``Models/RawGnn.py``): embeddings -> L hypergraph layers -> concat -> row gathers -> HEM.

Same constructor keywords, ``forward(user_indices, query_indices, item_indices=None)``,
``save_features_for_test`` / ``clear_saved_feature`` and state-dict keys (``embeddings.*``, ``gnn_{l}.*``,
``prediction_layer.items_bias``) as the reference, so its driver and checkpoints carry over.
"""
from typing import Optional, Type

import torch
import torch.nn as nn
from torch import Tensor

from ..Helpers.GlobalSettings import Gs
from .EmbeddingLayers import EmbeddingLayer
from .GnnLayers import GATLayer, GCNLayer, HGCNLayer, IHGNNLayer
from .PredictionLayers import HemPredictionLayer


class RawGnn(nn.Module):
    _saved_output_feature: Optional[Tensor] = None

    def __init__(self, device: torch.device, dataset, embedding_size: int, gnn_layer_type: Type,
                 gnn_layer_count: int, feature_interaction_order: int, phase2_attention: bool,
                 predictions: Type, lambda_muq: float):
        super().__init__()
        self.device = device
        self.dataset = dataset
        self.embedding_size = embedding_size
        self.gnn_layer_type = gnn_layer_type
        self.gnn_layer_count = gnn_layer_count
        self.feature_interaction_order = feature_interaction_order
        self.phase2_attention = phase2_attention
        self.prediction_layer_type = predictions
        self.output_feature_size = embedding_size * (1 + gnn_layer_count)
        # the width the kernels run at: the embedding size itself where it is one of the tiled widths (32 / 64 / 128 / 256), otherwise the next of them with zero columns
        # appended to the features and zero rows / columns to the weights (ops.padded_width: 96 -> 128, 160 / 192 / 224 -> 256; the reference takes any --emb,
        # Helpers/ArgsParser.py:94-95) - parameters and state-dict keep the embedding size
        from .. import ops as _ops
        self.compute_width = _ops.padded_width(embedding_size)
        if self.compute_width * (1 + gnn_layer_count) > self.MAX_SCORED_WIDTH:
            self.compute_width = embedding_size                  # (padding would push the scored row past the evaluation kernel's limit: the any-width kernels instead)
        if self.output_feature_size > self.MAX_SCORED_WIDTH:
            # refused HERE, not at the first evaluation after an epoch of training: the scoring kernel (ihg_score_topk) keeps the mixed rows of 32
            # (user, query) pairs in LDS for its whole run, which bounds the feature width d (L + 1)
            raise NotImplementedError(f'RawGnn: feature width embedding_size * (layers + 1) = {self.output_feature_size} exceeds {self.MAX_SCORED_WIDTH}, the widest '
                                      'matrix the MI355X evaluation kernel scores (32 mixed rows in 160 KB of LDS); use a smaller embedding or fewer layers')

        self.embeddings = EmbeddingLayer(dataset=dataset, embedding_size=embedding_size)

        self.gnns = []
        for depth in range(gnn_layer_count):
            if gnn_layer_type is IHGNNLayer:
                # only the first layer interacts at the requested order; deeper layers are first-order (RawGnn.py:76-78)
                order = feature_interaction_order if depth == 0 else min(feature_interaction_order, 1)
                layer = IHGNNLayer(device=device, dataset=dataset, input_dimension=embedding_size,
                                   output_dimension=embedding_size, feature_interaction_order=order,
                                   phase2_attention=phase2_attention)
            elif gnn_layer_type in (HGCNLayer, GCNLayer, GATLayer):
                layer = gnn_layer_type(device=device, dataset=dataset, input_dimension=embedding_size,
                                       output_dimension=embedding_size)
            else:
                raise NotImplementedError(f'unsupported GNN layer type: {gnn_layer_type}')
            self.gnns.append(layer)
            self.add_module(f'gnn_{depth}', layer)

        if predictions is not HemPredictionLayer:
            raise NotImplementedError(f'unsupported prediction layer type: {predictions}')
        self.prediction_layer = HemPredictionLayer(feature_dimension=self.output_feature_size, lambda_muq=lambda_muq,
                                                   item_count=dataset.item_count)

    # bce_loss: evaluate the last layer's hyperedge -> node pass only at the rows the loss reads (same loss, same gradients)
    batch_rows_only_last_layer = True
    MAX_SCORED_WIDTH = 1264                                   # = ihg_score_topk_max_dim() (tests/test_abi.py): 32 mixed rows as two fp16 planes in 160 KB of LDS

    def _compact_layout(self):
        """The hypergraph layout when it numbers its nodes WITHOUT the isolated ones (``IncidenceLayout.compact``: config C5, where two thirds of the nodes are in no
        hyperedge), else ``None``.  Every layer output of an isolated node is exactly zero (an empty sum times ``Dv^-1``), so the layers run on the
        layout's N' nodes and this class translates at its edges: X0 is gathered from the public ``[N, d]`` rows, the batch tail reads layer 0 by public row and the layers
        above through ``layout.node_map``, public callers get ``[N, d]`` matrices with zero rows put back."""
        lay = getattr(self.gnns[0], 'layout', None) if self.gnns else None
        return lay if (lay is not None and getattr(lay, 'compact', False)) else None

    def propagate_layers(self, tail_gradients=None, batch_rows=None, restrict_last_layer=True):
        """Full-graph propagation: the list ``[X0, X1, ..., XL]`` of ``[N, d]`` node features (input embeddings and every
        layer's output).  With ``tail_gradients`` (an ``ops.TailGradients``) every output is tapped: the returned tensors
        are the batch tail's halves, whose gradients travel through the holder instead of dense ``[N, d]`` tensors.
        ``batch_rows`` (int64 node rows): nobody reads ``XL`` outside these rows (a training step scores the batch only).  With
        ``restrict_last_layer`` the last hypergraph layer computes just them (plus the split rows of its plan) and leaves the rest
        unwritten; without it every row is computed and the layer is only told that its cotangent is zero outside them.

        Over a layout without the isolated nodes (``_compact_layout``): with ``tail_gradients`` the halves above layer 0 are ``[N', d]`` in the LAYOUT's numbering (the
        holder carries the row map; ``bce_loss`` is their only consumer), without it every output is returned in the public numbering."""
        from .. import ops
        last = len(self.gnns)
        x = None
        padded = self.compute_width != self.embedding_size
        compact = self._compact_layout()
        tables = None
        if (tail_gradients is not None and last >= 1 and ops.NODE_TABLES and not padded
                and (batch_rows is None or int(batch_rows.shape[0]) <= ops.SCATTER_CHUNK_ROWS)):
            # a training step through the fused batch tail: X0 is not assembled - the first layer's transform and the tail read the embedding tables in place
            tables = self.embeddings.node_tables(tail_gradients)
        if tables is not None:
            # ... over a layout without the isolated nodes the active nodes' rows are gathered straight from the tables ([N', d]; the public [N, d] is never assembled), the
            # tail reads its layer-0 rows from the tables in place and the gather's backward adds their gradients to the tables' gradients
            x = tables if compact is None else ops.gather_active_nodes(tables, compact)
        if x is None:
            x = self.embeddings.all_nodes()
            if padded:
                x = ops.pad_columns(x, self.compute_width)   # zero columns up to the next tiled width; every layer keeps them zero (its weights are padded with zeros)
        layer_rows = batch_rows
        if compact is not None and batch_rows is not None:
            # the rows the LAYERS are told (computed / differentiated rows of the last layer): the layout's own; an isolated batch node maps to row 0 - one more row listed
            layer_rows = compact.compact_rows(batch_rows, isolated_to=0)
        outputs = []
        for depth in range(last + 1):
            sparse_top = None
            if depth > 0:
                layer = self.gnns[depth - 1]
                if depth == last and batch_rows is not None and isinstance(layer, (IHGNNLayer, HGCNLayer)):
                    rows = getattr(layer_rows, 'as_int32', None)
                    if rows is None:
                        rows = layer_rows.to(torch.int32)
                    x = layer(x, output_rows=rows) if restrict_last_layer else layer(x, cotangent_rows=rows)
                    # the layer's backward pulls the listed rows of its cotangent only (the masked two-hop pull): the tap writes them and fills nothing
                    if ((restrict_last_layer or ops.SPARSE_LAST_COTANGENT) and not ops.CHECK_SPARSE_COTANGENT and layer.reads_cotangent_rows_only()
                            and int(batch_rows.shape[0]) <= ops.SCATTER_CHUNK_ROWS):
                        sparse_top = layer.layout
                else:
                    x = layer(x)
            if tail_gradients is not None:
                if depth == 0 and tables is not None:
                    outputs.append(tables)                   # (no tap: the first layer's transform - over a compact layout the gather's backward - adds the tail's layer-0 gradients itself)
                    continue
                x, for_tail = ops.tap(x, tail_gradients, depth, sparse_top)
                outputs.append(for_tail)
            elif compact is not None and depth > 0:
                outputs.append(self._to_public_rows(x, compact))
            else:
                outputs.append(x)
            if compact is not None and depth == 0 and tables is None:
                x = x.index_select(0, compact.active_nodes)  # X0 of the nodes that have hyperedges: what the layers run on
        return outputs

    @staticmethod
    def _to_public_rows(x: Tensor, compact) -> Tensor:
        """``[N', d]`` in the layout's numbering -> ``[N, d]`` in the public one, zero rows for the isolated nodes (differentiable)."""
        return torch.zeros(compact.public_node_count, x.shape[1], dtype=x.dtype, device=x.device).index_copy(0, compact.active_nodes, x)

    def propagate(self) -> Tensor:
        """``[N, d*(L+1)]``: all layer outputs side by side (``RawGnn.py:122``).  Outside autograd (the evaluation cache,
        ``save_features_for_test``) the matrix is allocated once and every layer WRITES ITS COLUMN SLICE of it - the kernels take row
        strides, layer l reads columns ``(l-1) d ..`` and writes columns ``l d ..`` of the same buffer - so there is no concatenation
        pass over ``[N, D]``.  Under autograd the outputs are separate tensors and are concatenated."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._without_padding_columns(torch.cat(self.propagate_layers(), 1))
        d, cw = self.embedding_size, self.compute_width
        w = self.embeddings.embedding_bag_vocabulary.weight
        features = torch.empty(self.dataset.node_count, cw * (1 + self.gnn_layer_count), dtype=torch.float32, device=w.device)
        self.embeddings.all_nodes(out=features[:, :d])
        if cw != d:
            features[:, d:cw].zero_()                        # (a width between the tiled ones: zero padding columns, kept zero by every layer; the scores do not see them)
        x = features[:, :cw]
        compact = self._compact_layout()
        if compact is not None:
            # the layers run on the layout's N' nodes (the ones that have hyperedges); their rows go back to the public matrix, the isolated nodes' rows are zero
            x = x.index_select(0, compact.active_nodes)
            features[:, cw:].zero_()
            for depth, layer in enumerate(self.gnns, 1):
                x = layer(x)
                features[:, depth * cw:(depth + 1) * cw].index_copy_(0, compact.active_nodes, x)
            return self._without_padding_columns(features)
        for depth, layer in enumerate(self.gnns, 1):
            x = layer(x, out=features[:, depth * cw:(depth + 1) * cw])
        return self._without_padding_columns(features)

    def _without_padding_columns(self, features: Tensor) -> Tensor:
        """``[N, cw (L + 1)]`` computed at a padded width -> the reference's ``[N, d (L + 1)]`` (``RawGnn.py:122``): the zero columns between the layers' blocks cut out."""
        d, cw = self.embedding_size, self.compute_width
        if cw == d:
            return features
        n = features.shape[0]
        return features.view(n, 1 + self.gnn_layer_count, cw)[:, :, :d].reshape(n, self.output_feature_size)

    def forward(self, user_indices: Tensor, query_indices: Tensor, item_indices: Optional[Tensor] = None) -> Tensor:
        """Indices are 0-based per type.  ``item_indices=None`` scores the given (user, query) against every item."""
        ds = self.dataset
        if self._saved_output_feature is None and item_indices is not None:
            # Training step.  The reference concatenates all layer outputs into [N, D] and gathers three [B, D] row sets
            # from it (RawGnn.py:122-131); here the 3B rows are gathered from each layer's [N, d] output with ONE index
            # op and concatenated afterwards ([3B, D] instead of [N, D]): same values, and the backward is one
            # scatter per layer instead of three dense [N, D] gradients that autograd would have to add up.
            rows = torch.cat([user_indices, query_indices + ds.query_start_index_in_graph,
                              item_indices + ds.item_start_index_in_graph])
            layers = self.propagate_layers()
            head = self.prediction_layer
            if layers[0].is_cuda and len(layers) <= 8:
                from .. import ops
                return ops.hem_score(layers, rows, item_indices, head.items_bias, head.lambda_muq, ds.item_start_index_in_graph,
                                     cosine=Gs.Prediction.use_cosine_similarity)      # fused batch tail (either head: the setting is read at every call, PredictionLayers.py:38)
            picked = torch.cat([x[rows] for x in layers], 1)
            b = user_indices.shape[0]
            return head(picked[:b], picked[b:2 * b], picked[2 * b:], item_indices)
        features = self._saved_output_feature if self._saved_output_feature is not None else self.propagate()
        if item_indices is None:
            item_feature = features[ds.item_start_index_in_graph:]
            if user_indices.dim() == 1 and user_indices.numel() > 1 and user_indices.stride(0) == 0 and query_indices.stride(0) == 0:
                user_indices, query_indices = user_indices[:1], query_indices[:1]      # one pair broadcast over all items
        else:
            item_feature = features[item_indices + ds.item_start_index_in_graph]
        user_feature = features[user_indices]
        query_feature = features[query_indices + ds.query_start_index_in_graph]
        return self.prediction_layer(user_feature, query_feature, item_feature, item_indices)

    def bce_loss(self, user_indices: Tensor, query_indices: Tensor, item_indices: Tensor, labels: Tensor, cotangent_sync=None) -> Tensor:
        """``nn.BCEWithLogitsLoss()(self(u, q, i), labels)`` with scoring, loss and their backward fused into the batch-tail
        kernels (the training loops use it when the loss function is a plain ``BCEWithLogitsLoss``).

        ``cotangent_sync`` (an ``ihgnn_amd.distributed.CotangentSync``; data parallel): this rank's loss on ITS batch, with a backward that yields the gradient of the
        MEAN of all ranks' losses - the ranks exchange the batch rows' cotangents (not the dense gradients) and every rank runs the propagation backward on their
        union; the layers are told the union of the ranks' batch rows (where the last layer's output is read / its cotangent is non-zero).  A COLLECTIVE: every
        rank calls it, with batches of the same size."""
        from .. import ops
        return self.training_loss(user_indices, query_indices, item_indices, ops.bce_objective(), labels, cotangent_sync)

    def ranking_loss(self, user_indices: Tensor, query_indices: Tensor, item_indices: Tensor, positives: int, kind: Optional[str] = None, cotangent_sync=None) -> Tensor:
        """``ops.ranking_loss(self(u, q, i), positives, kind)`` through the fused batch tail: ``bce_loss`` with the BPR (``'bpr'``) or sampled-softmax (``'softmax'``)
        loss of every positive against its own negatives in place of the BCE.  The batch is ``positives`` positives followed by the ``k`` negatives of each (the negatives
        of positive ``p`` at rows ``P + p k ..``: ``collate_fn``'s layout); no labels.  ``kind=None`` reads ``Gs.Training.loss`` at every call, as the head flag is
        read; ``'bce'`` needs labels and is ``bce_loss``'s.  ``cotangent_sync``: as in ``bce_loss`` (every rank's groups stay its own: the exchange moves row gradients)."""
        from .. import ops
        kind = Gs.Training.loss if kind is None else kind
        if kind == 'bce':
            raise ValueError('RawGnn.ranking_loss: the BCE needs labels - use bce_loss (Gs.Training.loss is \'bce\')')
        objective = ops.ranking_objective(int(item_indices.shape[0]), positives, kind)
        return self.training_loss(user_indices, query_indices, item_indices, objective, cotangent_sync=cotangent_sync)

    def hard_negative_loss(self, user_indices: Tensor, query_indices: Tensor, item_indices: Tensor, positives: int, keep: int, kind: Optional[str] = None,
                           cotangent_sync=None, return_selected: bool = False):
        """``ops.hard_negative_loss(self(u, q, i), positives, keep, kind)`` through the fused batch tail: the batch is ``positives`` positives followed by the ``M`` pool
        candidates of each (the candidates of positive ``p`` at rows ``P + p M ..``: ``collate_fn``'s layout with M in place of k), the ``keep`` candidates of a pool that
        the model scores highest are the positive's negatives, and the loss is ``bce_loss``'s (``'bce'``: labels 1 / 0) or ``ranking_loss``'s (``'bpr'`` / ``'softmax'``)
        over the positive and those.  The pool rows are ordinary batch rows; the rows of the other candidates get zero row gradients.  ``kind=None`` reads
        ``Gs.Training.loss`` at every call.  ``return_selected``: also the ``[P, keep]`` pool positions of the negatives, best first (int64, detached).
        ``cotangent_sync``: as in ``bce_loss``."""
        from .. import ops
        kind = Gs.Training.loss if kind is None else kind
        objective = ops.hard_negative_objective(int(item_indices.shape[0]), positives, keep, kind)
        loss = self.training_loss(user_indices, query_indices, item_indices, objective, cotangent_sync=cotangent_sync)
        return (loss, objective.selected.to(torch.int64)) if return_selected else loss

    def training_loss(self, user_indices: Tensor, query_indices: Tensor, item_indices: Tensor, objective, labels: Optional[Tensor] = None, cotangent_sync=None) -> Tensor:
        """The training loss of a batch under ``objective`` (an ``ops.Objective``: the BCE over ``labels``, a ranking loss, or either over hard negatives - after which it
        holds ``selected``) through the fused batch tail: the shared body of ``bce_loss``, ``ranking_loss`` and ``hard_negative_loss``, and what the training loops call.
        ``cotangent_sync``: as in ``bce_loss``."""
        from .. import ops
        ds, head = self.dataset, self.prediction_layer
        cosine = bool(Gs.Prediction.use_cosine_similarity)       # read at every call, as the reference's head does (PredictionLayers.py:38)
        rows = ops.batch_node_rows(user_indices, query_indices, item_indices, ds.query_start_index_in_graph, ds.item_start_index_in_graph)
        if cotangent_sync is not None and torch.is_grad_enabled():
            holder = ops.TailGradients(exchange=cotangent_sync.exchange, grad_scale=1.0 / cotangent_sync.world_size)
            read_rows = cotangent_sync.gather_rows(rows)           # the union of the ranks' batch rows (users | queries | items), int64 with .as_int32
        else:
            holder = ops.TailGradients() if torch.is_grad_enabled() else None
            read_rows = rows
        compact = self._compact_layout()
        if compact is not None and holder is None:
            # (no gradient wanted: the public matrices, the plain tail)
            scores = ops.hem_score(self.propagate_layers(), rows, item_indices, head.items_bias, head.lambda_muq, ds.item_start_index_in_graph, cosine=cosine)
            if objective.grouped:
                return ops.objective_loss(scores, objective)
            # (the plain BCE of this route has always been torch's: an evaluation loss computed here keeps its bits only with this call, not with the HIP launch)
            return nn.functional.binary_cross_entropy_with_logits(scores, labels.float())
        if compact is not None:
            holder.row_map = compact.node_map
        layers = self.propagate_layers(holder, read_rows, self.batch_rows_only_last_layer)
        rows_upper = compact.compact_rows(rows) if compact is not None else None
        return ops.hem_loss(layers, rows, item_indices, objective, head.items_bias, head.lambda_muq, ds.item_start_index_in_graph, holder,
                            rows_upper=rows_upper, cosine=cosine, labels=labels)

    def supports_fused_loss(self, loss_function) -> bool:
        return (isinstance(loss_function, nn.BCEWithLogitsLoss) and loss_function.reduction == 'mean' and loss_function.weight is None
                and loss_function.pos_weight is None and self.supports_fused_tail())

    def supports_fused_tail(self) -> bool:
        """The fused batch tail (``bce_loss`` / ``ranking_loss``) runs on this model as it stands."""
        return self._saved_output_feature is None and len(self.gnns) + 1 <= 8 and next(self.parameters()).is_cuda

    def score_all_items(self, user_indices: Tensor, query_indices: Tensor) -> Tensor:
        """Scores of ``C`` (user, query) pairs against every item as a dense ``[C, I]`` matrix (torch; a checker for tests and
        notebooks - the evaluation loop uses ``top_items``, which never builds that matrix).

        Same arithmetic as ``forward(u * ones(I), q * ones(I), None)`` per pair (``RawGnn.py:124-137`` +
        ``PredictionLayers.py:35-43``), batched: ``(lam*F[q] + (1-lam)*F[u]) @ F_items^T + bias``; under ``Gs.Prediction.use_cosine_similarity`` both sides'
        rows are divided by ``max(norm, 1e-8)`` first (``torch.cosine_similarity``)."""
        features = self._saved_output_feature if self._saved_output_feature is not None else self.propagate()
        ds, head = self.dataset, self.prediction_layer
        item_feature = features[ds.item_start_index_in_graph:]
        lam = head.lambda_muq
        mixed = lam * features[query_indices + ds.query_start_index_in_graph] + (1 - lam) * features[user_indices]
        if Gs.Prediction.use_cosine_similarity:
            mixed = mixed / mixed.norm(dim=1, keepdim=True).clamp_min(1e-8)
            item_feature = item_feature / item_feature.norm(dim=1, keepdim=True).clamp_min(1e-8)
        return torch.addmm(head.items_bias.unsqueeze(0), mixed, item_feature.t())

    def top_items(self, user_indices: Tensor, query_indices: Tensor, k: int = 10, exclude=None, candidate_lists=None):
        """``(items [C, k] int32, scores [C, k])``: the ``k`` best items of each (user, query) pair over the whole catalogue, best
        first - what ``Metrics.calculate_on_all_items`` keeps of ``forward(u, q, None)`` (``Metrics.py:60-61``) - from the fused
        HIP scoring + running top-k kernel; the ``[C, I]`` scores are never stored.  Ties: ascending item id.  ``k`` up to ``ops.score_topk_max_k()`` = 128
        (beyond ten the kernel runs in passes, ``ops.score_topk_deep``; the reference itself stops at ten).  No torch path: any feature width
        ``d (L + 1)`` up to ``MAX_SCORED_WIDTH`` (checked at construction).  Scores with the head that ``Gs.Prediction.use_cosine_similarity`` names.
        ``exclude=(offsets [C + 1], items)``: pair ``c`` is ranked without ``items[offsets[c]:offsets[c + 1]]`` (any order, repeats allowed) - the scores of the
        other items are the same bits, and a row with fewer than ``k`` items left ends in ``-1``.
        ``candidate_lists=(offsets [C + 1], items)``: pair ``c`` is ranked among ``items[offsets[c]:offsets[c + 1]]`` only (any order, repeats allowed; int32 items
        are taken as ``ops.candidate_lists`` returned them) by the list kernels (``ops.search_candidates``): only the listed rows are read, and the scores are plain
        float32 sums, close to but not the bits of the whole-catalogue kernels'.  Composes with ``exclude``."""
        from .. import ops
        features = self._saved_output_feature if self._saved_output_feature is not None else self.propagate()
        ds = self.dataset
        if k > ops.score_topk_max_k():
            raise ValueError(f'RawGnn.top_items ranks at most {ops.score_topk_max_k()} items per pair, got k = {k}')
        k = min(k, ds.item_count)
        lists = None if exclude is None else ops.exclusion_lists(torch.as_tensor(exclude[0]), torch.as_tensor(exclude[1]), ds.item_count)
        shortlists = None if candidate_lists is None else (torch.as_tensor(candidate_lists[0]), torch.as_tensor(candidate_lists[1]))
        return self._ranked(features, user_indices, k, queries=query_indices, exclude=lists, shortlists=shortlists, as_search=False)[:2]

    def _ranked(self, features, users, k, *, queries=None, query_rows=None, candidates=None, exclude=None, exclude_rows=None, shortlists=None, return_scores=False,
                as_search=True):
        """The one place that picks the ranking call of ``top_items`` and ``search``: the list kernels with ``shortlists``, else the search entry points
        (``as_search``, or with exclusion lists), else ``ihg_score_topk`` - the evaluation path of ``top_items`` without lists.  Returns what the call returns."""
        from .. import ops
        ds, head = self.dataset, self.prediction_layer
        rows0, cosine = (ds.query_start_index_in_graph, ds.item_start_index_in_graph), Gs.Prediction.use_cosine_similarity
        if shortlists is not None:
            return ops.search_candidates(features, users, *rows0, head.items_bias, head.lambda_muq, k, lists=shortlists, queries=queries, query_rows=query_rows,
                                         candidates=candidates, exclude=exclude, exclude_rows=exclude_rows, cosine=cosine, return_scores=return_scores)
        if as_search or exclude is not None:
            return ops.search_topk(features, users, *rows0, head.items_bias, head.lambda_muq, k, queries=queries, query_rows=query_rows, candidates=candidates, cosine=cosine,
                                   exclude=exclude, exclude_rows=exclude_rows)
        return ops.score_topk(features, users, queries, *rows0, head.items_bias, head.lambda_muq, k, cosine=cosine)

    def _check_search_inputs(self, users, queries, words, offsets, candidates, exclude=None, exclude_seen=False, candidate_lists=None):
        """The host-side checks of ``search``, before anything is launched (a tensor that already lives on the device is taken as checked: reading it back would
        stall the stream the answer is waited on).  Returns ``(words, offsets)`` as int64 numpy arrays (``None, None`` with ``queries``)."""
        import numpy as np
        ds = self.dataset
        for layer in self.gnns:
            if getattr(getattr(layer, 'graph', None), 'self_loops', False):
                # (with a self connection an isolated node's layer output is its own transformed row, not zero: an unseen query has rows above layer 0)
                raise NotImplementedError('RawGnn.search scores an unseen query as an isolated node with zero layer outputs; a pairwise graph with self connections gives it others')

        def on_host(t):
            if t is None or (isinstance(t, Tensor) and t.is_cuda):
                return None
            return np.asarray(t.detach() if isinstance(t, Tensor) else t)

        if (queries is None) == (words is None):
            raise ValueError('RawGnn.search: give exactly one of queries= and words= (with offsets=)')
        if (words is None) != (offsets is None):
            raise ValueError('RawGnn.search: words= and offsets= go together')
        u = on_host(users)
        if u is not None and u.size and (u.min() < -1 or u.max() >= ds.user_count):
            raise ValueError(f'RawGnn.search: user outside [-1, {ds.user_count}) (-1: no user)')
        n_pairs = int(users.shape[0]) if hasattr(users, 'shape') else len(users)
        q = on_host(queries)
        if q is not None and q.size and (q.min() < 0 or q.max() >= ds.query_count):
            raise ValueError(f'RawGnn.search: query outside [0, {ds.query_count})')
        if queries is not None and (int(queries.shape[0]) if hasattr(queries, 'shape') else len(queries)) != n_pairs:
            raise ValueError('RawGnn.search: one query per user')
        c = on_host(candidates)
        if c is not None and c.dtype != np.bool_ and c.size and (c.min() < 0 or c.max() >= ds.item_count):
            raise ValueError(f'RawGnn.search: candidate item id outside [0, {ds.item_count})')
        if c is not None and c.dtype == np.bool_ and c.shape != (ds.item_count,):
            raise ValueError(f'RawGnn.search: a candidate mask is a bool tensor of [{ds.item_count}]')
        if exclude is not None and exclude_seen:
            raise ValueError('RawGnn.search: give exclude= or exclude_seen=True, not both')
        def check_lists(keyword, lists, which):
            """``keyword=(offsets [C + 1], items)``; ``which`` words the id message"""
            if not isinstance(lists, (tuple, list)) or len(lists) != 2:
                raise ValueError(f'RawGnn.search: {keyword}= is (offsets [C + 1], items)')
            o, i = on_host(lists[0]), on_host(lists[1])
            if o is not None and (o.ndim != 1 or o.size != n_pairs + 1):
                raise ValueError(f'RawGnn.search: {keyword}= needs {n_pairs + 1} offsets for {n_pairs} searches')
            if o is not None and i is not None and (o[0] != 0 or np.any(np.diff(o) < 0) or o[-1] != i.size):
                raise ValueError(f'RawGnn.search: the offsets of {keyword}= start at 0, do not decrease and end at the number of items')
            if i is not None and i.size and (i.min() < 0 or i.max() >= ds.item_count):
                raise ValueError(f'RawGnn.search: {which} item id outside [0, {ds.item_count})')

        if exclude is not None:
            check_lists('exclude', exclude, 'excluded')
        if candidate_lists is not None:
            check_lists('candidate_lists', candidate_lists, 'listed candidate')
        if words is None:
            return None, None
        w = np.asarray(words.detach().cpu() if isinstance(words, Tensor) else words, dtype=np.int64).reshape(-1)
        o = np.asarray(offsets.detach().cpu() if isinstance(offsets, Tensor) else offsets, dtype=np.int64).reshape(-1)
        if w.size and (w.min() < 0 or w.max() >= ds.vocab_size):
            raise ValueError(f'RawGnn.search: word id outside [0, {ds.vocab_size})')
        if o.size != n_pairs:
            raise ValueError(f'RawGnn.search: {o.size} bags for {n_pairs} users')
        if o.size and (o[0] != 0 or np.any(np.diff(o) < 0) or o[-1] > w.size):
            raise ValueError('RawGnn.search: offsets start at 0, do not decrease and stay within the words')
        return w, o

    @torch.no_grad()
    def search(self, users, *, queries=None, words=None, offsets=None, k: int = 10, candidates=None, exclude=None, exclude_seen: bool = False, candidate_lists=None,
               return_list_scores: bool = False):
        """``(items [C, k] int32, scores [C, k])``: ``top_items`` for a search as it arrives.  ``users`` int64 ``[C]``, ``-1`` = nobody logged in: the head's
        ``user_feature is None`` branch (``PredictionLayers.py:34-37``), the mixed row is the query row.  The query is EITHER ``queries`` (training query indices) OR
        ``words`` with ``offsets`` (flat 0-based word ids and the start of every bag, as for ``nn.EmbeddingBag``): a query the graph has not seen is an isolated node -
        its layer-0 row is ``EmbeddingLayer.embed_bags`` of its words, every layer output above is exactly zero (``Graph.py:120``) - scored as if appended to
        ``queries_multihot.txt`` with no interaction.  A bag that happens to equal a training query's words is still scored this way (its layer-0 row equals that
        query's, bit for bit; its upper rows are zero).  ``candidates``: a bool ``[I]`` mask or int64 item ids - only these are ranked; with fewer than ``k`` of them
        the rest of a row is ``-1``.  ``exclude=(offsets [C + 1], items)``: search ``c`` is answered without ``items[offsets[c]:offsets[c + 1]]`` (any order,
        repeats allowed), a different set per search where ``candidates`` is one for all.  ``exclude_seen=True``: every search of a logged-in user is answered
        without the items that user interacted with in training (``GraphDataset.user_item_lists``, one copy on the device shared by all searches; ``-1`` excludes
        nothing).  Both compose with everything else, and the scores of the items that remain do not change by a bit.
        ``candidate_lists=(offsets [C + 1], items)``: a different SHORTLIST per search - search ``c`` ranks ``items[offsets[c]:offsets[c + 1]]`` only (any order,
        repeats allowed; int32 items are taken as ``ops.candidate_lists`` returned them), what a first retrieval stage hands over for re-ranking.  The list kernels
        (``ops.search_candidates``) read only the listed item rows, so the cost is the lists' length, not the catalogue's; their scores are plain float32 sums,
        within a derived bound of the float64 score but NOT the bits of the whole-catalogue call.  Composes with ``queries`` / ``words``, ``-1`` users, ``candidates``,
        ``exclude`` / ``exclude_seen`` and both heads; a search ranks ``min(k, what its list, the mask and its exclusions leave)`` items, then ``-1``.  Without the
        keyword the call takes the whole-catalogue path and returns its bits.
        Features, head and ``k`` as in ``top_items``; no retraining, no new parameter, no ``[C, I]`` matrix."""
        from .. import ops
        w, o = self._check_search_inputs(users, queries, words, offsets, candidates, exclude, exclude_seen, candidate_lists)
        if return_list_scores and candidate_lists is None:
            raise ValueError('RawGnn.search: return_list_scores needs candidate_lists=')
        ds = self.dataset
        if k < 1 or k > ops.score_topk_max_k():
            raise ValueError(f'RawGnn.search ranks 1 to {ops.score_topk_max_k()} items per pair, got k = {k}')
        k = min(k, ds.item_count)
        features = self._saved_output_feature if self._saved_output_feature is not None else self.propagate()
        users = torch.as_tensor(users, dtype=torch.int64)
        query_rows = None
        if w is not None:
            query_rows = self.embeddings.embed_bags(w, o)
        else:
            queries = torch.as_tensor(queries, dtype=torch.int64)
        if candidates is not None and not isinstance(candidates, Tensor):
            candidates = torch.as_tensor(candidates)
        lists = rows = None
        if exclude_seen:
            lists, rows = ds.user_item_lists_on(features.device), users         # (a user IS the row of the shared lists; -1 names none)
        elif exclude is not None:
            lists = ops.exclusion_lists(torch.as_tensor(exclude[0]), torch.as_tensor(exclude[1]), ds.item_count)
        shortlists = None
        if candidate_lists is not None:
            shortlists = (torch.as_tensor(candidate_lists[0]), torch.as_tensor(candidate_lists[1]))
            if shortlists[1].dtype != torch.int32:
                shortlists = ops.candidate_lists(shortlists[0], shortlists[1], ds.item_count)
        out = self._ranked(features, users, k, queries=queries, query_rows=query_rows, candidates=candidates, exclude=lists, exclude_rows=rows, shortlists=shortlists,
                           return_scores=return_list_scores)
        if return_list_scores:
            return out[0], out[1], (shortlists[0], shortlists[1], out[3])
        return out[0], out[1]

    @torch.no_grad()
    def score_candidates(self, users, *, candidate_lists, queries=None, words=None, offsets=None):
        """``(ptr [C + 1], items int32, scores float32)``: the score of EVERY candidate of every search at its slot in the sorted lists (``ops.candidate_lists`` of
        ``candidate_lists=(offsets [C + 1], items)``: each run ascending, repeats removed) - for callers who blend the model's score with a first-stage score.  The
        launch is ``search``'s with ``candidate_lists=``; ``users`` / ``queries`` / ``words`` with ``offsets`` as there."""
        _, _, listed = self.search(users, queries=queries, words=words, offsets=offsets, k=1, candidate_lists=candidate_lists, return_list_scores=True)
        return listed

    def save_features_for_test(self) -> None:
        """Cache one propagation for the evaluation loop (call under ``torch.no_grad()``)."""
        self._saved_output_feature = self.propagate()

    def clear_saved_feature(self) -> None:
        self._saved_output_feature = None
