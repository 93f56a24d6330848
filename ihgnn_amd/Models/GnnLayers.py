"""Hypergraph layers (reference ``Models/GnnLayers.py:118-236``): ``IHGNNLayer`` and ``HGCNLayer``.

Constructor signatures, sub-module names (``feature_transform``, ``feature_interactor.aggregation``) and the
absence of any non-linearity follow the reference; the sparse work runs in the HIP kernels of
libihgnn_hip.so through :mod:`ihgnn_amd.ops` instead of ``torch_sparse.matmul``.
``GCNLayer`` (pairwise-graph baseline) runs on the same segment-sum kernel over a weighted CSR; ``GATLayer`` (the attention
baseline) adds the score and softmax kernels of csrc/gat.hip in front of it, and ``IHGNNLayer(phase2_attention=True)`` those of csrc/phase2.hip
(the same attention over the node <- hyperedge incidence).
"""
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from .. import ops
from ..Helpers.GlobalSettings import Gsv
from .CommonLayers import FeatureInteractor


def _transform(linear: nn.Linear, x: Tensor, layout) -> Tensor:
    """``nn.Linear`` (square) on every node row through the HIP node-level kernels (split-arithmetic / MFMA row-GEMM for d in {32,64,128,256},
    the any-width kernels otherwise).  There is no torch path: a rectangular transform - which RawGnn never builds
    (``RawGnn.py:59-91``: input and output dimension are both the embedding size) - is refused."""
    if linear.in_features != linear.out_features:
        raise NotImplementedError(f'feature_transform {linear.in_features} -> {linear.out_features}: the MI355X path has square node-level transforms only '
                                  '(RawGnn builds every layer with input_dimension == output_dimension)')
    wide = _row_width(x)
    if wide != linear.in_features:
        # features zero-padded to the next tiled width (RawGnn at a width between 32 / 64 / 128 / 256, ops.padded_width): the weight as the top-left block of a zero matrix
        return ops.node_linear(x, ops.pad_square(linear.weight, wide), ops.pad_vector(linear.bias, wide), layout)
    return ops.node_linear(x, linear.weight, linear.bias, layout)


def _row_width(x) -> int:
    return int(x.shape[1])


def _check_rows(x, layout) -> None:
    """A layer's input has one row per node of ITS layout - which, for a hypergraph whose isolated nodes the layout leaves out (``IncidenceLayout.compact``), is not the
    public node count: ``RawGnn`` translates (``RawGnn._compact_layout``); a direct caller must pass ``x[layout.active_nodes]``."""
    if int(x.shape[0]) != layout.node_count:
        raise ValueError(f'layer input has {int(x.shape[0])} rows, the hypergraph layout {layout.node_count} nodes'
                         + (f' (the layout leaves out the {layout.public_node_count - layout.node_count} isolated nodes of the graph: pass x[layout.active_nodes], or build the '
                            'dataset under IHG_COMPACT_NODES=0)' if getattr(layout, 'compact', False) else ''))


class HGCNLayer(nn.Module):
    """``Y = Dv^-1/2 H De^-1 H^T Dv^-1/2 (X W^T + b)``  (``GnnLayers.py:142-153``)."""

    def __init__(self, device: torch.device, dataset, input_dimension: int, output_dimension: int):
        super().__init__()
        self.device = device
        self.dataset = dataset
        from ..layout import LogHyperLayout
        graph = dataset.graph if getattr(dataset, 'graph_type', None) is not None else dataset.hypergraph      # GnnLayers.py:131
        self.layout = graph.layout
        self.general = isinstance(self.layout, LogHyperLayout)  # per-search-log hyperedges of variable arity (PpsLogHyperGraph)
        if not self.general:
            self.edge_scale = float(torch.tensor(3.0).pow(-1))      # De^-1 of a 3-uniform hypergraph, as fp32
            self.out_scale = self.layout.inv_sqrt_deg_times(self.edge_scale)      # (one vector per layout, shared by its layers)
        self.feature_transform = nn.Linear(input_dimension, output_dimension)

    def reads_cotangent_rows_only(self) -> bool:
        """With ``output_rows`` / ``cotangent_rows`` the backward reads its cotangent at those rows only (``ops.node_two_hop``'s masked pull)."""
        return not self.general

    def forward(self, input_features: Tensor, output_rows: Optional[Tensor] = None, cotangent_rows: Optional[Tensor] = None,
                out: Optional[Tensor] = None) -> Tensor:
        """``out`` (inference only): the ``[N, d]`` destination, e.g. a column slice of the ``[N, d (L + 1)]`` feature matrix.
        ``output_rows`` (int32 node rows, not in the reference signature): the caller reads only these rows of the result
        (last layer of a training step); other rows may be left unwritten.  ``cotangent_rows``: every row is computed, but the caller
        promises that the gradient of the result is zero outside these rows (``ops.node_two_hop``)."""
        lay = self.layout
        _check_rows(input_features, lay)
        if self.general:
            # general incidence: node -> hyperedge (x Dv^-1/2 in, De^-1 out), hyperedge -> node (x Dv^-1/2 out): two K7 launches
            h = _transform(self.feature_transform, input_features, lay)
            edge_features = ops.hyper_node_to_edge(h, lay, src_scale=lay.inv_sqrt_deg, out_scale=lay.inv_edge_degree)
            return ops.hyper_edge_to_node(edge_features, lay, out_scale=lay.inv_sqrt_deg, out=out)
        h = _transform(self.feature_transform, input_features, lay)
        # node -> hyperedge -> node in one two-hop pass over the node table: Dv^-1/2 on the way in, Dv^-1/2 De^-1 on the way out
        return ops.node_two_hop(h, lay, in_scale=lay.inv_sqrt_deg, out_scale=self.out_scale, rows=output_rows, cotangent_rows=cotangent_rows, out=out)


class IHGNNLayer(nn.Module):
    """``Y = Dv^-1 H Interact(X W^T + b)``  (``GnnLayers.py:221-236``); with ``phase2_attention`` the mean over a node's hyperedges gives way to attention
    weights: ``Y[v] = sum over e containing v of alpha(e, v) Ef'[e]`` (``GnnLayers.py:200-216, 227-230``, :class:`_Phase2Attention`)."""

    def __init__(self, device: torch.device, dataset, input_dimension: int, output_dimension: int,
                 feature_interaction_order: int, phase2_attention: bool):
        super().__init__()
        if feature_interaction_order not in (1, 2, 3):
            raise AssertionError('feature interaction order must be 1, 2 or 3')
        self.device = device
        self.dataset = dataset
        self.feature_interaction_order = feature_interaction_order
        self.attention_phase2 = bool(phase2_attention)
        self.layout = dataset.hypergraph.layout
        # construction order as in the reference (interactor, fake_gat, feature_transform): a seeded layer draws its weights
        self.feature_interactor = FeatureInteractor(dataset=dataset, max_order=feature_interaction_order,
                                                    node_feature_dimension=input_dimension,
                                                    output_dimension=input_dimension)
        if self.attention_phase2:
            self.fake_gat = _Phase2Attention(output_dimension)
        self.feature_transform = nn.Linear(input_dimension, output_dimension)

    def reads_cotangent_rows_only(self) -> bool:
        """First-order layers run the two-hop operator, whose backward under ``output_rows`` / ``cotangent_rows`` is the masked pull; the attention's backward
        reads every row of its cotangent."""
        return self.feature_interaction_order == 1 and not self.attention_phase2

    def forward(self, input_features: Tensor, output_rows: Optional[Tensor] = None, cotangent_rows: Optional[Tensor] = None,
                out: Optional[Tensor] = None) -> Tensor:
        """``output_rows`` / ``cotangent_rows`` / ``out``: as in ``HGCNLayer.forward`` (with ``phase2_attention`` every row is computed: ``output_rows`` only
        permits leaving the others unwritten)."""
        _check_rows(input_features, self.layout)
        if self.attention_phase2:
            # the hyperedge rows exist here ([E, d]): both row sets go through fake_gat's transform, then the attention - one autograd node behind the transform
            h = _transform(self.feature_transform, input_features, self.layout)
            return self.fake_gat(h, self.feature_interactor, self.layout, out=out)
        if self.feature_interaction_order == 1:
            # first-order layer: hoisted node-level blocks, then node -> hyperedge -> node fused into one two-hop pass
            return ops.node_two_hop(self._first_order_of_input(input_features), self.layout, out_scale=self.layout.inv_deg, rows=output_rows,
                                    cotangent_rows=cotangent_rows, out=out)
        h = _transform(self.feature_transform, input_features, self.layout)
        return self.feature_interactor.to_nodes(h, out_scale=self.layout.inv_deg, rows=output_rows, out=out)

    def _first_order_of_input(self, x: Tensor) -> Tensor:
        """``first_order(feature_transform(x))``.  With no non-linearity between them (``GnnLayers.py:224-227`` +
        ``CommonLayers.py:60-66``) the two linear maps of a first-order layer compose: node type t sees
        ``x (A_t W)^T + (A_t b + [t = user] c)``, one typed row-GEMM over ``[N, d]`` instead of two (and one instead of two in
        each backward direction); the ``[d, d]`` products are formed per call by a tiny kernel (``ihg_compose_first_order_fwd``).  Same reassociation class as the hoisting itself:
        <= 5e-7 relative against the reference's order of operations."""
        lin, agg = self.feature_transform, self.feature_interactor.aggregation
        if lin.bias is None:
            return self.feature_interactor.first_order(_transform(lin, x, self.layout))
        wide = _row_width(x)                                 # (> in_features: zero-padded features, ops.padded_width)
        weight, bias = ops.compose_first_order(ops.pad_blocks(agg.weight, wide), ops.pad_vector(agg.bias, wide), ops.pad_square(lin.weight, wide),
                                               ops.pad_vector(lin.bias, wide))      # [d, 3 d]: A_t W side by side; [3, d]
        return ops.node_linear(x, weight, bias, self.layout, typed=True, bias_mask=0b111)


class GCNLayer(nn.Module):
    """``Y = D^-1/2 A D^-1/2 (X W^T + b)`` over the pairwise graph (``GnnLayers.py:9-45``).

    The reference orders transform and propagation by which side is narrower (``GnnLayers.py:33-43``); RawGnn builds square layers
    (transform first).  Propagation is the weighted-CSR form of the K7 kernel with both ``D^-1/2`` scalings fused in."""

    def __init__(self, device: torch.device, dataset, input_dimension: int, output_dimension: int):
        super().__init__()
        self.device = device
        self.dataset = dataset
        self.input_dimension = input_dimension
        self.output_dimension = output_dimension
        self.graph = dataset.graph2d.layout
        self.feature_transform = nn.Linear(input_dimension, output_dimension)

    def forward(self, input_features: Tensor, out: Optional[Tensor] = None) -> Tensor:
        # the reference transforms first when the output is not wider (GnnLayers.py:33-43); RawGnn's layers are square, so that is the only order here
        return ops.pair_spmm(_transform(self.feature_transform, input_features, self.graph), self.graph, out=out)


_GAT_ACTIVATIONS = {'leaky_relu': nn.LeakyReLU, 'relu': nn.ReLU, 'tanh': nn.Tanh}


def _attention_settings(who: str):
    """``(head, activation class, activation name)`` from ``Gs.Gnn``, refused unless the kernels have them."""
    from ..Helpers.GlobalSettings import Gs
    head = Gs.Gnn.gat_head
    act_type, act_name = Gs.Gnn.gat_activation
    if head not in (Gsv.concat, Gsv.product):
        raise ValueError(f'{who}: unknown head {head!r} (Gsv.concat or Gsv.product)')
    if _GAT_ACTIVATIONS.get(act_name) is not act_type:
        raise ValueError(f'{who}: activation {act_name!r} / {act_type} is not one of {sorted(_GAT_ACTIVATIONS)} with its nn class')
    return head, act_type, act_name


def _feature_aggregate(dimension: int, head: str, act_type, act_name: str) -> nn.Sequential:
    """``feature_aggregate`` of ``GATLayer.__init__`` (``GnnLayers.py:65-84``): Linear to one score, its weight re-drawn by ``xavier_uniform_`` with the activation's gain."""
    linear = nn.Linear(2 * dimension if head == Gsv.concat else dimension, 1)
    nn.init.xavier_uniform_(linear.weight, gain=nn.init.calculate_gain(act_name))
    return nn.Sequential(linear, act_type())


def _attention_weight(w: Tensor, d: int, head: str, wide: int) -> Tensor:
    """``feature_aggregate.0.weight`` as the kernel's vector at the width the features run at: each half of a concatenation weight zero-padded on its own."""
    if wide == d:
        return w
    if head == Gsv.concat:
        return ops.pad_columns(w.view(2, d), wide).reshape(1, 2 * wide)
    return ops.pad_vector(w, wide)


class _Phase2Attention(nn.Module):
    """``IHGNNLayer.fake_gat``: the reference builds a ``GATLayer`` over a "fake" graph of ``N + E`` vertices whose edges run hyperedge -> member node
    (``GnnLayers.py:200-216``) and feeds it ``cat([h, Ef])``.  Same parameters and state-dict keys (``feature_aggregate.0.*``, ``feature_transform.*``) drawn in the same
    order; the forward keeps the two row sets apart: ``feature_transform`` - the SAME Linear - on each, then the attention of csrc/phase2.hip + K7 over the
    layout's node-major CSR (``ops.phase2_layer``: interactor, transform and ``ops.hyper_attention``'s kernels as one autograd node).  No ``[N + E, d]`` concatenation, no ``[3 E, 2, d]`` rows.  Kept: ``Ef`` and ``Ef'``, ``2 E d`` floats per layer."""

    def __init__(self, dimension: int):
        super().__init__()
        self.dimension = dimension
        self.head, act_type, self.activation = _attention_settings('IHGNNLayer(phase2_attention=True)')
        self.feature_aggregate = _feature_aggregate(dimension, self.head, act_type, self.activation)
        self.feature_transform = nn.Linear(dimension, dimension)

    def forward(self, node_features: Tensor, interactor: FeatureInteractor, layout, out: Optional[Tensor] = None) -> Tensor:
        """``node_features``: the layer's ``feature_transform(x)``; ``interactor``: the layer's, whose hyperedge rows are formed inside the op."""
        wide = _row_width(node_features)
        lin, agg = self.feature_transform, self.feature_aggregate[0]
        agg_w, agg_b = interactor._operands(node_features)
        return ops.phase2_layer(node_features, agg_w, agg_b, ops.pad_square(lin.weight, wide), ops.pad_vector(lin.bias, wide),
                                _attention_weight(agg.weight, self.dimension, self.head, wide), agg.bias, layout, interactor.max_order, self.head, self.activation, out=out)


class GATLayer(nn.Module):
    """Single-head attention over the pairwise graph (``GnnLayers.py:48-115``): ``h = X W^T + b``, for every edge ``u -> v`` a score
    ``act(w . [h_u | h_v] + c)`` (head ``Gs.Gnn.gat_head`` = concatenation) or ``act(w . (h_u * h_v) + c)`` (product), a softmax over ``v``'s incoming
    edges, ``Y[v] = sum alpha h_u``.

    Construction order, initialisation and state-dict keys follow the reference (``feature_aggregate`` = Linear + activation, its weight re-drawn by
    ``xavier_uniform_`` with the activation's gain, then ``feature_transform``), so a seeded model draws the reference's weights.  The attention runs in
    ``ops.gat_attention`` (csrc/gat.hip + K7) over the graph's symmetric CSR; no ``[nnz, 2, d]`` rows are formed."""

    def __init__(self, device: torch.device, dataset, input_dimension: int, output_dimension: int):
        super().__init__()
        self.device = device
        self.dataset = dataset
        self.input_dimension = input_dimension
        self.output_dimension = output_dimension
        self.graph = dataset.graph2d.layout
        self.head, act_type, self.activation = _attention_settings('GATLayer')
        self.feature_aggregate = _feature_aggregate(output_dimension, self.head, act_type, self.activation)
        self.feature_transform = nn.Linear(input_dimension, output_dimension)

    def _attention_weight(self, wide: int) -> Tensor:
        """``feature_aggregate.0.weight`` as the kernel's vector at the width the features run at: each half of a concatenation weight zero-padded on its own."""
        return _attention_weight(self.feature_aggregate[0].weight, self.output_dimension, self.head, wide)

    def forward(self, input_features, out: Optional[Tensor] = None) -> Tensor:
        """``input_features``: ``[N, d]`` (or ``ops.NodeTables``); ``out`` (inference only): the ``[N, d]`` destination, e.g. a column slice of the feature matrix."""
        h = _transform(self.feature_transform, input_features, self.graph)
        return ops.gat_attention(h, self.graph, self._attention_weight(_row_width(h)), self.feature_aggregate[0].bias, self.head, self.activation, out=out)
