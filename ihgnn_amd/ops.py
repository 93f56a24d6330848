"""Differentiable operators of the hypergraph path, each a thin ``torch.autograd.Function`` over the C ABI.

PyTorch is plumbing here (device memory, current stream, autograd tape); every forward and backward below
is one or two launches of a hand-written gfx950 kernel in libihgnn_hip.so.  Tensors must live on the GPU:
there is no CPU implementation to fall back to.

Operator               forward kernel              backward kernel(s)
---------------------  --------------------------  ------------------------------------------------
edge_gather_sum  (K5)  ihg_edge_gather_sum         ihg_node_segment_sum   (its transpose)
node_segment_sum (K7)  ihg_node_segment_sum         ihg_edge_gather_sum    (its transpose)
bag_mean         (K2)  ihg_bag_mean_fwd            ihg_bag_mean_bwd
 + query transform     ihg_rows_linear_act_fwd     ihg_rows_linear_act_bwd  (in front of ihg_bag_mean_bwd)
 or the GRU encoder    ihg_gru_fwd                 ihg_gru_bwd              (instead of the bag mean: QueryTransform('gru', ...))
interact     (K5+K6)   ihg_interact_fwd            ihg_interact_bwd + 4x ihg_node_segment_sum
gat_attention          ihg_gat_attention_fwd + K7  ihg_gat_scores_bwd, K7, ihg_gat_finish_bwd
hyper_attention        ihg_phase2_attention_fwd    ihg_phase2_scores_bwd, ihg_phase2_edges_bwd, (K7,) ihg_phase2_finish_bwd
                       + K7
cat_linear (Srrl)      ihg_cat_linear_fwd          ihg_cat_linear_bwd (+ ihg_batch_combine / ihg_batch_rows_add for a gathered source)
rows_dot (Srrl)        ihg_rows_dot_fwd            ihg_rows_dot_bwd
kg_loss (Srrl)         ihg_kg_loss                 (its gradients come from the forward launch)
"""
from __future__ import annotations

import ctypes
import os as _os
from typing import Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from . import profiler
from .layout import Csr, CsrRows, IncidenceLayout

_void = ctypes.c_void_p


def _ptr(t: Optional[Tensor]):
    return None if t is None else _void(t.data_ptr())


def _stream():
    return _void(torch.cuda.current_stream().cuda_stream)


def _rows(t: Tensor, name: str) -> Tensor:
    """A 2-D fp32 GPU tensor whose rows are contiguous (any row stride); copies only if it must."""
    if not t.is_cuda:
        raise _lib.IhgnnHipError(f'{name} must be a GPU tensor: ihgnn_amd has no CPU path (got device {t.device})')
    if t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError(f'{name} must be a 2-D float32 tensor, got {tuple(t.shape)} {t.dtype}')
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _ld(t: Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _workspace(n_bytes: int, device: torch.device) -> Tensor:
    """Scratch for one launch (torch's caching allocator hands back the same block step after step)."""
    return torch.empty(max(n_bytes, 16) // 4, dtype=torch.float32, device=device)


def _plan_args(csr: Union[Csr, CsrRows], seg_row: bool = False):
    """The split-row plan of ``csr`` in the order every entry point takes it - threshold, ``seg_begin``, ``seg_end``, (``seg_row``: the attention calls only,) segment
    count, ``heavy_rows``, ``heavy_segptr``, row count; without split rows: zeros and nulls."""
    if csr.n_heavy == 0:
        return (0, None, None) + ((None,) if seg_row else ()) + (0, None, None, 0)
    return ((csr.heavy_threshold, _ptr(csr.seg_begin), _ptr(csr.seg_end)) + ((_ptr(csr.seg_row),) if seg_row else ())
            + (csr.n_segments, _ptr(csr.heavy_rows), _ptr(csr.heavy_segptr), csr.n_heavy))


# ---------------------------------------------------------------------------------------------
# raw launches (no autograd)
# ---------------------------------------------------------------------------------------------
def edge_gather_sum_raw(src: Tensor, i3: Tensor, node_scale: Optional[Tensor] = None, bias: Optional[Tensor] = None,
                        alpha: float = 1.0, out: Optional[Tensor] = None, edge_scale: Optional[Tensor] = None) -> Tensor:
    """``edge_scale`` (``[E]``): every hyperedge's sum times its own factor - ``layout.edge_weight`` where the result is the cotangent of all copies of a hyperedge."""
    lib = _lib.load()
    src = _rows(src, 'src')
    n_edges, dim = int(i3.shape[0]), int(src.shape[1])
    if out is None:
        out = torch.empty(n_edges, dim, dtype=torch.float32, device=src.device)
    with profiler.kernel('edge_gather_sum', n_edges, dim):
        _lib.check(lib.ihg_edge_gather_sum(_ptr(src), _ld(src), _ptr(i3), _ptr(node_scale), _ptr(bias), float(alpha), _ptr(edge_scale),
                                           _ptr(out), _ld(out), n_edges, dim, _stream()), 'ihg_edge_gather_sum')
    return out


def node_segment_sum_raw(src: Tensor, csr: Union[Csr, CsrRows], src_scale: Optional[Tensor] = None,
                         out_scale: Optional[Tensor] = None, mode: int = _lib.SCALE_NONE,
                         out: Optional[Tensor] = None, entry_scale: Optional[Tensor] = None,
                         self_weight: Optional[Tensor] = None, rows: Optional[Tensor] = None, src_mask: Optional[Tensor] = None,
                         role: Optional[str] = None, accumulate: bool = False, read_once: bool = False, src_scale_in_entries: bool = False,
                         role_names_rows: bool = True) -> Tensor:
    """``role`` names the launch for the profiler (one kernel, several jobs with different byte counts: ``bench.py`` reports each).
    ``rows`` (int32, device): only these output rows are needed.  The split rows of the plan are always computed; of the
    others only the listed ones are, and the rest of ``out`` is left unwritten.  ``src_mask`` (uint8 per source row): rows with a 0
    are all-zero and are not fetched.  ``accumulate``: ``out +=`` instead of ``out =`` (``out`` required; the hyperedge chunks of one scatter; with ``rows``: the listed rows and the plan's split rows).
    ``read_once``: every source row is read exactly once by this launch (non-temporal loads).  ``src_scale_in_entries``: ``entry_scale[p]`` already holds
    ``src_scale[ids[p]]`` (times the entry's weight; ``IncidenceLayout.two_hop_source_weights``) - the gather does not fetch ``src_scale`` per id, the row's own
    term still takes it.  ``role_names_rows=False``: the launch keeps its role's name with a row list (otherwise ``<role>_rows``)."""
    lib = _lib.load()
    src = _rows(src, 'src')
    dim = int(src.shape[1])
    if accumulate:
        if out is None:
            raise ValueError('accumulate needs an existing `out`')
        mode = mode | _lib.SCALE_ACCUMULATE
    if read_once:
        mode = mode | _lib.SRC_READ_ONCE
    if src_scale_in_entries:
        mode = mode | _lib.SRC_SCALE_IN_ENTRIES
    if out is None:
        out = torch.empty(csr.n_rows, dim, dtype=torch.float32, device=src.device)
    if rows is not None and rows.dtype != torch.int32:
        raise TypeError('rows must be an int32 tensor')
    order, n_light = (rows, int(rows.shape[0])) if rows is not None else (csr.row_order, csr.n_rows)
    with profiler.kernel((role or 'node_segment_sum') + ('' if rows is None or not role_names_rows else '_rows'), n_light, dim):
        _lib.check(lib.ihg_node_segment_sum(
            _ptr(src), _ld(src), _ptr(csr.ptr), _ptr(csr.ids), _ptr(order), _ptr(src_scale), _ptr(entry_scale), _ptr(out_scale), mode,
            _ptr(out), _ld(out), n_light, dim, *_plan_args(csr), _ptr(csr.partials(dim)) if csr.n_heavy > 0 else None,
            _ptr(self_weight), _ptr(src_mask), _stream()), 'ihg_node_segment_sum')
    return out


def node_pair_sums_raw(h: Tensor, layout: IncidenceLayout, out: Optional[Tensor] = None) -> Tensor:
    """``[N, 3 d]``: per node the sums over its incident hyperedges' OTHER two members ``(a, b)`` of ``h[a]``, ``h[b]`` and ``h[a] * h[b]``
    (``ihg_node_pair_sums`` over ``layout.hop2_csr``) - the gather half of the interactive layer's node-level form."""
    lib = _lib.load()
    h = _rows(h, 'h')
    dim = int(h.shape[1])
    csr = layout.hop2_csr
    if out is None:
        out = torch.empty(layout.node_count, 3 * dim, dtype=torch.float32, device=h.device)
    with profiler.kernel('node_pair_sums', layout.node_count, dim):
        _lib.check(lib.ihg_node_pair_sums(
            _ptr(h), _ld(h), _ptr(csr.ptr), _ptr(csr.ids), _ptr(csr.row_order), _ptr(out), _ld(out), csr.n_rows, dim,
            *_plan_args(csr), _ptr(csr.partials(3 * dim)) if csr.n_heavy > 0 else None, _ptr(layout.pair_weight), _stream()), 'ihg_node_pair_sums')
    return out


def _check_out(out: Optional[Tensor], *inputs: Tensor) -> Optional[Tensor]:
    """``out=``: a caller-owned ``[rows, d]`` destination (any row stride - a column slice of the ``[N, d (L + 1)]`` feature matrix,
    ``RawGnn.propagate``).  Only outside autograd: a recorded op must own its output."""
    if out is not None and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in inputs):
        raise ValueError('out= is for inference (torch.no_grad()): a differentiable op allocates its own output')
    return out


# ---------------------------------------------------------------------------------------------
# K5 / K7 as a transposed pair
# ---------------------------------------------------------------------------------------------
class _EdgeGatherSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src: Tensor, layout: IncidenceLayout, node_scale: Optional[Tensor], alpha: float) -> Tensor:
        ctx.layout, ctx.node_scale, ctx.alpha = layout, node_scale, alpha
        return edge_gather_sum_raw(src, layout.i3, node_scale, None, alpha)

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        scale = ctx.node_scale
        if ctx.alpha != 1.0:
            scale = (scale * ctx.alpha) if scale is not None else torch.full(
                (ctx.layout.node_count,), ctx.alpha, dtype=torch.float32, device=grad_out.device)
        mode = _lib.SCALE_NONE if scale is None else _lib.SCALE_MULTIPLY
        # (grad_out is the cotangent of the layout's rows - one per DISTINCT hyperedge under edge_weight -: each row is added once, whatever its multiplicity)
        return node_segment_sum_raw(grad_out, ctx.layout.node_csr, None, scale, mode, role='k7.edges_to_nodes_bwd_of_k5'), None, None, None


def _edges_to_nodes(src: Tensor, layout: IncidenceLayout, out_scale: Optional[Tensor], rows: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """K7's hyperedge -> node pass ``out_scale * H src`` over ``layout.node_csr``."""
    mode = _lib.SCALE_NONE if out_scale is None else _lib.SCALE_MULTIPLY
    # layout.edge_weight (duplicate triples collapsed): a row stands for m_e hyperedges of the reference's incidence and enters the sum m_e times
    return node_segment_sum_raw(src, layout.node_csr, layout.edge_weight, out_scale, mode, rows=rows, role='k7.edges_to_nodes', out=out)


class _NodeSegmentSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src: Tensor, layout: IncidenceLayout, out_scale: Optional[Tensor], rows: Optional[Tensor], out: Optional[Tensor]) -> Tensor:
        ctx.layout, ctx.out_scale = layout, out_scale
        return _edges_to_nodes(src, layout, out_scale, rows, _check_out(out, src))

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        return edge_gather_sum_raw(grad_out, ctx.layout.i3, ctx.out_scale, None, 1.0, edge_scale=ctx.layout.edge_weight), None, None, None, None


def edge_gather_sum(src: Tensor, layout: IncidenceLayout, node_scale: Optional[Tensor] = None, alpha: float = 1.0) -> Tensor:
    """node -> hyperedge: ``out[e] = alpha * sum_{v in e} node_scale[v] * src[v]``  (``[N,d] -> [E,d]``)."""
    return _EdgeGatherSum.apply(src, layout, node_scale, float(alpha))


def node_segment_sum(src: Tensor, layout: IncidenceLayout, out_scale: Optional[Tensor] = None, rows: Optional[Tensor] = None,
                     out: Optional[Tensor] = None) -> Tensor:
    """hyperedge -> node: ``out[v] = out_scale[v] * sum_{e containing v} src[e]``  (``[E,d] -> [N,d]``; over ALL hyperedges of the reference's incidence: a layout
    that keeps a repeated triple once weights its row by the multiplicity).

    ``rows`` (int32): the caller reads only these rows of the result (the batch rows of the last layer's output in a training
    step); rows outside the list and outside the split-row plan are left UNWRITTEN.  The gradient must then be zero outside
    ``rows`` too - which it is when only those rows were read."""
    return _NodeSegmentSum.apply(src, layout, out_scale, rows, out)


# The first-order layers' gather launches walk the two-hop list either as it is (two ids per incidence) or with the repeated (destination, source) entries of a row merged
# into one weighted entry (layout.two_hop_merged).  The LAYOUT decides (IncidenceLayout.two_hop_merged_default: merged when >= 25 % of the entries are repeats, or when it
# carries hyperedge multiplicities): measured in round 5 on the C2 - C4 stand-ins, 8.6 - 17.9 % fewer gathers bought NOT A MICROSECOND (the repeats were cache hits:
# profiles/r5/01_ab_two_hop_merged.txt) - at C5 79 % of the entries are repeats, its 10 GB node table is far beyond the caches, and the three launches go from 22.5 / 14.4 /
# 23.9 ms to 13.0 / 6.4 / 12.8 (profiles/r6/01_ab_two_hop_C5_*.json: 326.8 -> 297.7 ms per step).  IHG_TWO_HOP_MERGED=1 / 0 (or this attribute: True / False) overrides.
_two_hop_env = _os.environ.get('IHG_TWO_HOP_MERGED', 'auto')
TWO_HOP_MERGED = {'1': True, '0': False}.get(_two_hop_env)          # None: per layout


def two_hop_merged_for(layout: IncidenceLayout) -> bool:
    """Whether this layout's first-order launches walk the merged (weighted) two-hop list."""
    if layout.edge_weight is not None:
        return True                                           # (its plain list has one entry per DISTINCT hyperedge: not the operator without the weights)
    return layout.two_hop_merged_default if TWO_HOP_MERGED is None else bool(TWO_HOP_MERGED)


def _two_hop_list(layout: IncidenceLayout):
    """``(csr, entry weights or None)`` of the two-hop operator's off-diagonal part ``H H^T - diag(deg)``."""
    if two_hop_merged_for(layout):
        csr, weights, _ = layout.two_hop_merged()
        return csr, weights
    return layout.hop2_csr, None


# A two-hop launch with a per-source scale (the backward of a first-order layer: the two diagonal scalings swapped; HGCN's forward) gathered src_scale[id] for every
# id of the list - a divergent 4-byte load per entry, and one more dependent round trip in front of the row loads (ids -> scale -> rows): 772 / 767 us against the
# unscaled forward's 700 at C3.  The scale vectors are graph data, so the layout keeps scale[ids[p]] (x the merged list's weight) per ENTRY and the launch reads it beside
# the id.  Lists whose weights would take more than SOURCE_WEIGHTS_MAX_BYTES keep the per-id gather: 128 MiB covers C3 (13.2 M entries, 53 MB) and C4 (19.8 M, 79 MB);
# C5's merged list is past it and stays as it was.  IHG_K7_SOURCE_WEIGHTS=0 (or this attribute) turns it off: same bits either way.
SOURCE_WEIGHTS_MAX_BYTES = 128 << 20
SOURCE_WEIGHTS = _os.environ.get('IHG_K7_SOURCE_WEIGHTS', '1') != '0'


def two_hop_scaled_list(layout: IncidenceLayout, src_scale: Optional[Tensor]):
    """``(csr, entry weights or None, src_scale_in_entries)`` for a two-hop launch that scales its source rows by ``src_scale``."""
    csr, weights = _two_hop_list(layout)
    if src_scale is None or not SOURCE_WEIGHTS:
        return csr, weights, False
    merged = weights is not None
    if src_scale.is_cuda and torch.cuda.is_current_stream_capturing() and not layout.has_two_hop_source_weights(src_scale, merged):
        return csr, weights, False                            # (a capture without its warm-up steps: the build is no part of the recorded step)
    folded = layout.two_hop_source_weights(src_scale, merged, SOURCE_WEIGHTS_MAX_BYTES)
    if folded is None:
        return csr, weights, False
    return csr, folded, True


def _two_hop_first_order_gradient(dy: Tensor, layout: IncidenceLayout, out_scale: Optional[Tensor], rows: Optional[Tensor] = None,
                                  out: Optional[Tensor] = None) -> Tensor:
    """``d P = H H^T (out_scale * dy)``: the first-order blocks' gradient of the interactive layer by the two-hop operator on the node-level cotangent
    (``rows`` / ``out``: only these rows, and the plan's split rows, into an existing ``[N, d]``)."""
    csr, weights, folded = two_hop_scaled_list(layout, out_scale)
    return node_segment_sum_raw(dy, csr, out_scale, None, _lib.SCALE_NONE, entry_scale=weights, self_weight=layout.self_weight, role='k7.two_hop_first_order_gradient',
                                src_scale_in_entries=folded, rows=rows, out=out, role_names_rows=False)


class _TwoHop(torch.autograd.Function):
    """``out = Do * (H H^T) (Di * x)``: node -> hyperedge -> node in ONE pass over the node table (no ``[E,d]`` round trip).

    ``H H^T`` is symmetric, so the backward is the same launch with the two diagonal scalings swapped."""

    @staticmethod
    def forward(ctx, x: Tensor, layout: IncidenceLayout, in_scale: Optional[Tensor], out_scale: Optional[Tensor], rows: Optional[Tensor],
                cotangent_rows: Optional[Tensor], out: Optional[Tensor]) -> Tensor:
        ctx.layout, ctx.in_scale, ctx.out_scale = layout, in_scale, out_scale
        # rows outside which the cotangent is zero: the rows that were computed at all, or the caller's explicit promise
        ctx.cot_rows = rows if rows is not None else (cotangent_rows if SPARSE_LAST_COTANGENT else None)
        mode = _lib.SCALE_NONE if out_scale is None else _lib.SCALE_MULTIPLY
        csr, weights, folded = two_hop_scaled_list(layout, in_scale)
        return node_segment_sum_raw(x, csr, in_scale, out_scale, mode, entry_scale=weights, self_weight=layout.self_weight, rows=rows, role='k7.two_hop',
                                    out=_check_out(out, x), src_scale_in_entries=folded)

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        lay = ctx.layout
        mode = _lib.SCALE_NONE if ctx.in_scale is None else _lib.SCALE_MULTIPLY
        mask = None
        if ctx.cot_rows is not None:
            # grad_out is zero outside these rows: the pull skips the gathers of the zero rows (two thirds of them - every neighbour that
            # is not a query - and the ones that would miss the cache); same gradient as the dense pull.  The byte-per-row mask is the layout's, all zero
            # between uses: the listed rows are set here and cleared after the pull (two launches over 3 B ids instead of a fill of N bytes + an index fill)
            lib = _lib.load()
            mask = lay.row_mask()
            rows = ctx.cot_rows
            r64, r32 = (_ptr(rows), None) if rows.dtype == torch.int64 else (None, _ptr(rows))
            _lib.check(lib.ihg_mark_rows(r64, r32, int(rows.shape[0]), _ptr(mask), 1, _stream()), 'ihg_mark_rows')
            if CHECK_SPARSE_COTANGENT and bool((grad_out[mask == 0] != 0).any()):
                _lib.check(lib.ihg_mark_rows(r64, r32, int(rows.shape[0]), _ptr(mask), 0, _stream()), 'ihg_mark_rows')
                raise RuntimeError('node_two_hop: the cotangent is not zero outside cotangent_rows / rows - the output has a consumer the caller did not declare')
        try:
            # (the masked pull keeps the per-id gather: it fetches the scale of the LISTED ids only, a per cent or two of the list, while the per-entry weights
            # are a stream over every entry - measured at C3: 149 us by id, 169 with the weights)
            csr, weights, folded = two_hop_scaled_list(lay, ctx.out_scale if mask is None else None)
            out = node_segment_sum_raw(grad_out, csr, ctx.out_scale, ctx.in_scale, mode, entry_scale=weights, self_weight=lay.self_weight, src_mask=mask,
                                       role='k7.two_hop_bwd' if mask is None else 'k7.two_hop_bwd_masked', src_scale_in_entries=folded)
            if mask is not None:
                _lib.check(lib.ihg_mark_rows(r64, r32, int(rows.shape[0]), _ptr(mask), 0, _stream()), 'ihg_mark_rows')
        except BaseException:
            # the mask belongs to the layout and must be all zero between uses: a pull that raised leaves it so (a stale bit would make the next
            # masked pull gather rows of a cotangent buffer that only has its batch rows written)
            if mask is not None:
                lay.drop_row_mask()
            raise
        return out, None, None, None, None, None, None


def node_two_hop(x: Tensor, layout: IncidenceLayout, in_scale: Optional[Tensor] = None, out_scale: Optional[Tensor] = None,
                 rows: Optional[Tensor] = None, cotangent_rows: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``out[v] = out_scale[v] * sum_{e containing v} sum_{w in e} in_scale[w] * x[w]`` - the first-order
    node -> hyperedge -> node step (K5 followed by K7) without materialising the hyperedge features.  ``rows``: as in
    ``node_segment_sum``.  ``cotangent_rows`` (int32 / int64 node rows): the caller's PROMISE that the gradient with respect to the
    output is zero outside these rows - true of the last layer of a training step, whose output is read at the batch rows only - so
    the backward pulls just them.  The promise is carried by the op itself (not looked up by address); ``IHG_CHECK_SPARSE_COTANGENT=1``
    verifies it at every backward.  ``IHG_SPARSE_LAST_COTANGENT=0`` ignores it (dense pull, same gradient)."""
    return _TwoHop.apply(x, layout, in_scale, out_scale, rows, cotangent_rows, out)


class _PairSpmm(torch.autograd.Function):
    """``out = Ds (A (Ds x))`` for a symmetric weighted adjacency: its own transpose, so backward is the same launch."""

    @staticmethod
    def forward(ctx, x: Tensor, graph, out: Optional[Tensor]) -> Tensor:
        ctx.graph = graph
        return node_segment_sum_raw(x, graph.csr, graph.inv_sqrt_deg, graph.inv_sqrt_deg, _lib.SCALE_MULTIPLY, entry_scale=graph.values, role='k7.pair_graph',
                                    out=_check_out(out, x))

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        g = ctx.graph
        return node_segment_sum_raw(grad_out, g.csr, g.inv_sqrt_deg, g.inv_sqrt_deg, _lib.SCALE_MULTIPLY, entry_scale=g.values, role='k7.pair_graph'), None, None


class _CsrSpmm(torch.autograd.Function):
    """``out = Do (A (Ds x))`` for a sparse ``A`` given as CSR over its rows together with the CSR of its transpose: the backward
    is the same launch over the transpose with the two scalings swapped."""

    @staticmethod
    def forward(ctx, x: Tensor, csr, csr_t, values, values_t, src_scale, out_scale, role: str, out: Optional[Tensor]) -> Tensor:
        ctx.args = (csr, csr_t, values, values_t, src_scale, out_scale, role)
        mode = _lib.SCALE_NONE if out_scale is None else _lib.SCALE_MULTIPLY
        return node_segment_sum_raw(x, csr, src_scale, out_scale, mode, entry_scale=values, role=role, out=_check_out(out, x))

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        csr, csr_t, values, values_t, src_scale, out_scale, role = ctx.args
        mode = _lib.SCALE_NONE if src_scale is None else _lib.SCALE_MULTIPLY
        return (node_segment_sum_raw(grad_out, csr_t, out_scale, src_scale, mode, entry_scale=values_t, role=role + '_bwd'),) + (None,) * 8


def hyper_node_to_edge(x: Tensor, layout, src_scale: Optional[Tensor] = None, out_scale: Optional[Tensor] = None) -> Tensor:
    """node -> hyperedge over a general (variable-arity) incidence: ``out[e] = out_scale[e] * sum_{v in e} val(v,e) src_scale[v] x[v]``
    (``thsp.matmul(incidence_t, .)``, ``GnnLayers.py:148``) - ``layout`` is a :class:`ihgnn_amd.layout.LogHyperLayout`."""
    return _CsrSpmm.apply(x, layout.edge_csr, layout.node_csr, layout.edge_values, layout.node_values, src_scale, out_scale, 'k7.hyper_node_to_edge', None)


def hyper_edge_to_node(x: Tensor, layout, src_scale: Optional[Tensor] = None, out_scale: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """hyperedge -> node over a general incidence: ``out[v] = out_scale[v] * sum_{e containing v} val(v,e) src_scale[e] x[e]``
    (``thsp.matmul(incidence, .)``, ``GnnLayers.py:151``)."""
    return _CsrSpmm.apply(x, layout.node_csr, layout.edge_csr, layout.node_values, layout.edge_values, src_scale, out_scale, 'k7.hyper_edge_to_node', out)


def pair_spmm(x: Tensor, graph, out: Optional[Tensor] = None) -> Tensor:
    """GCN propagation ``D^-1/2 A D^-1/2 x`` over a :class:`ihgnn_amd.layout.PairLayout` (``GnnLayers.py:35-38``)."""
    return _PairSpmm.apply(x, graph, out)


# ---------------------------------------------------------------------------------------------
# GAT attention over the pairwise graph (csrc/gat.hip + K7)
# ---------------------------------------------------------------------------------------------
GAT_HEADS = {'concatenation': 0, 'product': 1}                  # Gsv.concat / Gsv.product -> IHG_GAT_CONCAT / IHG_GAT_PRODUCT
GAT_ACTIVATIONS = {'leaky_relu': 0, 'relu': 1, 'tanh': 2}       # the names of Gs.Gnn.gat_activation -> IHG_GAT_*


def _split_row_args(csr: Csr):
    """The plan arguments of the attention entry points: their kernels read ``seg_row`` too."""
    return _plan_args(csr, seg_row=True)
_gat_plan = _split_row_args                                     # (its earlier name: the attention tests of earlier revisions call it, and run on this build)


def _attention_codes(caller: str, head: str, activation: str):
    for kind, name, codes in (('head', head, GAT_HEADS), ('activation', activation, GAT_ACTIVATIONS)):
        if name not in codes:
            raise ValueError(f'{caller}: unknown {kind} {name!r} (one of {sorted(codes)})')
    return GAT_HEADS[head], GAT_ACTIVATIONS[activation]


def _check_attention_operands(caller: str, weight: Tensor, bias: Tensor, head: int, dim: int) -> None:
    if int(weight.numel()) != (2 * dim if head == 0 else dim) or int(bias.numel()) != 1:
        raise ValueError(f'{caller}: weight of {int(weight.numel())} / bias of {int(bias.numel())} floats for width {dim}')


class _GatAttention(torch.autograd.Function):
    """``out[v] = sum over v's incoming edges u -> v of softmax_v(act(score(u, v))) h[u]`` (``GnnLayers.py:98-115``): scores and softmax in
    ``ihg_gat_attention_fwd``, the weighted sum in K7; backward: ``ihg_gat_scores_bwd``, K7 over the cotangent with the mirrored weights (and, product head,
    over ``h`` with ``ds + ds[mirror]``), ``ihg_gat_finish_bwd``."""

    @staticmethod
    def forward(ctx, h: Tensor, weight: Tensor, bias: Tensor, graph, head: int, activation: int, out: Optional[Tensor]) -> Tensor:
        lib = _lib.load()
        h = _rows(h, 'h')
        csr = graph.csr
        n, dim = int(h.shape[0]), int(h.shape[1])
        if n != graph.node_count:
            raise ValueError(f'gat_attention: h has {n} rows, the graph {graph.node_count} nodes')
        weight, bias = weight.contiguous(), bias.contiguous()
        _check_attention_operands('gat_attention', weight, bias, head, dim)
        nnz = csr.nnz
        z = torch.empty(max(nnz, 1), dtype=torch.float32, device=h.device)
        alpha = torch.empty_like(z)
        alpha_mirror = torch.empty_like(z)
        ws_bytes = int(lib.ihg_gat_workspace_bytes(n, csr.n_segments, dim, head))
        ws = _workspace(ws_bytes, h.device)
        with profiler.kernel('gat_scores', n, dim):
            _lib.check(lib.ihg_gat_attention_fwd(_ptr(h), _ld(h), _ptr(csr.ptr), _ptr(csr.ids), _ptr(graph.mirror), _ptr(csr.row_order), n, dim, _ptr(weight),
                                                 _ptr(bias), head, activation, *_split_row_args(csr), _ptr(z), _ptr(alpha), _ptr(alpha_mirror), _ptr(ws), ws_bytes,
                                                 _stream()), 'ihg_gat_attention_fwd')
        y = node_segment_sum_raw(h, csr, None, None, _lib.SCALE_NONE, entry_scale=alpha, role='k7.gat_aggregate', out=_check_out(out, h, weight, bias))
        ctx.graph, ctx.head, ctx.activation = graph, head, activation
        ctx.save_for_backward(h, weight, bias, z, alpha, alpha_mirror)
        return y

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        lib = _lib.load()
        h, weight, bias, z, alpha, alpha_mirror = ctx.saved_tensors
        graph, head = ctx.graph, ctx.head
        csr = graph.csr
        dy = _rows(grad_out, 'grad_out')
        n, dim = int(h.shape[0]), int(h.shape[1])
        ds = torch.empty_like(z)
        node_sums = torch.empty(n, 2, dtype=torch.float32, device=h.device)
        ws_bytes = int(lib.ihg_gat_workspace_bytes(n, csr.n_segments, dim, head))
        ws = _workspace(ws_bytes, h.device)
        with profiler.kernel('gat_scores_bwd', n, dim):
            _lib.check(lib.ihg_gat_scores_bwd(_ptr(h), _ld(h), _ptr(dy), _ld(dy), _ptr(csr.ptr), _ptr(csr.ids), _ptr(graph.mirror), _ptr(csr.row_order), n, dim,
                                              head, ctx.activation, *_split_row_args(csr), _ptr(z), _ptr(alpha), _ptr(ds), _ptr(node_sums), _ptr(ws), ws_bytes,
                                              _stream()), 'ihg_gat_scores_bwd')
        # the transposed aggregation: row u gathers the cotangents of the rows its edges u -> v point to, weighted by alpha of u -> v
        dh = node_segment_sum_raw(dy, csr, None, None, _lib.SCALE_NONE, entry_scale=alpha_mirror, role='k7.gat_aggregate_bwd')
        b = None
        if head == GAT_HEADS['product']:
            sym = torch.empty_like(z)
            with profiler.kernel('gat_symmetrize', csr.nnz, 1):
                _lib.check(lib.ihg_gat_symmetrize(_ptr(ds), _ptr(graph.mirror), csr.nnz, _ptr(sym), _stream()), 'ihg_gat_symmetrize')
            b = node_segment_sum_raw(h, csr, None, None, _lib.SCALE_NONE, entry_scale=sym, role='k7.gat_score_bwd')
        dweight = torch.empty_like(weight)
        dbias = torch.empty_like(bias)
        with profiler.kernel('gat_finish_bwd', n, dim):
            _lib.check(lib.ihg_gat_finish_bwd(_ptr(h), _ld(h), _ptr(b), _ld(b) if b is not None else 0, _ptr(node_sums), _ptr(weight), head, n, dim, _ptr(dh),
                                              _ld(dh), _ptr(dweight), _ptr(dbias), _ptr(ws), ws_bytes, _stream()), 'ihg_gat_finish_bwd')
        return dh, dweight, dbias, None, None, None, None


def gat_attention(h: Tensor, graph, weight: Tensor, bias: Tensor, head: str = 'concatenation', activation: str = 'leaky_relu',
                  out: Optional[Tensor] = None) -> Tensor:
    """The attention half of ``GATLayer.forward`` (``GnnLayers.py:100-115``) over a :class:`ihgnn_amd.layout.PairLayout`: for every edge ``u -> v`` (entry ``u``
    of CSR row ``v``) ``z = act(w_src . h[u] + w_dst . h[v] + c)`` (``head`` 'concatenation', ``weight`` = ``[w_src | w_dst]``, ``2 d`` floats) or
    ``act(w . (h[u] * h[v]) + c)`` ('product', ``d`` floats); ``alpha`` = softmax of ``z`` over ``v``'s incoming edges; ``out[v] = sum alpha h[u]`` (a node
    without edges: a zero row).  ``activation``: 'leaky_relu' (slope 0.01), 'relu' or 'tanh'.  ``bias``: the one-float ``c`` (read on the device)."""
    return _GatAttention.apply(h, weight.reshape(-1), bias.reshape(-1), graph, *_attention_codes('gat_attention', head, activation), out)


# ---------------------------------------------------------------------------------------------
# Phase-2 attention of IHGNNLayer over the node <- hyperedge incidence (csrc/phase2.hip + K7)
# ---------------------------------------------------------------------------------------------
def _phase2_forward_raw(h2: Tensor, ef2: Tensor, weight: Tensor, bias: Tensor, layout: IncidenceLayout, head: int, activation: int, out: Optional[Tensor]):
    """``(y, z, alpha, alpha_edge)``: scores and softmax (``ihg_phase2_attention_fwd``), then K7 over ``ef2`` with ``entry_scale = alpha``."""
    lib = _lib.load()
    csr = layout.node_csr
    n, e, dim = int(h2.shape[0]), int(ef2.shape[0]), int(h2.shape[1])
    if n != layout.node_count or e != layout.edge_count or int(ef2.shape[1]) != dim:
        raise ValueError(f'hyper_attention: h2 {tuple(h2.shape)} / ef2 {tuple(ef2.shape)} for a layout of {layout.node_count} nodes and {layout.edge_count} hyperedges')
    _check_attention_operands('hyper_attention', weight, bias, head, dim)
    z = torch.empty(max(3 * e, 1), dtype=torch.float32, device=h2.device)
    alpha = torch.empty_like(z)
    alpha_edge = torch.empty_like(z)
    ws_bytes = int(lib.ihg_phase2_workspace_bytes(n, e, csr.n_segments, dim, head))
    ws = _workspace(ws_bytes, h2.device)
    with profiler.kernel('phase2_scores', n, dim):
        _lib.check(lib.ihg_phase2_attention_fwd(_ptr(h2), _ld(h2), _ptr(ef2), _ld(ef2), _ptr(csr.ptr), _ptr(csr.ids), _ptr(layout.member_csr.ids), _ptr(csr.row_order),
                                                n, e, dim, _ptr(weight), _ptr(bias), _ptr(layout.edge_weight), head, activation, *_split_row_args(csr), _ptr(z), _ptr(alpha),
                                                _ptr(alpha_edge), _ptr(ws), ws_bytes, _stream()), 'ihg_phase2_attention_fwd')
    # (alpha carries the multiplicity of a hyperedge kept once: no src_scale)
    y = node_segment_sum_raw(ef2, csr, None, None, _lib.SCALE_NONE, entry_scale=alpha, role='k7.phase2_aggregate', out=out)
    return y, z, alpha, alpha_edge


def _phase2_backward_raw(h2: Tensor, ef2: Tensor, weight: Tensor, z: Tensor, alpha: Tensor, alpha_edge: Tensor, dy: Tensor, layout: IncidenceLayout,
                         head: int, activation: int):
    """``(d h2, d ef2, d weight, d bias)`` from ``dy``: ``ihg_phase2_scores_bwd``, the edge-major ``ihg_phase2_edges_bwd`` for the hyperedge rows (product head: K7 over
    ``ef2`` with ``ds`` for the node rows), ``ihg_phase2_finish_bwd``."""
    lib = _lib.load()
    csr = layout.node_csr
    n, e, dim = int(h2.shape[0]), int(ef2.shape[0]), int(h2.shape[1])
    ds = torch.empty_like(z)
    ds_edge = torch.empty_like(z)
    node_sums = torch.empty(n, 2, dtype=torch.float32, device=h2.device)
    ws_bytes = int(lib.ihg_phase2_workspace_bytes(n, e, csr.n_segments, dim, head))
    ws = _workspace(ws_bytes, h2.device)
    with profiler.kernel('phase2_scores_bwd', n, dim):
        _lib.check(lib.ihg_phase2_scores_bwd(_ptr(ef2), _ld(ef2), _ptr(dy), _ld(dy), _ptr(csr.ptr), _ptr(csr.ids), _ptr(layout.member_csr.ids), _ptr(csr.row_order),
                                             n, e, dim, head, activation, *_split_row_args(csr), _ptr(z), _ptr(alpha), _ptr(ds), _ptr(ds_edge), _ptr(node_sums),
                                             _ptr(ws), ws_bytes, _stream()), 'ihg_phase2_scores_bwd')
    def2 = torch.empty(e, dim, dtype=torch.float32, device=h2.device)
    with profiler.kernel('phase2_edges_bwd', e, dim):
        _lib.check(lib.ihg_phase2_edges_bwd(_ptr(dy), _ld(dy), _ptr(h2), _ld(h2), _ptr(layout.i3), _ptr(alpha_edge), _ptr(ds_edge), _ptr(weight), head, e, dim,
                                            _ptr(def2), _ld(def2), _stream()), 'ihg_phase2_edges_bwd')
    b = None
    if head == GAT_HEADS['product']:
        b = node_segment_sum_raw(ef2, csr, None, None, _lib.SCALE_NONE, entry_scale=ds, role='k7.phase2_score_bwd')
    dh2 = torch.empty(n, dim, dtype=torch.float32, device=h2.device)
    dweight = torch.empty_like(weight)
    dbias = torch.empty(1, dtype=torch.float32, device=h2.device)
    with profiler.kernel('phase2_finish_bwd', n, dim):
        _lib.check(lib.ihg_phase2_finish_bwd(_ptr(h2), _ld(h2), _ptr(ef2), _ld(ef2), _ptr(b), _ld(b) if b is not None else 0, _ptr(node_sums), _ptr(ds_edge),
                                             _ptr(weight), head, n, e, dim, _ptr(dh2), _ld(dh2), _ptr(dweight), _ptr(dbias), _ptr(ws), ws_bytes, _stream()),
                   'ihg_phase2_finish_bwd')
    return dh2, def2, dweight, dbias


class _HyperAttention(torch.autograd.Function):
    """``out[v] = sum over v's hyperedges e of softmax_v(act(score(e, v))) ef2[e]`` (``GnnLayers.py:227-230`` through ``GATLayer.forward``); saved: ``z``, ``alpha``,
    ``alpha_edge`` (and the operands)."""

    @staticmethod
    def forward(ctx, h2: Tensor, ef2: Tensor, weight: Tensor, bias: Tensor, layout: IncidenceLayout, head: int, activation: int, out: Optional[Tensor]) -> Tensor:
        h2, ef2 = _rows(h2, 'h2'), _rows(ef2, 'ef2')
        weight, bias = weight.contiguous(), bias.contiguous()
        y, z, alpha, alpha_edge = _phase2_forward_raw(h2, ef2, weight, bias, layout, head, activation, _check_out(out, h2, ef2, weight, bias))
        ctx.layout, ctx.head, ctx.activation = layout, head, activation
        ctx.save_for_backward(h2, ef2, weight, z, alpha, alpha_edge)
        return y

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        h2, ef2, weight, z, alpha, alpha_edge = ctx.saved_tensors
        dh2, def2, dweight, dbias = _phase2_backward_raw(h2, ef2, weight, z, alpha, alpha_edge, _rows(grad_out, 'grad_out'), ctx.layout, ctx.head, ctx.activation)
        return dh2, def2, dweight, dbias, None, None, None, None


def _plain_type_begin(n_rows: int):
    """Type boundaries of a table whose rows have no node types: every row is of the first type."""
    return (ctypes.c_int64 * 4)(0, n_rows, n_rows, n_rows)


def _node_linear_fwd(x: Tensor, w: Tensor, w_type_stride: int, bias: Optional[Tensor], bias_mask: int, type_begin, out: Optional[Tensor] = None) -> Tensor:
    """``out[v] = x[v] @ W_type(v).T (+ bias)`` (``ihg_node_linear_fwd``).  ``w_type_stride``: ``d`` - node type t uses the column block t of ``w`` -, or 0: one weight for
    every row.  ``bias`` is ``[d]`` or one vector per type, ``[3, d]``, added to the types in ``bias_mask``."""
    lib = _lib.load()
    dim = int(x.shape[1])
    if out is None:
        out = torch.empty(x.shape[0], dim, dtype=torch.float32, device=x.device)
    ws = _workspace(int(lib.ihg_node_linear_workspace_bytes(dim)), x.device)
    with profiler.kernel('node_linear_fwd', x.shape[0], dim):
        _lib.check(lib.ihg_node_linear_fwd(_ptr(x), _ld(x), _ptr(w), int(w.stride(0)), w_type_stride, _ptr(bias), bias_mask, dim if bias is not None and bias.dim() == 2 else 0,
                                           type_begin, _ptr(out), _ld(out), _ptr(ws), ws.numel() * 4, dim, _stream()), 'ihg_node_linear_fwd')
    return out


def _bias_gradient(has_bias: bool, per_type_bias: bool, dim: int, device: torch.device) -> Optional[Tensor]:
    return torch.empty((3, dim) if per_type_bias else (dim,), dtype=torch.float32, device=device) if has_bias else None


def _node_linear_bwd(g: Tensor, x: Tensor, w: Tensor, w_type_stride: int, type_begin, dw: Tensor, dx: Optional[Tensor], dx_accumulate: bool, has_bias: bool,
                     per_type_bias: bool, bias_mask: int) -> Optional[Tensor]:
    """The gradients of ``_node_linear_fwd`` from ``g`` in one call (``ihg_node_linear_bwd_weight``): the weight gradient into ``dw``, the input gradient into ``dx`` (``None``:
    not wanted; ``dx_accumulate``: added onto what ``dx`` holds) from the same pass over ``g`` where the width allows.  Returns the bias gradient (``None`` without a bias)."""
    lib = _lib.load()
    dim = int(x.shape[1])
    dbias = _bias_gradient(has_bias, per_type_bias, dim, x.device)
    ws = _workspace(int(lib.ihg_node_linear_workspace_bytes(dim)), x.device)
    with profiler.kernel('node_linear_bwd', x.shape[0], dim):
        _lib.check(lib.ihg_node_linear_bwd_weight(_ptr(g), _ld(g), _ptr(x), _ld(x), type_begin, _ptr(dw), int(dw.stride(0)), w_type_stride, _ptr(dbias), bias_mask,
                                                  dim if per_type_bias else 0, _ptr(w), int(w.stride(0)), _ptr(dx), _ld(dx) if dx is not None else 0, 1 if dx_accumulate else 0,
                                                  _ptr(ws), ws.numel() * 4, dim, _stream()), 'ihg_node_linear_bwd_weight')
    return dbias


def _linear_rows(x: Tensor, w: Tensor, bias: Optional[Tensor], type_begin) -> Tensor:
    """``x @ w.T + bias`` on every row (one weight for all rows)."""
    return _node_linear_fwd(x, w, 0, bias, 0b111, type_begin)


def _linear_rows_backward(g: Tensor, x: Tensor, w: Tensor, type_begin, has_bias: bool):
    """``(d x, d w, d bias)`` of ``_linear_rows`` from ``g``."""
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    return dx, dw, _node_linear_bwd(g, x, w, 0, type_begin, dw, dx, False, has_bias, False, 0b111)


def _add_rows(dst: Tensor, src: Tensor) -> None:
    """``dst += src`` over ``[rows, d]`` (``ihg_phase2_add_rows``)."""
    _lib.check(_lib.load().ihg_phase2_add_rows(_ptr(dst), _ld(dst), _ptr(src), _ld(src), int(dst.shape[0]), int(dst.shape[1]), _stream()), 'ihg_phase2_add_rows')


class _Phase2Layer(torch.autograd.Function):
    """The whole IHGNN layer with phase-2 attention behind ``feature_transform`` as ONE autograd node (``CommonLayers.py:58-87`` + ``GnnLayers.py:227-230``): hoisted
    first-order blocks -> hyperedge rows ``ef`` (K5 at order 1, ``ihg_interact_fwd`` above) -> ``fake_gat.feature_transform`` on the node rows and on the hyperedge
    rows -> attention.  Backward: the attention's, the transform's on both row sets, the interactor's; the gradients that two of these passes share (the
    transform's parameters, the node features) are added by the library (``ihg_phase2_add_rows`` / the row GEMM's accumulating epilogue), so a step launches
    library kernels only.  Kept for the backward: ``ef`` and ``ef2`` (``2 E d`` floats), ``h2``, ``z`` / ``alpha`` / ``alpha_edge`` (``9 E`` floats)."""

    @staticmethod
    def forward(ctx, h: Tensor, agg_w: Tensor, agg_b: Optional[Tensor], wg: Tensor, bg: Tensor, weight: Tensor, bias: Tensor, layout: IncidenceLayout, order: int,
                head: int, activation: int, out: Optional[Tensor]) -> Tensor:
        h, agg_w, wg = _rows(h, 'h'), _rows(agg_w, 'aggregation weight'), _rows(wg, 'transform weight')
        weight, bias, bg = weight.contiguous(), bias.contiguous(), bg.contiguous()
        _check_out(out, h, agg_w, agg_b, wg, bg, weight, bias)
        p = _first_order_rows(h, agg_w, agg_b, layout)
        ef = edge_gather_sum_raw(p, layout.i3) if order == 1 else _interact_rows(h, p, agg_w, layout, order)
        del p
        h2 = _linear_rows(h, wg, bg, _type_begin(layout))
        ef2 = _linear_rows(ef, wg, bg, _plain_type_begin(layout.edge_count))
        y, z, alpha, alpha_edge = _phase2_forward_raw(h2, ef2, weight, bias, layout, head, activation, out)
        ctx.layout, ctx.order, ctx.head, ctx.activation, ctx.has_bias = layout, order, head, activation, agg_b is not None
        ctx.save_for_backward(h, agg_w, wg, weight, ef, h2, ef2, z, alpha, alpha_edge)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        h, agg_w, wg, weight, ef, h2, ef2, z, alpha, alpha_edge = ctx.saved_tensors
        layout, order = ctx.layout, ctx.order
        dh2, def2, dweight, dbias = _phase2_backward_raw(h2, ef2, weight, z, alpha, alpha_edge, _rows(dy, 'dy'), layout, ctx.head, ctx.activation)
        # fake_gat.feature_transform, hyperedge rows: def is the cotangent of the layout's rows (a row kept once: already the sum over its copies)
        d_ef, dwg, dbg = _linear_rows_backward(def2, ef, wg, _plain_type_begin(layout.edge_count), True)
        del def2
        dagg_w = torch.empty_like(agg_w)                       # product blocks from the interact kernels, first-order blocks from the row-GEMM pass
        if order == 1:
            dh = None
            dp = node_segment_sum_raw(d_ef, layout.node_csr, role='k7.edges_to_nodes_bwd_of_k5')
        else:
            dp = node_segment_sum_raw(d_ef, layout.node_csr, role='k7.first_order_gradient')
            dh = _interact_backward(h, agg_w, d_ef, layout, order, dagg_w)
        del d_ef
        # ... node rows
        dh_nodes, dwg_nodes, dbg_nodes = _linear_rows_backward(dh2, h, wg, _type_begin(layout), True)
        if dh is None:
            dh = dh_nodes
        else:
            _add_rows(dh, dh_nodes)
        _add_rows(dwg, dwg_nodes)
        _add_rows(dbg.view(1, -1), dbg_nodes.view(1, -1))
        dagg_b = _first_order_backward(dp, h, agg_w, layout, dagg_w, dh, ctx.has_bias)
        return dh, dagg_w, dagg_b, dwg, dbg, dweight, dbias, None, None, None, None, None


def phase2_layer(h: Tensor, agg_w: Tensor, agg_b: Optional[Tensor], wg: Tensor, bg: Tensor, weight: Tensor, bias: Tensor, layout: IncidenceLayout, order: int,
                 head: str = 'concatenation', activation: str = 'leaky_relu', out: Optional[Tensor] = None) -> Tensor:
    """``hyper_attention(rows_linear(h; wg, bg), rows_linear(FeatureInteractor(h; agg_w, agg_b); wg, bg), ...)`` as one differentiable op: what
    ``IHGNNLayer(phase2_attention=True)`` runs behind its ``feature_transform``.  All operands at the width of ``h`` (``pad_blocks`` / ``pad_square`` / ...)."""
    codes = _attention_codes('phase2_layer', head, activation)
    if order not in (1, 2, 3):
        raise ValueError('phase2_layer: interaction order 1, 2 or 3')
    return _Phase2Layer.apply(h, agg_w, agg_b, wg, bg, weight.reshape(-1), bias.reshape(-1), layout, int(order), *codes, out)


def hyper_attention(h2: Tensor, ef2: Tensor, layout: IncidenceLayout, weight: Tensor, bias: Tensor, head: str = 'concatenation', activation: str = 'leaky_relu',
                    out: Optional[Tensor] = None) -> Tensor:
    """The attention half of ``IHGNNLayer.forward`` with ``phase2_attention`` (``GnnLayers.py:227-230`` through ``GATLayer.forward``, lines 100-115) over an
    :class:`ihgnn_amd.layout.IncidenceLayout`: ``h2 [N, d]`` and ``ef2 [E, d]`` are the node and hyperedge features after ``fake_gat.feature_transform``; for every
    incidence (``e`` contains ``v``) ``z = act(w_src . ef2[e] + w_dst . h2[v] + c)`` (``head`` 'concatenation', ``weight`` = ``[w_src | w_dst]``: the hyperedge is the
    edge's source) or ``act(w . (ef2[e] * h2[v]) + c)`` ('product'); ``alpha`` = softmax of ``z`` over ``v``'s hyperedges - every copy of a hyperedge that the layout
    keeps once (``layout.edge_weight``) counted; ``out[v] = sum alpha ef2[e]`` (a node in no hyperedge: a zero row).  ``activation`` / ``bias``: as ``gat_attention``."""
    return _HyperAttention.apply(h2, ef2, weight.reshape(-1), bias.reshape(-1), layout, *_attention_codes('hyper_attention', head, activation), out)


# ---------------------------------------------------------------------------------------------
# K2 query embedding bag (mean)
# ---------------------------------------------------------------------------------------------
class BagLayout:
    """Query -> word-row lists (``nn.EmbeddingBag`` input/offsets of Dataset.py:161-186) and their transpose."""

    def __init__(self, bag_input, bag_offsets, table_rows: int, device: torch.device):
        import numpy as np
        words = np.ascontiguousarray(np.asarray(bag_input, dtype=np.int64).reshape(-1))
        offsets = np.asarray(bag_offsets, dtype=np.int64).reshape(-1)
        if words.size and (words.min() < 0 or words.max() >= table_rows):
            raise ValueError('bag word id outside the embedding table')
        ptr = np.append(offsets, words.shape[0]).astype(np.int32)
        self.n_bags, self.table_rows = int(offsets.shape[0]), int(table_rows)
        self.bags = Csr(ptr, words.astype(np.int32), device, heavy_threshold=0)
        self.words_of = self.bags.transpose(table_rows)
        if words.size == 0:
            # no query has a word: every row of both lists is empty and no id is ever read, but the library refuses a null id list - one id that nobody reads
            self.bags.ids = self.words_of.ids = torch.zeros(1, dtype=torch.int32, device=device)
        lens = np.diff(ptr.astype(np.int64)).astype(np.float32)
        self.bag_len = torch.from_numpy(lens).to(device)
        # for the recurrent encoder (ihg_gru_fwd / ihg_gru_bwd): the bags by decreasing length, ties in bag order (None: they already are) - a workgroup takes 32
        # neighbours of that order and runs to the longest of them -, and every word's positions in `words`, ascending: word w's are
        # word_positions[words_of.ptr[w] : words_of.ptr[w + 1]] (the per-occurrence gradients are summed over them in that order)
        self.n_words = int(words.shape[0])
        by_length = np.argsort(-lens, kind='stable').astype(np.int32)
        self.length_order = None if np.array_equal(by_length, np.arange(self.n_bags, dtype=np.int32)) else torch.from_numpy(by_length).to(device)
        positions = np.argsort(words, kind='stable').astype(np.int32)
        self.word_positions = torch.from_numpy(positions if positions.size else np.zeros(1, np.int32)).to(device)
        inv = np.where(lens > 0, 1.0 / np.maximum(lens, 1), 0).astype(np.float32)
        self.inv_len = torch.from_numpy(inv).to(device)


QUERY_ACTIVATIONS = {'relu': 1, 'tanh': 2}                          # the names of Gs.Query.transform_activation -> IHG_ACT_RELU / IHG_ACT_TANH


def _query_activation(name: Optional[str]) -> int:
    if name not in QUERY_ACTIVATIONS:
        raise ValueError(f'query transform: unknown activation {name!r} (one of {sorted(QUERY_ACTIVATIONS)})')
    return QUERY_ACTIVATIONS[name]


def _query_transform_operands(wq: Optional[Tensor], bq: Optional[Tensor], dim: int):
    """``(W_q, b_q)`` of the query transform as the library takes them (``None, None``: the plain bag mean)."""
    if wq is None:
        return None, None
    if bq is None or tuple(wq.shape) != (dim, dim) or tuple(bq.shape) != (dim,):
        raise ValueError(f'the query transform is a [{dim}, {dim}] weight with a [{dim}] bias, got {tuple(wq.shape)} and {None if bq is None else tuple(bq.shape)}')
    return _rows(wq, 'query transform weight'), bq.contiguous()


class QueryTransform:
    """What turns a query's words into its row of X0 (``Gs.Query.transform``), for every producer of those rows: its ``kind`` and its parameter ``tensors`` -
    ``'mean'``: the bag mean, no tensors; ``'activation'``: ``act(mean wq^T + bq)``, tensors ``(wq [d, d], bq [d])`` and ``act`` the library's activation code;
    ``'gru'``: the last state of ``nn.GRU(d, d)`` over the words in order, tensors ``(weight_ih_l0 [3d, d], weight_hh_l0 [3d, d], bias_ih_l0 [3d], bias_hh_l0 [3d])``.
    The tensors travel through the producers' autograd functions as trailing arguments, so each returns one gradient per tensor."""
    MEAN, ACTIVATION, GRU = 'mean', 'activation', 'gru'

    def __init__(self, kind: str = 'mean', tensors=(), activation: Optional[str] = None, act: Optional[int] = None):
        if kind not in (self.MEAN, self.ACTIVATION, self.GRU):
            raise ValueError(f'query transform: unknown kind {kind!r} (mean, activation or gru)')
        self.kind, self.tensors = kind, tuple(tensors)
        if len(self.tensors) != {self.MEAN: 0, self.ACTIVATION: 2, self.GRU: 4}[kind]:
            raise ValueError(f'query transform {kind!r}: {len(self.tensors)} tensors given')
        self.act = 0 if kind != self.ACTIVATION else (act if act is not None else _query_activation(activation))

    @classmethod
    def of(cls, wq: Optional[Tensor], bq: Optional[Tensor], activation=None) -> 'QueryTransform':
        """The ``(wq, bq, activation)`` spelling of the mean / activation transforms (``activation``: a name of ``QUERY_ACTIVATIONS`` or the library's code)."""
        if isinstance(wq, cls):
            return wq
        if wq is None:
            return cls()
        return cls(cls.ACTIVATION, (wq, bq), **({'act': int(activation)} if isinstance(activation, int) else {'activation': activation}))

    def operands(self, tensors, dim: int):
        """``tensors`` (this transform's, as an autograd function received them) checked against the width and laid out as the library takes them."""
        if self.kind == self.MEAN:
            return ()
        if self.kind == self.ACTIVATION:
            return _query_transform_operands(tensors[0], tensors[1], dim)
        w_ih, w_hh, b_ih, b_hh = tensors
        if any(tuple(w.shape) != (3 * dim, dim) for w in (w_ih, w_hh)) or any(tuple(b.shape) != (3 * dim,) for b in (b_ih, b_hh)):
            raise ValueError(f'the GRU query transform takes two [{3 * dim}, {dim}] weights and two [{3 * dim}] biases, got {[tuple(t.shape) for t in tensors]}')
        return tuple(t.contiguous() for t in tensors)


def _tape(*tensors) -> bool:
    """True when autograd records the op that is about to run on ``tensors``: its backward will ask for what the forward keeps."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _gru_width(dim: int) -> int:
    """The width the GRU kernels run a ``dim``-wide encoder at: the next tiled one.  Zero columns / rows appended to every operand change nothing: a padded unit has
    ``r = z = 1/2``, ``n = tanh(0) = 0`` and stays ``h = 0`` from ``h_0 = 0``, and contributes exact zeros to every other unit's sums."""
    if dim < 1 or dim > FAST_WIDTHS[-1]:
        raise ValueError(f'the GRU query transform runs at embedding widths 1 .. {FAST_WIDTHS[-1]}, got {dim}')
    return next(wd for wd in FAST_WIDTHS if wd >= dim)


def _pad_gates(w: Tensor, dim: int, width: int) -> Tensor:
    """``[3 d, d]`` (or ``[3 d]``) of the gates r, z, n as ``[3 width, width]`` (``[3 width]``): every gate's block in the top-left of its own zero block."""
    if dim == width:
        return w
    if w.dim() == 1:
        return torch.nn.functional.pad(w.reshape(3, dim), (0, width - dim)).reshape(-1)
    return torch.nn.functional.pad(w.reshape(3, dim, dim), (0, width - dim, 0, width - dim)).reshape(3 * width, width)


def _gru_rows_forward(word_table: Tensor, bag: BagLayout, params, out: Tensor, keep: bool):
    """``ihg_gru_fwd`` into ``out``; returns what ``_gru_rows_backward`` reads - the saved gates and states and the operands at the kernels' width - or ``()``."""
    lib = _lib.load()
    q, dim = bag.n_bags, int(word_table.shape[1])
    width = _gru_width(dim)
    dev = word_table.device
    table = pad_columns(word_table, width).contiguous()
    w_ih, w_hh, b_ih, b_hh = (_pad_gates(t, dim, width) for t in params)
    dest = out if width == dim else torch.empty(q, width, dtype=torch.float32, device=dev)
    saved = torch.empty(int(lib.ihg_gru_saved_bytes(bag.n_words, width)) // 4, dtype=torch.float32, device=dev) if keep and q > 0 and bag.n_words > 0 else None
    if q > 0:
        with profiler.kernel('query_gru_fwd', q, width):
            _lib.check(lib.ihg_gru_fwd(_ptr(table), _ld(table), _ptr(bag.bags.ptr), _ptr(bag.bags.ids), _ptr(bag.length_order), q, bag.n_words, _ptr(w_ih), _ptr(w_hh),
                                       _ptr(b_ih), _ptr(b_hh), _ptr(dest), _ld(dest), _ptr(saved), None, 0, width, _stream()), 'ihg_gru_fwd')
    if dest is not out:
        out.copy_(dest[:, :dim])
    if not keep:
        return ()
    return (saved if saved is not None else torch.empty(0, dtype=torch.float32, device=dev), table, w_ih, w_hh)


def _gru_rows_backward(d_query: Tensor, bag: BagLayout, state):
    """``(d word table, (d w_ih, d w_hh, d b_ih, d b_hh))`` from the complete cotangent of the query rows (``ihg_gru_bwd``); rows and columns of the padding are dropped."""
    lib = _lib.load()
    saved, table, w_ih, w_hh = state
    q, dim, width = bag.n_bags, int(d_query.shape[1]), int(table.shape[1])
    dev = d_query.device
    if width != dim:
        d_query = pad_columns(d_query, width)
    d_table = torch.empty(bag.table_rows, width, dtype=torch.float32, device=dev)
    dw_ih, dw_hh = torch.empty(3 * width, width, dtype=torch.float32, device=dev), torch.empty(3 * width, width, dtype=torch.float32, device=dev)
    db_ih, db_hh = torch.empty(3 * width, dtype=torch.float32, device=dev), torch.empty(3 * width, dtype=torch.float32, device=dev)
    ws = _workspace(int(lib.ihg_gru_workspace_bytes(q, bag.n_words, width)), dev)
    with profiler.kernel('query_gru_bwd', q, width):
        _lib.check(lib.ihg_gru_bwd(_ptr(d_query), _ld(d_query), _ptr(table), _ld(table), _ptr(bag.bags.ptr), _ptr(bag.bags.ids), _ptr(bag.length_order), q, bag.n_words,
                                   _ptr(bag.words_of.ptr), _ptr(bag.word_positions), bag.table_rows, _ptr(w_ih), _ptr(w_hh), _ptr(saved) if saved.numel() else None,
                                   _ptr(d_table), _ptr(dw_ih), _ptr(dw_hh), _ptr(db_ih), _ptr(db_hh), _ptr(ws), ws.numel() * 4, width, _stream()), 'ihg_gru_bwd')
    if width != dim:
        d_table = d_table[:, :dim].contiguous()
        dw_ih, dw_hh = (w.reshape(3, width, width)[:, :dim, :dim].reshape(3 * dim, dim) for w in (dw_ih, dw_hh))
        db_ih, db_hh = (b.reshape(3, width)[:, :dim].reshape(-1) for b in (db_ih, db_hh))
    return d_table, (dw_ih, dw_hh, db_ih, db_hh)


def _query_rows_forward(word_table: Tensor, bag: BagLayout, transform, bq: Optional[Tensor] = None, act: int = 0, out: Optional[Tensor] = None, keep: bool = True):
    """The query rows of X0 into ``out`` (``[Q, d]``, any row stride - a row block of X0 or of a column slice of the feature matrix) under ``transform``, a
    ``QueryTransform`` with its tensors as the library takes them (or the ``wq, bq, act`` spelling of the first two kinds): the bag means ``m`` of the queries' words
    (``ihg_bag_mean_fwd``); with ``'activation'`` ``act(m wq^T + bq)`` (``ihg_rows_linear_act_fwd``; an empty bag gives ``act(bq)``); with ``'gru'`` the encoder's last state
    (``ihg_gru_fwd``; an empty bag gives a zero row).  Returns the tensors the backward of that kind reads beside ``out`` - ``()``, ``(m,)``, or the GRU's saved state and
    operands, which ``keep=False`` (outside autograd: search, the evaluation cache) does not store."""
    qt = QueryTransform.of(transform, bq, int(act))
    if qt.kind == QueryTransform.GRU:
        return _gru_rows_forward(word_table, bag, qt.tensors, out, keep)
    wq, bq = qt.tensors if qt.kind == QueryTransform.ACTIVATION else (None, None)
    act = qt.act
    lib = _lib.load()
    q, dim = bag.n_bags, int(word_table.shape[1])
    means = out if wq is None else torch.empty(q, dim, dtype=torch.float32, device=word_table.device)
    if q > 0:
        with profiler.kernel('bag_mean_fwd', q, dim):
            _lib.check(lib.ihg_bag_mean_fwd(_ptr(word_table), _ld(word_table), _ptr(bag.bags.ptr), _ptr(bag.bags.ids), _ptr(bag.bag_len),
                                            _ptr(means), _ld(means), q, dim, _stream()), 'ihg_bag_mean_fwd')
    if wq is None:
        return ()
    if q > 0:
        ws = _workspace(int(lib.ihg_node_linear_workspace_bytes(dim)), word_table.device)
        with profiler.kernel('query_transform_fwd', q, dim):
            _lib.check(lib.ihg_rows_linear_act_fwd(_ptr(means), dim, _ptr(wq), int(wq.stride(0)), _ptr(bq), act, _ptr(out), _ld(out), q, _ptr(ws), ws.numel() * 4, dim,
                                                   _stream()), 'ihg_rows_linear_act_fwd')
    return (means,)


def _query_rows_backward(d_query: Tensor, bag: BagLayout, qt: QueryTransform, state, y: Optional[Tensor]):
    """``(d word table, gradients of the transform's tensors)`` from the COMPLETE cotangent ``d_query`` of the query rows (``[Q, d]``, any row stride) and what the
    forward returned (``state``) - ``'activation'``: the transform's backward (``ihg_rows_linear_act_bwd`` on ``d_query`` and the rows ``y`` themselves:
    ``dz = d_query * act'(y)`` is never stored; ``state[1]`` = ``wq``), then the bag mean's; ``'gru'``: ``ihg_gru_bwd``."""
    if qt.kind == QueryTransform.GRU:
        return _gru_rows_backward(d_query, bag, state)
    lib = _lib.load()
    q, dim = bag.n_bags, int(d_query.shape[1])
    grads = ()
    if qt.kind == QueryTransform.ACTIVATION:
        means, wq = state
        dm = torch.empty(q, dim, dtype=torch.float32, device=d_query.device)
        dwq, dbq = torch.empty_like(wq), torch.empty(dim, dtype=torch.float32, device=d_query.device)
        ws = _workspace(int(lib.ihg_node_linear_workspace_bytes(dim)), d_query.device)
        with profiler.kernel('query_transform_bwd', q, dim):
            _lib.check(lib.ihg_rows_linear_act_bwd(_ptr(d_query), _ld(d_query), _ptr(y), _ld(y), _ptr(means), dim, _ptr(wq), int(wq.stride(0)), qt.act,
                                                   _ptr(dwq), int(dwq.stride(0)), _ptr(dbq), _ptr(dm), dim, q, _ptr(ws), ws.numel() * 4, dim, _stream()),
                       'ihg_rows_linear_act_bwd')
        d_query, grads = dm, (dwq, dbq)
    d_word = torch.empty(bag.table_rows, dim, dtype=torch.float32, device=d_query.device)
    with profiler.kernel('bag_mean_bwd', bag.table_rows, dim):
        _lib.check(lib.ihg_bag_mean_bwd(_ptr(d_query), _ld(d_query), _ptr(bag.words_of.ptr), _ptr(bag.words_of.ids), _ptr(bag.inv_len), _ptr(d_word), dim,
                                        bag.table_rows, dim, _stream()), 'ihg_bag_mean_bwd')
    return d_word, grads


def _transform_state(qt: QueryTransform, state, params):
    """What a producer saves for ``_query_rows_backward`` beside its own tensors: ``'activation'``: the bag means and ``wq``; ``'gru'``: what its forward returned."""
    return (state[0], params[0]) if qt.kind == QueryTransform.ACTIVATION else tuple(state)


class _BagMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table: Tensor, bag: BagLayout, qt: QueryTransform, keep: bool, *params: Tensor) -> Tensor:
        table = _rows(table, 'table')
        dim = int(table.shape[1])
        params = qt.operands(params, dim)
        out = torch.empty(bag.n_bags, dim, dtype=torch.float32, device=table.device)
        state = _query_rows_forward(table, bag, QueryTransform(qt.kind, params, act=qt.act), out=out, keep=keep)
        ctx.bag, ctx.qt = bag, qt
        if qt.kind != QueryTransform.MEAN:
            ctx.save_for_backward(out, *_transform_state(qt, state, params))
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        grad_out = _rows(grad_out, 'grad_out')
        y, state = (ctx.saved_tensors[0], ctx.saved_tensors[1:]) if ctx.qt.kind != QueryTransform.MEAN else (None, ())
        dtable, grads = _query_rows_backward(grad_out, ctx.bag, ctx.qt, state, y)
        return (dtable, None, None, None) + tuple(grads)


def bag_mean(table: Tensor, bag: BagLayout, wq: Optional[Tensor] = None, bq: Optional[Tensor] = None, activation: Optional[str] = None,
             transform: Optional[QueryTransform] = None) -> Tensor:
    """``nn.EmbeddingBag(mode='mean')`` over every query: ``[V+1,d] -> [Q,d]``; with ``wq [d,d]``, ``bq [d]`` and ``activation`` ('relu' | 'tanh') the reference's
    ``query_transform`` on top (``Models/EmbeddingLayers.py:40-44, 83-84``): ``act(mean wq^T + bq)``.  ``transform``: any ``QueryTransform`` instead of that triple - with
    ``'gru'`` the rows are the GRU encoder's last states over the words in order, not a function of the mean."""
    qt = transform if transform is not None else QueryTransform.of(wq, bq, activation)
    return _BagMean.apply(table, bag, qt, _tape(table, *qt.tensors), *qt.tensors)


class _EmbedAllNodes(torch.autograd.Function):
    """``X0 = [user table rows 1.. ; bag means of the query words ; item table rows 1..]`` assembled in one buffer (the bag
    kernel writes its rows in place), with a backward that hands each table its gradient without a full-size zero fill."""

    @staticmethod
    def forward(ctx, user_table: Tensor, item_table: Tensor, word_table: Tensor, bag: BagLayout, out: Optional[Tensor], qt: QueryTransform, keep: bool, *params: Tensor) -> Tensor:
        word_table = _rows(word_table, 'word table')
        u, q, i = int(user_table.shape[0]) - 1, bag.n_bags, int(item_table.shape[0]) - 1
        dim = int(word_table.shape[1])
        params = qt.operands(params, dim)
        x = _check_out(out, user_table, item_table, word_table, *params)
        if x is None:
            x = torch.empty(u + q + i, dim, dtype=torch.float32, device=word_table.device)
        x[:u].copy_(user_table[1:])
        x[u + q:].copy_(item_table[1:])
        state = _query_rows_forward(word_table, bag, QueryTransform(qt.kind, params, act=qt.act), out=x[u:u + q], keep=keep and out is None)
        ctx.bag, ctx.counts, ctx.qt = bag, (u, q, i), qt
        if qt.kind != QueryTransform.MEAN and out is None:
            ctx.save_for_backward(x, *_transform_state(qt, state, params))
        return x

    @staticmethod
    def backward(ctx, grad: Tensor):
        bag, (u, q, i) = ctx.bag, ctx.counts
        grad = _rows(grad, 'grad')
        dim = int(grad.shape[1])
        d_user = torch.empty(u + 1, dim, dtype=torch.float32, device=grad.device)
        d_user[0].zero_()                                     # the padding row gets no gradient
        d_user[1:].copy_(grad[:u])
        d_item = torch.empty(i + 1, dim, dtype=torch.float32, device=grad.device)
        d_item[0].zero_()
        d_item[1:].copy_(grad[u + q:])
        x, state = (ctx.saved_tensors[0], ctx.saved_tensors[1:]) if ctx.qt.kind != QueryTransform.MEAN else (None, ())
        d_word, grads = _query_rows_backward(grad[u:u + q], bag, ctx.qt, state, x[u:u + q] if x is not None else None)
        return (d_user, d_item, d_word, None, None, None, None) + tuple(grads)


def embed_all_nodes(user_table: Tensor, item_table: Tensor, word_table: Tensor, bag: BagLayout, out: Optional[Tensor] = None, wq: Optional[Tensor] = None,
                    bq: Optional[Tensor] = None, activation: Optional[str] = None, transform: Optional[QueryTransform] = None) -> Tensor:
    """The full-graph input features ``EmbeddingLayer(None, None, None)`` concatenated (``RawGnn.py:112-113``): ``[U+Q+I, d]``
    from the ``[U+1, d]`` / ``[I+1, d]`` tables (row 0 = padding) and the ``[V+1, d]`` word table; ``wq``, ``bq``, ``activation`` / ``transform``: the query transform, as in ``bag_mean``."""
    qt = transform if transform is not None else QueryTransform.of(wq, bq, activation)
    return _EmbedAllNodes.apply(user_table, item_table, word_table, bag, out, qt, _tape(user_table, item_table, word_table, *qt.tensors), *qt.tensors)


# ---------------------------------------------------------------------------------------------
# K4: node-level dense transforms (feature_transform and the hoisted u / q / i blocks of the aggregation)
# ---------------------------------------------------------------------------------------------
def node_linear_supported(x: Tensor, w: Tensor) -> bool:
    """True when the HIP node-level transform kernels take this input: fp32 GPU rows of any width (d in {32,64,128,256} with
    16-byte aligned rows runs on the MFMA row-GEMM, everything else on the any-width kernels of the same library)."""
    d = int(x.shape[1])
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and w.dtype == torch.float32 and x.stride(-1) == 1 and w.stride(-1) == 1
            and int(w.shape[0]) == d and int(w.shape[1]) >= d)


def _type_begin(layout: IncidenceLayout):
    tb = getattr(layout, '_type_begin_c', None)
    if tb is None:
        u, q = layout.user_count, layout.query_count
        tb = (ctypes.c_int64 * 4)(0, u, u + q, layout.node_count)
        layout._type_begin_c = tb
    return tb


def _per_type_bias(bias: Optional[Tensor], typed: bool, dim: int):
    """``(bias, per_type_bias)``: a 2-D bias is ``[3, d]``, one vector per node type, and goes with typed weights."""
    if bias is None or bias.dim() != 2:
        return bias, False
    if not typed or tuple(bias.shape) != (3, dim):
        raise ValueError(f'a per-type bias is [3, {dim}] and needs typed weights, got {tuple(bias.shape)}')
    return bias.contiguous(), True


def _cotangent_rows(grad_out: Tensor) -> Tensor:
    """``grad_out`` as the weight-gradient kernels take it: rows 16-byte aligned."""
    g = _rows(grad_out, 'grad_out')
    return g.contiguous() if g.stride(0) % 4 or g.data_ptr() % 16 else g


def _weight_gradient(w: Tensor, typed: bool, dim: int) -> Tensor:
    """Where ``dw`` goes: the product-block columns of a ``[d, k*d]`` weight, which a node-level map does not touch, stay 0."""
    return torch.zeros_like(w) if w.shape[1] != dim * (3 if typed else 1) else torch.empty_like(w)


class _NodeLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, bias: Optional[Tensor], type_begin, typed: bool, bias_mask: int) -> Tensor:
        x = _rows(x, 'x')
        dim = int(x.shape[1])
        bias, per_type_bias = _per_type_bias(bias, typed, dim)
        out = _node_linear_fwd(x, w, dim if typed else 0, bias, bias_mask, type_begin)
        ctx.save_for_backward(x, w)
        ctx.type_begin, ctx.typed, ctx.bias_mask, ctx.has_bias, ctx.per_type_bias = type_begin, typed, bias_mask, bias is not None, per_type_bias
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        x, w = ctx.saved_tensors
        dim = int(x.shape[1])
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = _weight_gradient(w, ctx.typed, dim)
        dbias = _node_linear_bwd(_cotangent_rows(grad_out), x, w, dim if ctx.typed else 0, ctx.type_begin, dw, dx, False, ctx.has_bias, ctx.per_type_bias, ctx.bias_mask)
        return dx, dw, dbias, None, None, None


class _ComposeFirstOrder(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a: Tensor, c: Optional[Tensor], w: Tensor, b: Tensor):
        lib = _lib.load()
        a, w = _rows(a, 'aggregation weight'), _rows(w, 'transform weight')
        b = b.contiguous()
        c = c.contiguous() if c is not None else None
        dim = int(w.shape[0])
        w_eff = torch.empty(dim, 3 * dim, dtype=torch.float32, device=w.device)
        b_eff = torch.empty(3, dim, dtype=torch.float32, device=w.device)
        _lib.check(lib.ihg_compose_first_order_fwd(_ptr(a), _ld(a), _ptr(c), _ptr(w), _ld(w), _ptr(b), _ptr(w_eff), 3 * dim, _ptr(b_eff), dim, _stream()),
                   'ihg_compose_first_order_fwd')
        ctx.save_for_backward(a, w, b)
        ctx.has_c = c is not None
        return w_eff, b_eff

    @staticmethod
    def backward(ctx, dw_eff: Tensor, db_eff: Tensor):
        lib = _lib.load()
        a, w, b = ctx.saved_tensors
        dim = int(w.shape[0])
        dw_eff, db_eff = _rows(dw_eff, 'dw_eff'), db_eff.contiguous()
        da, dw, db = torch.empty_like(a), torch.empty_like(w), torch.empty_like(b)
        dc = torch.empty(dim, dtype=torch.float32, device=w.device) if ctx.has_c else None
        _lib.check(lib.ihg_compose_first_order_bwd(_ptr(a), _ld(a), _ptr(w), _ld(w), _ptr(b), _ptr(dw_eff), _ld(dw_eff), _ptr(db_eff), _ptr(da), _ld(da),
                                                   _ptr(dc), _ptr(dw), _ld(dw), _ptr(db), dim, _stream()), 'ihg_compose_first_order_bwd')
        return da, dc, dw, db


def compose_first_order(a: Tensor, c: Optional[Tensor], w: Tensor, b: Tensor):
    """``(W_eff [d, 3d], b_eff [3, d])`` of ``first_order(linear(x; w, b); a, c)``: ``W_eff = [A_u w | A_q w | A_i w]``,
    ``b_eff[t] = A_t b`` (+ ``c`` for users).  Differentiable in all four arguments."""
    if tuple(a.shape) != (w.shape[0], 3 * w.shape[0]) or w.shape[0] != w.shape[1]:
        raise ValueError(f'compose_first_order takes a [d, 3d] block weight and a [d, d] transform, got {tuple(a.shape)} and {tuple(w.shape)}')
    return _ComposeFirstOrder.apply(a, c, w, b)


class NodeTables:
    """The input features ``X0 = [user_table[1:] ; bag means of the queries ; item_table[1:]]`` (``RawGnn.py:112-113``) WITHOUT assembling them: the
    first node-level transform of the model reads the three row blocks where they are (``ihg_node_linear_fwd_typed``), its backward writes the tables'
    gradients in place (no ``[N, d]`` gradient that autograd then cuts apart), and the batch tail reads / scatters its layer-0 rows the same way.
    Stands in for the ``[N, d]`` tensor between ``EmbeddingLayer.node_tables()`` and the first layer; ``node_linear`` resolves it (bag means, autograd token)."""

    def __init__(self, user_table: Tensor, item_table: Tensor, word_table: Tensor, bag: 'BagLayout', holder: 'TailGradients', wq: Optional[Tensor] = None,
                 bq: Optional[Tensor] = None, activation: Optional[str] = None, transform: Optional[QueryTransform] = None):
        self.user_table, self.item_table, self.word_table, self.bag, self.holder = user_table, item_table, word_table, bag, holder
        qt = transform if transform is not None else QueryTransform.of(wq, bq, activation)
        self.transform = QueryTransform(qt.kind, qt.operands(qt.tensors, int(user_table.shape[1])), act=qt.act)      # the query transform (Gs.Query.transform), its tensors as the library takes them
        self.query_rows: Optional[Tensor] = None        # [Q, d] query rows of X0 (bag means, transformed where a transform is set), set by the first node_linear
        self.token: Optional[Tensor] = None             # carries the autograd edge from the batch tail to that op
        self.dim = int(user_table.shape[1])
        self.shape = (int(user_table.shape[0]) - 1 + bag.n_bags + int(item_table.shape[0]) - 1, self.dim)
        self.device = user_table.device

    def row_pointers(self):
        """HOST array of three device pointers: the first row of the users, the queries, the items (row 0 of either table is its padding row)."""
        step = self.dim * 4
        return (ctypes.c_void_p * 3)(self.user_table.data_ptr() + step, self.query_rows.data_ptr(), self.item_table.data_ptr() + step)

    def type_begin(self):
        """First row of every node type in the numbering the TABLES are addressed by (the public one: ``[0, U, U + Q, N]``) - the layout's own unless it leaves the isolated
        nodes out (``gather_active_nodes`` sets it then)."""
        tb = getattr(self, '_public_type_begin', None)
        return tb if tb is not None else _type_begin(self.layout)

    @staticmethod
    def supported(user_table: Tensor, item_table: Tensor, word_table: Tensor) -> bool:
        lib = _lib.load()
        d = int(user_table.shape[1])
        return (user_table.is_cuda and all(t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (user_table, item_table, word_table))
                and d % 4 == 0 and bool(lib.ihg_node_linear_typed_supported(d, d, d)))


class _LinearFromTables(torch.autograd.Function):
    """``node_linear(X0)`` with X0 given by its tables (``NodeTables``): bag means of the queries + the typed-rows row GEMM forward; backward: weight / bias gradient
    and the input gradient written straight into the tables' gradients (padding rows zeroed by the library), the batch tail's layer-0 row gradients added
    there (this op is also the tap of layer 0), then the bag-mean backward."""

    @staticmethod
    def forward(ctx, user_table: Tensor, item_table: Tensor, word_table: Tensor, w: Tensor, bias: Optional[Tensor], nodes: NodeTables, layout: IncidenceLayout, typed: bool,
                bias_mask: int, keep: bool, *params: Tensor):
        lib = _lib.load()
        bag, dim, qt = nodes.bag, nodes.dim, nodes.transform
        n = nodes.shape[0]
        query_rows = torch.empty(bag.n_bags, dim, dtype=torch.float32, device=word_table.device)
        state = _query_rows_forward(word_table, bag, qt, out=query_rows, keep=keep)
        nodes.query_rows, nodes.layout = query_rows, layout
        nodes.token = torch.empty(1, dtype=torch.float32, device=word_table.device)
        out = torch.empty(n, dim, dtype=torch.float32, device=word_table.device)
        ws = _workspace(int(lib.ihg_node_linear_workspace_bytes(dim)), word_table.device)
        bias, per_type_bias = _per_type_bias(bias, typed, dim)
        with profiler.kernel('node_linear_fwd', n, dim):
            _lib.check(lib.ihg_node_linear_fwd_typed(nodes.row_pointers(), dim, _ptr(w), int(w.stride(0)), dim if typed else 0, _ptr(bias), bias_mask, dim if per_type_bias else 0,
                                                     _type_begin(layout), _ptr(out), dim, _ptr(ws), ws.numel() * 4, dim, _stream()), 'ihg_node_linear_fwd_typed')
        ctx.save_for_backward(user_table, item_table, w, query_rows, *_transform_state(qt, state, params))
        ctx.nodes, ctx.layout, ctx.typed, ctx.bias_mask, ctx.has_bias, ctx.per_type_bias = nodes, layout, typed, bias_mask, bias is not None, per_type_bias
        ctx.mark_non_differentiable(query_rows)
        ctx.set_materialize_grads(False)                     # (the token's and the bag means' gradients are never read: no zero tensors made for them)
        return out, nodes.token, query_rows

    @staticmethod
    def backward(ctx, grad_out: Tensor, _grad_token, _grad_rows):
        lib = _lib.load()
        user_table, item_table, w, query_rows = ctx.saved_tensors[:4]
        state = ctx.saved_tensors[4:]
        nodes, layout = ctx.nodes, ctx.layout
        bag, dim = nodes.bag, nodes.dim
        if grad_out is None:
            raise RuntimeError('the output of the first node-level transform received no gradient')
        g = _cotangent_rows(grad_out)
        dev = g.device
        d_user, d_item = torch.empty_like(user_table), torch.empty_like(item_table)
        d_query = torch.empty_like(query_rows)
        dw = _weight_gradient(w, ctx.typed, dim)
        dbias = _bias_gradient(ctx.has_bias, ctx.per_type_bias, dim, dev)
        step = dim * 4
        x_rows = (ctypes.c_void_p * 3)(user_table.data_ptr() + step, query_rows.data_ptr(), item_table.data_ptr() + step)
        dx_rows = (ctypes.c_void_p * 3)(d_user.data_ptr() + step, d_query.data_ptr(), d_item.data_ptr() + step)
        ws = _workspace(int(lib.ihg_node_linear_workspace_bytes(dim)), dev)
        with profiler.kernel('node_linear_bwd', nodes.shape[0], dim):
            _lib.check(lib.ihg_node_linear_bwd_weight_typed(_ptr(g), _ld(g), x_rows, dim, _type_begin(layout), _ptr(dw), int(dw.stride(0)), dim if ctx.typed else 0,
                                                            _ptr(dbias), ctx.bias_mask, dim if ctx.per_type_bias else 0, _ptr(w), int(w.stride(0)), dx_rows, dim, 0b101,
                                                            _ptr(ws), ws.numel() * 4, dim, _stream()), 'ihg_node_linear_bwd_weight_typed')
        holder = nodes.holder
        if holder is not None and holder.rowgrad is not None:              # the batch tail's gradient of the layer-0 rows: this op is their tap
            holder.put_into_typed(dx_rows, dim, layout, 0, dim)
        # d_query is complete now (layer 0's input gradient + the batch tail's layer-0 rows): the query transform's backward, then the bag mean's
        d_word, grads = _query_rows_backward(d_query, bag, nodes.transform, state, query_rows)
        return (d_user, d_item, d_word, dw, dbias, None, None, None, None, None) + tuple(grads)


class _GatherActiveNodes(torch.autograd.Function):
    """``X0`` of the nodes that have hyperedges, ``[N', d]`` in the numbering of a layout that leaves the isolated nodes out (``IncidenceLayout.compact``), gathered from the
    embedding tables' rows and the query bag means - the public ``[N, d]`` matrix is never assembled.  Resolves the ``NodeTables`` for the batch tail as the first
    node-level transform does otherwise: the tail reads its layer-0 rows from the tables in place (public ids) and this op's backward adds their gradients to the tables'
    gradients - dense ``[U + 1, d]`` / ``[I + 1, d]`` / ``[V + 1, d]`` tensors whose rows are zero for nodes that are neither active nor in the batch."""

    @staticmethod
    def forward(ctx, user_table: Tensor, item_table: Tensor, word_table: Tensor, nodes: NodeTables, layout: IncidenceLayout, keep: bool, *params: Tensor):
        bag, dim, qt = nodes.bag, nodes.dim, nodes.transform
        u_pub, q_pub = layout.public_user_count, layout.public_query_count
        query_rows = torch.empty(bag.n_bags, dim, dtype=torch.float32, device=word_table.device)
        state = _query_rows_forward(word_table, bag, qt, out=query_rows, keep=keep)
        nodes.query_rows, nodes.layout = query_rows, layout
        nodes._public_type_begin = (ctypes.c_int64 * 4)(0, u_pub, u_pub + q_pub, layout.public_node_count)
        nodes.token = torch.empty(1, dtype=torch.float32, device=word_table.device)
        picks = getattr(layout, '_active_table_rows', None)
        if picks is None:
            act = layout.active_nodes
            ua, qa = layout.user_count, layout.query_count
            picks = layout._active_table_rows = (act[:ua] + 1, act[ua:ua + qa] - u_pub, act[ua + qa:] - (u_pub + q_pub) + 1)      # table rows (row 0 = padding), query ids
        ua, qa = int(picks[0].shape[0]), int(picks[1].shape[0])
        x = torch.empty(layout.node_count, dim, dtype=torch.float32, device=word_table.device)
        torch.index_select(user_table, 0, picks[0], out=x[:ua])
        torch.index_select(query_rows, 0, picks[1], out=x[ua:ua + qa])
        torch.index_select(item_table, 0, picks[2], out=x[ua + qa:])
        ctx.save_for_backward(user_table, item_table, query_rows, *_transform_state(qt, state, params))
        ctx.nodes, ctx.layout, ctx.picks = nodes, layout, picks
        ctx.mark_non_differentiable(query_rows)
        ctx.set_materialize_grads(False)
        return x, nodes.token, query_rows

    @staticmethod
    def backward(ctx, grad_x: Tensor, _grad_token, _grad_rows):
        user_table, item_table, query_rows = ctx.saved_tensors[:3]
        state = ctx.saved_tensors[3:]
        nodes, layout, picks = ctx.nodes, ctx.layout, ctx.picks
        bag, dim = nodes.bag, nodes.dim
        if grad_x is None:
            raise RuntimeError('the gathered input features received no gradient')
        g = _rows(grad_x, 'grad of the gathered input features')
        ua, qa = int(picks[0].shape[0]), int(picks[1].shape[0])
        d_user, d_item = torch.zeros_like(user_table), torch.zeros_like(item_table)
        d_query = torch.zeros(bag.n_bags, dim, dtype=torch.float32, device=g.device)
        d_user.index_copy_(0, picks[0], g[:ua])
        d_query.index_copy_(0, picks[1], g[ua:ua + qa])
        d_item.index_copy_(0, picks[2], g[ua + qa:])
        holder = nodes.holder
        if holder is not None and holder.rowgrad is not None:              # the batch tail's gradient of its layer-0 rows (public ids; isolated batch nodes included)
            step = dim * 4
            dx_rows = (ctypes.c_void_p * 3)(d_user.data_ptr() + step, d_query.data_ptr(), d_item.data_ptr() + step)
            holder.put_into_typed(dx_rows, dim, layout, 0, dim, type_begin=nodes._public_type_begin)
        d_word, grads = _query_rows_backward(d_query, bag, nodes.transform, state, query_rows)      # (on the complete d_query, as in _LinearFromTables)
        return (d_user, d_item, d_word, None, None, None) + tuple(grads)


def gather_active_nodes(nodes: NodeTables, layout: IncidenceLayout) -> Tensor:
    """``[N', d]`` input features of the nodes of a compact layout straight from the embedding tables (``NodeTables``), which it resolves for the batch tail."""
    if not getattr(layout, 'compact', False):
        raise ValueError('gather_active_nodes is for a layout that leaves the isolated nodes out')
    if nodes.query_rows is not None:
        raise RuntimeError('NodeTables: the input features were already consumed (one per forward)')
    params = nodes.transform.tensors
    x, _token, _rows_q = _GatherActiveNodes.apply(nodes.user_table, nodes.item_table, nodes.word_table, nodes, layout,
                                                  _tape(nodes.user_table, nodes.item_table, nodes.word_table, *params), *params)
    return x


def node_linear(x, w: Tensor, bias: Optional[Tensor], layout: IncidenceLayout, typed: bool = False, bias_mask: int = 0b111) -> Tensor:
    """``out[v] = x[v] @ W_type(v).T (+ bias)``.  ``typed=False``: one ``[d,d]`` weight for every node; ``typed=True``:
    ``w`` is ``[d, k*d]`` and node type t uses its column block ``w[:, t*d:(t+1)*d]``; a ``[d]`` bias is added to the types in
    ``bias_mask``, a ``[3, d]`` bias gives every (masked) type its own vector.  ``x`` may be a ``NodeTables`` (the input features given by their tables)."""
    if isinstance(x, NodeTables):
        if x.query_rows is not None:
            raise RuntimeError('NodeTables: the input features were already consumed by a node-level transform (one per forward)')
        params = x.transform.tensors
        out, _token, _rows_q = _LinearFromTables.apply(x.user_table, x.item_table, x.word_table, w, bias, x, layout, bool(typed), int(bias_mask),
                                                       _tape(x.user_table, x.item_table, x.word_table, w, bias, *params), *params)
        return out
    return _NodeLinear.apply(x, w, bias, _type_begin(layout), bool(typed), int(bias_mask))


def rows_linear(x: Tensor, w: Tensor, bias: Optional[Tensor]) -> Tensor:
    """``out[r] = x[r] @ w.T (+ bias)`` for every row of ANY ``[rows, d]`` table (``w`` square) on the same row-GEMM kernels as ``node_linear`` - which takes its type
    boundaries from a layout's node counts; this is for tables that are not node tables: the ``[E, d]`` hyperedge features of the phase-2 attention."""
    return _NodeLinear.apply(x, w, bias, _plain_type_begin(int(x.shape[0])), False, 0b111)


# ---------------------------------------------------------------------------------------------
# Widths between the tiled ones: zero-padded to the next width the MFMA kernels take
# ---------------------------------------------------------------------------------------------
FAST_WIDTHS = (32, 64, 128, 256)
# IHG_PAD_WIDTHS=1 (default): an embedding width that is a multiple of 4 below 256 and not one of FAST_WIDTHS - the reference takes any --emb (Helpers/ArgsParser.py:94-95,
# Main.py:23): 48, 96, 160, 192, 224 ... - runs on the kernels of the NEXT fast width with zero columns appended: zero weight rows / columns and zero bias entries keep the
# padding columns exactly zero through every layer (a linear map of zeros, products with zeros), so the first d columns are the d-wide model's values - the same sums with
# exact zeros added - and the parameters keep their shapes.  0: the any-width kernels (one thread per output), which is what every width ran on before round 6.
PAD_WIDTHS = _os.environ.get('IHG_PAD_WIDTHS', '1') != '0'


def padded_width(dim: int) -> int:
    """The width the kernels run a ``dim``-wide model at: ``dim`` itself when it is tiled (or padding is off / does not apply), else the next of ``FAST_WIDTHS``."""
    dim = int(dim)
    if not PAD_WIDTHS or dim in FAST_WIDTHS or dim > FAST_WIDTHS[-1] or dim < 1:
        return dim
    return next(wd for wd in FAST_WIDTHS if wd >= dim)


def pad_columns(x: Tensor, width: int) -> Tensor:
    """``[n, d] -> [n, width]`` with zero columns appended (differentiable; ``x`` itself when it is already that wide)."""
    return x if int(x.shape[-1]) == width else torch.nn.functional.pad(x, (0, width - int(x.shape[-1])))


def pad_square(w: Tensor, width: int) -> Tensor:
    """A ``[d, d]`` weight as the top-left block of a zero ``[width, width]`` one."""
    d = int(w.shape[0])
    return w if d == width else torch.nn.functional.pad(w, (0, width - d, 0, width - d))


def pad_blocks(w: Tensor, width: int) -> Tensor:
    """A ``[d, k d]`` block weight (``aggregation.weight``: blocks u, q, i, uq, qi, iu, uqi side by side) as ``[width, k width]``: every ``[d, d]`` block in the top-left of its own
    zero ``[width, width]`` block."""
    d = int(w.shape[0])
    if d == width:
        return w
    k = int(w.shape[1]) // d
    return torch.nn.functional.pad(w.reshape(d, k, d), (0, width - d, 0, 0, 0, width - d)).reshape(width, k * width)


def pad_vector(b: Optional[Tensor], width: int) -> Optional[Tensor]:
    if b is None or int(b.shape[-1]) == width:
        return b
    return torch.nn.functional.pad(b, (0, width - int(b.shape[-1])))


# ---------------------------------------------------------------------------------------------
# K5+K6 interactive step (orders 2 and 3)
# ---------------------------------------------------------------------------------------------
# the [E, 3, d] member-gradient buffer of the interactive backward is produced in hyperedge chunks beyond this many bytes
MEMBER_BUFFER_LIMIT_BYTES = 48 << 30
# use ihg_interact_bwd_user_reduced (user slot summed on chip, [E, 2, d] member buffer) where the library offers it (tests set this attribute to compare with the
# [E, 3, d] form, which every shape without such a kernel runs anyway)
USER_REDUCED_BACKWARD = _os.environ.get('IHG_USER_REDUCED_BACKWARD', '1') != '0'
# the last layer of a training step is told which rows of its output are read (node_two_hop's cotangent_rows): its backward pulls only those
SPARSE_LAST_COTANGENT = _os.environ.get('IHG_SPARSE_LAST_COTANGENT', '1') != '0'
CHECK_SPARSE_COTANGENT = _os.environ.get('IHG_CHECK_SPARSE_COTANGENT', '0') == '1'
# the forward of the interactive layer in its node-level form (no [E, d] rows: ihg_node_pair_sums + ihg_node_interact_fwd) where the library has it;
# IHG_NODE_LEVEL_FORWARD=0: the hyperedge form (typed first-order GEMM -> ihg_interact_fwd -> K7) everywhere (A/B, tests)
NODE_LEVEL_FORWARD = _os.environ.get('IHG_NODE_LEVEL_FORWARD', '1') != '0'
# ... and the product blocks' weight gradients from node-level data (ihg_node_interact_bwd_weight) after such a forward; IHG_NODE_LEVEL_WEIGHT=0: the hyperedge kernel
NODE_LEVEL_WEIGHT = _os.environ.get('IHG_NODE_LEVEL_WEIGHT', '1') != '0'
# the first-order gradient d P = H H^T (scale * dy): a scatter of the stored [E, d] cotangents - or, for tables beyond this many bytes, the two-hop operator on dy
# (at C3 the scatter wins, 8.74 against 8.81 ms per step; at C5 the 51 GB table's scatter reads HBM at random and the two-hop form wins, 22 against 32 ms)
FIRST_ORDER_TWO_HOP_BYTES = int(_os.environ.get('IHG_FIRST_ORDER_TWO_HOP_BYTES', 8 << 30))     # where the member-gradient kernel does not form the hyperedges' cotangents itself: [E, d] tables larger than this take the two-hop form
# the hyperedges' cotangents of the interactive layer's backward written by K5 as the member-gradient kernel's operand (two fp16 planes per row + the row's inverse scale)
# where nothing else reads them (d = 256 beyond FIRST_ORDER_TWO_HOP_BYTES: config C5); IHG_COTANGENT_PLANES=0: fp32 rows, scaled and split by every column part of the kernel
COTANGENT_PLANES = _os.environ.get('IHG_COTANGENT_PLANES', '1') != '0'


def _node_level_forward_ok(h: Tensor, w: Tensor, bias: Optional[Tensor], out: Optional[Tensor], dim: int, order: int) -> bool:
    lib = _lib.load()
    ld_out = dim if out is None else _ld(out)
    return (bool(lib.ihg_node_interact_fwd_supported(dim, order, _ld(h), 3 * dim, ld_out)) and h.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and _ld(w) % 4 == 0
            and (bias is None or bias.data_ptr() % 16 == 0) and (out is None or out.data_ptr() % 16 == 0))


# the input features read from the embedding tables in place (NodeTables) in a training step through the fused batch tail; IHG_NODE_TABLES=0: X0 assembled by copies (A/B, tests)
NODE_TABLES = _os.environ.get('IHG_NODE_TABLES', '1') != '0'
# Layer-0 backward where the member-gradient kernel gathers the node-level cotangent (d = 128): hyperedges are numbered by user, so a user's row of the first-order
# gradient, sum over its hyperedges of dout[e], is a run sum of the cotangents that kernel forms anyway - it writes those rows (ihg_interact_bwd_gathered_first_order)
# and the two-hop launch behind it computes the query and item rows only (2 E of its 6 E entries and N_u of its N self terms fewer).  The users' rows are then summed in
# hyperedge order instead of two-hop list order; every other output keeps its bits.  IHG_FIRST_ORDER_USER_SUMS=0 (or this attribute) turns it off: the full two-hop launch.
FIRST_ORDER_USER_SUMS = _os.environ.get('IHG_FIRST_ORDER_USER_SUMS', '1') != '0'


def _user_reduced_ok(h: Tensor, w: Tensor, grad_out: Tensor, layout: IncidenceLayout, order: int) -> bool:
    """The interactive backward can run ``ihg_interact_bwd_user_reduced`` on these operands."""
    lib = _lib.load()
    return bool(USER_REDUCED_BACKWARD and layout.edge_count > 0 and getattr(layout, 'user_sorted', False)
                and lib.ihg_interact_bwd_user_reduced_supported(int(h.shape[1]), order, _ld(h)) and h.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
                and _ld(w) % 4 == 0 and _ld(grad_out) % 4 == 0 and grad_out.data_ptr() % 16 == 0)


def _first_order_rows(h: Tensor, w: Tensor, bias: Optional[Tensor], layout: IncidenceLayout) -> Tensor:
    """``[N, d]`` first-order blocks per node: the typed row GEMM with ``w``'s blocks u / q / i, the bias on the users (bias mask ``0b001``)."""
    return _node_linear_fwd(h, w, int(h.shape[1]), bias, 0b001, _type_begin(layout))


def _interact_rows(h: Tensor, p: Tensor, w: Tensor, layout: IncidenceLayout, order: int) -> Tensor:
    """``[E, d]`` hyperedge rows (``ihg_interact_fwd``): the first-order part gathered from ``p``, the products of ``h``'s member rows contracted with ``w``."""
    lib = _lib.load()
    dim = int(h.shape[1])
    out = torch.empty(layout.edge_count, dim, dtype=torch.float32, device=h.device)
    ws = _workspace(int(lib.ihg_interact_fwd_workspace_bytes(layout.edge_count, dim, order)), h.device)
    with profiler.kernel('interact_fwd', layout.edge_count, dim):
        _lib.check(lib.ihg_interact_fwd(_ptr(h), _ld(h), _ptr(p), _ld(p), _ptr(layout.i3), _ptr(w), _ld(w), order,
                                        _ptr(out), _ld(out), _ptr(ws), ws.numel() * 4, layout.edge_count, dim, _stream()), 'ihg_interact_fwd')
    return out


def _first_order_backward(dp: Tensor, h: Tensor, w: Tensor, layout: IncidenceLayout, dw: Tensor, dh: Tensor, has_bias: bool) -> Optional[Tensor]:
    """The first-order blocks' gradients from ``dp``: weights into ``dw``'s blocks u / q / i, the input gradient ADDED onto ``dh`` - by the kernel (``dx_accumulate``: no
    separate ``[N, d]`` add) where it can.  Returns the bias gradient (``None`` without a bias)."""
    dim = int(h.shape[1])
    accumulate = (bool(_lib.load().ihg_node_linear_bwd_accumulates(dim, _ld(dp), _ld(h), _ld(dh))) and h.data_ptr() % 16 == 0 and dh.data_ptr() % 16 == 0
                  and dp.data_ptr() % 16 == 0)
    dx = dh if accumulate else torch.empty_like(dh)
    dbias = _node_linear_bwd(dp, h, w, dim, _type_begin(layout), dw, dx, accumulate, has_bias, False, 0b001)
    if not accumulate:
        dh.add_(dx)
    return dbias


def _member_gradients(h: Tensor, layout: IncidenceLayout, order: int, dw: Optional[Tensor], user_reduced: bool, launch) -> Tensor:
    """The member gradients of the interactive backward scattered to nodes (returned), the product blocks' weight gradients into ``dw`` (its columns from ``3 d`` on;
    ``None``: not wanted).  ``launch(e0, e1, g, dh, dw_part, ws)`` runs the member-gradient kernel on hyperedges ``e0:e1`` into ``dw_part`` and the member buffer ``g``:
    ``[n, 3 d]``, or ``[n, 2 d]`` with ``user_reduced`` (hyperedges numbered by user: the kernel sums the user slot on chip and writes ``dh[users]`` itself).  Beyond
    ``MEMBER_BUFFER_LIMIT_BYTES`` hyperedge chunks, each with its own member lists (user-reduced: cut where the user changes), the K7 passes after the first
    adding onto ``dh`` inside the kernel: same sums, associated chunk by chunk."""
    lib = _lib.load()
    n_edges, dim = layout.edge_count, int(h.shape[1])
    slots = 2 if user_reduced else 3
    n_chunks = max(1, -(-(n_edges * slots * dim * 4) // MEMBER_BUFFER_LIMIT_BYTES))
    if user_reduced:
        parts = [(0, n_edges) + layout.member_csr_qi()] if n_chunks == 1 else layout.member_csr_qi_chunks(n_chunks)
        dh = torch.empty(layout.node_count, dim, dtype=torch.float32, device=h.device)
        idx = layout.users_without_hyperedges()          # not written by the user-reduced kernels: an index fill of their rows (a fill of the user block is 118 MB at C3)
        if idx.numel():
            _lib.check(lib.ihg_zero_rows(_ptr(dh), _ld(dh), dim, _ptr(idx), int(idx.numel()), _stream()), 'ihg_zero_rows')
    else:                                                # (node v, hyperedge e) reads row 3 (e - e0) + type(v)
        parts = [(0, n_edges, layout.member_csr)] if n_chunks == 1 else layout.member_csr_chunks(n_chunks)
        parts = [part + (None,) for part in parts]
        dh = None
    for index, (e0, e1, csr, csr_rows) in enumerate(parts):
        g = torch.empty(e1 - e0, slots * dim, dtype=torch.float32, device=h.device)
        dw_part = dw if index == 0 or dw is None else torch.empty_like(dw)
        ws = _workspace(int(lib.ihg_interact_bwd_workspace_bytes(e1 - e0, dim, order)), h.device)
        with profiler.kernel('interact_bwd', e1 - e0, dim):
            launch(e0, e1, g, dh, dw_part, ws)
        if index > 0 and dw is not None:
            dw[:, 3 * dim:].add_(dw_part[:, 3 * dim:])
        dh = node_segment_sum_raw(g.view(slots * (e1 - e0), dim), csr, out=dh, rows=csr_rows, role='k7.member_gradients', accumulate=index > 0, read_once=True)
        del g
    return dh


def _interact_backward(h: Tensor, w: Tensor, grad_out: Tensor, layout: IncidenceLayout, order: int, dw: Optional[Tensor], inv_scale: Optional[Tensor] = None) -> Tensor:
    """``_member_gradients`` from the hyperedges' cotangents ``grad_out`` (``[E, d]``; with ``inv_scale`` (``[E]``): fp16 planes written by
    ``ihg_edge_gather_sum_planes``, read by the user-reduced kernel only)."""
    lib = _lib.load()
    dim = int(h.shape[1])
    reduced = _user_reduced_ok(h, w, grad_out, layout, order)
    if inv_scale is not None and (dw is not None or not reduced):
        raise RuntimeError('cotangent planes are read by the user-reduced member-gradient kernel only')
    def launch(e0, e1, g, dh, dw_part, ws):
        n, go, i3, ld_dw = e1 - e0, grad_out[e0:e1], layout.i3[e0:e1], _ld(dw_part) if dw_part is not None else 0
        if inv_scale is not None:
            _lib.check(lib.ihg_interact_bwd_user_reduced_planes(_ptr(h), _ld(h), _ptr(i3), _ptr(w), _ld(w), order, _ptr(go), _ptr(inv_scale[e0:e1]),
                                                                _ptr(g), _ptr(dh), dim, _ptr(ws), ws.numel() * 4, n, dim, _stream()), 'ihg_interact_bwd_user_reduced_planes')
        elif reduced:
            _lib.check(lib.ihg_interact_bwd_user_reduced(_ptr(h), _ld(h), _ptr(i3), _ptr(w), _ld(w), order, _ptr(go), _ld(grad_out), _ptr(g),
                                                         _ptr(dh), dim, _ptr(dw_part), ld_dw, _ptr(ws), ws.numel() * 4, n, dim, _stream()), 'ihg_interact_bwd_user_reduced')
        else:
            _lib.check(lib.ihg_interact_bwd(_ptr(h), _ld(h), _ptr(i3), _ptr(w), _ld(w), order, _ptr(go), _ld(grad_out),
                                            _ptr(g), _ptr(dw_part), ld_dw, _ptr(ws), ws.numel() * 4, n, dim, _stream()), 'ihg_interact_bwd')
    return _member_gradients(h, layout, order, dw, reduced, launch)


def _gathered_backward_ok(h: Tensor, w: Tensor, dy: Tensor, layout: IncidenceLayout, order: int) -> bool:
    # (the gathering kernel forms sum_m scale[m] dy[m] itself and has no per-hyperedge factor: a layout with multiplicities takes the K5 + member-kernel sequence)
    dim = int(h.shape[1])
    return (layout.edge_weight is None and layout.edge_count * 3 * dim * 4 <= MEMBER_BUFFER_LIMIT_BYTES and _user_reduced_ok(h, w, dy, layout, order)
            and bool(_lib.load().ihg_interact_bwd_gathered_supported(dim, order, _ld(h), _ld(dy))))


def _interact_to_nodes_backward(h: Tensor, w: Tensor, dy: Tensor, layout: IncidenceLayout, order: int, out_scale: Optional[Tensor], dw: Tensor,
                                sums: Optional[Tensor] = None):
    """``(d h, d p)`` of ``y = out_scale * H interact(h, p, w)`` from ``dy``, the product blocks' weight gradients into ``dw`` (from node-level data where the forward
    left the pair sums ``sums``).  The member-gradient kernel gathers the three ``dy`` rows of a hyperedge itself where it can (``ihg_interact_bwd_gathered``: no
    node -> hyperedge launch); otherwise K5 forms the hyperedges' cotangents for ``_interact_backward``."""
    lib = _lib.load()
    n_edges, dim = layout.edge_count, int(h.shape[1])
    # the product blocks' weight gradients from node-level data (N rows, no gathers) where the forward left the pair sums
    node_weight = (sums is not None and NODE_LEVEL_WEIGHT and dy.data_ptr() % 16 == 0 and _ld(dw) % 4 == 0 and h.data_ptr() % 16 == 0
                   and bool(lib.ihg_node_interact_bwd_weight_supported(dim, order, _ld(h), _ld(sums), _ld(dy))))
    if node_weight:
        ws_w = _workspace(int(lib.ihg_node_interact_bwd_weight_workspace_bytes(dim, order)), h.device)
        with profiler.kernel('node_interact_bwd_weight', layout.node_count, dim):
            _lib.check(lib.ihg_node_interact_bwd_weight(_ptr(h), _ld(h), _ptr(sums), _ld(sums), _ptr(dy), _ld(dy), _ptr(out_scale), order, _type_begin(layout),
                                                        _ptr(dw), _ld(dw), _ptr(ws_w), ws_w.numel() * 4, dim, _stream()), 'ihg_node_interact_bwd_weight')
    if _gathered_backward_ok(h, w, dy, layout, order):
        # with the weight gradients taken at node level nobody but the first-order scatter would read the hyperedges' cotangents: then that gradient is
        # the two-hop operator applied to the node-level cotangent and the [E, d] rows are not stored at all.  (Round 3 measured the opposite order - 8.81 against
        # 8.74 ms per C3 step; since the member-gradient kernel became bound by its memory traffic the 1.1 GB it no longer writes are worth more than the two-hop
        # launch costs over the scatter: C3 7.89 -> 7.78 ms, C2 1.92 -> 1.87, C4 10.59 -> 10.45; member kernel 1,426-1,467 -> 1,188 us, first-order gradient 672-681 -> 823-833)
        keep_dout = not node_weight
        dout = torch.empty(n_edges, dim, dtype=torch.float32, device=h.device) if keep_dout else None
        # the users' rows of the first-order gradient from the member kernel's run sums (a user's degree is its run's length: layout.self_weight without multiplicities)
        user_sums = (FIRST_ORDER_USER_SUMS and not keep_dout and bool(lib.ihg_interact_bwd_gathered_first_order_supported(dim, order, _ld(h), _ld(dy))))
        dp = None
        if user_sums:
            dp = torch.empty(layout.node_count, dim, dtype=torch.float32, device=h.device)
            idx = layout.users_without_hyperedges()
            if idx.numel():
                _lib.check(lib.ihg_zero_rows(_ptr(dp), _ld(dp), dim, _ptr(idx), int(idx.numel()), _stream()), 'ihg_zero_rows')
        def launch(e0, e1, g2, dh, dw_part, ws):             # (one launch: _gathered_backward_ok keeps even the [E, 3, d] buffer within MEMBER_BUFFER_LIMIT_BYTES)
            if user_sums:
                _lib.check(lib.ihg_interact_bwd_gathered_first_order(_ptr(h), _ld(h), _ptr(layout.i3), _ptr(w), _ld(w), order, _ptr(dy), _ld(dy), _ptr(out_scale),
                                                                     _ptr(dout), dim, _ptr(g2), _ptr(dh), dim, _ptr(dp), _ld(dp), _ptr(dw_part), _ld(dw), _ptr(ws),
                                                                     ws.numel() * 4, n_edges, dim, _stream()), 'ihg_interact_bwd_gathered_first_order')
                return
            _lib.check(lib.ihg_interact_bwd_gathered(_ptr(h), _ld(h), _ptr(layout.i3), _ptr(w), _ld(w), order, _ptr(dy), _ld(dy), _ptr(out_scale),
                                                     _ptr(dout), dim, _ptr(g2), _ptr(dh), dim, _ptr(dw_part), _ld(dw), _ptr(ws), ws.numel() * 4,
                                                     n_edges, dim, _stream()), 'ihg_interact_bwd_gathered')
        dh = _member_gradients(h, layout, order, None if node_weight else dw, True, launch)
        if keep_dout:
            return dh, node_segment_sum_raw(dout, layout.node_csr, role='k7.first_order_gradient')
        if user_sums:                                        # the query and item rows (member_csr_qi keeps their list on the layout) into the same [N, d]
            return dh, _two_hop_first_order_gradient(dy, layout, out_scale, rows=layout.member_csr_qi()[1], out=dp)
        return dh, _two_hop_first_order_gradient(dy, layout, out_scale)
    two_hop_first = n_edges * dim * 4 > FIRST_ORDER_TWO_HOP_BYTES
    inv = None
    if (COTANGENT_PLANES and node_weight and two_hop_first and dy.data_ptr() % 16 == 0 and bool(lib.ihg_edge_gather_sum_planes_supported(dim, _ld(dy)))
            and bool(lib.ihg_interact_bwd_user_reduced_planes_supported(dim, order, _ld(h)))):
        # only the member-gradient kernel reads the hyperedges' cotangents here: K5 writes them as that kernel's operand (same bytes per row), scaled and split once
        # instead of once per column part of the kernel
        dout = torch.empty(n_edges, dim, dtype=torch.float32, device=h.device)
        if _user_reduced_ok(h, w, dout, layout, order):
            inv = torch.empty(n_edges, dtype=torch.float32, device=h.device)
            with profiler.kernel('edge_gather_sum', n_edges, dim):
                _lib.check(lib.ihg_edge_gather_sum_planes(_ptr(dy), _ld(dy), _ptr(layout.i3), _ptr(out_scale), _ptr(layout.edge_weight), _ptr(dout), _ptr(inv), n_edges,
                                                          dim, _stream()), 'ihg_edge_gather_sum_planes')
        else:
            del dout
    if inv is None:
        dout = edge_gather_sum_raw(dy, layout.i3, out_scale, None, 1.0, edge_scale=layout.edge_weight)      # (x m_e: the cotangent of all copies of the row)
    if two_hop_first:
        # a [E, d] table far beyond the caches (config C5: 51 GB): its scatter reads HBM at random, the two-hop operator on the node-level
        # cotangent (10 GB) gathers twice the rows and is still the shorter launch (22 against 32 ms)
        dp = _two_hop_first_order_gradient(dy, layout, out_scale)
    else:
        # the scatter of dout goes first: K5 has just written it, so most of its rows are still in the Infinity Cache for these random
        # reads; the interact kernels read it as a stream and do not care
        dp = node_segment_sum_raw(dout, layout.node_csr, role='k7.first_order_gradient')
    dh = _interact_backward(h, w, dout, layout, order, None if node_weight else dw, inv_scale=inv)
    return dh, dp


class _Interact(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h: Tensor, p: Tensor, w: Tensor, layout: IncidenceLayout, order: int) -> Tensor:
        h, p, w = _rows(h, 'h'), _rows(p, 'p'), _rows(w, 'w')
        ctx.save_for_backward(h, w)
        ctx.layout, ctx.order = layout, order
        return _interact_rows(h, p, w, layout, order)

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        h, w = ctx.saved_tensors
        grad_out, dw = _rows(grad_out, 'grad_out'), torch.zeros_like(w)
        dh = _interact_backward(h, w, grad_out, ctx.layout, ctx.order, dw)
        dp = node_segment_sum_raw(grad_out, ctx.layout.node_csr, role='k7.first_order_gradient')
        return dh, dp, dw, None, None


def interact(h: Tensor, p: Tensor, w: Tensor, layout: IncidenceLayout, order: int) -> Tensor:
    """Interactive node -> hyperedge step: first-order part from ``p`` (hoisted), products contracted with ``w``."""
    if order not in (2, 3):
        raise ValueError('interact handles interaction orders 2 and 3; order 1 is edge_gather_sum on the hoisted features')
    return _Interact.apply(h, p, w, layout, int(order))


class _InteractToNodes(torch.autograd.Function):
    """Interactive node -> hyperedge step and the hyperedge -> node pass behind it (``GnnLayers.py:229-236``) as ONE autograd node:
    ``y = out_scale * H interact(h, p, w)``.  Forward: the two kernels of the separate ops.  Backward: ``_interact_to_nodes_backward``, the
    interactive layer's own (without pair sums)."""

    @staticmethod
    def forward(ctx, h: Tensor, p: Tensor, w: Tensor, layout: IncidenceLayout, order: int, out_scale: Optional[Tensor], rows: Optional[Tensor],
                out: Optional[Tensor]) -> Tensor:
        h, p, w = _rows(h, 'h'), _rows(p, 'p'), _rows(w, 'w')
        _check_out(out, h, p, w)
        ctx.save_for_backward(h, w)
        ctx.layout, ctx.order, ctx.out_scale = layout, order, out_scale
        return _edges_to_nodes(_interact_rows(h, p, w, layout, order), layout, out_scale, rows, out)

    @staticmethod
    def backward(ctx, dy: Tensor):
        h, w = ctx.saved_tensors
        dy, dw = _rows(dy, 'dy'), torch.zeros_like(w)
        dh, dp = _interact_to_nodes_backward(h, w, dy, ctx.layout, ctx.order, ctx.out_scale, dw)
        return dh, dp, dw, None, None, None, None, None


def interact_to_nodes(h: Tensor, p: Tensor, w: Tensor, layout: IncidenceLayout, order: int, out_scale: Optional[Tensor] = None,
                      rows: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``node_segment_sum(interact(h, p, w, layout, order), layout, out_scale, rows)`` with a backward that has no node -> hyperedge launch."""
    if order not in (2, 3):
        raise ValueError('interact_to_nodes handles interaction orders 2 and 3')
    return _InteractToNodes.apply(h, p, w, layout, int(order), out_scale, rows, out)


class _InteractLayer(torch.autograd.Function):
    """The whole interactive layer behind ``feature_transform`` as ONE autograd node (``CommonLayers.py:70-85`` + ``GnnLayers.py:229-236``): hoisted first-order blocks
    (typed row GEMM) -> product blocks (``ihg_interact_fwd``) -> hyperedge -> node pass, or the node-level form (pair sums + ``ihg_node_interact_fwd``).  Backward:
    ``_interact_to_nodes_backward``, then the first-order epilogue, which ADDS its input gradient onto ``d h``; both halves of ``d aggregation.weight`` land in one tensor."""

    @staticmethod
    def forward(ctx, h: Tensor, w: Tensor, bias: Optional[Tensor], layout: IncidenceLayout, order: int, out_scale: Optional[Tensor], rows: Optional[Tensor],
                out: Optional[Tensor]) -> Tensor:
        lib = _lib.load()
        h, w = _rows(h, 'h'), _rows(w, 'w')
        dim = int(h.shape[1])
        _check_out(out, h, w, bias)
        ctx.layout, ctx.order, ctx.out_scale, ctx.has_bias = layout, order, out_scale, bias is not None
        if NODE_LEVEL_FORWARD and rows is None and _node_level_forward_ok(h, w, bias, out, dim, order):
            # no hyperedge rows: sums over each node's other members, then a node-level contraction (ihg_node_interact_fwd)
            sums = node_pair_sums_raw(h, layout)
            ctx.save_for_backward(h, w, sums)                  # the pair sums: the backward's node-level weight gradients read them again
            y = out if out is not None else torch.empty(layout.node_count, dim, dtype=torch.float32, device=h.device)
            ws = _workspace(int(lib.ihg_node_interact_fwd_workspace_bytes(dim)), h.device)
            with profiler.kernel('node_interact_fwd', layout.node_count, dim):
                _lib.check(lib.ihg_node_interact_fwd(_ptr(h), _ld(h), _ptr(sums), _ld(sums), _ptr(layout.self_weight), _ptr(out_scale), _ptr(bias), _ptr(w), _ld(w),
                                                     order, _type_begin(layout), _ptr(y), _ld(y), _ptr(ws), ws.numel() * 4, dim, _stream()),
                           'ihg_node_interact_fwd')
            return y
        ctx.save_for_backward(h, w)
        p = _first_order_rows(h, w, bias, layout)
        return _edges_to_nodes(_interact_rows(h, p, w, layout, order), layout, out_scale, rows, out)

    @staticmethod
    def backward(ctx, dy: Tensor):
        h, w = ctx.saved_tensors[:2]
        sums = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        dw = torch.empty_like(w)                               # product blocks from the interact kernels, first-order blocks from the row-GEMM pass
        dh, dp = _interact_to_nodes_backward(h, w, _rows(dy, 'dy'), ctx.layout, ctx.order, ctx.out_scale, dw, sums)
        dbias = _first_order_backward(dp, h, w, ctx.layout, dw, dh, ctx.has_bias)
        return dh, dw, dbias, None, None, None, None, None


def interact_layer(h: Tensor, w: Tensor, bias: Optional[Tensor], layout: IncidenceLayout, order: int, out_scale: Optional[Tensor] = None,
                   rows: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``out_scale * H FeatureInteractor(h)`` for interaction orders 2 / 3 with ``w = [A_u | A_q | A_i | W_uq | W_qi | W_iu (| W_uqi)]`` and
    ``bias`` = the aggregation's bias: ``node_segment_sum(interact(h, first_order(h), w), out_scale, rows)`` as one differentiable op."""
    if order not in (2, 3):
        raise ValueError('interact_layer handles interaction orders 2 and 3')
    dim, wide = int(h.shape[1]), padded_width(int(h.shape[1]))
    if wide != dim and int(w.shape[0]) == dim and h.is_cuda:
        # a width between the tiled ones: the same layer at the next tiled width on zero-padded operands (the padding columns of the result are exactly zero and are cut off)
        _check_out(out, h, w, bias)
        y = _InteractLayer.apply(pad_columns(h, wide), pad_blocks(w, wide), pad_vector(bias, wide), layout, int(order), out_scale, rows, None)[:, :dim]
        return y if out is None else out.copy_(y)
    return _InteractLayer.apply(h, w, bias, layout, int(order), out_scale, rows, out)


# ---------------------------------------------------------------------------------------------
# Batch tail: HEM scores of a training batch straight from the layer outputs
# ---------------------------------------------------------------------------------------------
def _tail_shape(layers, tables):
    """``(n_layers, dim, width)`` of a batch tail over the matrices ``layers``, below them layer 0 in the embedding tables (``tables``, optional); ``width = n_layers * dim``."""
    n_layers = len(layers) + (1 if tables is not None else 0)
    dim = int(layers[0].shape[1]) if layers else tables.dim
    return n_layers, dim, n_layers * dim


def _hem_operands(layers, tables, dim: int):
    """``(layers, (layer0_rows, ld0, type_begin))`` of the HEM entry points: plain matrices, or layer 0 as the embedding tables in place."""
    if tables is None:
        return (ctypes.c_void_p * len(layers))(*[x.data_ptr() for x in layers]), (None, 0, None)
    ptrs = (ctypes.c_void_p * (len(layers) + 1))(tables.query_rows.data_ptr(), *[x.data_ptr() for x in layers])     # (slot 0 is replaced by the typed rows)
    return ptrs, (tables.row_pointers(), dim, tables.type_begin())


def _hem_forward(layers, tables, rows: Tensor, rows_upper: Optional[Tensor], items: Tensor, bias: Tensor, lam: float, cosine: bool, scores: Tensor) -> Optional[Tensor]:
    """The scores of a batch into ``scores`` (the caller names the launch to the profiler).  The cosine head returns the rows' ``[B, 4]`` stats (``a . m``, ``||a||^2``, ``||m||^2``, 0:
    include/ihgnn_hip.h) for the backward, the dot product ``None``.  One entry point per head for plain matrices, the embedding tables in place (``tables``) and a layout's own
    numbering above layer 0 (``rows_upper``)."""
    lib = _lib.load()
    batch = int(items.shape[0])
    n_layers, dim, _ = _tail_shape(layers, tables)
    ptrs, typed0 = _hem_operands(layers, tables, dim)
    args = (ptrs, n_layers, _ld(layers[0]) if layers else dim, dim, *typed0, _ptr(rows), _ptr(rows_upper), _ptr(items), _ptr(bias), float(lam), _ptr(scores))
    if not cosine:
        _lib.check(lib.ihg_hem_score_fwd_typed0(*args, batch, _stream()), 'ihg_hem_score_fwd_typed0')
        return None
    stats = torch.empty(batch, 4, dtype=torch.float32, device=bias.device)
    _lib.check(lib.ihg_hem_cosine_fwd(*args, _ptr(stats), batch, _stream()), 'ihg_hem_cosine_fwd')
    return stats


def _hem_row_gradients(layers, rows: Tensor, items: Tensor, bias: Tensor, lam: float, dscores: Tensor, grad_scale: float, tables=None, grad_scale_device=None, rows_upper=None,
                       stats: Optional[Tensor] = None):
    """Per-batch-row gradients of the tail: ``[3B, (L+1) d + 4]``, layer l in columns ``l d .. (l+1) d``, d bias in column ``(L+1) d``.  ``tables`` (a resolved
    ``NodeTables``): layer 0 is read from the embedding tables in place and ``layers`` are the outputs of the layers above it.  ``stats`` (``[B, 4]``, left by the
    cosine head's forward): the cosine head's row gradients, same layout."""
    lib = _lib.load()
    batch = int(items.shape[0])
    n_layers, dim, width = _tail_shape(layers, tables)
    rowgrad = torch.empty(3 * batch, width + 4, dtype=torch.float32, device=bias.device)
    if grad_scale_device is not None and (grad_scale_device.dtype != torch.float32 or grad_scale_device.numel() != 1):
        raise TypeError('grad_scale_device is a float32 device scalar')
    ptrs, typed0 = _hem_operands(layers, tables, dim)
    args = (ptrs, n_layers, _ld(layers[0]) if layers else dim, dim, *typed0, _ptr(rows), _ptr(rows_upper), _ptr(dscores))
    out = (_ptr(grad_scale_device), float(grad_scale), float(lam), _ptr(rowgrad), width + 4, batch, _stream())
    with profiler.kernel('hem_score_bwd' if stats is None else 'hem_cosine_bwd', batch, dim):
        if stats is None:
            _lib.check(lib.ihg_hem_score_bwd_typed0(*args, *out), 'ihg_hem_score_bwd_typed0')
        else:
            _lib.check(lib.ihg_hem_cosine_bwd(*args, _ptr(stats), *out), 'ihg_hem_cosine_bwd')
    return rowgrad


SCATTER_CHUNK_ROWS = 32768          # rows one ihg_batch_scatter_add / ihg_batch_combine launch takes (= ihg_batch_scatter_max_rows(): its id list lives in LDS; tests/test_abi.py)


def _scatter_rows(rowgrad: Tensor, col0: int, width: int, rows: Tensor, dense: Optional[Tensor], tail: Optional[Tensor] = None, tail_offset: int = 0, block_stride: int = 0):
    """``dense[rows[k]] += rowgrad[k, col0 : col0 + width]`` (duplicates combined in a fixed order; deterministic).  With
    ``tail``: the LAST of the ``width`` columns goes to ``tail[rows[k] - tail_offset]`` instead.  With ``block_stride``: ``dense`` is the first of several
    matrices, ``block_stride`` floats apart, and every further ``dense.shape[1]`` columns land in the next of them.  Batches beyond one launch's
    capacity go through in row chunks, in order (same sums, associated chunk by chunk)."""
    lib = _lib.load()
    n = int(rows.shape[0])
    target = dense if dense is not None else tail
    block = int(dense.shape[1]) if dense is not None else 1
    for lo in range(0, n, SCATTER_CHUNK_ROWS):
        hi = min(lo + SCATTER_CHUNK_ROWS, n)
        src = rowgrad[lo:hi, col0:]
        with profiler.kernel('batch_scatter_add', hi - lo, width):
            _lib.check(lib.ihg_batch_scatter_add(_ptr(src), int(rowgrad.stride(0)), width, _ptr(rows[lo:hi]), hi - lo, _ptr(target),
                                                 _ld(target) if dense is not None else 1, block, int(block_stride), _ptr(tail), int(tail_offset),
                                                 int(tail.shape[0]) if tail is not None else 0, _stream()), 'ihg_batch_scatter_add')


def _combine_rows(rowgrad: Tensor, rows: Tensor, width: int) -> Optional[Tensor]:
    """Sums the rows of ``rowgrad[:, 0 : width + 1]`` (the layers' columns and d bias) that share a destination into the first of them, in place; -> ``leader`` (int32, 1 on those
    first occurrences), or ``None`` (nothing done) beyond one launch's capacity.  ``rows`` = users | queries | items: its thirds share no destination."""
    lib = _lib.load()
    n = int(rows.shape[0])
    if lib.ihg_batch_scatter_workspace_bytes(n) < 0:
        return None
    leader = torch.empty(n, dtype=torch.int32, device=rows.device)
    with profiler.kernel('batch_combine', n, width + 1):
        _lib.check(lib.ihg_batch_combine(_ptr(rowgrad), int(rowgrad.stride(0)), width + 1, _ptr(rows), n, n // 3, _ptr(leader), _stream()), 'ihg_batch_combine')
    return leader


def _hem_backward(layers, rows: Tensor, items: Tensor, bias: Tensor, lam: float, dscores: Tensor, grad_scale: float, item_row_offset: int, stats: Optional[Tensor] = None):
    """Backward of the batch tail without taps: per-row gradients (one kernel), then ONE deterministic scatter that lands every
    layer's gradient in its own contiguous ``[N, d]`` matrix and d bias beside them.  -> (d bias, layer gradients)."""
    n_layers, dim, width = _tail_shape(layers, None)
    n_nodes = int(layers[0].shape[0])
    rowgrad = _hem_row_gradients(layers, rows, items, bias, lam, dscores, grad_scale, stats=stats)
    flat = torch.zeros(n_layers * n_nodes * dim + int(bias.shape[0]), dtype=torch.float32, device=bias.device)
    dense = flat[:n_layers * n_nodes * dim].view(n_layers * n_nodes, dim)
    dbias = flat[n_layers * n_nodes * dim:]
    _scatter_rows(rowgrad, 0, width + 1, rows, dense, dbias, item_row_offset, block_stride=n_nodes * dim)      # one launch lands every layer's block and the bias column
    return dbias, tuple(dense[l * n_nodes:(l + 1) * n_nodes] for l in range(n_layers))


class TailGradients:
    """Side channel from the batch tail's backward to the taps on the layer outputs (one per training step).

    A layer output ``X_l`` feeds the next layer AND the batch tail; the tail's gradient for it has 3B non-zero rows out of N.
    Handing autograd a dense ``[N, d]`` tensor per layer costs a zero fill plus one full add per layer; instead the tail's
    backward leaves its ``[3B, .]`` row gradients here and every ``tap`` adds its own columns into the gradient that came
    down from the next layer, in place."""

    def __init__(self, exchange=None, grad_scale: float = 1.0):
        self.rows: Optional[Tensor] = None
        self.rowgrad: Optional[Tensor] = None      # [3B, .], rows of equal destination already summed into their first occurrence
        self.leader: Optional[Tensor] = None       # int32 [3B]: 1 on those first occurrences (None: rowgrad is not combined)
        # data parallel, cotangent exchange (ihgnn_amd.distributed.CotangentSync): ``exchange(rows, rowgrad) -> (rows, rowgrad)`` of ALL ranks' batches, called by the
        # batch tail's backward between its row-gradient kernel and the combine; ``grad_scale`` = 1 / world size (the average over ranks) applied by that kernel
        self.exchange = exchange
        self.grad_scale = float(grad_scale)
        # a layout that numbers its nodes without the isolated ones (IncidenceLayout.node_map): layer 0 is addressed by the public rows (``rows``), the layers above by
        # ``rows_upper`` = row_map[rows] (-1: an isolated node, whose rows above layer 0 are zero constants - the add / put kernels skip it)
        self.row_map: Optional[Tensor] = None
        self.rows_upper: Optional[Tensor] = None

    def _rows_of(self, upper: bool) -> Tensor:
        return self.rows_upper if (upper and self.rows_upper is not None) else self.rows

    def put_into_typed(self, dense_rows, ld_dense: int, layout, col0: int, width: int, type_begin=None) -> None:
        """``add_into`` for a destination whose node types start at their own addresses (``dense_rows``: host array of three device pointers; ``type_begin``: the first row
        of every type in the destination's numbering when that is not the layout's - the embedding tables under a layout without the isolated nodes)."""
        _put_rows(self, dense_rows, ld_dense, layout, col0, width, False, False, type_begin)

    def assign_into(self, dense: Tensor, layout, col0: int, width: int, upper: bool = False) -> None:
        """``dense[rows[k]] = rowgrad[k, col0 : col0 + width]`` on the (combined) batch rows, nothing else written: a gradient that is zero outside the batch rows
        and READ at those rows only (the last layer's cotangent under the sparse pull) needs no ``[N, d]`` zero fill."""
        base = dense.data_ptr()
        tb = _type_begin(layout)
        step = _ld(dense) * 4
        _put_rows(self, (ctypes.c_void_p * 3)(base + tb[0] * step, base + tb[1] * step, base + tb[2] * step), _ld(dense), layout, col0, width, True, upper)

    def add_into(self, dense: Optional[Tensor], col0: int, width: int, tail: Optional[Tensor] = None, tail_offset: int = 0, upper: bool = False) -> None:
        """``dense[rows[k]] += rowgrad[k, col0 : col0 + width]`` (or ``tail[rows[k] - tail_offset] += rowgrad[k, col0]``); ``upper``: the destination is a layer above layer 0
        (addressed by ``rows_upper`` where the layout's numbering differs from the public one)."""
        rows = self._rows_of(upper)
        if self.leader is None:
            # (beyond one combine launch: the scatter in row chunks; a negative row - an isolated node above layer 0, a rank's own non-leader duplicate after the
            #  exchange - is skipped by the kernel like every other row that takes no part)
            _scatter_rows(self.rowgrad, col0, width, rows, dense, tail, tail_offset)
            return
        lib = _lib.load()
        n = int(rows.shape[0])
        src = self.rowgrad[:, col0:]
        with profiler.kernel('batch_rows_add', n, width):
            _lib.check(lib.ihg_batch_rows_add(_ptr(src), int(self.rowgrad.stride(0)), width, _ptr(rows), _ptr(self.leader), n, _ptr(dense),
                                              _ld(dense) if dense is not None else 0, _ptr(tail), int(tail_offset),
                                              int(tail.shape[0]) if tail is not None else 0, _stream()), 'ihg_batch_rows_add')


def _put_rows(holder: 'TailGradients', dense_rows, ld_dense: int, layout, col0: int, width: int, assign: bool, upper: bool = False, type_begin=None) -> None:
    lib = _lib.load()
    if holder.leader is None:
        raise _lib.IhgnnHipError('typed / assigning row scatter needs the combined row gradients (batches of at most 32,768 rows)')
    rows = holder._rows_of(upper)
    n = int(rows.shape[0])
    src = holder.rowgrad[:, col0:]
    with profiler.kernel('batch_rows_add', n, width):
        _lib.check(lib.ihg_batch_rows_put(_ptr(src), int(holder.rowgrad.stride(0)), width, _ptr(rows), _ptr(holder.leader), n, dense_rows, ld_dense,
                                          type_begin if type_begin is not None else _type_begin(layout), 1 if assign else 0, _stream()), 'ihg_batch_rows_put')


class _Tap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, holder: TailGradients, index: int, sparse_layout):
        ctx.holder, ctx.index, ctx.sparse_layout = holder, int(index), sparse_layout
        ctx.shape, ctx.device = tuple(x.shape), x.device
        ctx.set_materialize_grads(False)
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, g_next: Optional[Tensor], g_tail: Optional[Tensor]):
        holder, (n, dim) = ctx.holder, ctx.shape
        if holder.rowgrad is None:                           # the tail did not run a backward through this holder
            if g_next is None or g_tail is None:
                return (g_next if g_next is not None else g_tail), None, None, None
            return g_next + g_tail, None, None, None
        if g_next is None:
            # the last layer's output feeds the batch tail only: its cotangent is zero outside the batch rows (RawGnn tells that layer so)
            if ctx.sparse_layout is not None and holder.leader is not None:
                # ... and that layer's backward READS it at those rows only (the masked pull of node_two_hop): the rows are written, nothing is filled
                g = torch.empty(n, dim, dtype=torch.float32, device=ctx.device)
                if ctx.index > 0 and holder.rows_upper is not None:
                    # (a layout without the isolated nodes lists row 0 in place of every isolated batch node - RawGnn.propagate_layers -: the pull reads that row, so it
                    #  holds zeros unless it is a batch row itself, in which case the assignment below overwrites it)
                    _lib.check(_lib.load().ihg_zero_floats(_ptr(g), dim, _stream()), 'ihg_zero_floats')
                holder.assign_into(g, ctx.sparse_layout, ctx.index * dim, dim, upper=ctx.index > 0)
                return g, None, None, None
            g = torch.empty(n, dim, dtype=torch.float32, device=ctx.device)
            _lib.check(_lib.load().ihg_zero_floats(_ptr(g), n * dim, _stream()), 'ihg_zero_floats')
        else:
            g = g_next if (g_next.is_contiguous() and g_next.dtype == torch.float32) else g_next.contiguous().float()
        holder.add_into(g, ctx.index * dim, dim, upper=ctx.index > 0)
        return g, None, None, None


def tap(x: Tensor, holder: TailGradients, index: int, sparse_layout=None):
    """``(x for the next layer, x for the batch tail)``: same values; see ``TailGradients``.  ``sparse_layout`` (an ``IncidenceLayout``; only for an output that
    feeds NOTHING but the tail): the caller's promise that the backward of the op that produced ``x`` reads its cotangent at the batch rows only (the last layer
    under ``cotangent_rows`` / ``rows``) - the tap then writes those rows of an uninitialised ``[N, d]`` tensor instead of filling it with zeros first."""
    return _Tap.apply(x, holder, int(index), sparse_layout)


_ZERO_SCALARS = {}


def _zero_like_expanded(shape, device: torch.device) -> Tensor:
    """A zero tensor of ``shape`` that owns one element (stride 0): placeholder gradient, never read."""
    z = _ZERO_SCALARS.get(device)
    if z is None:
        z = _ZERO_SCALARS[device] = torch.zeros((), dtype=torch.float32, device=device)
    return z.expand(*shape)


def _same_layout(layers):
    layers = tuple(_rows(x, 'layer output') for x in layers)
    ld = _ld(layers[0])
    if any(_ld(x) != ld or x.shape[1] != layers[0].shape[1] for x in layers):
        layers = tuple(x.contiguous() for x in layers)
    return layers


class _HemScore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows: Tensor, items: Tensor, bias: Tensor, lam: float, item_row_offset: int, cosine: bool, *layers: Tensor) -> Tensor:
        layers = _same_layout(layers)
        batch, dim = int(items.shape[0]), int(layers[0].shape[1])
        scores = torch.empty(batch, dtype=torch.float32, device=bias.device)
        with profiler.kernel('hem_cosine_fwd' if cosine else 'hem_score_fwd', batch, dim):
            stats = _hem_forward(layers, None, rows, None, items, bias, lam, cosine, scores)
        ctx.save_for_backward(rows, items, bias, *layers)
        ctx.lam, ctx.offset, ctx.stats = float(lam), int(item_row_offset), stats
        return scores

    @staticmethod
    def backward(ctx, dscores: Tensor):
        rows, items, bias, *layers = ctx.saved_tensors
        dbias, grads = _hem_backward(layers, rows, items, bias, ctx.lam, dscores.contiguous(), 1.0, ctx.offset, ctx.stats)
        return (None, None, dbias, None, None, None) + grads


class _HemBceLoss(torch.autograd.Function):
    """Scores + mean BCE-with-logits in the forward; d loss / d scores is produced there too, so the backward starts at the
    per-row gradient kernel.  With a ``TailGradients`` holder the layer gradients leave through the taps (placeholders are
    returned here); without one they are returned dense."""

    @staticmethod
    def forward(ctx, rows: Tensor, items: Tensor, labels: Optional[Tensor], bias: Tensor, lam: float, item_row_offset: int, holder, tables, rows_upper, cosine: bool,
                objective: 'Objective', *layers: Tensor) -> Tensor:
        # objective: which loss launch follows the scores (``Objective.launch``: the one launch that differs); ``labels`` are read by the plain BCE only
        # tables (a resolved NodeTables): layer 0 is the embedding tables in place; layers[0] is then its token (the autograd edge), not a matrix
        # rows_upper (a layout without the isolated nodes): layer 0 is in the public numbering (rows), the layers above are in the layout's (rows_upper; -1: zero row)
        real = _same_layout(layers[1:] if tables is not None else layers)
        batch, dim = int(items.shape[0]), _tail_shape(real, tables)[1]
        scores = torch.empty(batch, dtype=torch.float32, device=bias.device)
        dscores = torch.empty(batch, dtype=torch.float32, device=bias.device)
        loss = torch.empty((), dtype=torch.float32, device=bias.device)
        if not objective.grouped:
            labels = labels.to(torch.float32).contiguous()
        with profiler.kernel('hem_cosine_fwd' if cosine else 'hem_score_fwd', batch, dim):
            stats = _hem_forward(real, tables, rows, rows_upper, items, bias, lam, cosine, scores)
            objective.launch(scores, labels, loss, dscores)
        ctx.save_for_backward(rows, items, bias, dscores, *real)
        ctx.rows_upper, ctx.stats = rows_upper, stats
        ctx.lam, ctx.offset, ctx.holder, ctx.tables = float(lam), int(item_row_offset), holder, tables
        ctx.token_shape = tuple(layers[0].shape) if tables is not None else None
        return loss

    @staticmethod
    def backward(ctx, grad_loss: Tensor):
        rows, items, bias, dscores, *layers = ctx.saved_tensors
        tables = ctx.tables
        if ctx.holder is None:
            if tables is not None or ctx.rows_upper is not None:
                raise _lib.IhgnnHipError('hem_bce_loss over NodeTables / a compact layout needs a TailGradients holder')
            dbias, grads = _hem_backward(layers, rows, items, bias, ctx.lam, dscores * grad_loss, 1.0, ctx.offset, ctx.stats)
            return (None, None, None, dbias, None, None, None, None, None, None, None) + grads
        holder = ctx.holder
        rowgrad = _hem_row_gradients(layers, rows, items, bias, ctx.lam, dscores, holder.grad_scale, tables, grad_loss.contiguous(), ctx.rows_upper, ctx.stats)     # d loss stays on the device: no host read, no multiply launch
        width = _tail_shape(layers, tables)[2]
        if holder.exchange is not None:
            # every rank's propagation is the same function of the same parameters and its backward is linear in the cotangent of the layer outputs, which is non-zero on
            # the batch rows only: the ranks exchange THOSE rows (3B x (D + 1) floats each) and every rank runs the one propagation backward on the union - the averaged
            # gradient of all parameters without a dense all-reduce (RawGnn.py:122-142: the batch reads F at 3B rows).
            # A rank's own duplicates are summed BEFORE the exchange (a batch repeats every positive's user and query with its ten negatives: ~ 1,300 of 3,300 rows are
            # first occurrences) and marked in a spare column of the row gradients, which travels with them: the union's combine then skips the other rows (and the
            # zero rows that pad a shorter batch) - its duplicate search is quadratic in the rows that take part
            own = _combine_rows(rowgrad, rows, width)
            rowgrad[:, width + 1] = own.to(torch.float32) if own is not None else 1.0
            rows, rowgrad = holder.exchange(rows, rowgrad)
            rows = torch.where(rowgrad[:, width + 1] > 0, rows, torch.full_like(rows, -1))
        holder.rows, holder.rowgrad = rows, rowgrad
        # (the union's rows after an exchange; this batch's otherwise - through the layout's map where it numbers its nodes without the isolated ones)
        if holder.row_map is None:
            holder.rows_upper = None
        elif holder.exchange is None and ctx.rows_upper is not None:
            holder.rows_upper = ctx.rows_upper
        else:
            mapped = holder.row_map[rows.clamp_min(0)]
            holder.rows_upper = torch.where(rows < 0, torch.full_like(mapped, -1), mapped)
        holder.leader = _combine_rows(rowgrad, rows, width)      # one pass sums duplicate destinations; the taps then add plain rows (None: beyond one launch - they scatter)
        dbias = torch.empty_like(bias)
        _lib.check(_lib.load().ihg_zero_floats(_ptr(dbias), dbias.numel(), _stream()), 'ihg_zero_floats')
        holder.add_into(None, width, 1, dbias, ctx.offset)
        placeholders = tuple(_zero_like_expanded(x.shape, x.device) for x in layers)
        if tables is not None:
            placeholders = (_zero_like_expanded(ctx.token_shape, bias.device),) + placeholders
        return (None, None, None, dbias, None, None, None, None, None, None, None) + placeholders


def score_topk_max_width() -> int:
    """The widest feature row ``ihg_score_topk`` scores (1264): asked of the library, the one place that knows its LDS budget."""
    return int(_lib.load().ihg_score_topk_max_dim())


def _scored_matrix(features: Tensor, width: int) -> bool:
    """Float32 GPU rows of any width up to ``width``, any row stride: the feature matrix the ranking entry points take."""
    return (features.is_cuda and features.dtype == torch.float32 and features.dim() == 2 and features.stride(1) == 1 and 0 < features.shape[1] <= width
            and (features.shape[0] <= 1 or features.stride(0) >= features.shape[1]))


def score_topk_supported(features: Tensor) -> bool:
    """True when ``ihg_score_topk`` takes this feature matrix: float32 GPU rows of any width up to ``score_topk_max_width()`` (any row stride)."""
    return _scored_matrix(features, score_topk_max_width())


# The four public ranking functions below are these helpers and one library call each.
def _rank_features(entry: str, features: Tensor, item_row0: int, item_bias: Tensor, width: int):
    """The feature-matrix test of ``entry`` -> ``(n_items, dim, bias)``."""
    if not _scored_matrix(features, width):
        raise _lib.IhgnnHipError(f'{entry} needs a float32 GPU feature matrix of width <= {width}, got {tuple(features.shape)} {features.dtype} on {features.device}')
    return int(features.shape[0]) - int(item_row0), int(features.shape[1]), item_bias.detach().to(torch.float32).contiguous()


def _rank_pairs(what: Optional[str], features: Tensor, users: Tensor, queries: Optional[Tensor], query_rows: Optional[Tensor] = None):
    """The pair sources on the features' device -> ``(users, queries, query_rows, ld_q, q_dim, n_pairs)``.  ``what`` names a search function: exactly one of
    ``queries`` / ``query_rows``, one per user."""
    if what is not None and (queries is None) == (query_rows is None):
        raise ValueError(f'{what}: give exactly one of queries and query_rows')
    n_pairs = int(users.shape[0])
    users = users.to(device=features.device, dtype=torch.int64).contiguous()
    ld_q = q_dim = 0
    if queries is not None:
        queries = queries.to(device=features.device, dtype=torch.int64).contiguous()
        source = int(queries.shape[0])
    else:
        query_rows = _rows(query_rows, 'query_rows')
        source, q_dim, ld_q = int(query_rows.shape[0]), int(query_rows.shape[1]), _ld(query_rows)
    if what is not None and source != n_pairs:
        raise ValueError(f'{what}: {n_pairs} users but {source} queries')
    return users, queries, query_rows, ld_q, q_dim, n_pairs


def _rank_outputs(n_pairs: int, depth: int, device):
    """``(top_items [C, depth] int32, top_scores [C, depth], passes [C] int32)``, uninitialised."""
    return (torch.empty(n_pairs, depth, dtype=torch.int32, device=device), torch.empty(n_pairs, depth, dtype=torch.float32, device=device),
            torch.empty(n_pairs, dtype=torch.int32, device=device))


def _search_lists(what: str, lists, rows: Optional[Tensor], build, noun: str, rows_name: str, n_pairs: int, n_items: int, device, need_a_run: bool = False):
    """Per-search lists as the entry points read them -> ``(ptr, ids, rows, n_runs, total)`` on ``device``.  ``lists = (ptr, items)``: int32 items are taken as
    ``build`` (``exclusion_lists`` / ``candidate_lists``) returned them, any other integer type goes through it first.  ``rows`` (the ``rows_name=`` keyword) maps
    searches to runs; without it there is one run per search.  An empty id tensor has no address, and a null list means "no lists": it becomes a one-entry dummy that
    no offset reaches (``total`` stays 0)."""
    ptr, ids = lists
    if ids.dtype != torch.int32:
        ptr, ids = build(ptr, ids, n_items)
    ptr = ptr.reshape(-1).to(device=device, dtype=torch.int64).contiguous()
    ids = ids.reshape(-1).to(device=device).contiguous()
    n_runs, total = int(ptr.shape[0]) - 1, int(ids.shape[0])
    if need_a_run and n_runs < 1 and n_pairs > 0:
        raise ValueError(f'{what}: the offsets hold at least one run')
    if rows is not None:
        if rows.dim() != 1 or int(rows.shape[0]) != n_pairs:
            raise ValueError(f'{what}: {n_pairs} searches but {rows_name} of {tuple(rows.shape)}')
        rows = rows.to(device=device, dtype=torch.int64).contiguous()
    elif n_runs != n_pairs:
        raise ValueError(f'{what}: {n_pairs} searches but {n_runs} {noun} lists ({rows_name}= maps searches to shared lists)')
    return ptr, (ids if total else ids.new_zeros(1)), rows, n_runs, total


def score_topk(features: Tensor, users: Tensor, queries: Tensor, query_row0: int, item_row0: int, item_bias: Tensor, lam: float, k: int = 10, cosine: bool = False):
    """Evaluation scoring: for every (user, query) pair the ``k`` best items over ALL items and their HEM scores,
    ``(top_items [C, k] int32, top_scores [C, k])``, best first, ties in ascending item order; the ``[C, I]`` score matrix is
    never materialised.  ``features`` = the cached ``[N, D]`` propagation output (any width up to ``score_topk_max_width()``); items are its rows from ``item_row0`` on.
    ``cosine``: the cosine-similarity head (``Gs.Prediction.use_cosine_similarity``) - same kernels, the rows' inverse norms folded into their scale factors.
    ``k`` > 10 goes to ``score_topk_deep`` (up to ``score_topk_max_k()``)."""
    if k > 10:
        return score_topk_deep(features, users, queries, query_row0, item_row0, item_bias, lam, k, cosine=cosine)[:2]
    lib = _lib.load()
    n_items, dim, bias = _rank_features('ihg_score_topk', features, item_row0, item_bias, score_topk_max_width())
    users, queries, _, _, _, n_pairs = _rank_pairs(None, features, users, queries)
    top_items, top_scores, _ = _rank_outputs(n_pairs, k, features.device)
    ws = _workspace(int(lib.ihg_score_topk_workspace_bytes(n_pairs, n_items, dim)), features.device)
    name = 'score_topk_cosine' if cosine else 'score_topk'
    with profiler.kernel(name, n_pairs, dim):
        _lib.check(getattr(lib, 'ihg_' + name)(_ptr(features), _ld(features), dim, int(query_row0), int(item_row0), n_items, _ptr(bias),
                                               _ptr(users), _ptr(queries), float(lam), n_pairs, int(k), _ptr(top_scores), _ptr(top_items), _ptr(ws),
                                               ws.numel() * 4, _stream()), 'ihg_' + name)
    return top_items, top_scores


def score_topk_max_k() -> int:
    """The deepest ranking ``ihg_score_topk_deep`` returns (128)."""
    return int(_lib.load().ihg_score_topk_max_k())


def score_topk_deep(features: Tensor, users: Tensor, queries: Tensor, query_row0: int, item_row0: int, item_bias: Tensor, lam: float, k: int, cosine: bool = False):
    """``score_topk`` for any ``1 <= k <= score_topk_max_k()``: ``(top_items [C, k] int32, top_scores [C, k], passes [C] int32)``.  The kernels keep their lists of ten
    and the call runs in passes that each rank at least ten more items of every pair that is not complete yet (``include/ihgnn_hip.h`` has the scheme);
    ``passes[c]`` = the passes that found pair ``c`` incomplete, at most ``ceil(min(k, I) / 10)``.  Exact, with the tie order and the ``-1`` tail of ``score_topk``."""
    lib = _lib.load()
    n_items, dim, bias = _rank_features('ihg_score_topk_deep', features, item_row0, item_bias, score_topk_max_width())
    users, queries, _, _, _, n_pairs = _rank_pairs(None, features, users, queries)
    top_items, top_scores, passes = _rank_outputs(n_pairs, max(int(k), 0), features.device)
    ws = _workspace(int(lib.ihg_score_topk_deep_workspace_bytes(n_pairs, n_items, dim, int(k))), features.device)
    with profiler.kernel('score_topk_deep_cosine' if cosine else 'score_topk_deep', n_pairs, dim):
        _lib.check(lib.ihg_score_topk_deep(_ptr(features), _ld(features), dim, int(query_row0), int(item_row0), n_items, _ptr(bias), _ptr(users), _ptr(queries), float(lam),
                                           n_pairs, int(k), _ptr(top_scores), _ptr(top_items), _ptr(ws), ws.numel() * 4, int(bool(cosine)), _ptr(passes), _stream()),
                   'ihg_score_topk_deep')
    return top_items, top_scores, passes


def pack_item_mask(candidates: Tensor, n_items: int) -> Tensor:
    """The candidate filter as ``ihg_search_topk`` reads it: ``ceil(n_items / 32)`` words (int32 holding the uint32 bits) on the device of ``candidates``, bit
    ``i % 32`` of word ``i // 32`` set where item ``i`` is a candidate.  ``candidates`` is a bool ``[n_items]`` tensor or an int64 tensor of item ids (in any order,
    repeats allowed; in ``[0, n_items)`` - the caller's to check where they live on the device).  Torch ops only: no host read."""
    n_items = int(n_items)
    if candidates.dtype == torch.bool:
        if candidates.dim() != 1 or int(candidates.shape[0]) != n_items:
            raise ValueError(f'a candidate mask is a bool tensor of [{n_items}], got {tuple(candidates.shape)}')
        flags = candidates
    elif candidates.dtype in (torch.int64, torch.int32):
        ids = candidates.reshape(-1).to(torch.int64)
        if not ids.is_cuda and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_items):
            raise ValueError(f'candidate item id outside [0, {n_items})')
        flags = torch.zeros(n_items, dtype=torch.bool, device=ids.device).index_fill_(0, ids, True)
    else:
        raise TypeError(f'candidates: a bool mask or integer item ids, got {candidates.dtype}')
    n_words = (n_items + 31) // 32
    bits = torch.zeros(n_words * 32, dtype=torch.int64, device=flags.device)
    bits[:n_items] = flags.to(torch.int64)
    words = (bits.view(n_words, 32) << torch.arange(32, dtype=torch.int64, device=flags.device)).sum(1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def _sorted_unique_lists(what: str, which: str, offsets: Tensor, items: Tensor, n_items: int) -> Tuple[Tensor, Tensor]:
    """The one-sort construction behind ``exclusion_lists`` and ``candidate_lists``: one sort of the keys ``row * n_items + id`` orders every run and brings repeats
    together; the new offsets are a search for each row's first key.  ``what`` / ``which`` only word the messages."""
    n_items = int(n_items)
    offsets = offsets.reshape(-1).to(torch.int64)
    ids = items.reshape(-1).to(device=offsets.device, dtype=torch.int64)
    if offsets.numel() < 1:
        raise ValueError(f'{what}: offsets holds at least the leading 0')
    n_rows = int(offsets.shape[0]) - 1
    if not offsets.is_cuda:
        if int(offsets[0]) != 0 or int(offsets[-1]) != ids.numel() or bool((offsets[1:] < offsets[:-1]).any()):
            raise ValueError(f'{what}: offsets run from 0 to the {ids.numel()} ids without decreasing')
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_items):
            raise ValueError(f'{which} item id outside [0, {n_items})')
    rows = torch.repeat_interleave(torch.arange(n_rows, dtype=torch.int64, device=offsets.device), offsets[1:] - offsets[:-1], output_size=int(ids.shape[0]))
    keys = torch.unique(rows * n_items + ids)                               # (sorted)
    ptr = torch.searchsorted(keys, torch.arange(n_rows + 1, dtype=torch.int64, device=offsets.device) * n_items)
    return ptr, (keys % n_items).to(torch.int32)


def exclusion_lists(offsets: Tensor, items: Tensor, n_items: int) -> Tuple[Tensor, Tensor]:
    """Per-row item lists as ``ihg_search_topk_excluding`` reads them: ``(ptr int64 [R + 1], items int32)`` with every run strictly ascending.  Input: ``offsets``
    ``[R + 1]`` (non-decreasing, from 0 to ``len(items)``) and the flat ids of the rows, in any order, repeats allowed, in ``[0, n_items)``.  One sort of the keys
    ``row * n_items + id`` orders every run and brings repeats together; the new offsets are a search for each row's first key.  Torch ops on the tensors' own
    device, so it serves host tensors as well; the range of host tensors is checked here, that of device tensors is the caller's."""
    return _sorted_unique_lists('exclusion_lists', 'excluded', offsets, items, n_items)


def candidate_lists(offsets: Tensor, items: Tensor, n_items: int) -> Tuple[Tensor, Tensor]:
    """Per-search shortlists as ``ihg_search_candidates`` reads them: ``(ptr int64 [R + 1], items int32)`` with every run strictly ascending and free of repeats, from
    raw lists (``offsets`` ``[R + 1]`` and the flat ids, in any order, repeats allowed, in ``[0, n_items)``).  The construction is ``exclusion_lists``'s; host tensors
    are range-checked here, device tensors are the caller's to check."""
    return _sorted_unique_lists('candidate_lists', 'candidate', offsets, items, n_items)


def search_topk(features: Tensor, users: Tensor, query_row0: int, item_row0: int, item_bias: Tensor, lam: float, k: int, *, queries: Optional[Tensor] = None,
                query_rows: Optional[Tensor] = None, candidates: Optional[Tensor] = None, cosine: bool = False,
                exclude: Optional[Tuple[Tensor, Tensor]] = None, exclude_rows: Optional[Tensor] = None):
    """``score_topk_deep`` for a search (``ihg_search_topk``): ``(top_items [C, k] int32, top_scores [C, k], passes [C] int32)``.  Exactly one of ``queries`` (int64
    ``[C]`` query indices) and ``query_rows`` (float32 ``[C, q]``, ``q <= D``: the rows of queries that are not in the graph - columns ``q ..`` count as zero);
    ``users[c] < 0``: no user, the mixed row is the query row; ``candidates`` (``pack_item_mask``'s input): only these items are ranked, a pair is complete at
    ``min(k, candidates)`` and the rest of its row is the ``-1`` tail.
    ``exclude`` (``ihg_search_topk_excluding``): per-search lists of items that are never ranked, ``(ptr [R + 1], items)``.  int32 ``items`` are taken as
    ``exclusion_lists`` returned them (every run strictly ascending); items of any other integer type are raw (any order, repeats) and go through it first.
    ``exclude_rows`` (int64 ``[C]``): search ``c`` leaves out run ``exclude_rows[c]``, nothing where that is negative; without it search ``c`` leaves out run ``c``
    and ``R = C``.  A search is then complete at ``min(k, its candidates that it does not exclude)``.  Without ``exclude`` the call is ``ihg_search_topk``'s."""
    if exclude is None and exclude_rows is not None:
        raise ValueError('search_topk: exclude_rows without exclude')
    lib = _lib.load()
    n_items, dim, bias = _rank_features('ihg_search_topk', features, item_row0, item_bias, score_topk_max_width())
    users, queries, query_rows, ld_q, q_dim, n_pairs = _rank_pairs('search_topk', features, users, queries, query_rows)
    mask = None if candidates is None else pack_item_mask(candidates.to(features.device), n_items)
    top_items, top_scores, passes = _rank_outputs(n_pairs, max(int(k), 0), features.device)
    entry, lists = 'search_topk', ()
    if exclude is not None:
        ptr, ids, exclude_rows, n_rows, _ = _search_lists('search_topk', exclude, exclude_rows, exclusion_lists, 'exclusion', 'exclude_rows', n_pairs, n_items, features.device)
        entry, lists = 'search_topk_excluding', (_ptr(ptr), _ptr(ids), _ptr(exclude_rows), n_rows)
    ws = _workspace(int(getattr(lib, f'ihg_{entry}_workspace_bytes')(n_pairs, n_items, dim, int(k))), features.device)
    with profiler.kernel(entry + '_cosine' if cosine else entry, n_pairs, dim):
        _lib.check(getattr(lib, 'ihg_' + entry)(_ptr(features), _ld(features), dim, int(query_row0), int(item_row0), n_items, _ptr(bias), _ptr(users), _ptr(queries), _ptr(query_rows),
                                                ld_q, q_dim, _ptr(mask), *lists, float(lam), n_pairs, int(k), _ptr(top_scores), _ptr(top_items), _ptr(ws), ws.numel() * 4,
                                                int(bool(cosine)), _ptr(passes), _stream()), 'ihg_' + entry)
    return top_items, top_scores, passes


def search_candidates_max_width() -> int:
    """The widest feature row ``ihg_search_candidates`` scores (2048): the LDS image of its mixed row, not the pair block of ``ihg_score_topk``."""
    return int(_lib.load().ihg_search_candidates_max_dim())


def search_candidates(features: Tensor, users: Tensor, query_row0: int, item_row0: int, item_bias: Tensor, lam: float, k: int, *, lists: Tuple[Tensor, Tensor],
                      list_rows: Optional[Tensor] = None, queries: Optional[Tensor] = None, query_rows: Optional[Tensor] = None, candidates: Optional[Tensor] = None,
                      exclude: Optional[Tuple[Tensor, Tensor]] = None, exclude_rows: Optional[Tensor] = None, cosine: bool = False, return_scores: bool = False):
    """Re-rank a shortlist per search (``ihg_search_candidates``): ``(top_items [C, k] int32, top_scores [C, k], passes [C] int32)``, and with ``return_scores`` the
    float32 ``[total]`` score of every list entry at its slot in the sorted lists (``-inf`` where ``candidates`` or ``exclude`` removes the entry).  Only the listed
    items are scored: the cost is the lists' total length times the width, with no pass over the catalogue.
    ``lists`` = ``(ptr [R + 1], items)``: int32 ``items`` are taken as ``candidate_lists`` returned them (every run strictly ascending); items of any other integer type
    are raw (any order, repeats) and go through it first.  ``list_rows`` (int64 ``[C]``): search ``c`` ranks run ``list_rows[c]``, nothing where that is negative;
    without it search ``c`` ranks run ``c`` and ``R = C``.  ``users`` / ``queries`` / ``query_rows`` / ``candidates`` / ``exclude`` / ``exclude_rows`` / ``cosine`` are
    ``search_topk``'s: a search ranks what is in its list, in ``candidates`` and not in its exclusion run, and is complete at ``min(k, that many)``.
    The scores are plain float32 sums (a per-lane chain, then a tree) and NOT the bits of ``search_topk``, whose operands are two fp16 terms each; both are within their
    bounds of the float64 score (``tests/candidates_reference.py``).  With ``return_scores`` and ``list_rows`` a run's slots hold the scores of the lowest-numbered search
    that names it, so searches that share a run must be the same search: a host ``list_rows`` that names a run twice is refused, a device one is the caller's."""
    if exclude is None and exclude_rows is not None:
        raise ValueError('search_candidates: exclude_rows without exclude')
    if not isinstance(lists, (tuple, list)) or len(lists) != 2:
        raise ValueError('search_candidates: lists is (offsets, items)')
    lib = _lib.load()
    n_items, dim, bias = _rank_features('ihg_search_candidates', features, item_row0, item_bias, search_candidates_max_width())
    users, queries, query_rows, ld_q, q_dim, n_pairs = _rank_pairs('search_candidates', features, users, queries, query_rows)
    cand_ptr, cand_ids, cand_rows, n_runs, total = _search_lists('search_candidates', lists, list_rows, candidate_lists, 'candidate', 'list_rows', n_pairs, n_items,
                                                                 features.device, need_a_run=True)
    if return_scores and list_rows is not None and not list_rows.is_cuda:
        named = list_rows[list_rows >= 0]
        if named.numel() != torch.unique(named).numel():
            raise ValueError('search_candidates: return_scores with a list that two searches share (a slot holds one score)')
    mask = None if candidates is None else pack_item_mask(candidates.to(features.device), n_items)
    excl_ptr, excl_ids, exclude_rows, n_excl, _ = (None, None, None, 0, 0) if exclude is None else _search_lists(
        'search_candidates', exclude, exclude_rows, exclusion_lists, 'exclusion', 'exclude_rows', n_pairs, n_items, features.device)
    top_items, top_scores, passes = _rank_outputs(n_pairs, max(int(k), 0), features.device)
    all_scores = torch.empty(total, dtype=torch.float32, device=features.device) if return_scores else None
    ws = _workspace(int(lib.ihg_search_candidates_workspace_bytes(n_pairs, total, dim, int(k))), features.device)
    with profiler.kernel('search_candidates_cosine' if cosine else 'search_candidates', n_pairs, dim):
        _lib.check(lib.ihg_search_candidates(_ptr(features), _ld(features), dim, int(query_row0), int(item_row0), n_items, _ptr(bias), _ptr(users), _ptr(queries),
                                             _ptr(query_rows), ld_q, q_dim, _ptr(mask), _ptr(excl_ptr), _ptr(excl_ids), _ptr(exclude_rows), n_excl, _ptr(cand_ptr),
                                             _ptr(cand_ids), _ptr(cand_rows), n_runs, total, float(lam), n_pairs, int(k), _ptr(top_scores), _ptr(top_items),
                                             _ptr(all_scores) if total else None, _ptr(ws), ws.numel() * 4, int(bool(cosine)), _ptr(passes), _stream()),
                   'ihg_search_candidates')
    if return_scores:
        return top_items, top_scores, passes, all_scores
    return top_items, top_scores, passes


def batch_node_rows(users: Tensor, queries: Tensor, items: Tensor, query_row0: int, item_row0: int) -> Tensor:
    """``torch.cat([users, queries + query_row0, items + item_row0])`` (``RawGnn.py:128-131``): the global node rows of a batch, int64 ``[3 B]``, one launch."""
    lib = _lib.load()
    if not users.is_cuda:
        return torch.cat([users, queries + query_row0, items + item_row0])
    u, q, i = (t.to(torch.int64).contiguous() for t in (users, queries, items))
    b = int(u.shape[0])
    rows = torch.empty(3 * b, dtype=torch.int64, device=u.device)
    rows32 = torch.empty(3 * b, dtype=torch.int32, device=u.device)
    _lib.check(lib.ihg_batch_node_rows(_ptr(u), _ptr(q), _ptr(i), b, int(query_row0), int(item_row0), _ptr(rows), _ptr(rows32), _stream()), 'ihg_batch_node_rows')
    rows.as_int32 = rows32                                   # the layers' row lists are int32: written by the same launch instead of a cast
    return rows


_UNIT = {}


def backward(loss: Tensor) -> None:
    """``loss.backward()`` with the root gradient taken from a cached ones scalar (autograd otherwise fills a fresh one every step: a framework launch)."""
    one = _UNIT.get(loss.device)
    if one is None:
        one = _UNIT[loss.device] = torch.ones((), dtype=loss.dtype, device=loss.device)
    loss.backward(one)


def hem_score(layers, rows: Tensor, items: Tensor, bias: Tensor, lam: float, item_row_offset: int, cosine: bool = False) -> Tensor:
    """HEM scores of a batch: ``rows`` = global node rows of users, queries, items (``[3B]`` int64), ``items`` = 0-based item
    ids (``[B]``), ``layers`` = the ``[N,d]`` outputs ``X_0..X_L`` whose concatenation the reference scores on.  ``cosine``: the cosine-similarity head
    (``Gs.Prediction.use_cosine_similarity``, ``PredictionLayers.py:38-40``) instead of the dot product."""
    return _HemScore.apply(rows, items, bias, float(lam), int(item_row_offset), bool(cosine), *layers)


def hem_bce_loss(layers, rows: Tensor, items: Tensor, labels: Tensor, bias: Tensor, lam: float, item_row_offset: int,
                 holder: Optional[TailGradients] = None, rows_upper: Optional[Tensor] = None, cosine: bool = False) -> Tensor:
    """``nn.BCEWithLogitsLoss()(hem_score(...), labels)`` as one differentiable op (scalar).  ``holder``: the layers are the
    tail halves of ``tap`` outputs made with this holder, and their gradients travel through it (see ``TailGradients``).  ``rows_upper`` (with ``holder.row_map``): the
    layers above layer 0 are numbered by the layout's own node ids (a layout without the isolated nodes): their rows of the batch, -1 = isolated = zero.  ``layers[0]`` may be a
    ``NodeTables`` (resolved by the first layer's transform): the head reads its layer-0 rows from the embedding tables in place.  ``cosine``: as in ``hem_score``."""
    return hem_loss(layers, rows, items, bce_objective(), bias, lam, item_row_offset, holder, rows_upper, cosine, labels)


def hem_loss(layers, rows: Tensor, items: Tensor, objective: Objective, bias: Tensor, lam: float, item_row_offset: int,
             holder: Optional[TailGradients] = None, rows_upper: Optional[Tensor] = None, cosine: bool = False, labels: Optional[Tensor] = None) -> Tensor:
    """``objective_loss(hem_score(...), objective, labels)`` as one differentiable op (scalar): the fused batch tail under any ``Objective`` - its launch is the one that
    differs.  ``labels`` are read by the plain BCE only; every other argument as in ``hem_bce_loss``."""
    objective.check_rows(int(items.shape[0]))
    tables = None
    layers = list(layers)
    if layers and isinstance(layers[0], NodeTables):
        tables = layers[0]
        if tables.query_rows is None or tables.token is None:
            raise RuntimeError('hem_loss: the NodeTables were not consumed by a node-level transform (a model without layers?)')
        layers[0] = tables.token
    if rows_upper is not None and holder is not None and holder.row_map is None:
        raise ValueError('rows_upper comes with holder.row_map (the layout\'s public -> own node map)')
    return _HemBceLoss.apply(rows, items, labels, bias, float(lam), int(item_row_offset), holder, tables, rows_upper, bool(cosine), objective, *layers)


class Objective:
    """The training objective of a batch of scores, checked on the host before anything is launched - the one description every layer passes on, from the training loop
    to the loss launch.  ``positives`` None: the BCE over labels (``kind`` is ``IHG_LOSS_BCE``).  Otherwise the batch is ``positives`` positives followed by the same
    number ``pool >= 1`` of negatives for each (``B % positives == 0``; those of positive ``p`` at rows ``P + p pool ..``), and neither labels nor a loss function are
    read: with ``keep`` None a ranking loss over all of them (``kind`` ``'bpr'`` / ``'softmax'``, or ``IHG_LOSS_BPR`` / ``IHG_LOSS_SOFTMAX``), else the loss ``kind``
    (``'bce'`` / ``IHG_LOSS_BCE`` too) over every positive and the ``keep`` candidates of its pool that score highest, ``1 <= keep <= pool <= 256``; the launch then leaves
    ``selected`` - int32 ``[positives, keep]``, the pool positions of every group's negatives, best first - so an ``Objective`` is made per call."""
    __slots__ = ('kind', 'positives', 'pool', 'keep', 'selected')

    def __init__(self, kind='bce', batch_rows: Optional[int] = None, positives: Optional[int] = None, keep: Optional[int] = None):
        self.selected = None
        if positives is None:
            if kind not in ('bce', _lib.HARD_NEGATIVE_KINDS['bce']) or isinstance(kind, bool) or keep is not None:
                raise ValueError(f'objective: kind {kind!r}' + (f' over the best {keep}' if keep is not None else '') + ' is a loss over groups: it needs positives')
            self.kind, self.positives, self.pool, self.keep = _lib.HARD_NEGATIVE_KINDS['bce'], None, None, None
            return
        what, kinds = ('ranking loss', _lib.LOSS_KINDS) if keep is None else ('hard negatives', _lib.HARD_NEGATIVE_KINDS)
        code = kinds.get(kind, kind) if isinstance(kind, str) else kind
        if isinstance(code, bool) or not isinstance(code, int) or code not in kinds.values():
            raise ValueError(f'{what}: kind is one of {sorted(kinds)}, got {kind!r}')
        batch_rows, positives = int(batch_rows), int(positives)
        if positives < 1 or batch_rows % positives != 0 or batch_rows // positives - 1 < 1:
            raise ValueError(f'{what}: a batch is P positives followed by the same number >= 1 of negatives (or pool candidates) for each: {batch_rows} rows cannot be '
                             f'split into {positives} groups')
        pool = batch_rows // positives - 1
        if keep is not None:
            keep = int(keep)
            if not 1 <= keep <= pool <= _lib.POOL_MAX:
                raise ValueError(f'hard negatives: need 1 <= keep <= pool <= {_lib.POOL_MAX}, got keep = {keep} of a pool of {pool}')
        self.kind, self.positives, self.pool, self.keep = code, positives, pool, keep

    @property
    def grouped(self) -> bool:
        """A loss over groups: no labels and no ``loss_function`` are needed."""
        return self.positives is not None

    @property
    def hard(self) -> bool:
        return self.keep is not None

    @property
    def label(self) -> str:
        """The profiler's name of the loss launch on the module path."""
        return 'hard_negative_loss' if self.hard else 'ranking_loss' if self.grouped else 'bce_with_logits'

    def key(self) -> tuple:
        """What a recording of the step holds of the objective (``CapturedTrainingStep`` compares it at every replay)."""
        return self.kind, self.positives, self.pool, self.keep

    def check_rows(self, batch_rows: int) -> None:
        if self.grouped and self.positives * (1 + self.pool) != batch_rows:
            raise ValueError(f'objective: made for {self.positives * (1 + self.pool)} rows, the batch has {batch_rows}')

    def launch(self, scores: Tensor, labels: Optional[Tensor], loss: Tensor, dscores: Tensor) -> None:
        """The loss launch: ``loss`` and ``dscores`` (d loss / d scores) of the float32 ``scores``; ``labels`` (float32) are read by the plain BCE only."""
        lib = _lib.load()
        if self.hard:
            self.selected = torch.empty(self.positives, self.keep, dtype=torch.int32, device=scores.device)
            _lib.check(lib.ihg_hard_negative_loss(_ptr(scores), self.positives, self.pool, self.keep, self.kind, _ptr(loss), _ptr(dscores), _ptr(self.selected), _stream()),
                       'ihg_hard_negative_loss')
        elif self.grouped:
            _lib.check(lib.ihg_ranking_loss(_ptr(scores), self.positives, self.pool, self.kind, _ptr(loss), _ptr(dscores), _stream()), 'ihg_ranking_loss')
        else:
            _lib.check(lib.ihg_bce_with_logits(_ptr(scores), _ptr(labels), int(scores.numel()), _ptr(loss), _ptr(dscores), _stream()), 'ihg_bce_with_logits')


def bce_objective() -> Objective:
    """The BCE over the batch's labels."""
    return Objective()


def ranking_objective(batch_rows: int, positives: int, kind) -> Objective:
    """The ranking loss ``kind`` (``'bpr'`` / ``'softmax'``) over a batch of ``batch_rows`` scores in ``positives`` groups."""
    return Objective(kind, batch_rows, positives)


def hard_negative_objective(batch_rows: int, positives: int, keep: int, kind) -> Objective:
    """The loss ``kind`` (``'bce'`` / ``'bpr'`` / ``'softmax'``) over every positive and the best ``keep`` of its pool, for a batch of ``batch_rows`` scores in
    ``positives`` groups."""
    return Objective(kind, batch_rows, positives, int(keep))


def training_objective(batch_rows: int, positives: Optional[int]) -> Objective:
    """The objective the settings name for a batch of ``batch_rows`` rows of which the first ``positives`` are the positives - the one reader of ``Gs.Training.loss``,
    ``Gs.Training.negative_pool`` (M > 0: the loader drew M candidates per positive) and ``Gs.random_negative_sample_size`` (of which a step then keeps this many) for
    the choice of a step; read at every call, as the model reads its head.  The plain BCE does not look at ``positives``."""
    from .Helpers.GlobalSettings import Gs
    kind, pool = Gs.Training.loss, int(Gs.Training.negative_pool)
    if kind == 'bce' and not pool:
        return bce_objective()
    if positives is None:
        raise ValueError(f'Gs.Training.loss = {kind!r}' + (f' with a pool of {pool}' if pool else '') +
                         ' needs positives= (the batch is P positives followed by the negatives of each)')
    batch_rows, positives = int(batch_rows), int(positives)
    if pool and batch_rows != positives * (1 + pool):
        raise ValueError(f'Gs.Training.negative_pool = {pool}, but the loader drew {batch_rows - positives} negatives for {positives} positives ({batch_rows} rows over '
                         f'{positives} positives carry a pool of {(batch_rows - positives) / max(positives, 1):g}): build the dataset with '
                         'random_negative_sample_size = the pool size (Main does)')
    return Objective(kind, batch_rows, positives, int(Gs.random_negative_sample_size) if pool else None)


def hem_hard_negative_loss(layers, rows: Tensor, items: Tensor, objective: Objective, bias: Tensor, lam: float, item_row_offset: int,
                           holder: Optional[TailGradients] = None, rows_upper: Optional[Tensor] = None, cosine: bool = False) -> Tensor:
    """``hard_negative_loss(hem_score(...), positives, keep, kind)`` as one differentiable op (scalar): ``hem_bce_loss`` with ``ihg_hard_negative_loss`` as its loss launch
    and no labels.  ``objective`` is ``hard_negative_objective``'s and holds ``selected`` afterwards.  The pool rows are ordinary batch rows; the rows of the candidates
    that are not selected get zero row gradients.  Every other argument as in ``hem_bce_loss``."""
    return hem_loss(layers, rows, items, objective, bias, lam, item_row_offset, holder, rows_upper, cosine)


def sample_pool(seed: int, counter: int, n_rows: int, n_items: int, m: int, device=None) -> Tensor:
    """``[n_rows, m]`` int64: ``m`` distinct items below ``n_items`` per row, ``1 <= m <= min(256, n_items)`` - ``ihg_sample_negatives``' stream continued past 16 draws
    (``ihg_sample_pool``: the first ``c`` columns are what ``m = c`` gives)."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty(max(int(n_rows), 0), max(int(m), 0), dtype=torch.int64, device=device)
    mask = (1 << 64) - 1
    with profiler.kernel('sample_pool', int(n_rows), int(m)):
        _lib.check(_lib.load().ihg_sample_pool(int(seed) & mask, int(counter) & mask, int(n_rows), int(n_items), int(m), _ptr(out), _stream()), 'ihg_sample_pool')
    return out


def sample_pool_excluding(seed: int, counter: int, n_rows: int, n_items: int, m: int, rows: Tensor, lists: Tuple[Tensor, Tensor], max_list_len: int,
                          device=None) -> Tensor:
    """``sample_pool`` without the items of a per-row list (``ihg_sample_pool_excluding``): ``[n_rows, m]`` int64, row ``r`` being row ``r`` of ``sample_pool``'s stream
    with the values of list ``rows[r]`` deleted.  ``lists = (ptr int64 [R + 1], items int32)`` as ``exclusion_lists`` returns them (every run strictly ascending), on the
    device; ``rows`` int64 ``[n_rows]`` names each row's run, a value outside ``[0, R)`` meaning none.  ``max_list_len`` is the longest run, known on the host (the
    launch never reads it back): ``m + max_list_len <= n_items`` is what lets every row find its ``m`` values.  One kernel for every ``1 <= m <= 256``."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    ptr, ids = lists
    n_rows = int(n_rows)
    operands = (('rows', rows, torch.int64), ('lists[0]', ptr, torch.int64), ('lists[1]', ids, torch.int32))
    for name, t, dtype in operands:
        if t.dtype != dtype or t.dim() != 1:
            raise TypeError(f'sample_pool_excluding: {name} must be a 1-D {dtype} tensor, got {tuple(t.shape)} {t.dtype}')
    for name, t, _ in operands:
        _gpu(t, f'sample_pool_excluding: {name}')
        if device.index is not None and t.device.index != device.index:
            raise ValueError(f'sample_pool_excluding: {name} is on {t.device}, the draw on {device}')
    if int(rows.shape[0]) != max(n_rows, 0):
        raise ValueError(f'sample_pool_excluding: {n_rows} rows but rows of {tuple(rows.shape)}')
    if int(ptr.shape[0]) < 1:
        raise ValueError('sample_pool_excluding: lists[0] holds at least the leading 0')
    rows, ptr, ids = rows.contiguous(), ptr.contiguous(), ids.contiguous()
    if not ids.numel():
        ids = ids.new_zeros(1)                                                  # (an empty tensor has no address; no offset reaches this entry)
    out = torch.empty(max(n_rows, 0), max(int(m), 0), dtype=torch.int64, device=device)
    mask = (1 << 64) - 1
    with profiler.kernel('sample_pool_excluding', n_rows, int(m)):
        _lib.check(_lib.load().ihg_sample_pool_excluding(int(seed) & mask, int(counter) & mask, n_rows, int(n_items), int(m), _ptr(rows), int(ptr.shape[0]) - 1, _ptr(ptr),
                                                         _ptr(ids), int(max_list_len), _ptr(out), _stream()), 'ihg_sample_pool_excluding')
    return out


def item_sampling_table(weights, device=None) -> Tuple[Tensor, int]:
    """The table ``ihg_sample_pool_weighted`` draws from: ``(cum, total)`` with ``cum`` int64 ``[I + 1]`` on the device, ``cum[0] = 0``, ``cum[i + 1] = cum[i] + weights[i]``,
    and ``total = cum[I]`` as a Python int.  ``weights`` is int64 ``[I]``, a host array or tensor (the table then goes to ``device``, default the current GPU) or a device
    tensor (the table stays beside it).  Every weight must be >= 1 and the sum below 2^63: this is the one place where the launch's promise of a strictly ascending
    ``cum`` is checked - before anything is copied for host weights, with one read-back for device weights."""
    w = weights if isinstance(weights, Tensor) else torch.from_numpy(np.ascontiguousarray(weights))
    if w.dtype != torch.int64 or w.dim() != 1 or not w.numel():
        raise TypeError(f'item_sampling_table: weights must be a non-empty 1-D int64 array, got {tuple(w.shape)} {w.dtype}')
    if w.is_cuda and device is not None and torch.device(device).index not in (None, w.device.index):
        raise ValueError(f'item_sampling_table: weights are on {w.device}, the table was asked for on {torch.device(device)}')
    cum = torch.zeros(int(w.shape[0]) + 1, dtype=torch.int64, device=w.device)
    torch.cumsum(w, 0, out=cum[1:])                                             # (int64 wraps: positive weights whose sum passes 2^63 show as a step down)
    smallest, ascending = int(w.min()), bool((cum[1:] > cum[:-1]).all())
    if smallest < 1:
        raise ValueError(f'item_sampling_table: every weight must be >= 1 (an item of weight 0 can never be drawn, and the draw would not end once the others are used up), '
                         f'got a smallest weight of {smallest}')
    if not ascending:
        raise ValueError('item_sampling_table: the weights sum to 2^63 or more; the thresholds of the draw are int64')
    total = int(cum[-1])
    if not cum.is_cuda:
        cum = cum.to(torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device))
    return cum, total


def sample_pool_weighted(seed: int, counter: int, n_rows: int, n_items: int, m: int, table: Tuple[Tensor, int], rows: Optional[Tensor] = None,
                         lists: Optional[Tuple[Tensor, Tensor]] = None, max_list_len: int = 0, device=None) -> Tensor:
    """``sample_pool`` / ``sample_pool_excluding`` with item weights (``ihg_sample_pool_weighted``): ``[n_rows, m]`` int64, ``m`` distinct items per row, every attempt
    falling on item ``i`` with probability ``weights[i] / total``.  ``table = (cum, total)`` is ``item_sampling_table``'s, on the device, ``cum`` of ``n_items + 1`` entries.
    ``rows`` and ``lists`` are ``sample_pool_excluding``'s and come together or not at all (``None``: no row has a list); ``max_list_len`` is the longest run, known on the
    host.  With weights all equal the output is ``sample_pool_excluding``'s / ``sample_pool``'s bit for bit.  One kernel for every ``1 <= m <= 256``."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    cum, total = table
    n_rows = int(n_rows)
    if (rows is None) != (lists is None):
        raise ValueError('sample_pool_weighted: rows and lists come together (both None: no row has a list)')
    ptr, ids = lists if lists is not None else (None, None)
    operands = (('table[0]', cum, torch.int64),) + ((('rows', rows, torch.int64), ('lists[0]', ptr, torch.int64), ('lists[1]', ids, torch.int32)) if lists is not None else ())
    for name, t, dtype in operands:
        if not isinstance(t, Tensor) or t.dtype != dtype or t.dim() != 1:
            raise TypeError(f'sample_pool_weighted: {name} must be a 1-D {dtype} tensor, got {tuple(t.shape)} {t.dtype}' if isinstance(t, Tensor) else
                            f'sample_pool_weighted: {name} must be a 1-D {dtype} tensor, got {type(t).__name__}')
    for name, t, _ in operands:
        _gpu(t, f'sample_pool_weighted: {name}')
        if device.index is not None and t.device.index != device.index:
            raise ValueError(f'sample_pool_weighted: {name} is on {t.device}, the draw on {device}')
    if int(cum.shape[0]) != int(n_items) + 1:
        raise ValueError(f'sample_pool_weighted: a table of {int(cum.shape[0])} entries does not belong to {int(n_items)} items (item_sampling_table gives n_items + 1)')
    cum = cum.contiguous()
    n_lists = 0
    if lists is not None:
        if int(rows.shape[0]) != max(n_rows, 0):
            raise ValueError(f'sample_pool_weighted: {n_rows} rows but rows of {tuple(rows.shape)}')
        if int(ptr.shape[0]) < 1:
            raise ValueError('sample_pool_weighted: lists[0] holds at least the leading 0')
        rows, ptr, ids = rows.contiguous(), ptr.contiguous(), ids.contiguous()
        if not ids.numel():
            ids = ids.new_zeros(1)                                              # (an empty tensor has no address; no offset reaches this entry)
        n_lists = int(ptr.shape[0]) - 1
        if n_lists == 0:
            rows = ptr = ids = None                                             # (no run at all: the launch's form without lists)
    out = torch.empty(max(n_rows, 0), max(int(m), 0), dtype=torch.int64, device=device)
    mask = (1 << 64) - 1
    with profiler.kernel('sample_pool_weighted', n_rows, int(m)):
        _lib.check(_lib.load().ihg_sample_pool_weighted(int(seed) & mask, int(counter) & mask, n_rows, int(n_items), int(m), _ptr(cum), int(total), _ptr(rows), n_lists,
                                                        _ptr(ptr), _ptr(ids), int(max_list_len), _ptr(out), _stream()), 'ihg_sample_pool_weighted')
    return out


def hem_ranking_loss(layers, rows: Tensor, items: Tensor, positives: int, kind, bias: Tensor, lam: float, item_row_offset: int,
                     holder: Optional[TailGradients] = None, rows_upper: Optional[Tensor] = None, cosine: bool = False) -> Tensor:
    """``ranking_loss(hem_score(...), positives, kind)`` as one differentiable op (scalar): ``hem_bce_loss`` with ``ihg_ranking_loss`` as its loss launch and no labels.
    The batch rows are ``positives`` positives followed by the ``k`` negatives of each (``collate_fn``'s layout); every other argument as in ``hem_bce_loss``."""
    return hem_loss(layers, rows, items, ranking_objective(int(items.shape[0]), positives, kind), bias, lam, item_row_offset, holder, rows_upper, cosine)


# ---------------------------------------------------------------------------------------------
# the Srrl baseline (Models/Srrl.py): block = F.normalize(cat(a, b)) -> Linear -> LeakyReLU, row dots, KG loss, dense top-k
# ---------------------------------------------------------------------------------------------
def _gpu(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:
        raise _lib.IhgnnHipError(f'{name} must be a GPU tensor: ihgnn_amd has no CPU path (got device {t.device})')
    return t


def _index(idx: Optional[Tensor], name: str) -> Optional[Tensor]:
    if idx is None:
        return None
    _gpu(idx, name)
    return idx.to(torch.int64).contiguous()


def scatter_row_gradients(rowgrad: Tensor, idx: Tensor, n_rows: int) -> Tensor:
    """``zeros [n_rows, w]`` with ``out[idx[k]] += rowgrad[k]``: the rows of equal destination are combined in batch order (``ihg_batch_combine``), then added
    (``ihg_batch_rows_add``) - no atomics, at most ``SCATTER_CHUNK_ROWS`` rows per launch.  ``rowgrad`` is used up (combined in place)."""
    lib = _lib.load()
    _gpu(rowgrad, 'rowgrad')
    width = int(rowgrad.shape[1])
    dense = torch.zeros(n_rows, width, dtype=torch.float32, device=rowgrad.device)
    n = int(idx.shape[0])
    for lo in range(0, n, SCATTER_CHUNK_ROWS):
        hi = min(lo + SCATTER_CHUNK_ROWS, n)
        part, rows = rowgrad[lo:hi], idx[lo:hi]
        leader = torch.empty(hi - lo, dtype=torch.int32, device=rowgrad.device)
        with profiler.kernel('batch_combine', hi - lo, width):
            _lib.check(lib.ihg_batch_combine(_ptr(part), _ld(rowgrad), width, _ptr(rows), hi - lo, 0, _ptr(leader), _stream()), 'ihg_batch_combine')
        with profiler.kernel('batch_rows_add', hi - lo, width):
            _lib.check(lib.ihg_batch_rows_add(_ptr(part), _ld(rowgrad), width, _ptr(rows), _ptr(leader), hi - lo, _ptr(dense), _ld(dense), None, 0, 0, _stream()),
                       'ihg_batch_rows_add')
    return dense


def _cat_source(t: Optional[Tensor], idx: Optional[Tensor], rep: int):
    """The five arguments of one source of the block."""
    if t is None:
        return (None, 0, 0, None, 1)
    return (_ptr(t), _ld(t), int(t.shape[1]), _ptr(idx), int(rep))


def _source_groups(t: Tensor, idx: Optional[Tensor]) -> int:
    return int(t.shape[0]) if idx is None else int(idx.shape[0])


class _CatLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a: Tensor, b: Optional[Tensor], w: Tensor, bias: Optional[Tensor], idx_a: Optional[Tensor], rep_a: int, idx_b: Optional[Tensor], rep_b: int,
                normalize: bool, activation: int) -> Tensor:
        lib = _lib.load()
        a = _rows(a.detach(), 'a')
        b = None if b is None else _rows(b.detach(), 'b')
        wd = _rows(w.detach(), 'w')
        bd = None if bias is None else _gpu(bias.detach(), 'bias').contiguous()
        idx_a, idx_b = _index(idx_a, 'idx_a'), _index(idx_b, 'idx_b')
        n_rows = _source_groups(a, idx_a) * rep_a
        if b is not None and _source_groups(b, idx_b) * rep_b != n_rows:
            raise ValueError(f'cat_linear: {n_rows} rows of a against {_source_groups(b, idx_b) * rep_b} of b')
        m = int(wd.shape[0])
        out = torch.empty(n_rows, m, dtype=torch.float32, device=a.device)
        inv_norm = torch.empty(n_rows, dtype=torch.float32, device=a.device) if normalize else None
        with profiler.kernel('cat_linear_fwd', n_rows, m):
            _lib.check(lib.ihg_cat_linear_fwd(*_cat_source(a, idx_a, rep_a), *_cat_source(b, idx_b, rep_b), _ptr(wd), _ld(wd), _ptr(bd), m, int(normalize), activation,
                                              _ptr(out), m, _ptr(inv_norm), n_rows, _stream()), 'ihg_cat_linear_fwd')
        ctx.save_for_backward(a, b, wd, idx_a, idx_b, inv_norm, out)      # (out through save_for_backward: an attribute would tie the node to its own output)
        ctx.args = (rep_a, rep_b, normalize, activation, bias is not None)
        return out

    @staticmethod
    def backward(ctx, dy: Tensor):
        lib = _lib.load()
        a, b, w, idx_a, idx_b, inv_norm, out = ctx.saved_tensors
        rep_a, rep_b, normalize, activation, has_bias = ctx.args
        need_a, need_b = ctx.needs_input_grad[0], b is not None and ctx.needs_input_grad[1]
        dy = _rows(dy, 'dy')
        n_rows, m = int(out.shape[0]), int(out.shape[1])
        wa, wb = int(a.shape[1]), 0 if b is None else int(b.shape[1])
        dw = torch.empty_like(w, memory_format=torch.contiguous_format)
        dbias = torch.empty(m, dtype=torch.float32, device=w.device) if has_bias else None
        da = torch.empty(n_rows // rep_a, wa, dtype=torch.float32, device=w.device) if need_a else None
        db = torch.empty(n_rows // rep_b, wb, dtype=torch.float32, device=w.device) if need_b else None
        ws = _workspace(int(lib.ihg_cat_linear_workspace_bytes(n_rows, wa + wb, m)), w.device)
        with profiler.kernel('cat_linear_bwd', n_rows, m):
            _lib.check(lib.ihg_cat_linear_bwd(_ptr(dy), _ld(dy), _ptr(out), m, *_cat_source(a, idx_a, rep_a), *_cat_source(b, idx_b, rep_b), _ptr(inv_norm), _ptr(w), _ld(w), m,
                                              int(normalize), activation, _ptr(dw), wa + wb, _ptr(dbias), _ptr(da), wa, _ptr(db), wb, n_rows, _ptr(ws), ws.numel() * 4,
                                              _stream()), 'ihg_cat_linear_bwd')
        if need_a and idx_a is not None:
            da = scatter_row_gradients(da, idx_a, int(a.shape[0]))
        if need_b and idx_b is not None:
            db = scatter_row_gradients(db, idx_b, int(b.shape[0]))
        return da, db, dw, dbias, None, None, None, None, None, None


def cat_linear_max_width() -> int:
    """The widest concatenated row, and the widest output row, ``cat_linear`` takes (256)."""
    return int(_lib.load().ihg_cat_linear_max_width())


def cat_linear(a: Tensor, b: Optional[Tensor], w: Tensor, bias: Optional[Tensor], idx_a: Optional[Tensor] = None, rep_a: int = 1, idx_b: Optional[Tensor] = None,
               rep_b: int = 1, normalize: bool = True, leaky: bool = False) -> Tensor:
    """``act(F.normalize(cat(a[idx_a].repeat_interleave(rep_a), b[idx_b].repeat_interleave(rep_b)), dim=-1) @ w.T + bias)`` as one launch, ``[rows, m]``; its backward is one
    call too (``ihg_cat_linear_bwd``), and a gathered source's gradient reaches its table through the deterministic batch-row scatter.  ``b`` may be ``None``;
    ``normalize=False`` is a plain Linear; ``leaky``: ``nn.LeakyReLU()``."""
    if w.dim() != 2 or w.shape[1] != a.shape[1] + (0 if b is None else b.shape[1]):
        raise ValueError(f'cat_linear: weight {tuple(w.shape)} against sources of width {a.shape[1]} + {0 if b is None else b.shape[1]}')
    return _CatLinear.apply(a, b, w, bias, idx_a, int(rep_a), idx_b, int(rep_b), bool(normalize), _lib.ACT_LEAKY_RELU if leaky else _lib.ACT_NONE)


class _RowsDot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, y: Tensor, rep: int) -> Tensor:
        lib = _lib.load()
        x, y = _rows(x.detach(), 'x'), _rows(y.detach(), 'y')
        n_rows, width = int(x.shape[0]), int(x.shape[1])
        if int(y.shape[0]) * rep != n_rows or int(y.shape[1]) != width:
            raise ValueError(f'rows_dot: x {tuple(x.shape)} against y {tuple(y.shape)} repeated {rep} times')
        s = torch.empty(n_rows, dtype=torch.float32, device=x.device)
        with profiler.kernel('rows_dot_fwd', n_rows, width):
            _lib.check(lib.ihg_rows_dot_fwd(_ptr(x), _ld(x), _ptr(y), _ld(y), rep, _ptr(s), n_rows, width, _stream()), 'ihg_rows_dot_fwd')
        ctx.save_for_backward(x, y)
        ctx.rep = rep
        return s

    @staticmethod
    def backward(ctx, ds: Tensor):
        lib = _lib.load()
        x, y = ctx.saved_tensors
        rep = ctx.rep
        ds = ds.contiguous()
        n_rows, width = int(x.shape[0]), int(x.shape[1])
        dx = torch.empty(n_rows, width, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[0] else None
        dy = torch.empty(n_rows // rep, width, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[1] else None
        with profiler.kernel('rows_dot_bwd', n_rows, width):
            _lib.check(lib.ihg_rows_dot_bwd(_ptr(ds), _ptr(x), _ld(x), _ptr(y), _ld(y), rep, _ptr(dx), width, _ptr(dy), width, n_rows, width, _stream()), 'ihg_rows_dot_bwd')
        return dx, dy, None


def rows_dot(x: Tensor, y: Tensor, rep: int = 1) -> Tensor:
    """``(x * y.repeat_interleave(rep, 0)).sum(-1)``: the KG scores of ``Models/Srrl.py`` with their broadcast over the negatives, ``[rows]``."""
    return _RowsDot.apply(x, y, int(rep))


class _KgLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos: Tensor, neg: Tensor, weight: Optional[Tensor]) -> Tensor:
        lib = _lib.load()
        pos = _gpu(pos.detach(), 'pos').contiguous().view(-1)
        neg = _rows(neg.detach(), 'neg')
        weight = None if weight is None else _gpu(weight, 'weight').to(torch.float32).contiguous()
        batch, k = int(neg.shape[0]), int(neg.shape[1])
        if int(pos.shape[0]) != batch or (weight is not None and int(weight.shape[0]) != batch):
            raise ValueError(f'kg_loss: pos {tuple(pos.shape)}, neg {tuple(neg.shape)}')
        loss = torch.empty((), dtype=torch.float32, device=pos.device)
        dpos = torch.empty(batch, dtype=torch.float32, device=pos.device)
        dneg = torch.empty(batch, k, dtype=torch.float32, device=pos.device)
        with profiler.kernel('kg_loss', batch, k):
            _lib.check(lib.ihg_kg_loss(_ptr(pos), _ptr(neg), _ld(neg), _ptr(weight), batch, k, _ptr(loss), _ptr(dpos), _ptr(dneg), k, _stream()), 'ihg_kg_loss')
        ctx.save_for_backward(dpos, dneg)
        return loss

    @staticmethod
    def backward(ctx, grad_loss: Tensor):
        dpos, dneg = ctx.saved_tensors
        return dpos * grad_loss, dneg * grad_loss, None


def kg_loss(pos: Tensor, neg: Tensor, weight: Optional[Tensor] = None) -> Tensor:
    """The KG loss of ``Helpers/TrainTestHelper.py:185-201``: ``(-sum w logsigmoid(pos) / sum w - sum w logsigmoid(-neg).mean(1) / sum w) / 2`` with its gradient, one launch;
    ``weight=None``: uniform (``Gs.Srrl.uni_weight``).  ``pos [B]``, ``neg [B, k]``."""
    return _KgLoss.apply(pos, neg, weight)


def rows_topk(scores: Tensor, k: int):
    """The ``k`` best entries of every row of a dense ``[C, I]`` score matrix, best first, equal scores in ascending item id (``score_topk``'s order):
    ``(items [C, k] int64, scores [C, k])``, ``-1`` / ``-inf`` beyond ``I`` entries."""
    lib = _lib.load()
    scores = _rows(scores.detach(), 'scores')
    n_rows, n_items = int(scores.shape[0]), int(scores.shape[1])
    items = torch.empty(n_rows, max(int(k), 0), dtype=torch.int64, device=scores.device)
    top = torch.empty(n_rows, max(int(k), 0), dtype=torch.float32, device=scores.device)
    with profiler.kernel('rows_topk', n_rows, int(k)):
        _lib.check(lib.ihg_rows_topk(_ptr(scores), _ld(scores), n_rows, n_items, int(k), _ptr(items), _ptr(top), _stream()), 'ihg_rows_topk')
    return items, top


class _ScoreLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores: Tensor, objective: Objective, labels: Optional[Tensor]) -> Tensor:
        scores = _gpu(scores.detach(), 'scores').to(torch.float32).contiguous()
        if not objective.grouped:
            labels = _gpu(labels, 'labels').to(torch.float32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=scores.device)
        dscores = torch.empty_like(scores)
        with profiler.kernel(objective.label, int(scores.numel()), 1):
            objective.launch(scores, labels, loss, dscores)
        ctx.save_for_backward(dscores)
        return loss

    @staticmethod
    def backward(ctx, grad_loss: Tensor):
        return ctx.saved_tensors[0] * grad_loss, None, None


def _score_vector(scores: Tensor, what: str) -> int:
    if scores.dim() != 1:
        raise ValueError(f'{what} takes the scores of a batch as a vector, got {tuple(scores.shape)}')
    return int(scores.shape[0])


def objective_loss(scores: Tensor, objective: Objective, labels: Optional[Tensor] = None) -> Tensor:
    """The loss of ``scores`` under ``objective`` (``labels``: the plain BCE's) with its gradient from the objective's one launch: the module path, where the fused tail
    (``hem_loss``) does not apply."""
    if objective.grouped:
        objective.check_rows(_score_vector(scores, 'objective_loss'))
    return _ScoreLoss.apply(scores, objective, labels)


def bce_with_logits(scores: Tensor, labels: Tensor) -> Tensor:
    """``nn.BCEWithLogitsLoss()(scores, labels)`` with its gradient from the one launch of ``ihg_bce_with_logits``."""
    return objective_loss(scores, bce_objective(), labels)


def ranking_loss(scores: Tensor, positives: int, kind) -> Tensor:
    """The BPR (``kind='bpr'``) or sampled-softmax (``'softmax'``) loss of ``scores`` ``[P (1 + k)]`` - ``positives = P`` positives followed by the ``k`` negatives of
    each, ``collate_fn``'s layout - with its gradient from the one launch of ``ihg_ranking_loss``: the sibling of ``bce_with_logits`` where the fused tail
    (``hem_ranking_loss``) does not apply."""
    return objective_loss(scores, ranking_objective(_score_vector(scores, 'ranking_loss'), positives, kind))


def hard_negative_loss(scores: Tensor, positives: int, keep: int, kind, return_selected: bool = False):
    """The loss ``kind`` (``'bce'``, ``'bpr'``, ``'softmax'``) of ``scores`` ``[P (1 + M)]`` - ``positives = P`` positives followed by the ``M`` pool candidates of each -
    over every positive and the ``keep`` candidates of its pool that score highest (ties: the lower pool position), with its gradient - exactly zero on the other
    candidates - from the one launch of ``ihg_hard_negative_loss``: the sibling of ``ranking_loss`` where the fused tail (``hem_hard_negative_loss``) does not apply.
    ``return_selected``: also the ``[P, keep]`` pool positions of the negatives, best first (int64, detached)."""
    objective = hard_negative_objective(_score_vector(scores, 'hard_negative_loss'), positives, keep, kind)
    loss = objective_loss(scores, objective)
    return (loss, objective.selected.to(torch.int64)) if return_selected else loss


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table: Tensor, idx: Tensor) -> Tensor:
        _gpu(table, 'table')
        idx = _index(idx, 'idx')
        ctx.save_for_backward(idx)
        ctx.n_rows = int(table.shape[0])
        return table.detach().index_select(0, idx)

    @staticmethod
    def backward(ctx, grad: Tensor):
        return scatter_row_gradients(_rows(grad, 'grad').clone(), ctx.saved_tensors[0], ctx.n_rows), None


def gather_rows(table: Tensor, idx: Tensor) -> Tensor:
    """``table[idx]`` whose backward is the deterministic batch-row scatter (``scatter_row_gradients``) instead of autograd's atomic ``index_put_``."""
    return _GatherRows.apply(table, idx)
